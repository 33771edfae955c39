// The error bound of a one-pass search (fp16 "hi" parts only, lvs_nearest_hi / lvs_nearest3), stated once: its five
// coefficients and its evaluation from the corpus statistics.  Every exactness certificate and the Hamerly bounds of the
// k-means rest on it: margin_select_kernel (lvs_capi.hip), nearest3_select_kernel (lvs_assign.hip), km_bounds_set_kernel and
// km_bounds_fix_kernel (lvs_kmeans.hip), lvs_kmeans_iteration (lvs_kmiter.hip) and HipBackend._nearest_coef (the entry point
// lvs_nearest_bound_coef).  Host-only in the sense of lvs_plan.h: no HIP header, a plain C++17 host compiler builds this file
// (tests/native/plan_check.cpp answers `bound_coef` from it); the evaluation also runs in the kernels.
#pragma once
#include <math.h>

#include "lvs_plan.h"

// bound(q) = (c[0] E + c[1] R) |q| + c[2] + c[3] R + c[4] R^2 with R = largest row norm, E = largest lo-part norm of the corpus
// rows (include/lotus_hip.h, lvs_margin_select_stats).  Five consecutive floats: passed to a kernel by value.
struct LvsBoundCoef {
    float c[5];
};

// Error bound per unit of |q|: E = largest lo-part norm and R = largest norm over the corpus rows (a small matrix in the
// k-means use: the centroids).  bound = scale |q| + slack with
//   scale = c (E + 2^-11 R [queries split] + 8e-6 R) + 2^-16 cm R     (c = 2 / 4, cm = 1 / 2 for IP / L2; 8e-6: fp32
//   slack = 1e-6 (2^exp_sum + R^2) + [L2] 2^-16 R^2 + [queries split] c sqrt(dpad) 2^-25 R      accumulation noise of both searches)
// lvs_nearest_hi tags every running score in its low six mantissa bits (relative perturbation < 2^-17 of u = q.y or
// 2 q.y - |y|^2, for the winner and for the runner-up): the 2^-16 terms.  |lo_q| <= 2^-11 |q| + sqrt(dpad) 2^-25: the second
// term covers components in fp16's subnormal range.  exp_sum: the pack exponents of the two operands added (the scores carry
// 2^exp_sum); dpad = d rounded up to a K-step.  Computed in double, rounded to float at the end.
static inline int32_t lvs_nearest_bound_coef(int32_t metric, int32_t xq_pack, int32_t d, int32_t exp_sum, LvsBoundCoef& out) {
    const bool ip = metric == LVS_METRIC_IP;
    if ((!ip && metric != LVS_METRIC_L2) || (xq_pack != LVS_PACK_F16 && xq_pack != LVS_PACK_SPLIT) || d <= 0) return LVS_EINVAL;
    const double c = ip ? 2.0 : 4.0, qsplit = xq_pack == LVS_PACK_SPLIT ? 1.0 : 0.0;
    const double dpad = (double)lvs_round_up(d, LVS_BK);
    out.c[0] = (float)c;
    out.c[1] = (float)(c * (ldexp(1.0, -11) * qsplit + 8e-6) + ldexp(1.0, -16) * (ip ? 1.0 : 2.0));
    out.c[2] = (float)(1e-6 * ldexp(1.0, exp_sum));
    out.c[3] = (float)(qsplit * c * sqrt(dpad) * ldexp(1.0, -25));
    out.c[4] = (float)(1e-6 + (ip ? 0.0 : ldexp(1.0, -16)));
    return LVS_OK;
}

// The bound from the statistics a k-means keeps on the device: stats[0] = R^2, stats[1] = E^2.
//   scale(), slack()  the certificates evaluate scale |q| + slack per query;
//   at(qnorm)         the bound at |q| = qnorm, summed left to right from scale |q| on, as the Hamerly bounds always have it
//                     (the two roundings differ in the last bit: each user keeps its own so that no result moves).
struct LvsBound {
    const LvsBoundCoef& k;
    float R, E;
    LVS_HD LvsBound(const LvsBoundCoef& coef, const float* stats) : k(coef), R(sqrtf(stats[0])), E(sqrtf(stats[1])) {}
    LVS_HD float scale() const { return k.c[0] * E + k.c[1] * R; }
    LVS_HD float slack() const { return rest(k.c[2]); }
    LVS_HD float at(float qnorm) const { return rest(scale() * qnorm + k.c[2]); }
    LVS_HD float rest(float head) const { return head + k.c[3] * R + k.c[4] * R * R; }
};
