// Device helpers shared by the exactness certificates: the exact score of (query, row) pairs (rescore_keys_kernel in
// lvs_capi.hip, resolve_pairs_kernel in lvs_assign.hip), the launch dispatch on the operands' pack modes, and the two-sweep
// append of query indices to lists (margin_select_kernel, nearest3_select_kernel, km_bounds_step_kernel in lvs_kmeans.hip).
#pragma once
#include <type_traits>

#include "lvs_bound.h"
#include "lvs_common.h"

// One wave per query: the exact dot products (fp32, hi + lo parts of both operands) of the query row qr with NR corpus rows.
// Lane l takes halfs [8 l, 8 l + 8) of every 512; the hi + lo sums are formed before the multiply; every lane returns the
// wave's sums.  Every multiply-add and the squared-L2 finish are FUSED by name (fmaf), not left to the compiler's contraction:
// left alone it fused resolve_pairs_kernel's and not rescore_keys_kernel's, and the two "same" scores of a pair were up to 32
// float32 ulps apart (tests/test_gpu_certificates.py::test_resolve_pairs).  Both kernels now round as resolve_pairs_kernel did.
// (NR = 1 or 2, the second row written out beside the first: as a loop over rows the compiler orders the sums otherwise.)
struct LvsDots {
    float a, b;  // b: NR == 2 only
};
template <int QS, int BS, int NR>
__device__ __forceinline__ LvsDots lvs_exact_dots(const _Float16* qr, const _Float16* ar, const _Float16* br, int dpad, int lane) {
    static_assert(NR == 1 || NR == 2, "one or two rows");
    float sa = 0.f, sb = 0.f;
    for (int j = lane * 8; j < dpad; j += 512) {
        const half8 qh = *(const half8*)(qr + j), ah = *(const half8*)(ar + j);
        half8 bh, ql, al, bl;
        if (NR > 1) bh = *(const half8*)(br + j);
        if (QS) ql = *(const half8*)(qr + dpad + j);
        if (BS) {
            al = *(const half8*)(ar + dpad + j);
            if (NR > 1) bl = *(const half8*)(br + dpad + j);
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float x = (float)qh[t] + (QS ? (float)ql[t] : 0.f);
            sa = fmaf(x, (float)ah[t] + (BS ? (float)al[t] : 0.f), sa);
            if (NR > 1) sb = fmaf(x, (float)bh[t] + (BS ? (float)bl[t] : 0.f), sb);
        }
    }
    sa = lvs_wave_sum(sa);
    if (NR > 1) sb = lvs_wave_sum(sb);
    return {sa, sb};
}
// the squared-L2 score ("larger = better") of a pair from its exact dot product s and the two squared norms
__device__ __forceinline__ float lvs_l2_score(float qn, float bn, float s) { return -fmaxf(fmaf(-2.0f, s, qn + bn), 0.f); }

// launch(QS, BS) with the two pack modes as compile-time constants: launch = [&](auto qs, auto bs) { kernel<qs(), bs()> ... }
template <class Launch>
inline void lvs_split_dispatch(int32_t xq_pack, int32_t xb_pack, Launch&& launch) {
    if (xq_pack == LVS_PACK_SPLIT && xb_pack == LVS_PACK_SPLIT) launch(std::true_type{}, std::true_type{});
    else if (xq_pack == LVS_PACK_SPLIT) launch(std::true_type{}, std::false_type{});
    else if (xb_pack == LVS_PACK_SPLIT) launch(std::false_type{}, std::true_type{});
    else launch(std::false_type{}, std::false_type{});
}

// Two-sweep append of query indices to NL index lists (order unspecified).  A workgroup owns per_block consecutive queries of the
// nq: first(q) and again(q) -> 0 = not listed, i = list i (out[i - 1], counts[i - 1]).  It counts its listed queries with first,
// reserves their output ranges with ONE atomic per list (10 M queries at 0.4 % uncertified were 30 000 same-address atomics =
// 1.2 ms when every wave reserved its own), then writes them in a second sweep over the same few bytes per query with again -
// which must class every query as first did (the same function, unless first also updates what again reads).
// lvs_append_per_block: at most 2048 workgroups, each at least 1024 queries; the grid is ceil(nq / per_block) x 256 threads.
inline long long lvs_append_per_block(long long nq) {
    return lvs_round_up(lvs_ceil_div(nq, 2048) < 1024 ? 1024 : lvs_ceil_div(nq, 2048), 256);
}
template <int NL, class First, class Again>
__device__ __forceinline__ void lvs_append_lists(long long per_block, long long nq, First&& first, Again&& again,
                                                 long long* const (&out)[NL], unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long s_base[NL];
    __shared__ unsigned s_count[NL];
    const long long q_begin = (long long)blockIdx.x * per_block;
    const long long q_end = q_begin + per_block < nq ? q_begin + per_block : nq;
    if (threadIdx.x < NL) s_count[threadIdx.x] = 0;
    __syncthreads();
    unsigned mine[NL] = {};
    for (long long q = q_begin + threadIdx.x; q < q_end; q += blockDim.x) {
        const int c = first(q);
        if (c) ++mine[c - 1];
    }
#pragma unroll
    for (int i = 0; i < NL; ++i)
        if (mine[i]) atomicAdd(&s_count[i], mine[i]);
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int i = 0; i < NL; ++i) any |= s_count[i] != 0;
    if (!any) return;
    if (threadIdx.x < NL) {
        s_base[threadIdx.x] = s_count[threadIdx.x] ? atomicAdd(&counts[threadIdx.x], (unsigned long long)s_count[threadIdx.x]) : 0ull;
        s_count[threadIdx.x] = 0;
    }
    __syncthreads();
    for (long long q = q_begin + threadIdx.x; q < q_end; q += blockDim.x) {
        const int c = again(q);
#pragma unroll
        for (int i = 0; i < NL; ++i)
            if (c == i + 1) out[i][s_base[i] + atomicAdd(&s_count[i], 1u)] = q;
    }
}
