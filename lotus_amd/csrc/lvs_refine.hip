// Exact re-ranking of a few dozen candidates per query: the kernel of lvs_refine_keys (lvs_capi.hip), the second stage of
// an IVF-SQ8 / IVF-PQ search with "Refine(Flat)".
//
// The first stage hands over kc <= 64 result keys per query, ranked by their code scores.  Only the ROW NUMBER of a key is
// read here: every named row is scored again against the stored rows of the flat packed image (fp16, or the fp32-accurate
// hi|lo pair), and the best k by that score are written, best first.
//   * one wave per query, LVS_REFINE_WAVES waves per workgroup, no LDS and no barrier; a wave past nq returns;
//   * the lanes split a row along d: lane v loads the 16 B at halfs [512 p + 8 v, + 8) of pass p, so one wave-instruction
//     covers 512 contiguous halfs of ONE row (whole 128-B lines), and the row's base is wave-uniform (v_readlane of the
//     candidate's lane -> scalar base + per-lane offset).  A lane past dpad reads at offset 0 of the same row and multiplies
//     by a zeroed query fragment: no branch around a load (hipcc waits vmcnt(0) per element for loads under a condition);
//   * the query's fragments stay in registers for the whole candidate loop up to dpad = 3 072 (NP = 1, 2, 3, 4 or 6 passes
//     of 512 halfs, hi|lo queries: up to 48 VGPRs); wider rows (NP = 0) read them again per group of rows - from L1/L2,
//     the wave just loaded them;
//   * the candidates are taken four at a time, compacted by the ballot of the non-empty slots, and the loads of all four
//     rows of a pass are issued before the first is multiplied: 4 rows in flight per wave (MI355X: random whole rows into
//     registers read at 5.5 - 5.8 TB/s in this shape at 16 waves per CU).  A last group of fewer than four repeats its
//     first row - a valid row, read again from L1;
//   * a slot is EMPTY when its key is 0 or names a row >= nb (the keys come from device memory); an empty slot is never
//     loaded from, may stand anywhere in the list and sorts last (key 0);
//   * inner products accumulate in fp32, hi|lo operands as the project's K segments hi.hi + hi.lo + lo.hi; squared L2 is
//     -max(|q|^2 + |x|^2 - 2 <q, x>, 0) from the two norm arrays, as in the scans;
//   * after lvs_wave_sum lane c holds the key lvs_pack_key(score, row) of candidate slot c (0: empty); one
//     lvs_wave_sort_desc, lanes below k write.  Equal exact scores come out in ascending row order, and every candidate is
//     scored by the same instruction sequence whatever its place in the list, so equal rows score bit-alike.
#include "lvs_common.h"
#include "lvs_tile.h"

namespace {

constexpr int RF_WAVES = LVS_REFINE_WAVES;
constexpr int RF_ROWS = 4;   // candidate rows in flight per wave
constexpr int RF_MAXNP = 6;  // passes of 512 halfs whose query fragments are kept in registers (dpad <= 3 072)

__device__ __forceinline__ float rf_dot8(const half8& x, const half8& y, float acc) {
#pragma unroll
    for (int t = 0; t < 8; ++t) acc = fmaf((float)x[t], (float)y[t], acc);
    return acc;
}

// the query's fragment of pass p: halfs [512 p + 8 lane, + 8) of the hi (and lo) part, zero past dpad
template <int QS>
__device__ __forceinline__ void rf_query_frag(const _Float16* xq, int dpad, int p, int lane, half8& hi, half8& lo) {
    const int col = p * 512 + lane * 8;
    const bool ok = col < dpad;
    const int off = ok ? col : 0;
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const half8 h = *(const half8*)(xq + off);
    hi = ok ? h : zero;
    if (QS) {
        const half8 l = *(const half8*)(xq + dpad + off);
        lo = ok ? l : zero;
    }
}

// 4 waves per SIMD (at most 128 VGPRs) - 16 waves per CU, the measured shape - except hi|lo queries of six passes: their 48
// fragment registers beside four rows of a pass need ~160, so 3 waves per SIMD, each with 8 KB of a pass in flight
template <int QS, int BS, int NP>
__global__ __launch_bounds__(RF_WAVES * 64, (QS && NP == RF_MAXNP) ? 3 : 4) void lvs_refine_kernel(const LvsRefineArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long q = (long long)blockIdx.x * RF_WAVES + wave;
    if (q >= a.nq) return;
    const int dpad = a.dpad;
    const int npass = NP > 0 ? NP : (dpad + 511) / 512;

    // lane c <- candidate slot c: the row number only; the score bits of the key are not read
    const u64 ck = lane < a.kc ? a.cand[q * a.kc + lane] : 0ull;
    const uint32_t row = 0xFFFFFFFFu - (uint32_t)(ck & 0xFFFFFFFFull);
    const bool have = ck != 0 && (long long)row < a.nb;
    unsigned long long m = __ballot(have);

    const _Float16* xq = (const _Float16*)a.xq + q * a.ldq;
    const _Float16* xb = (const _Float16*)a.xb;
    half8 qh[NP > 0 ? NP : 1], ql[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) rf_query_frag<QS>(xq, dpad, p, lane, qh[p], ql[p]);
    }

    float score = 0.f;
    while (m) {
        // the next (up to) four non-empty slots; a short last group repeats its first one
        int src[RF_ROWS];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < RF_ROWS; ++j) {
            if (m) {
                src[j] = __ffsll((long long)m) - 1;
                m &= m - 1;
                ++cnt;
            } else {
                src[j] = src[0];
            }
        }
        const _Float16* rp[RF_ROWS];
#pragma unroll
        for (int j = 0; j < RF_ROWS; ++j) rp[j] = xb + (long long)(uint32_t)__builtin_amdgcn_readlane((int)row, src[j]) * a.ldb;
        float acc[RF_ROWS];
#pragma unroll
        for (int j = 0; j < RF_ROWS; ++j) acc[j] = 0.f;
        auto pass = [&](int p) {
            const int col = p * 512 + lane * 8;
            const int off = col < dpad ? col : 0;
            half8 bh[RF_ROWS], bl[RF_ROWS];
#pragma unroll
            for (int j = 0; j < RF_ROWS; ++j) {
                bh[j] = *(const half8*)(rp[j] + off);
                if (BS) bl[j] = *(const half8*)(rp[j] + dpad + off);
            }
            __builtin_amdgcn_sched_barrier(0);  // all four rows' loads of the pass are issued ahead of the first multiply
            half8 fh, fl;
            if (NP > 0) {
                fh = qh[p];
                fl = ql[p];
            } else {
                rf_query_frag<QS>(xq, dpad, p, lane, fh, fl);
            }
#pragma unroll
            for (int j = 0; j < RF_ROWS; ++j) {
                acc[j] = rf_dot8(fh, bh[j], acc[j]);
                if (BS) acc[j] = rf_dot8(fh, bl[j], acc[j]);
                if (QS) acc[j] = rf_dot8(fl, bh[j], acc[j]);
            }
        };
        if (NP > 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) pass(p);
        } else {
            for (int p = 0; p < npass; ++p) pass(p);
        }
#pragma unroll
        for (int j = 0; j < RF_ROWS; ++j) {
            const float s = lvs_wave_sum(acc[j]);
            if (j < cnt && lane == src[j]) score = s;
        }
    }
    if (a.metric == LVS_METRIC_L2 && have) score = -fmaxf((a.qn[q] + a.bn[row]) - 2.0f * score, 0.f);
    u64 key = have ? lvs_pack_key(score, row) : 0ull;
    key = lvs_wave_sort_desc(key, lane);
    if (lane < a.k) a.out[q * a.k + lane] = key;
}

template <int QS, int BS, int NP>
hipError_t refine_launch_t(const LvsRefineArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL((lvs_refine_kernel<QS, BS, NP>), dim3((unsigned)lvs_ceil_div(a.nq, RF_WAVES)), dim3(RF_WAVES * 64), 0,
                       stream, a);
    return hipGetLastError();
}

template <int QS, int BS>
hipError_t refine_launch_np(const LvsRefineArgs& a, hipStream_t stream) {
    switch (a.dpad <= RF_MAXNP * 512 ? (a.dpad + 511) / 512 : 0) {
        case 1: return refine_launch_t<QS, BS, 1>(a, stream);
        case 2: return refine_launch_t<QS, BS, 2>(a, stream);
        case 3: return refine_launch_t<QS, BS, 3>(a, stream);
        case 4: return refine_launch_t<QS, BS, 4>(a, stream);
        case 5:  // a pass past dpad is masked like a lane past it: five passes run on the six-pass kernel
        case 6: return refine_launch_t<QS, BS, 6>(a, stream);
        default: return refine_launch_t<QS, BS, 0>(a, stream);
    }
}

}  // namespace

hipError_t lvs_refine_launch(const LvsRefineArgs& a, hipStream_t stream) {
    if (a.dpad < 64 || a.dpad % 64 != 0 || a.kc < 1 || a.kc > 64 || a.k < 1 || a.k > a.kc || a.nq < 0 || a.nb < 0 ||
        lvs_ceil_div(a.nq, RF_WAVES) > 0x7FFFFFFFll)
        return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    if (a.qsplit) return a.bsplit ? refine_launch_np<1, 1>(a, stream) : refine_launch_np<1, 0>(a, stream);
    return a.bsplit ? refine_launch_np<0, 1>(a, stream) : refine_launch_np<0, 0>(a, stream);
}
