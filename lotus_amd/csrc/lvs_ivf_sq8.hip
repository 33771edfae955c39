// IVF-SQ8: the 8-bit residual codec of an IVF index (faiss "IVF<nlist>,SQ8": ScalarQuantizer QT_8bit, by_residual) and
// its list scan, the hot kernel of lvs_ivf_sq8_search_keys (lvs_capi.hip).
//
// Codec (per dimension j, trained by the caller over the residuals of the k-means training rows):
//   r = x - c_l                      x: the row's stored value (hi + lo), c_l: its list's centroid (fp32)
//   code_j = floor(255 * clamp((r_j - vmin_j) / vdiff_j, 0, 1))            (vdiff_j == 0: code 0)
//   rhat_j = a_j + b_j * code_j,  b_j = vdiff_j / 255,  a_j = vmin_j + 0.5 b_j   (= vmin + (code + 0.5) vdiff / 255)
// The codes are written in LIST order (position p of the rows array, [n][ldc] bytes, ldc = d rounded up to 64), so a list
// is one contiguous block; |rhat|^2 is stored per position (fp32).
//
// Scan: the score of the decoded row c_l + rhat against a query q is a per-pair constant plus a dot product of a per-pair
// fp32 vector w with the integer codes:
//   inner product:  <q, c_l> + sum q_j a_j            + sum (q_j b_j) code_j
//   squared L2:     |u|^2 - 2 [sum u_j a_j + sum (u_j b_j) code_j] + |rhat|^2,   u = q - c_l
// A work item is one list and a tile of up to 16 (query, probe rank) pairs that probe it (the 32-pair work items of
// lvs_ivf_tiles_launch, halved: block 2 w + h takes pairs [16 h, 16 h + 16) of work item w).
//   * staging: every pair's w is formed in fp32 from the packed query and the fp32 centroid, scaled by a power of two
//     (per pair: max |w| lands in [2^13, 2^14), so w's lo half never drops into fp16's subnormal range), and split into
//     hi|lo fp16 B fragments of v_mfma_f32_16x16x32_f16 in LDS; the constant terms are fp32 sums (for L2, |q - c|^2 directly);
//   * rows: lane (m, g) of a wave loads 16 code bytes of row m of a 16-row block, bytes [64 kb + 16 g, + 16): bytes 0-7 are
//     its A operand of K step 2 kb, bytes 8-15 of K step 2 kb + 1 - so K index 8 g + t of step 2 kb + s is dimension
//     64 kb + 16 g + 8 s + t, and the B fragments are staged with the same permutation.  A code byte becomes an exact fp16
//     by v_perm_b32 (0x64XX = 1024 + code) and v_pk_add_f16 (-1024);
//   * acc = codes x w_hi + codes x w_lo (fp32 accumulation of exact products: fp32-accurate);
//   * hits go through the wave-cooperative sorted insertion (lvs_list_insert, lvs_common.h) into per-pair lists in LDS, keys carry
//     the GLOBAL row number, parts [nprobe][nq][k] are merged by lvs_merge_keys.
// LDS: 2 x (ldc / 32) fragments of 1 KB + 16 lists of kcap keys: ldc <= 2368 (d = 1536: 96 KB + 8 KB); wider rows are not
// served (lvs_ivf_sq8_fits).
#include "lvs_common.h"
#include "lvs_tile.h"

namespace {

constexpr int SQ8_TQ = LVS_SQ8_TILEQ;
constexpr int SQ8_THREADS = LVS_SQ8_WAVES * 64;

// 8 consecutive floats p[j .. j + 8) of a row of length d (zeros past d); vector loads when the row allows them
__device__ inline void sq8_load8(const float* __restrict__ p, int j, int d, bool vec, float (&v)[8]) {
    if (vec && j + 8 <= d) {
        const float4 x0 = *(const float4*)(p + j), x1 = *(const float4*)(p + j + 4);
        v[0] = x0.x, v[1] = x0.y, v[2] = x0.z, v[3] = x0.w, v[4] = x1.x, v[5] = x1.y, v[6] = x1.z, v[7] = x1.w;
        return;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = j + t < d ? p[j + t] : 0.f;
}

// the fp32 query values [j, j + 8) from the packed query row (hi, plus lo at +qdpad for hi|lo queries)
__device__ inline void sq8_query8(const _Float16* __restrict__ q, int j, int split, int qdpad, float (&v)[8]) {
    const half8 hi = *(const half8*)(q + j);
    if (split) {
        const half8 lo = *(const half8*)(q + qdpad + j);
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = (float)hi[t] + (float)lo[t];
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = (float)hi[t];
    }
}

// w_j (unscaled) of dimensions [j, j + 8) for query values qv, centroid cv and vdiff dv; per element also the two sums of
// the pair's constant: inner product s1 += q c, s2 += q a; squared L2 s1 += u u, s2 += u a
__device__ inline void sq8_w8(const float (&qv)[8], const float (&cv)[8], const float (&mv)[8], const float (&dv)[8],
                              bool l2, float (&w)[8], float& s1, float& s2, float& mx) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float b = dv[t] / 255.0f;
        const float a = mv[t] + 0.5f * b;
        const float u = l2 ? qv[t] - cv[t] : qv[t];
        w[t] = u * b;
        s1 += l2 ? u * u : qv[t] * cv[t];
        s2 += u * a;
        mx = fmaxf(mx, fabsf(w[t]));
    }
}

typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// 4 code bytes -> 4 exact fp16 values (two dwords): v_perm_b32 builds the halves 0x64XX (= 1024 + XX), v_pk_add_f16 -1024
__device__ inline void sq8_bytes_to_f16(uint32_t c4, uint32_t& h01, uint32_t& h23) {
    const uint32_t p01 = __builtin_amdgcn_perm(0x64646464u, c4, 0x04010400u);
    const uint32_t p23 = __builtin_amdgcn_perm(0x64646464u, c4, 0x04030402u);
    const half2v m = {(_Float16)-1024.0f, (_Float16)-1024.0f};
    const half2v r01 = __builtin_bit_cast(half2v, p01) + m;
    const half2v r23 = __builtin_bit_cast(half2v, p23) + m;
    h01 = __builtin_bit_cast(uint32_t, r01);
    h23 = __builtin_bit_cast(uint32_t, r23);
}

// 16 code bytes -> the A operands of two K steps (bytes 0-7, bytes 8-15)
__device__ inline void sq8_codes_to_frags(const uint4 c, half8& s0, half8& s1) {
    uint32_t h[8];
    sq8_bytes_to_f16(c.x, h[0], h[1]);
    sq8_bytes_to_f16(c.y, h[2], h[3]);
    sq8_bytes_to_f16(c.z, h[4], h[5]);
    sq8_bytes_to_f16(c.w, h[6], h[7]);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 a = {h[0], h[1], h[2], h[3]}, b = {h[4], h[5], h[6], h[7]};
    s0 = __builtin_bit_cast(half8, a);
    s1 = __builtin_bit_cast(half8, b);
}

// SEL: only the rows whose bit is set in a.sel take part, as in lvs_ivf_scan_kernel: a wave looks its 16 rows' bits up right
// after their numbers, skips the block before any code load when none is selected, and the 16-bit ballot of (inside the
// list and selected), indexed by the block row, masks the epilogue in place of the `< len` test.
template <int U, bool SEL>
__global__ __launch_bounds__(SQ8_THREADS) void lvs_ivf_sq8_scan_kernel(const LvsIvfSq8Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KCAP = a.kcap;
    const int nks = a.ldc / 32;                                             // K steps of 32 dimensions
    half8* bfrag = (half8*)smem;                                            // [2][nks][64]: w hi, then w lo
    u64* lists = (u64*)(smem + (size_t)nks * 2 * 1024);                     // [TQ][KCAP]
    uint32_t* locks = (uint32_t*)((char*)lists + (size_t)SQ8_TQ * KCAP * 8);  // [TQ]
    int* slot_q = (int*)(locks + SQ8_TQ);                                   // [TQ] query of every pair slot
    int* slot_p = slot_q + SQ8_TQ;                                          // [TQ] its probe rank
    float* cst = (float*)(slot_p + SQ8_TQ);                                 // [TQ] the pair's constant term
    int* sexp = (int*)(cst + SQ8_TQ);                                       // [TQ] the pair's power-of-two scale of w

    // ---- block -> (list, half of a 32-pair work item)
    const uint32_t wi = blockIdx.x >> 1;
    if (wi >= a.tile_offs[a.nlist]) return;  // the grid is an upper bound of the work items
    const int l = (int)a.item_list[wi];
    const uint32_t p0 = a.pair_offs[l] + (wi - a.tile_offs[l]) * (2 * SQ8_TQ) + (blockIdx.x & 1) * SQ8_TQ;
    const uint32_t pend = a.pair_offs[l + 1];
    if (p0 >= pend) return;
    const int npair = (int)(pend - p0 < (uint32_t)SQ8_TQ ? pend - p0 : (uint32_t)SQ8_TQ);  // >= 1
    lvs_ivf_tile_begin<SQ8_TQ, SQ8_THREADS>(a.pairs, p0, npair, a.nprobe, tid, lists, KCAP, locks, slot_q, slot_p);

    const bool l2 = a.metric == LVS_METRIC_L2;
    const int d = a.d, ldc = a.ldc;
    const bool vec = (d & 3) == 0;
    const float* cl = a.cent + (long long)l * d;
    const _Float16* xq = (const _Float16*)a.xq;
    const int ng8 = ldc / 8;  // groups of 8 dimensions
    // ---- pass 1: per pair, the constant term and max |w| (wave w takes pairs w, w + 4, ...; fixed reduction order)
    for (int n = wave; n < SQ8_TQ; n += LVS_SQ8_WAVES) {
        const _Float16* qrow = xq + (long long)slot_q[n] * a.ldq;
        float s1 = 0.f, s2 = 0.f, mx = 0.f;
        for (int g8 = lane; g8 < ng8; g8 += 64) {
            const int j = g8 * 8;
            float qv[8], cv[8], mv[8], dv[8], w[8];
            sq8_query8(qrow, j, a.qsplit, a.qdpad, qv);
            sq8_load8(cl, j, d, vec, cv);
            sq8_load8(a.vmin, j, d, vec, mv);
            sq8_load8(a.vdiff, j, d, vec, dv);
            sq8_w8(qv, cv, mv, dv, l2, w, s1, s2, mx);
        }
        s1 = lvs_wave_sum(s1);
        s2 = lvs_wave_sum(s2);
        mx = lvs_wave_max(mx);
        if (lane == 0) {
            cst[n] = l2 ? s1 - 2.0f * s2 : s1 + s2;
            int e = 0;
            if (mx > 0.f) {
                (void)frexpf(mx, &e);  // mx = m 2^e, m in [0.5, 1)
                e = 14 - e;
                e = e < -120 ? -120 : (e > 120 ? 120 : e);
            }
            sexp[n] = e;
        }
    }
    __syncthreads();
    // ---- pass 2: w x 2^e as hi|lo B fragments.  Group g8 = dims [8 g8, + 8): 64-dim block kb = g8 / 8, g = (g8 % 8) / 2,
    // s = g8 % 2 -> K step 2 kb + s, lane 16 g + pair
    for (int idx = tid; idx < SQ8_TQ * ng8; idx += SQ8_THREADS) {
        const int n = idx & (SQ8_TQ - 1), g8 = idx / SQ8_TQ;
        const int j = g8 * 8;
        float qv[8], cv[8], mv[8], dv[8], w[8];
        float s1 = 0.f, s2 = 0.f, mx = 0.f;
        sq8_query8(xq + (long long)slot_q[n] * a.ldq, j, a.qsplit, a.qdpad, qv);
        sq8_load8(cl, j, d, vec, cv);
        sq8_load8(a.vmin, j, d, vec, mv);
        sq8_load8(a.vdiff, j, d, vec, dv);
        sq8_w8(qv, cv, mv, dv, l2, w, s1, s2, mx);
        const int e = sexp[n];
        half8 hi, lo;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float ws = ldexpf(w[t], e);
            hi[t] = (_Float16)ws;
            lo[t] = (_Float16)(ws - (float)hi[t]);
        }
        const int kb = g8 >> 3, g = (g8 & 7) >> 1, s = g8 & 1;
        const int f = 2 * kb + s, ln = 16 * g + n;
        bfrag[f * 64 + ln] = hi;
        bfrag[(nks + f) * 64 + ln] = lo;
    }
    __syncthreads();

    const int qs = lane & 15;  // this lane's pair slot in the accumulators
    const bool qvalid = qs < npair;
    const float cq = cst[qs];
    const int eq = sexp[qs];
    float tauf = -INFINITY;
    const int k = a.k;
    const long long pos0 = a.offsets[l];
    const int len = (int)(a.offsets[l + 1] - pos0);
    const int nblk = (len + 15) / 16;
    const int nkb = ldc / 64;
    const half8* bhi = bfrag + lane;
    const half8* blo = bfrag + (long long)nks * 64 + lane;

    for (int blk = wave; blk < nblk; blk += LVS_SQ8_WAVES) {
        // the row this lane loads: row (lane & 15) of the block; past the list's end the last row is repeated (masked below)
        int rr = blk * 16 + (lane & 15);
        if (rr > len - 1) rr = len - 1;
        const long long pos = pos0 + rr;
        const uint32_t rid = a.rows[pos];
        uint32_t selm = 0;  // SEL: bit j = block row j is inside the list and selected (lanes j, j + 16, ... hold the same row)
        if constexpr (SEL) {
            const bool on = blk * 16 + (lane & 15) < len && ((a.sel[rid >> 5] >> (rid & 31)) & 1u);
            selm = (uint32_t)__ballot(on) & 0xFFFFu;
            if (selm == 0) continue;  // wave-uniform; the block loop has no workgroup barrier
        }
        const float rn = l2 ? a.rnorm[pos] : 0.f;
        const uint8_t* cp = a.codes + pos * ldc + (lane >> 4) * 16;
        uint4 cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = *(const uint4*)(cp + u * 64);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb0 = 0; kb0 < nkb; kb0 += U) {
            if (kb0 + U < nkb) {
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = *(const uint4*)(cp + (kb0 + U + u) * 64);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                half8 s0, s1;
                sq8_codes_to_frags(cur[u], s0, s1);
                const int f = 2 * (kb0 + u);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(s0, bhi[f * 64], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(s0, blo[f * 64], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(s1, bhi[(f + 1) * 64], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(s1, blo[(f + 1) * 64], acc, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
        // ---- block epilogue: lane holds pair slot qs, block rows 4 (lane >> 4) + r
        const int brow0 = blk * 16 + 4 * (lane >> 4);
        const uint32_t selw = selm >> (4 * (lane >> 4));  // SEL: bit r = this lane's block row 4 (lane >> 4) + r takes part
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dot = ldexpf(acc[r], -eq);
            if (l2) {
                const float rv = __shfl(rn, 4 * (lane >> 4) + r, 64);
                acc[r] = -fmaxf((cq - 2.0f * dot) + rv, 0.f);
            } else {
                acc[r] = cq + dot;
            }
        }
        {
            const uint32_t lo = (uint32_t)(lists[qs * KCAP + k - 1] >> 32);
            tauf = fmaxf(tauf, lvs_tau(lo));
        }
        float best = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool in = SEL ? (selw >> r) & 1u : brow0 + r < len;
            best = in ? fmaxf(best, acc[r]) : best;
        }
        const bool th = qvalid && best >= tauf;
        if (!__any(th)) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t id = (uint32_t)__shfl((int)rid, 4 * (lane >> 4) + r, 64);
            const bool in = SEL ? (selw >> r) & 1u : brow0 + r < len;
            const bool pending = th && in && acc[r] >= tauf;
            const u64 key = pending ? lvs_pack_key(acc[r], id) : 0ull;
            lvs_list_insert(__ballot(pending), key, qs, lists, KCAP, locks, k, lane, tauf);
        }
    }
    lvs_ivf_write_parts<SQ8_THREADS>(lists, KCAP, slot_q, slot_p, npair, k, a.nq, tid, a.out);
}

// one wave per list position: residual against the list's centroid, codes, |rhat|^2
__global__ __launch_bounds__(256) void lvs_ivf_sq8_encode_kernel(const _Float16* __restrict__ xb, long long ldb, int split,
                                                                 int xdpad, long long n, int d, int ldc,
                                                                 const int64_t* __restrict__ offsets, int nlist,
                                                                 const uint32_t* __restrict__ rows,
                                                                 const float* __restrict__ cent, const float* __restrict__ vmin,
                                                                 const float* __restrict__ vdiff, uint8_t* __restrict__ codes,
                                                                 float* __restrict__ rnorm) {
    const int lane = threadIdx.x & 63;
    const long long pos = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= n) return;
    int lo = 0, hi = nlist;  // the list holding pos: the last l with offsets[l] <= pos (empty lists are skipped)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= pos) lo = mid;
        else hi = mid;
    }
    const _Float16* x = xb + (long long)rows[pos] * ldb;
    const float* c = cent + (long long)lo * d;
    uint8_t* out = codes + pos * ldc;
    float nn = 0.f;
    for (int j = lane; j < ldc; j += 64) {
        uint32_t code = 0;
        if (j < d) {
            const float xv = split ? (float)x[j] + (float)x[xdpad + j] : (float)x[j];
            const float r = xv - c[j];
            const float dv = vdiff[j];
            if (dv > 0.f) {
                const float t = fminf(fmaxf((r - vmin[j]) / dv, 0.f), 1.f);
                code = (uint32_t)floorf(255.0f * t);
            }
            const float b = dv / 255.0f;
            const float rh = (vmin[j] + 0.5f * b) + b * (float)code;
            nn += rh * rh;
        }
        out[j] = (uint8_t)code;
    }
    nn = lvs_wave_sum(nn);
    if (lane == 0) rnorm[pos] = nn;
}

template <int U>
hipError_t sq8_scan_launch_u(const LvsIvfSq8Args& a, int64_t max_items, hipStream_t stream) {
    const dim3 grid((unsigned)(2 * max_items)), block(SQ8_THREADS);
    const size_t lds = lvs_ivf_sq8_lds_bytes(a.ldc, a.kcap);
    if (a.sel) return lvs_launch_lds<lvs_ivf_sq8_scan_kernel<U, true>>(grid, block, lds, stream, a);
    return lvs_launch_lds<lvs_ivf_sq8_scan_kernel<U, false>>(grid, block, lds, stream, a);
}

}  // namespace

hipError_t lvs_ivf_sq8_encode_launch(const void* xb, int64_t ldb, int split, int xdpad, int64_t n, int d,
                                     const int64_t* offsets, int nlist, const uint32_t* rows, const float* cent,
                                     const float* vmin, const float* vdiff, uint8_t* codes, float* rnorm, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lvs_ivf_sq8_encode_kernel, dim3((unsigned)lvs_ceil_div(n, 4)), dim3(256), 0, stream,
                       (const _Float16*)xb, (long long)ldb, split, xdpad, (long long)n, d, lvs_ivf_sq8_ldc(d), offsets, nlist,
                       rows, cent, vmin, vdiff, codes, rnorm);
    return hipGetLastError();
}

// batches of U 64-dimension blocks: 4 where they divide ldc / 64, else 2, else 1
hipError_t lvs_ivf_sq8_scan_launch(const LvsIvfSq8Args& a, int64_t max_items, hipStream_t stream) {
    if (a.ldc % 64 != 0 || a.ldc < a.d || a.ldc > a.qdpad || a.k < 1 || a.k > a.kcap || a.kcap > 64 ||
        lvs_ivf_sq8_lds_bytes(a.ldc, a.kcap) > LVS_LDS_MAX)
        return hipErrorInvalidValue;
    if (max_items <= 0) return hipSuccess;
    const int nkb = a.ldc / 64;
    if (nkb % 4 == 0) return sq8_scan_launch_u<4>(a, max_items, stream);
    if (nkb % 2 == 0) return sq8_scan_launch_u<2>(a, max_items, stream);
    return sq8_scan_launch_u<1>(a, max_items, stream);
}
