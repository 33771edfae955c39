// IVF-PQ: the product-quantizer codec of an IVF index (faiss "IVF<nlist>,PQ<M>": ProductQuantizer, 8-bit codes,
// by_residual) and its list scan, the hot kernels of lvs_ivf_pq_search_keys (lvs_capi.hip).
//
// Codec (codebooks cb [M][ksub][dsub], dsub = d / M, ksub <= 256, trained by the caller on the residuals of the k-means
// training rows):
//   r = x - c_l                       x: the row's stored value (hi + lo), c_l: its list's centroid (fp32)
//   code_m = argmin_{j < ksub} |r_m - cb[m][j]|^2   (fp32, ties to the smaller j; entries j >= ksub are never chosen)
//   rhat = concat_m cb[m][code_m],    beta = |rhat|^2 + 2 <c_l, rhat>   (fp32, per list position)
// The codes are written in LIST order (position p of the rows array, [n][ldc] bytes, ldc = M rounded up to 16), so a list
// is one contiguous block.
//
// Search, per query q (everything in the rows' stored scale):
//   LUT_q[m][j] = <q_m, cb[m][j]>                    (lvs_ivf_pq_lut_kernel: once per query, not once per probed list)
//   inner product:  <q, c_l> + sum_m LUT_q[m][code_m]
//   squared L2:     |q - c_l|^2 + beta - 2 sum_m LUT_q[m][code_m]
// lvs_ivf_pq_scan_kernel is query-major: a workgroup takes one query and a range of its probed lists, stages the query's
// fp32 table (M KB) in LDS, and every lane scores one row of the concatenated lists from its M code bytes (16-byte loads,
// then M ds_read_b32 lookups summed in the order m = 0 .. M-1).  Hits go through the wave-cooperative sorted insertion
// (the text of lvs_list_insert, lvs_common.h) into the workgroup's one list in LDS; keys carry the GLOBAL row number; parts [nranges][nq][k] are
// merged by lvs_merge_keys.  LDS: M KB of table + the list: M <= 159 (lvs_ivf_pq_lds_bytes), whatever d.
#include "lvs_common.h"
#include "lvs_tile.h"

namespace {

constexpr int PQ_THREADS = LVS_PQ_WAVES * 64;
constexpr int PQ_KS = LVS_PQ_KSUB;
constexpr int LUT_QB = 16;  // queries per workgroup of the table kernel
constexpr int LUT_T = 64;   // dimensions of a query tile staged in LDS

// the fp32 value of dimension j of a packed query / row (hi, plus lo at +dpad for hi|lo)
__device__ inline float pq_val(const _Float16* __restrict__ p, int j, int split, int dpad) {
    return split ? (float)p[j] + (float)p[dpad + j] : (float)p[j];
}

// ---- lookup tables: workgroup (m, 16 queries), thread j = codebook entry j.  lut [nq][M][256] fp32, entries >= ksub are 0.
__global__ __launch_bounds__(256) void lvs_ivf_pq_lut_kernel(const _Float16* __restrict__ xq, long long ldq, int split,
                                                             int qdpad, int nq, int d, int M, int ksub,
                                                             const float* __restrict__ cb, float* __restrict__ lut) {
    __shared__ __attribute__((aligned(16))) float qs[LUT_T][LUT_QB];
    const int m = blockIdx.x, q0 = blockIdx.y * LUT_QB, j = threadIdx.x;
    const int dsub = d / M;
    float acc[LUT_QB];
#pragma unroll
    for (int i = 0; i < LUT_QB; ++i) acc[i] = 0.f;
    const float* cj = cb + ((long long)m * ksub + (j < ksub ? j : 0)) * dsub;
    for (int t0 = 0; t0 < dsub; t0 += LUT_T) {
        const int tn = dsub - t0 < LUT_T ? dsub - t0 : LUT_T;
        for (int i = threadIdx.x; i < LUT_T * LUT_QB; i += 256) {
            const int t = i / LUT_QB, qq = i % LUT_QB;
            float v = 0.f;
            if (t < tn && q0 + qq < nq) v = pq_val(xq + (long long)(q0 + qq) * ldq, m * dsub + t0 + t, split, qdpad);
            qs[t][qq] = v;
        }
        __syncthreads();
        if (j < ksub) {
            for (int t = 0; t < tn; ++t) {
                const float c = cj[t0 + t];
                const float4* qv = (const float4*)qs[t];
#pragma unroll
                for (int i = 0; i < LUT_QB / 4; ++i) {
                    const float4 v = qv[i];
                    acc[4 * i] = fmaf(v.x, c, acc[4 * i]);
                    acc[4 * i + 1] = fmaf(v.y, c, acc[4 * i + 1]);
                    acc[4 * i + 2] = fmaf(v.z, c, acc[4 * i + 2]);
                    acc[4 * i + 3] = fmaf(v.w, c, acc[4 * i + 3]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < LUT_QB; ++i)
        if (q0 + i < nq) lut[((long long)(q0 + i) * M + m) * PQ_KS + j] = j < ksub ? acc[i] : 0.f;
}

// ---- the list scan: workgroup (probe range, query).  SEL: only the rows whose bit is set in a.sel take part: a lane reads
// its position's row number ahead of the table lookups, folds the bit into `valid`, and a wave skips its 64 positions when
// none is valid
template <bool SEL>
__global__ __launch_bounds__(PQ_THREADS) void lvs_ivf_pq_scan_kernel(const LvsIvfPqArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, KCAP = a.kcap, k = a.k;
    float* lut = (float*)smem;                                          // [M][256]
    u64* list = (u64*)(smem + (size_t)M * PQ_KS * 4);                   // [KCAP]
    uint32_t* lock = (uint32_t*)(list + KCAP);                          // [1]
    float* cst = (float*)(lock + 4);                                    // [LVS_PQ_MAXRANGE] per probe: <q, c_l> or |q - c_l|^2
    int* plist = (int*)(cst + LVS_PQ_MAXRANGE);                         // [LVS_PQ_MAXRANGE] list of every probe (-1: none)
    int* poff = plist + LVS_PQ_MAXRANGE;                                // [LVS_PQ_MAXRANGE + 1] row prefix sums

    const int r = blockIdx.x, q = blockIdx.y;
    const int pb = r * a.prange;
    const int np = a.nprobe - pb < a.prange ? a.nprobe - pb : a.prange;  // >= 1
    const float4* src = (const float4*)(a.lut + (long long)q * M * PQ_KS);
    for (int i = tid; i < M * (PQ_KS / 4); i += PQ_THREADS) ((float4*)lut)[i] = src[i];
    for (int i = tid; i < KCAP; i += PQ_THREADS) list[i] = 0;
    if (tid == 0) {
        lock[0] = 0;
        int run = 0;
        for (int p = 0; p < np; ++p) {
            const u64 key = a.coarse[(long long)q * a.nprobe + pb + p];
            const int l = key == 0 ? -1 : (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
            const bool ok = l >= 0 && l < a.nlist;
            plist[p] = ok ? l : -1;
            poff[p] = run;
            run += ok ? (int)(a.offsets[l + 1] - a.offsets[l]) : 0;
        }
        poff[np] = run;
    }
    __syncthreads();
    const bool l2 = a.metric == LVS_METRIC_L2;
    const int d = a.d;
    const _Float16* qrow = (const _Float16*)a.xq + (long long)q * a.ldq;
    // per probe the constant term, one wave per probe (fixed reduction order)
    for (int p = wave; p < np; p += LVS_PQ_WAVES) {
        const int l = plist[p];
        if (l < 0) continue;
        const float* cl = a.cent + (long long)l * d;
        float s = 0.f;
        for (int j = lane; j < d; j += 64) {
            const float qv = pq_val(qrow, j, a.qsplit, a.qdpad), cv = cl[j];
            s += l2 ? (qv - cv) * (qv - cv) : qv * cv;
        }
        s = lvs_wave_sum(s);
        if (lane == 0) cst[p] = s;
    }
    __syncthreads();

    const int total = poff[np];
    const int ldc = a.ldc, nfull = M / 16, tail = M - 16 * nfull;
    float tauf = -INFINITY;
    for (int base = wave * 64; base < total; base += PQ_THREADS) {
        const int v = base + lane;
        bool valid = v < total;
        const int vv = valid ? v : total - 1;
        int p = 0;
        while (p + 1 < np && poff[p + 1] <= vv) ++p;  // the probe holding virtual row vv (empty probes are skipped)
        const long long pos = a.offsets[plist[p]] + (vv - poff[p]);
        const uint8_t* cp = a.codes + pos * ldc;
        uint32_t rid = 0;
        if constexpr (SEL) {
            rid = a.rows[pos];
            valid = valid && ((a.sel[rid >> 5] >> (rid & 31)) & 1u);
            if (!__any(valid)) continue;  // wave-uniform; the position loop has no workgroup barrier
        }
        // sum_m LUT[m][code_m], m = 0 .. M-1 in order; the next 16 code bytes are in flight while the current ones are looked up
        float s = 0.f;
        uint4 cur = *(const uint4*)cp, nxt = cur;
        for (int c = 0; c < nfull; ++c) {
            if (c + 1 < (tail ? nfull + 1 : nfull)) nxt = *(const uint4*)(cp + 16 * (c + 1));
            const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
            const float* lc = lut + (16 * c) * PQ_KS;
#pragma unroll
            for (int b = 0; b < 16; ++b) s += lc[b * PQ_KS + ((w[b >> 2] >> (8 * (b & 3))) & 0xFF)];
            cur = nxt;
        }
        if (tail) {
            const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
            const float* lc = lut + (16 * nfull) * PQ_KS;
            for (int b = 0; b < tail; ++b) s += lc[b * PQ_KS + ((w[b >> 2] >> (8 * (b & 3))) & 0xFF)];
        }
        const float score = l2 ? -fmaxf((cst[p] + a.beta[pos]) - 2.0f * s, 0.f) : cst[p] + s;
        if constexpr (!SEL) rid = a.rows[pos];
        {
            const uint32_t lo = (uint32_t)(list[k - 1] >> 32);
            tauf = fmaxf(tauf, lvs_tau(lo));
        }
        bool pending = valid && score >= tauf;
        const u64 key = pending ? lvs_pack_key(score, rid) : 0ull;
        unsigned long long pm = __ballot(pending);
        if (__popcll(pm) > k) {
            // more candidates than slots (a fresh list): only the lanes at or above the k-th best score of this batch can
            // enter, so the batch's own k-th best is found first (bitwise search over the ordered scores) and the rest dropped
            const uint32_t ord = (uint32_t)(key >> 32);  // 0 for lanes that are not pending
            uint32_t kth = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = kth | (1u << bit);
                if (__popcll(__ballot(pending && ord >= cand)) >= k) kth = cand;
            }
            pending = pending && ord >= kth;
            pm = __ballot(pending);
        }
        // the text of lvs_list_insert (lvs_common.h) for one list and one lock: calling it here changes this kernel's instructions
        while (pm) {
            const int srcl = __ffsll((long long)pm) - 1;
            pm &= pm - 1;
            const uint32_t klo = __builtin_amdgcn_readlane((uint32_t)key, srcl);
            const uint32_t khi = __builtin_amdgcn_readlane((uint32_t)(key >> 32), srcl);
            const u64 ukey = ((u64)khi << 32) | klo;
            u64 mine = 0, prev = ~0ull;
            for (;;) {
                uint32_t seen = 0;
                if (lane == 0)
                    __hip_atomic_compare_exchange_strong(&lock[0], &seen, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_WORKGROUP);
                asm volatile("" ::: "memory");
                if (lane < k) {
                    mine = list[lane];
                    if (lane > 0) prev = list[lane - 1];
                }
                if (__builtin_amdgcn_readfirstlane(seen) == 0) break;
            }
            u64 newv = 0;
            if (lane < k) newv = mine > ukey ? mine : (prev > ukey ? ukey : prev);
            __builtin_amdgcn_wave_barrier();
            if (lane < k) list[lane] = newv;
            const uint32_t ntau = __builtin_amdgcn_readlane((uint32_t)(newv >> 32), k - 1);
            asm volatile("" ::: "memory");  // slot writes stay ahead of the unlock (LDS is in-order per wave)
            if (lane == 0) __hip_atomic_store(&lock[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            tauf = fmaxf(tauf, lvs_tau(ntau));
        }
    }
    __syncthreads();
    for (int i = tid; i < k; i += PQ_THREADS) a.out[((long long)r * a.nq + q) * k + i] = list[i];
}

// one wave per list position: residual against the list's centroid, per subspace the nearest codebook entry, beta.
// LDS: a 256-dimension tile of the wave's residual (broadcast reads)
__global__ __launch_bounds__(256) void lvs_ivf_pq_encode_kernel(const _Float16* __restrict__ xb, long long ldb, int split,
                                                                int xdpad, long long n, int d, int M, int ksub, int ldc,
                                                                const int64_t* __restrict__ offsets, int nlist,
                                                                const uint32_t* __restrict__ rows,
                                                                const float* __restrict__ cent, const float* __restrict__ cb,
                                                                uint8_t* __restrict__ codes, float* __restrict__ beta) {
    __shared__ float rt[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long pos = (long long)blockIdx.x * 4 + wave;
    if (pos >= n) return;  // wave-uniform: the kernel has no workgroup barrier
    int lo = 0, hi = nlist;  // the list holding pos: the last l with offsets[l] <= pos (empty lists are skipped)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= pos) lo = mid;
        else hi = mid;
    }
    const _Float16* x = xb + (long long)rows[pos] * ldb;
    const float* c = cent + (long long)lo * d;
    uint8_t* out = codes + pos * ldc;
    float* r = rt[wave];
    const int dsub = d / M;
    float bsum = 0.f;
    for (int m = 0; m < M; ++m) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < dsub; t0 += 256) {
            const int tn = dsub - t0 < 256 ? dsub - t0 : 256;
            __builtin_amdgcn_wave_barrier();
            for (int t = lane; t < tn; t += 64) {
                const int j = m * dsub + t0 + t;
                r[t] = pq_val(x, j, split, xdpad) - c[j];
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = lane + 64 * u;
                if (j < ksub) {
                    const float* e = cb + ((long long)m * ksub + j) * dsub + t0;
                    float s = acc[u];
                    for (int t = 0; t < tn; ++t) {
                        const float df = r[t] - e[t];
                        s = fmaf(df, df, s);
                    }
                    acc[u] = s;
                }
            }
        }
        // argmin over j = lane + 64 u: ascending j within the lane, then across lanes with ties to the smaller j
        float bd = INFINITY;
        int bj = 0x7FFFFFFF;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = lane + 64 * u;
            if (j < ksub && (acc[u] < bd || bj == 0x7FFFFFFF)) bd = acc[u], bj = j;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float od = __shfl_xor(bd, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
        }
        const int code = __builtin_amdgcn_readfirstlane(bj);
        if (lane == 0) out[m] = (uint8_t)code;
        const float* e = cb + ((long long)m * ksub + code) * dsub;
        for (int t = lane; t < dsub; t += 64) {
            const float rh = e[t];
            bsum += rh * rh + 2.0f * c[m * dsub + t] * rh;
        }
    }
    for (int m = M + lane; m < ldc; m += 64) out[m] = 0;
    bsum = lvs_wave_sum(bsum);
    if (lane == 0) beta[pos] = bsum;
}

}  // namespace

hipError_t lvs_ivf_pq_encode_launch(const void* xb, int64_t ldb, int split, int xdpad, int64_t n, int d, int M, int ksub,
                                    const int64_t* offsets, int nlist, const uint32_t* rows, const float* cent,
                                    const float* codebooks, uint8_t* codes, float* beta, hipStream_t stream) {
    if (M < 1 || d % M != 0 || ksub < 1 || ksub > PQ_KS) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lvs_ivf_pq_encode_kernel, dim3((unsigned)lvs_ceil_div(n, 4)), dim3(256), 0, stream, (const _Float16*)xb,
                       (long long)ldb, split, xdpad, (long long)n, d, M, ksub, lvs_ivf_pq_ldc(M), offsets, nlist, rows, cent,
                       codebooks, codes, beta);
    return hipGetLastError();
}

hipError_t lvs_ivf_pq_lut_launch(const void* xq, int64_t ldq, int split, int qdpad, int64_t nq, int d, int M, int ksub,
                                 const float* codebooks, float* lut, hipStream_t stream) {
    if (M < 1 || d % M != 0 || ksub < 1 || ksub > PQ_KS || nq > 0x7FFFFFFF) return hipErrorInvalidValue;
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(lvs_ivf_pq_lut_kernel, dim3((unsigned)M, (unsigned)lvs_ceil_div(nq, LUT_QB)), dim3(256), 0, stream,
                       (const _Float16*)xq, (long long)ldq, split, qdpad, (int)nq, d, M, ksub, codebooks, lut);
    return hipGetLastError();
}

hipError_t lvs_ivf_pq_scan_launch(const LvsIvfPqArgs& a, hipStream_t stream) {
    if (a.M < 1 || a.ldc != lvs_ivf_pq_ldc(a.M) || a.k < 1 || a.k > a.kcap || a.kcap > 64 || a.prange < 1 ||
        a.prange > LVS_PQ_MAXRANGE || a.nprobe < 1 || a.nq > 65535 || lvs_ivf_pq_lds_bytes(a.M, a.kcap) > LVS_LDS_MAX)
        return hipErrorInvalidValue;
    if (a.nq <= 0) return hipSuccess;
    const int nranges = (a.nprobe + a.prange - 1) / a.prange;
    const dim3 grid((unsigned)nranges, (unsigned)a.nq), block(PQ_THREADS);
    const size_t lds = lvs_ivf_pq_lds_bytes(a.M, a.kcap);
    if (a.sel) return lvs_launch_lds<lvs_ivf_pq_scan_kernel<true>>(grid, block, lds, stream, a);
    return lvs_launch_lds<lvs_ivf_pq_scan_kernel<false>>(grid, block, lds, stream, a);
}
