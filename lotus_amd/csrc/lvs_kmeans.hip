// k-means pieces behind lotus.utils.cluster (lotus/utils.py:61-65 -> faiss Kmeans.train + index.search(x, 1)).
//
// Assignment is the tile kernel in top-1 / squared-L2 mode (lvs_flat_search_keys with k = 1, or the certified one-pass
// lvs_nearest_hi).  This file holds everything else of an iteration, all of it on the device so that the host only
// enqueues launches:
//   * lvs_kmeans_accumulate(_keys): rows are bucketed by centroid with the STABLE bucket sort of lvs_count_sort.hip, then
//     every (centroid, 512-dim chunk) is reduced by one wave that walks its bucket in row order - the accumulation order
//     of faiss compute_centroids, so results are reproducible run to run;
//   * lvs_kmeans_objective: faiss's objective (sum of the assignment distances) from the sums the update needs anyway;
//   * lvs_kmeans_update_centroids: centroid division, faiss's empty-cluster split (std::mt19937 replayed by one device
//     thread: same draws, same decisions as faiss split_clusters), repacking of the centroids as fp16 hi|lo rows and the
//     two norms the one-pass assignment's certificate needs;
//   * lvs_rand_perm_host / lvs_kmeans_split_clusters_host: the host twins (training subsample, initial centroids; the
//     split routine is kept for callers that hold the centroids on the host) - SURVEY.md Appendix A.4.
#include <cstring>
#include <random>
#include <vector>

#include "lvs_certify.h"
#include "lvs_common.h"
#include "lvs_count_sort.h"
#include "lvs_tile.h"

namespace {

// grid = (k, ceil(dpad / (64 * DPL))), one wave per workgroup: a lane owns DPL consecutive dimensions (8, 4 or 2: 16-, 8- or
// 4-byte loads) of centroid blockIdx.x and walks the bucket in row order, U rows in flight at a time.  Per dimension the
// additions happen in exactly the bucket (= ascending row) order, so the sums do not depend on DPL, U or the launch shape -
// faiss's accumulation order (compute_centroids), bit for bit.
// A bucket is one dependent chain of additions per wave, and what a row costs a wave is mostly fixed (row number, 64-bit address,
// load issue) - so the LONGEST bucket sets the kernel's time when the sizes are skewed (configs[4]'s blob rows: up to 3-4 x the
// mean).  Narrower column slices put more waves on every bucket without touching the order of any column's sum.
template <int DPL>
struct KmVec;
template <>
struct KmVec<8> {
    typedef _Float16 type __attribute__((ext_vector_type(8)));
};
template <>
struct KmVec<4> {
    typedef _Float16 type __attribute__((ext_vector_type(4)));
};
template <>
struct KmVec<2> {
    typedef _Float16 type __attribute__((ext_vector_type(2)));
};

template <int SPLIT, int DPL>
__global__ __launch_bounds__(64) void km_reduce_kernel(const _Float16* __restrict__ x, long long ld, int d, int dpad,
                                                       const uint32_t* __restrict__ rows,
                                                       const uint32_t* __restrict__ offsets,
                                                       float* __restrict__ sums, float* __restrict__ cnt_out) {
    typedef typename KmVec<DPL>::type vec_t;
    const int c = blockIdx.x, lane = threadIdx.x;
    const int j0 = (blockIdx.y * 64 + lane) * DPL;
    const uint32_t b = offsets[c], e = offsets[c + 1];
    if (blockIdx.y == 0 && lane == 0) cnt_out[c] += (float)(e - b);
    if (j0 >= dpad) return;
    // rows in flight: 128 data VGPRs' worth (hi parts; half as many rows when the lo parts ride along), at most 64
    constexpr int U = (DPL == 8 ? 32 : 64) / (SPLIT ? 2 : 1);
    // the sums CONTINUE from what is there (zeros before the first rows): a caller may hand the rows over in consecutive ranges
    // - (s + x1) + x2 ... is the same chain of float32 additions whether it is cut into launches or not
    float acc[DPL];
#pragma unroll
    for (int t = 0; t < DPL; ++t) acc[t] = j0 + t < d ? sums[(long long)c * d + j0 + t] : 0.f;
    const _Float16* xc = x + j0;
    // many rows per batch, and the row NUMBERS of the next batch are fetched while this batch is added (they are wave-uniform:
    // scalar loads), so that a batch waits for one latency, not two
    const uint32_t nfull = (e - b) / U;
    uint32_t p = b;
    if (nfull) {
        uint32_t idx[U];
#pragma unroll
        for (int i = 0; i < U; ++i) idx[i] = rows[p + i];
        for (uint32_t kb = 0; kb < nfull; ++kb) {
            vec_t hi[U], lo[U];
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const _Float16* row = xc + (long long)idx[i] * ld;
                hi[i] = *(const vec_t*)row;
                if (SPLIT) lo[i] = *(const vec_t*)(row + dpad);
            }
            if (kb + 1 < nfull) {
#pragma unroll
                for (int i = 0; i < U; ++i) idx[i] = rows[p + U + i];
            }
#pragma unroll
            for (int i = 0; i < U; ++i)
#pragma unroll
                for (int t = 0; t < DPL; ++t) acc[t] += SPLIT ? (float)hi[i][t] + (float)lo[i][t] : (float)hi[i][t];
            p += U;
        }
    }
    for (; p < e; ++p) {
        const _Float16* row = xc + (long long)rows[p] * ld;
        vec_t h = *(const vec_t*)row, l;
        if (SPLIT) l = *(const vec_t*)(row + dpad);
#pragma unroll
        for (int t = 0; t < DPL; ++t) acc[t] += SPLIT ? (float)h[t] + (float)l[t] : (float)h[t];
    }
#pragma unroll
    for (int t = 0; t < DPL; ++t)
        if (j0 + t < d) sums[(long long)c * d + j0 + t] = acc[t];
}

// centroid update of faiss compute_centroids: c = sum * (1 / count) where the cluster is not empty, unchanged otherwise
// (an empty cluster keeps its previous centroid until split_clusters re-seeds it)
__global__ __launch_bounds__(256) void km_update_kernel(const float* __restrict__ sums, const float* __restrict__ counts,
                                                        long long total, int d, float* __restrict__ centroids) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const float cnt = counts[i / d];
        if (cnt > 0.f) {
            const float norm = 1.0f / cnt;  // IEEE division, then one rounded multiply per element (as faiss)
            centroids[i] = sums[i] * norm;
        }
    }
}

// dst[i][0..d) = float32 value of packed row ids[i] (row i when ids == NULL): hi (+ lo)
__global__ __launch_bounds__(256) void unpack_rows_kernel(const _Float16* __restrict__ src, long long ld, int d, int dpad,
                                                          int split, const long long* __restrict__ ids, long long n,
                                                          float unscale, float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const _Float16* row = src + (ids ? ids[i] : i) * ld;
    float* o = dst + i * (long long)d;
    for (int j = lane; j < d; j += 64) {
        float v = (float)row[j];
        if (split) v += (float)row[dpad + j];
        o[j] = v * unscale;
    }
}

}  // namespace

// ---- objective, empty-cluster split and centroid statistics on the device ------------------------------------------------
namespace {
__device__ inline double km_wave_sum_d(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const long long b = __double_as_longlong(v);
        const int lo = __shfl_xor((int)(b & 0xFFFFFFFFll), m, 64), hi = __shfl_xor((int)(b >> 32), m, 64);
        v += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    }
    return v;
}
// part[j] = -2 <c_j, S_j> + n_j |c_j|^2 in float64 (one wave per centroid; fixed summation order)
__global__ __launch_bounds__(256) void km_obj_part_kernel(const float* __restrict__ c, const float* __restrict__ sums,
                                                          const float* __restrict__ counts, int k, int d,
                                                          double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    double dot = 0.0, nn = 0.0;
    for (int t = lane; t < d; t += 64) {
        const double cv = (double)c[(long long)j * d + t];
        dot += cv * (double)sums[(long long)j * d + t];
        nn += cv * cv;
    }
    dot = km_wave_sum_d(dot);
    nn = km_wave_sum_d(nn);
    if (lane == 0) part[j] = -2.0 * dot + (double)counts[j] * nn;
}
// out[0] = x2 + sum_j part[j]  (one workgroup, fixed order)
__global__ __launch_bounds__(256) void km_obj_sum_kernel(const double* __restrict__ part, int k, const double* __restrict__ x2,
                                                         double* __restrict__ out) {
    __shared__ double sm[256];
    double acc = 0.0;
    for (int j = threadIdx.x; j < k; j += 256) acc += part[j];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (x2 ? x2[0] : 0.0) + sm[0];
}

// faiss split_clusters on the device: ONE wave replays std::mt19937(1234) and takes every decision exactly as the host twin
// (lvs_kmeans_split_clusters_host); all lanes copy / perturb the centroid rows.  hassign (= the counts) is modified in
// place as faiss does.  Nothing happens - not even the generator's set-up - unless some cluster is empty.
//
// A split walks the clusters cyclically and accepts cluster cj with probability (hassign[cj] - 1) / (n - k): ~k draws per
// split, 135 000 for the 132 empty clusters of configs[4]'s first iteration.  One thread doing that against global memory
// took 67 ms; here the 64 lanes test 64 consecutive (draw, cluster) pairs at once - the draws are consumed in faiss's order,
// the first accepting lane wins and the stream position advances by exactly the draws faiss would have used - with the
// sizes in LDS and the generator's 624-word state regenerated by all lanes (three dependency-free segments).
struct KmMtWave {
    uint32_t* mt;  // [624] in LDS
    __device__ void seed(uint32_t s, int lane) {
        if (lane == 0) {
            mt[0] = s;
            for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __device__ static uint32_t mix(uint32_t a, uint32_t b, uint32_t c) {  // next state word from mt[i], mt[i+1], mt[i+397]
        const uint32_t y = (a & 0x80000000u) | (b & 0x7FFFFFFFu);
        return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
    }
    // the standard in-place twist; word i needs OLD mt[i], mt[i+1] and mt[i+397 mod 624], which is old for i < 227 and already
    // NEW for i >= 227: segments [0,227), [227,454), [454,623) are each free of internal dependencies, word 623 comes last
    __device__ void twist(int lane) {
        for (int base = 0; base < 227; base += 64) {
            const int i = base + lane;
            uint32_t v = 0;
            if (i < 227) v = mix(mt[i], mt[i + 1], mt[i + 397]);
            __builtin_amdgcn_wave_barrier();
            if (i < 227) mt[i] = v;
            __builtin_amdgcn_wave_barrier();
        }
        // mt[i + 1] read by word i = 226 was still old when it was computed (all reads of a round precede its writes; rounds
        // run upwards, and word i only ever reads indices > i or, for i >= 227, the finished new words below i - 226)
        for (int seg = 227; seg < 623; seg += 227) {
            const int hi = seg + 227 < 623 ? seg + 227 : 623;
            for (int base = seg; base < hi; base += 64) {
                const int i = base + lane;
                uint32_t v = 0;
                if (i < hi) v = mix(mt[i], mt[i + 1], mt[i - 227]);
                __builtin_amdgcn_wave_barrier();
                if (i < hi) mt[i] = v;
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (lane == 0) mt[623] = mix(mt[623], mt[0], mt[396]);
        __builtin_amdgcn_wave_barrier();
    }
    __device__ static uint32_t temper(uint32_t y) {
        y ^= y >> 11;
        y ^= (y << 7) & 0x9D2C5680u;
        y ^= (y << 15) & 0xEFC60000u;
        y ^= y >> 18;
        return y;
    }
};
constexpr int KM_SPLIT_LDS_K = 15360;  // cluster sizes kept in LDS up to this k (with the generator's state: < 64 KB); beyond, global memory
__global__ __launch_bounds__(64) void km_split_kernel(int d, int k, long long n, float* hassign_, float* __restrict__ centroids,
                                                      int* __restrict__ out_nsplit) {
    extern __shared__ uint32_t km_split_smem[];
    uint32_t* state = km_split_smem;                 // [624] (+ 16 pad)
    float* hl = (float*)(km_split_smem + 640);       // [k] when k <= KM_SPLIT_LDS_K
    const int lane = threadIdx.x;
    volatile float* hg = hassign_;
    const bool in_lds = k <= KM_SPLIT_LDS_K;
    bool any = false;
    for (int c = lane; c < k; c += 64) {
        const float h = hg[c];
        if (in_lds) hl[c] = h;
        any |= h == 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (__builtin_amdgcn_ballot_w64(any) == 0ull || n <= k) {
        if (lane == 0 && out_nsplit) *out_nsplit = 0;
        return;
    }
    auto H = [&](int c) -> float { return in_lds ? hl[c] : hg[c]; };
    auto setH = [&](int c, float v) {
        if (in_lds) hl[c] = v;
        hg[c] = v;
    };
    KmMtWave rng{state};
    rng.seed(1234u, lane);
    int idx = 624;  // next unused word of the current state block (624: regenerate first), wave-uniform
    const float EPS = 1.0f / 1024.0f;
    const float denom = (float)(n - k);
    int nsplit = 0;
    for (int ci = 0; ci < k; ++ci) {
        if (H(ci) != 0.f) continue;  // wave-uniform (every lane reads the same word)
        // walk cj = 0, 1, 2, ... (cyclically) consuming one draw per step until r < p(cj)
        int cj0 = 0, found = -1;
        long long draws = 0;
        // the acceptance probabilities of one round over the clusters sum to 1, so a split takes ~k draws; the cap only
        // guards the device against counts that do not describe n points (faiss itself would spin forever)
        const long long cap = 4096ll * k + (1ll << 20);
        while (found < 0 && draws <= cap) {
            if (idx >= 624) {
                rng.twist(lane);
                idx = 0;
            }
            const int avail = 624 - idx < 64 ? 624 - idx : 64;  // draws this round (one per lane), wave-uniform
            bool acc = false;
            if (lane < avail) {
                const int cj = (cj0 + lane) % k;
                const float p = (H(cj) - 1.0f) / denom;
                const float r = (float)KmMtWave::temper(state[idx + lane]) / 4294967295.0f;  // faiss rand_float(): mt() / float(mt.max())
                acc = r < p;
            }
            const u64 m = __builtin_amdgcn_ballot_w64(acc);
            if (m) {
                const int w = __ffsll((long long)m) - 1;  // the first accepting step: later draws of this round stay unused
                found = (cj0 + w) % k;
                idx += w + 1;
                draws += w + 1;
            } else {
                idx += avail;
                draws += avail;
                cj0 = (cj0 + avail) % k;
            }
        }
        if (found < 0) {  // inconsistent counts: report and stop
            if (lane == 0 && out_nsplit) *out_nsplit = -1;
            return;
        }
        const int cj = found;
        if (lane == 0) {
            const float hj = H(cj);
            const float half = hj / 2;
            setH(ci, half);
            setH(cj, hj - half);
        }
        __builtin_amdgcn_wave_barrier();
        float* a = centroids + (long long)ci * d;
        float* b = centroids + (long long)cj * d;
        for (int j = lane; j < d; j += 64) {  // a lane only ever touches its own columns: later splits see these writes
            const float v = b[j];
            if (j % 2 == 0) {
                a[j] = v * (1 + EPS);
                b[j] = v * (1 - EPS);
            } else {
                a[j] = v * (1 - EPS);
                b[j] = v * (1 + EPS);
            }
        }
        ++nsplit;
    }
    if (lane == 0 && out_nsplit) *out_nsplit = nsplit;
}

// stats[0] = max |row|^2 (of the stored values), stats[1] = max |lo part of a row|^2: what the one-pass assignment's
// certificate needs of the centroids (non-negative floats order like their bit patterns: atomicMax on the bits)
__global__ __launch_bounds__(256) void km_stats_kernel(const _Float16* __restrict__ rows, long long ld, int dpad, int split,
                                                       const float* __restrict__ norms, int k, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    float e = 0.f;
    if (split)
        for (int t = lane; t < dpad; t += 64) {
            const float v = (float)rows[(long long)j * ld + dpad + t];
            e += v * v;
        }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) e += __shfl_xor(e, m, 64);
    if (lane == 0) {
        atomicMax((unsigned int*)&stats[0], __float_as_uint(norms[j]));
        atomicMax((unsigned int*)&stats[1], __float_as_uint(e));
    }
}

int32_t km_pack_and_stats(const float* centroids, int32_t k, int32_t d, int32_t pack_mode, void* packed_out, float* norms_out,
                          float* stats_out, hipStream_t st) {
    int32_t rc = lvs_pack_rows(centroids, LVS_DTYPE_F32, k, d, pack_mode, 0, packed_out, norms_out, st);
    if (rc != LVS_OK) return rc;
    if (stats_out) {
        const int dpad = (int)lvs_round_up(d, LVS_BK);
        const int split = pack_mode == LVS_PACK_SPLIT;
        LVS_HIP_CHECK(lvs_zero_async(stats_out, 2 * sizeof(float), st));
        hipLaunchKernelGGL(km_stats_kernel, dim3((unsigned)lvs_ceil_div(k, 4)), dim3(256), 0, st, (const _Float16*)packed_out,
                           (long long)(split ? 2 * dpad : dpad), dpad, split, (const float*)norms_out, k, stats_out);
        LVS_HIP_CHECK(hipGetLastError());
    }
    return LVS_OK;
}
}  // namespace

// ---- exact distance bounds across iterations (Hamerly 2010): which rows need no new search -------------------------------
// Per row i: assign[i], ub[i] >= |x_i - c_assign| and lb[i] <= min over the OTHER centroids of |x_i - c_j| (Euclidean, in
// the rows' scaled domain).  When the centroids move by delta_j, ub grows by delta_assign and lb shrinks by the largest
// delta among the others; while ub < lb (with a margin above float32 noise) the row's nearest centroid provably has not
// changed - faiss's exhaustive search would return the same id - and the row is skipped.  Every other row goes through the
// full search again, which also renews its bounds.  Results are identical to the exhaustive iteration; only work is saved.
namespace {
// delta[j] = |c_new_j - c_old_j| (one wave per centroid)
__global__ __launch_bounds__(256) void km_shift_kernel(const float* __restrict__ c_old, const float* __restrict__ c_new, int k,
                                                       int d, float* __restrict__ delta) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    float acc = 0.f;
    for (int t = lane; t < d; t += 64) {
        const float v = c_new[(long long)j * d + t] - c_old[(long long)j * d + t];
        acc += v * v;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) delta[j] = sqrtf(acc) * (1.0f + 1e-6f);  // rounded up
}
// top2[0] = largest delta, top2[1] = its centroid (as float bits of an int), top2[2] = second largest (one workgroup)
__global__ __launch_bounds__(256) void km_shift_top2_kernel(const float* __restrict__ delta, int k, float* __restrict__ top2) {
    __shared__ float m1[256], m2[256];
    __shared__ int a1[256];
    float b1 = 0.f, b2 = 0.f;
    int i1 = -1;
    for (int j = threadIdx.x; j < k; j += 256) {
        const float v = delta[j];
        if (v > b1 || i1 < 0) {
            b2 = i1 < 0 ? 0.f : b1;
            b1 = v;
            i1 = j;
        } else if (v > b2) {
            b2 = v;
        }
    }
    m1[threadIdx.x] = b1;
    m2[threadIdx.x] = b2;
    a1[threadIdx.x] = i1;
    __syncthreads();
    if (threadIdx.x == 0) {
        float g1 = 0.f, g2 = 0.f;
        int gi = -1;
        for (int t = 0; t < 256; ++t) {
            if (a1[t] < 0) continue;
            if (m1[t] > g1 || gi < 0) {
                g2 = gi < 0 ? m2[t] : fmaxf(g1, m2[t]);
                g1 = m1[t];
                gi = a1[t];
            } else {
                g2 = fmaxf(g2, m1[t]);
            }
        }
        top2[0] = g1;
        top2[1] = __int_as_float(gi);
        top2[2] = g2;
    }
}
// bounds of the rows pos[i] (NULL: rows 0 .. m) from a search result: keys[i] = winner key (score = -dist^2), second[i] =
// runner-up score; err_i = (coef[0] E + coef[1] R) |x| + coef[2] + coef[3] R + coef[4] R^2 is added to the winner's squared
// distance and subtracted from the runner-up's before the roots (the search's own error bound)
__global__ __launch_bounds__(256) void km_bounds_set_kernel(const u64* __restrict__ keys, long long key_stride,
                                                            const float* __restrict__ second, const float* __restrict__ qn,
                                                            const long long* __restrict__ pos, long long m,
                                                            const float* __restrict__ stats, float c0, float c1, float c2,
                                                            float c3, float c4, long long id_offset, int* __restrict__ assign,
                                                            float* __restrict__ ub, float* __restrict__ lb) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    // (five scalar parameters here and in km_bounds_fix_kernel: with the struct as the parameter the compiler sums err1 of the
    // fix kernel in another order and lb moves in its last bit, profiles/certify_refactor_check.md)
    const LvsBoundCoef coef{{c0, c1, c2, c3, c4}};
    const LvsBound b(coef, stats);
    const long long row = pos ? pos[i] : i;
    const u64 kq = keys[i * key_stride];
    const float err = b.at(sqrtf(qn[i]));
    const float d1 = kq ? fmaxf(-lvs_unord32((uint32_t)(kq >> 32)), 0.f) : 3.0e38f;
    const float s2 = second ? second[i] : lvs_unord32((uint32_t)(keys[i * key_stride + 1] >> 32));
    const float d2 = fmaxf(-s2, 0.f);  // -inf runner-up (a single centroid) -> +inf
    assign[row] = kq ? (int)((long long)(0xFFFFFFFFu - (uint32_t)(kq & 0xFFFFFFFFull)) - id_offset) : -1;
    ub[row] = sqrtf(d1 + err) * (1.0f + 1e-6f);
    lb[row] = sqrtf(fmaxf(d2 - err, 0.f)) * (1.0f - 1e-6f);
}
// rows whose one-pass winner was NOT certified: the exact (k = 1) search decided them.  exact[i] = its key; approx[i] = the
// one-pass key whose bounds km_bounds_set_kernel has just written for row pos[i].  The upper bound is renewed from the exact
// distance; the lower bound stays valid as it is when the winner is the same centroid (every other centroid's one-pass score
// was <= the runner-up's), and otherwise must also stay below the distance to the one-pass winner, now one of "the others".
__global__ __launch_bounds__(256) void km_bounds_fix_kernel(const u64* __restrict__ approx, const u64* __restrict__ exact,
                                                            const float* __restrict__ qn, const long long* __restrict__ pos,
                                                            long long m, const float* __restrict__ stats, float c0, float c1,
                                                            float c2, float c3, float c4, float e1, float e4, long long id_offset,
                                                            int* __restrict__ assign, float* __restrict__ ub,
                                                            float* __restrict__ lb) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const LvsBoundCoef coef{{c0, c1, c2, c3, c4}};
    const LvsBound b(coef, stats);
    const long long row = pos ? pos[i] : i;
    const u64 ka = approx[i], ke = exact[i];
    if (!ke) return;
    const float qnorm = sqrtf(qn[i]);
    const float err1 = b.at(qnorm);                        // the one-pass search's error bound
    const float err2 = e1 * b.R * qnorm + e4 * b.R * b.R;  // float32 rounding of the exact distance
    const float d1e = fmaxf(-lvs_unord32((uint32_t)(ke >> 32)), 0.f);
    assign[row] = (int)((long long)(0xFFFFFFFFu - (uint32_t)(ke & 0xFFFFFFFFull)) - id_offset);
    ub[row] = sqrtf(d1e + err2) * (1.0f + 1e-6f);
    if ((uint32_t)ka != (uint32_t)ke) {  // another centroid than the one-pass winner
        const float d1a = ka ? fmaxf(-lvs_unord32((uint32_t)(ka >> 32)), 0.f) : 0.f;
        lb[row] = fminf(lb[row], sqrtf(fmaxf(d1a - err1, 0.f)) * (1.0f - 1e-6f));
    }
}
// one iteration later: move the bounds by the centroid shifts and list the rows whose nearest centroid may have changed
__global__ __launch_bounds__(256) void km_bounds_step_kernel(const int* __restrict__ assign, float* __restrict__ ub,
                                                             float* __restrict__ lb, const float* __restrict__ delta,
                                                             const float* __restrict__ top2, long long n, long long per_block,
                                                             long long* __restrict__ out_idx,
                                                             unsigned long long* __restrict__ out_count) {
    const float g1 = top2[0], g2 = top2[2];
    const int gi = __float_as_int(top2[1]);
    auto move = [&](long long q) -> int {  // the first sweep is the one read-modify-write pass over the bounds
        const int a = assign[q];
        float u = ub[q], l = lb[q];
        if (a >= 0) {
            u += delta[a];
            l -= a == gi ? g2 : g1;
        }
        ub[q] = u;
        lb[q] = l;
        return a < 0 || !(u * (1.0f + 1e-5f) < l);
    };
    auto moved = [&](long long q) -> int { return assign[q] < 0 || !(ub[q] * (1.0f + 1e-5f) < lb[q]); };
    long long* const out[1] = {out_idx};
    lvs_append_lists<1>(per_block, n, move, moved, out, out_count);
}
}  // namespace

extern "C" int32_t lvs_kmeans_centroid_shift(const float* c_old, const float* c_new, int32_t k, int32_t d, float* out_delta,
                                             float* out_top2, void* stream) {
    LVS_REQUIRE(k > 0 && d > 0 && c_old && c_new && out_delta && out_top2, "bad arguments");
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_shift_kernel, dim3((unsigned)lvs_ceil_div(k, 4)), dim3(256), 0, st, c_old, c_new, k, d, out_delta);
    hipLaunchKernelGGL(km_shift_top2_kernel, dim3(1), dim3(256), 0, st, (const float*)out_delta, k, out_top2);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_kmeans_bounds_set(const uint64_t* keys, int32_t key_stride, const float* second, const float* q_norms_sq,
                                         const int64_t* positions, int64_t m, const float* corpus_stats, const float* coef5,
                                         int64_t id_offset, int32_t* assign, float* ub, float* lb, void* stream) {
    LVS_REQUIRE(m >= 0 && key_stride >= 1 && (second || key_stride >= 2), "bad arguments");
    if (m == 0) return LVS_OK;
    LVS_REQUIRE(keys && q_norms_sq && corpus_stats && coef5 && assign && ub && lb, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(km_bounds_set_kernel, dim3((unsigned)lvs_ceil_div(m, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)keys, (long long)key_stride, second, q_norms_sq, (const long long*)positions, (long long)m,
                       corpus_stats, coef5[0], coef5[1], coef5[2], coef5[3], coef5[4], (long long)id_offset, assign, ub, lb);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_kmeans_bounds_fix(const uint64_t* approx_keys, const uint64_t* exact_keys, const float* q_norms_sq,
                                         const int64_t* positions, int64_t m, const float* corpus_stats, const float* coef5,
                                         const float* exact_coef2, int64_t id_offset, int32_t* assign, float* ub, float* lb,
                                         void* stream) {
    LVS_REQUIRE(m >= 0, "bad arguments");
    if (m == 0) return LVS_OK;
    LVS_REQUIRE(approx_keys && exact_keys && q_norms_sq && corpus_stats && coef5 && exact_coef2 && assign && ub && lb, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(km_bounds_fix_kernel, dim3((unsigned)lvs_ceil_div(m, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)approx_keys, (const u64*)exact_keys, q_norms_sq, (const long long*)positions, (long long)m,
                       corpus_stats, coef5[0], coef5[1], coef5[2], coef5[3], coef5[4], exact_coef2[0], exact_coef2[1],
                       (long long)id_offset, assign, ub, lb);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_kmeans_bounds_step(const int32_t* assign, float* ub, float* lb, const float* delta, const float* top2,
                                          int64_t n, int64_t* out_idx, uint64_t* out_count, void* stream) {
    LVS_REQUIRE(n >= 0, "bad arguments");
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(assign && ub && lb && delta && top2 && out_idx && out_count, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    const long long per_block = lvs_append_per_block(n);
    hipLaunchKernelGGL(km_bounds_step_kernel, dim3((unsigned)lvs_ceil_div(n, per_block)), dim3(256), 0, (hipStream_t)stream,
                       assign, ub, lb, delta, top2, (long long)n, per_block, (long long*)out_idx,
                       (unsigned long long*)out_count);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int64_t lvs_kmeans_objective_workspace_bytes(int32_t k) { return k > 0 ? lvs_round_up((int64_t)k * 8, 256) : LVS_EINVAL; }

extern "C" int32_t lvs_kmeans_objective(const float* centroids, const float* sums, const float* counts, int32_t k, int32_t d,
                                        const double* x_norms_sq_sum, double* out_obj, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    LVS_REQUIRE(k > 0 && d > 0, "bad shape k=%d d=%d", k, d);
    LVS_REQUIRE(centroids && sums && counts && out_obj && workspace, "NULL buffer");
    if (workspace_bytes < lvs_kmeans_objective_workspace_bytes(k)) {  // LVS_ENOMEM as in every other entry, not LVS_REQUIRE's LVS_EINVAL
        lvs_set_error("workspace too small: need %lld bytes, got %lld", (long long)lvs_kmeans_objective_workspace_bytes(k),
                      (long long)workspace_bytes);
        return LVS_ENOMEM;
    }
    LVS_REQUIRE_WS_ALIGNED(workspace);
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(km_obj_part_kernel, dim3((unsigned)lvs_ceil_div(k, 4)), dim3(256), 0, st, centroids, sums, counts, k, d, part);
    hipLaunchKernelGGL(km_obj_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)part, k, x_norms_sq_sum, out_obj);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_kmeans_pack_centroids(const float* centroids, int32_t k, int32_t d, int32_t pack_mode, void* packed_out,
                                             float* norms_out, float* stats_out, void* stream) {
    LVS_REQUIRE(k > 0 && d > 0, "bad shape k=%d d=%d", k, d);
    LVS_REQUIRE(centroids && packed_out && norms_out, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    return km_pack_and_stats(centroids, k, d, pack_mode, packed_out, norms_out, stats_out, (hipStream_t)stream);
}

extern "C" int32_t lvs_kmeans_update_centroids(const float* sums, float* counts, int32_t k, int32_t d, int64_t n_train,
                                               float* centroids, int32_t* out_nsplit, int32_t pack_mode, void* packed_out,
                                               float* norms_out, float* stats_out, void* stream) {
    LVS_REQUIRE(k > 0 && d > 0, "bad shape k=%d d=%d", k, d);
    LVS_REQUIRE(sums && counts && centroids, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)k * d;
    const long long blocks = lvs_ceil_div(total, 256);
    hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, sums,
                       (const float*)counts, total, d, centroids);
    if (n_train > 0)  // faiss: split_clusters right after compute_centroids; n_train <= 0 skips it (caller splits on the host)
    {
        const size_t lds = (640 + (size_t)(k <= KM_SPLIT_LDS_K ? k : 0)) * 4;
        hipLaunchKernelGGL(km_split_kernel, dim3(1), dim3(64), lds, st, d, k, (long long)n_train, counts, centroids, out_nsplit);
    }
    LVS_HIP_CHECK(hipGetLastError());
    if (packed_out) {
        LVS_REQUIRE(norms_out, "norms_out is NULL");
        return km_pack_and_stats(centroids, k, d, pack_mode, packed_out, norms_out, stats_out, st);
    }
    return LVS_OK;
}

extern "C" int32_t lvs_unpack_rows(const void* src, int32_t d, int32_t pack_mode, const int64_t* ids, int64_t n,
                                   int32_t scale_exp, float* dst, void* stream) {
    LVS_REQUIRE(d > 0 && n >= 0, "bad shape n=%lld d=%d", (long long)n, d);
    LVS_REQUIRE(scale_exp >= -100 && scale_exp <= 100, "scale_exp %d out of range", scale_exp);
    LVS_REQUIRE(pack_mode == LVS_PACK_F16 || pack_mode == LVS_PACK_SPLIT, "bad pack_mode %d", pack_mode);
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(src && dst, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    const int dpad = (int)lvs_round_up(d, LVS_BK);
    const int split = pack_mode == LVS_PACK_SPLIT;
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)lvs_ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)src, (long long)(split ? 2 * dpad : dpad), d, dpad, split,
                       (const long long*)ids, (long long)n, ldexpf(1.0f, -scale_exp), dst);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

namespace {
// exactly one of keys (result keys, ids less id_offset) and assign is given
int32_t km_accumulate(const void* x, int64_t n, int32_t d, int32_t pack_mode, const uint64_t* keys, const int64_t* assign,
                      int64_t id_offset, int32_t k, float* sums, float* counts, void* workspace, int64_t workspace_bytes,
                      void* stream) {
    LVS_REQUIRE(n >= 0 && d > 0 && k > 0, "bad shape n=%lld d=%d k=%d", (long long)n, d, k);
    LVS_REQUIRE(pack_mode == LVS_PACK_F16 || pack_mode == LVS_PACK_SPLIT, "bad pack_mode");
    LVS_REQUIRE(n < 0xFFFFFFFFll, "n must be below 2^32");
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(x && (keys || assign) && sums && counts && workspace, "NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t *rows = nullptr, *offs = nullptr;
    const int32_t rc = lvs_bucket_positions(keys, assign, n, k, id_offset, workspace, workspace_bytes, st, &rows, &offs);
    if (rc != LVS_OK) return rc;
    LVS_DEVICE_GUARD(stream);
    const int dpad = (int)lvs_round_up(d, LVS_BK);
    const long long ld = pack_mode == LVS_PACK_SPLIT ? 2 * dpad : dpad;
    // column slices per bucket: two dimensions per lane (128 columns per wave; d = 768: six waves per bucket).  Measured neutral
    // against eight dimensions per lane on its own (profiles/r05s_km_reduce_dpl_sweep.log), but at 82 instead of 148 VGPRs a
    // wave of this kernel fits on a SIMD NEXT TO the two waves of the assignment kernel (2 x 199 + 82 <= 512), which is what lets
    // the sums of one half of the rows run under the assignment of the other half (lotus_amd/cluster.py)
    int dpl = 2;
    if (lvs_tune_set("LVS_KM_DPL")) {
        const int v = (int)lvs_tune("LVS_KM_DPL", 0);
        if (v == 2 || v == 4 || v == 8) dpl = v;
    }
    const dim3 grid((unsigned)k, (unsigned)lvs_ceil_div(dpad, 64 * dpl));
#define LVS_KM_REDUCE(SP, DP)                                                                                              \
    hipLaunchKernelGGL((km_reduce_kernel<SP, DP>), grid, dim3(64), 0, st, (const _Float16*)x, ld, d, dpad, rows, offs, sums, \
                       counts)
    if (pack_mode == LVS_PACK_SPLIT) {
        if (dpl == 2) LVS_KM_REDUCE(1, 2);
        else if (dpl == 4) LVS_KM_REDUCE(1, 4);
        else LVS_KM_REDUCE(1, 8);
    } else {
        if (dpl == 2) LVS_KM_REDUCE(0, 2);
        else if (dpl == 4) LVS_KM_REDUCE(0, 4);
        else LVS_KM_REDUCE(0, 8);
    }
#undef LVS_KM_REDUCE
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}
}  // namespace

extern "C" int64_t lvs_kmeans_accumulate_workspace_bytes(int64_t n, int32_t k) { return lvs_bucket_workspace_bytes(n, k); }

extern "C" int32_t lvs_kmeans_accumulate(const void* x, int64_t n, int32_t d, int32_t pack_mode, const int64_t* assign,
                                         int32_t k, float* sums, float* counts, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
    return km_accumulate(x, n, d, pack_mode, nullptr, assign, 0, k, sums, counts, workspace, workspace_bytes, stream);
}

extern "C" int32_t lvs_kmeans_accumulate_keys(const void* x, int64_t n, int32_t d, int32_t pack_mode, const uint64_t* keys,
                                              int64_t id_offset, int32_t k, float* sums, float* counts, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
    return km_accumulate(x, n, d, pack_mode, keys, nullptr, id_offset, k, sums, counts, workspace, workspace_bytes, stream);
}

// ---- host-side pieces of faiss Clustering (bit-exact: std::mt19937 is the generator faiss uses) -------------
extern "C" int32_t lvs_rand_perm_host(int64_t n, int64_t seed, int64_t* out_perm) {
    LVS_REQUIRE(n >= 0 && (n == 0 || out_perm), "bad arguments");
    std::mt19937 mt((unsigned)seed);
    for (int64_t i = 0; i < n; ++i) out_perm[i] = i;
    for (int64_t i = 0; i + 1 < n; ++i) {
        int64_t i2 = i + (int64_t)(mt() % (uint32_t)(n - i));  // faiss rand_int(max) = mt() % max
        int64_t t = out_perm[i];
        out_perm[i] = out_perm[i2];
        out_perm[i2] = t;
    }
    return LVS_OK;
}

// The first m entries of the same permutation in O(m): step i of the forward Fisher-Yates fixes perm[i] and touches only
// perm[i] and perm[i2 >= i], and both callers (training subsample, initial centroids) read a prefix - of 10 M entries at
// configs[4]'s size, where the full permutation costs 0.17 s of host time per call.  Positions >= m live in a hash map.
extern "C" int32_t lvs_rand_perm_prefix_host(int64_t n, int64_t seed, int64_t m, int64_t* out_prefix) {
    LVS_REQUIRE(n >= 0 && m >= 0 && m <= n && (m == 0 || out_prefix), "bad arguments");
    std::mt19937 mt((unsigned)seed);
    for (int64_t i = 0; i < m; ++i) out_prefix[i] = i;
    // open-addressing table (linear probing), key and value side by side (one cache line per probe), at most one new
    // entry per step: <= 50 % full.  position >= m -> its current content (absent: the position itself)
    struct Slot { int64_t key, val; };
    size_t cap = 16;
    while (cap < (size_t)m * 2) cap <<= 1;
    std::vector<Slot> tab(cap, Slot{-1, 0});
    for (int64_t i = 0; i < m && i + 1 < n; ++i) {
        const int64_t i2 = i + (int64_t)(mt() % (uint32_t)(n - i));
        if (i2 < m) {
            const int64_t t = out_prefix[i];
            out_prefix[i] = out_prefix[i2];
            out_prefix[i2] = t;
        } else {
            size_t h = (size_t)(((uint64_t)i2 * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
            while (tab[h].key != -1 && tab[h].key != i2) h = (h + 1) & (cap - 1);
            const int64_t v = tab[h].key == i2 ? tab[h].val : i2;
            tab[h].key = i2;
            tab[h].val = out_prefix[i];
            out_prefix[i] = v;
        }
    }
    return LVS_OK;
}

extern "C" int32_t lvs_kmeans_split_clusters_host(int32_t d, int32_t k, int64_t n, float* hassign, float* centroids,
                                                  int32_t* out_nsplit) {
    LVS_REQUIRE(d > 0 && k > 0 && n > k && hassign && centroids, "bad arguments");
    const float EPS = 1.0f / 1024.0f;
    std::mt19937 mt(1234u);
    int32_t nsplit = 0;
    for (int32_t ci = 0; ci < k; ++ci) {
        if (hassign[ci] != 0.f) continue;
        int32_t cj;
        for (cj = 0;; cj = (cj + 1) % k) {
            float p = (hassign[cj] - 1.0f) / (float)(n - k);
            float r = (float)mt() / (float)mt.max();  // faiss rand_float()
            if (r < p) break;
        }
        float* a = centroids + (int64_t)ci * d;
        float* b = centroids + (int64_t)cj * d;
        memcpy(a, b, sizeof(float) * (size_t)d);
        for (int32_t j = 0; j < d; ++j) {
            if (j % 2 == 0) {
                a[j] *= 1 + EPS;
                b[j] *= 1 - EPS;
            } else {
                a[j] *= 1 - EPS;
                b[j] *= 1 + EPS;
            }
        }
        hassign[ci] = hassign[cj] / 2;
        hassign[cj] -= hassign[ci];
        ++nsplit;
    }
    if (out_nsplit) *out_nsplit = nsplit;
    return LVS_OK;
}
