// C-ABI of liblotus_hip (see include/lotus_hip.h) + the small streaming kernels around the tile kernel:
// row packing (fp32/fp16 -> fp16 or fp16 hi|lo), row gather, candidate-list merge, key decoding.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "lvs_certify.h"
#include "lvs_common.h"
#include "lvs_count_sort.h"
#include "lvs_tile.h"

// ---------------------------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void lvs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* lvs_last_error(void) { return g_err; }
extern "C" int32_t lvs_abi_version(void) { return LVS_ABI_VERSION; }
extern "C" int32_t lvs_build_flags(void) {
    int32_t f = 0;
#ifdef LVS_TUNING
    f |= LVS_BUILD_TUNING;
#endif
#ifdef LVS_COUNT_EVENTS
    f |= LVS_BUILD_COUNT_EVENTS;
#endif
    return f;
}

extern "C" int32_t lvs_device_count(int32_t* out_count) {
    LVS_REQUIRE(out_count, "out_count is NULL");
    int n = 0;
    LVS_HIP_CHECK(hipGetDeviceCount(&n));
    *out_count = n;
    return LVS_OK;
}

extern "C" int32_t lvs_device_info(int32_t device, char* name, int32_t name_cap, int32_t* out_cus,
                                   int64_t* out_hbm_bytes) {
    hipDeviceProp_t p;
    LVS_HIP_CHECK(hipGetDeviceProperties(&p, device));
    if (name && name_cap > 0) {
        snprintf(name, (size_t)name_cap, "%s (%s)", p.name, p.gcnArchName);
    }
    if (out_cus) *out_cus = p.multiProcessorCount;
    if (out_hbm_bytes) *out_hbm_bytes = (int64_t)p.totalGlobalMem;
    return LVS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// timing hook (HIP events on the launch stream around the dominant kernel)
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct TimingState {
    std::mutex mu;
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0;
    int64_t launches = 0;
    int64_t calls = 0;   // entry-point calls that timed at least one launch (a chunked search times several per call)
    int32_t kernel = 0;  // LVS_KERNEL_* of the last timed launch
} g_timing;


struct ScopedKernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t s;
    bool on;
    // continuation: a further launch of the SAME search (its next chunk of queries) - counted as a launch, not as a call
    explicit ScopedKernelTimer(hipStream_t st, int32_t kernel = LVS_KERNEL_TILE, bool continuation = false) : s(st) {
        std::lock_guard<std::mutex> lk(g_timing.mu);
        on = g_timing.on;
        if (on) {
            g_timing.kernel = kernel;
            if (!continuation) ++g_timing.calls;
            if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
                on = false;
                return;
            }
            (void)hipEventRecord(e0, s);
        }
    }
    ~ScopedKernelTimer() {
        if (!on) return;
        (void)hipEventRecord(e1, s);
        std::lock_guard<std::mutex> lk(g_timing.mu);
        g_timing.pending.emplace_back(e0, e1);
    }
};
}  // namespace

LvsKernelTimer::LvsKernelTimer(hipStream_t st) : impl(new ScopedKernelTimer(st)) {}
LvsKernelTimer::~LvsKernelTimer() { delete (ScopedKernelTimer*)impl; }

extern "C" int32_t lvs_timing_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_timing.mu);
    g_timing.on = on != 0;
    for (auto& pr : g_timing.pending) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    g_timing.pending.clear();
    g_timing.total_ms = 0;
    g_timing.launches = 0;
    g_timing.calls = 0;
    return LVS_OK;
}

extern "C" int32_t lvs_timing_read(double* out_total_ms, int64_t* out_launches) {
    std::lock_guard<std::mutex> lk(g_timing.mu);
    for (auto& pr : g_timing.pending) {
        LVS_HIP_CHECK(hipEventSynchronize(pr.second));
        float ms = 0;
        LVS_HIP_CHECK(hipEventElapsedTime(&ms, pr.first, pr.second));
        g_timing.total_ms += ms;
        g_timing.launches += 1;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    g_timing.pending.clear();
    if (out_total_ms) *out_total_ms = g_timing.total_ms;
    if (out_launches) *out_launches = g_timing.launches;
    return LVS_OK;
}

extern "C" int32_t lvs_timing_read_calls(double* out_total_ms, int64_t* out_launches, int64_t* out_calls, int32_t* out_kernel) {
    const int32_t rc = lvs_timing_read(out_total_ms, out_launches);
    if (rc != LVS_OK) return rc;
    std::lock_guard<std::mutex> lk(g_timing.mu);
    if (out_calls) *out_calls = g_timing.calls;
    if (out_kernel) *out_kernel = g_timing.kernel;
    return LVS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------------------------------------------
extern "C" int32_t lvs_packed_ld(int32_t d, int32_t pack_mode) {
    LvsLayout l;
    return lvs_layout(d, pack_mode, pack_mode, false, l) == LVS_OK ? l.ldb : LVS_EINVAL;
}

namespace {

// one wave per row, one element per lane and step: the fallback for d % 8 != 0 (rows not 16-byte aligned)
// flags (nullable device word): LVS_PACK_FLAG_NONFINITE when an input value is inf / NaN, LVS_PACK_FLAG_RANGE when a finite
// value (after the optional normalisation) lies outside fp16's range (|x| > 65504 would be stored as inf)
__device__ inline uint32_t pack_check(float x) {
    const float ax = fabsf(x);
    return !(ax <= 3.4028234663852886e38f) ? (uint32_t)LVS_PACK_FLAG_NONFINITE : (ax > 65504.0f ? (uint32_t)LVS_PACK_FLAG_RANGE : 0u);
}
__device__ inline void pack_report(uint32_t bad, uint32_t* flags) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, m, 64);
    if (bad && flags && (threadIdx.x & 63) == 0) atomicOr(flags, bad);
}

template <typename SrcT>
__global__ __launch_bounds__(256) void pack_rows_kernel(const SrcT* __restrict__ src, long long n, int d, int dpad,
                                                        int split, int normalize, float pw, _Float16* __restrict__ dst,
                                                        float* __restrict__ norms, uint32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    const SrcT* s = src + row * (long long)d;
    const int ld = split ? 2 * dpad : dpad;
    _Float16* o = dst + row * (long long)ld;
    float scale = 1.0f;
    if (normalize) {
        float ss = 0.f;
        for (int j = lane; j < d; j += 64) {
            float x = (float)s[j];
            ss += x * x;
        }
        ss = lvs_wave_sum(ss);
        scale = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
    }
    float nn = 0.f;
    uint32_t bad = 0;
    for (int j = lane; j < dpad; j += 64) {
        float x = j < d ? ((float)s[j] * scale) * pw : 0.f;  // pw is a power of two: exact
        bad |= pack_check(x);
        _Float16 hi = (_Float16)x;
        float stored = (float)hi;
        o[j] = hi;
        if (split) {
            _Float16 lo = (_Float16)(x - (float)hi);
            o[dpad + j] = lo;
            stored += (float)lo;
        }
        nn += stored * stored;
    }
    if (norms) {
        nn = lvs_wave_sum(nn);
        if (lane == 0) norms[row] = nn;
    }
    pack_report(bad, flags);
}

typedef float pk_float4 __attribute__((ext_vector_type(4)));

__device__ inline void pack_load8(const float* s, float (&v)[8]) {
    pk_float4 a = *(const pk_float4*)s, b = *(const pk_float4*)(s + 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        v[t] = a[t];
        v[4 + t] = b[t];
    }
}
__device__ inline void pack_load8(const _Float16* s, float (&v)[8]) {
    half8 a = *(const half8*)s;
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = (float)a[t];
}

// one wave per row, 8 consecutive elements per lane and step (16-byte stores, 16/32-byte loads): d % 8 == 0
template <typename SrcT, int SPLIT>
__global__ __launch_bounds__(256) void pack_rows_vec_kernel(const SrcT* __restrict__ src, long long n, int d, int dpad,
                                                            int normalize, float pw, _Float16* __restrict__ dst,
                                                            float* __restrict__ norms, uint32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    const SrcT* s = src + row * (long long)d;
    _Float16* o = dst + row * (long long)(SPLIT ? 2 * dpad : dpad);
    float scale = 1.0f;
    if (normalize) {
        float ss = 0.f;
        for (int j = lane * 8; j < d; j += 512) {
            float v[8];
            pack_load8(s + j, v);
#pragma unroll
            for (int t = 0; t < 8; ++t) ss += v[t] * v[t];
        }
        ss = lvs_wave_sum(ss);
        scale = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
    }
    float nn = 0.f;
    uint32_t bad = 0;
    for (int j = lane * 8; j < dpad; j += 512) {
        float v[8];
        if (j < d) {
            pack_load8(s + j, v);
        } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = 0.f;
        }
        half8 hi, lo;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float x = (v[t] * scale) * pw;  // pw is a power of two: exact
            bad |= pack_check(x);
            hi[t] = (_Float16)x;
            float stored = (float)hi[t];
            if (SPLIT) {
                lo[t] = (_Float16)(x - (float)hi[t]);
                stored += (float)lo[t];
            }
            nn += stored * stored;
        }
        *(half8*)(o + j) = hi;
        if (SPLIT) *(half8*)(o + dpad + j) = lo;
    }
    if (norms) {
        nn = lvs_wave_sum(nn);
        if (lane == 0) norms[row] = nn;
    }
    pack_report(bad, flags);
}

// largest |x| over a matrix as the bit pattern of a non-negative float (atomicMax on the bits; inf / NaN propagate as the
// largest patterns, so the caller sees them)
template <typename SrcT>
__global__ __launch_bounds__(256) void absmax_kernel(const SrcT* __restrict__ src, long long total, uint32_t* __restrict__ out) {
    uint32_t m = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t b = __float_as_uint(fabsf((float)src[i])) & 0x7FFFFFFFu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o, 64);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, long long ld16,
                                                          const long long* __restrict__ ids, long long n_ids,
                                                          uint4* __restrict__ dst) {
    const long long total = n_ids * ld16;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long r = i / ld16, c = i - r * ld16;
        dst[i] = src[ids[r] * ld16 + c];
    }
}

__global__ __launch_bounds__(256) void gather_f32_kernel(const float* __restrict__ src, const long long* __restrict__ ids,
                                                         long long n_ids, float* __restrict__ dst) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ids) dst[i] = src[ids[i]];
}

// k == 1: one thread per query, the best key over the parts (k-means assignment: 10 M queries, a handful of parts)
__global__ __launch_bounds__(256) void merge_top1_kernel(const u64* __restrict__ parts, int nparts, long long nq,
                                                         u64* __restrict__ out, long long out_ld) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    u64 best = 0;
    for (int p = 0; p < nparts; ++p) {
        u64 v = parts[(long long)p * nq + q];
        best = v > best ? v : best;
    }
    out[q * out_ld] = best;
}

// one wave per query: merge nparts sorted-or-not candidate lists of k keys into the best k (k <= 64)
__global__ __launch_bounds__(256) void merge_keys_kernel(const u64* __restrict__ parts, int nparts, long long nq, int k,
                                                         u64* __restrict__ out, long long out_ld,
                                                         const uint32_t* __restrict__ pred) {
    if (pred && *pred == 0u) return;  // predicated launch, see lvs_flat_search_keys
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const long long total = (long long)nparts * k;
    u64 best = 0;
    for (long long c0 = 0; c0 < total; c0 += 64) {
        long long c = c0 + lane;
        u64 v = 0;
        if (c < total) {
            long long p = c / k, j = c - p * k;
            v = parts[(p * nq + q) * k + j];
        }
        v = lvs_wave_sort_desc(v, lane);
        if (c0 == 0) {
            best = v;
        } else {
            u64 w = lvs_shfl_u64(v, 63 - lane);  // ascending copy
            best = best > w ? best : w;          // top-64 of the union, bitonic
            best = lvs_wave_bitonic_merge_desc(best, lane);
        }
    }
    if (lane < k) out[q * out_ld + lane] = best;
}

// the same merge with ONE WORKGROUP of 16 waves per query: every wave merges a sixteenth of the parts (its loads in flight
// next to the other waves'), wave 0 merges the sixteen results.  For the small-batch kernel's 64 .. 256 partial lists of a
// few dozen queries, where one wave per query left the merge (a chain of dependent loads) as long as a tenth of the scan.
__global__ __launch_bounds__(1024) void merge_keys_wide_kernel(const u64* __restrict__ parts, int nparts, long long nq, int k,
                                                               u64* __restrict__ out, long long out_ld) {
    __shared__ u64 sm[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = blockIdx.x;
    const int per = (nparts + 15) / 16;
    const int p0 = wave * per, p1 = p0 + per < nparts ? p0 + per : nparts;
    const long long total = p1 > p0 ? (long long)(p1 - p0) * k : 0;
    u64 best = 0;
    for (long long c0 = 0; c0 < total; c0 += 64) {
        const long long c = c0 + lane;
        u64 v = 0;
        if (c < total) {
            const long long p = p0 + c / k, j = c % k;
            v = parts[(p * nq + q) * k + j];
        }
        if (__builtin_amdgcn_ballot_w64(v != 0) == 0ull) continue;  // empty lists (seeded thresholds): nothing to merge
        v = lvs_wave_sort_desc(v, lane);
        const u64 w = lvs_shfl_u64(v, 63 - lane);  // ascending copy
        best = best > w ? best : w;                // top-64 of the union, bitonic
        best = lvs_wave_bitonic_merge_desc(best, lane);
    }
    sm[wave][lane] = best;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll 1
    for (int o = 1; o < 16; ++o) {
        const u64 w = sm[o][63 - lane];
        if (__builtin_amdgcn_ballot_w64(w != 0) == 0ull) continue;
        best = best > w ? best : w;
        best = lvs_wave_bitonic_merge_desc(best, lane);
    }
    if (lane < k) out[q * out_ld + lane] = best;
}

__global__ __launch_bounds__(256) void keys_to_result_kernel(const u64* __restrict__ keys, long long n, int metric,
                                                             const long long* __restrict__ id_map, float unscale,
                                                             float* __restrict__ D, long long* __restrict__ I) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 key = keys[i];
    const float FLT_MAX_ = 3.4028234663852886e38f;
    if (key == 0) {
        D[i] = metric == LVS_METRIC_IP ? -FLT_MAX_ : FLT_MAX_;
        I[i] = -1;
        return;
    }
    float better = lvs_unord32((uint32_t)(key >> 32)) * unscale;  // a power of two (operands packed with a scale): exact
    long long id = (long long)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
    D[i] = metric == LVS_METRIC_IP ? better : (0.0f - better);
    I[i] = id_map ? id_map[id] : id;
}

// certified nearest-row search: combine the slabs' (winner key, runner-up score) pairs of every query
__global__ __launch_bounds__(256) void merge_top2_kernel(const u64* __restrict__ keys, const float* __restrict__ sec,
                                                         int nslab, long long nq, u64* __restrict__ out_keys,
                                                         float* __restrict__ out_sec) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    u64 best = 0;
    for (int p = 0; p < nslab; ++p) {
        const u64 v = keys[(long long)p * nq + q];
        best = v > best ? v : best;
    }
    float s2 = -INFINITY;
    for (int p = 0; p < nslab; ++p) {
        const u64 v = keys[(long long)p * nq + q];
        const float cand = v == best ? sec[(long long)p * nq + q] : (v ? lvs_unord32((uint32_t)(v >> 32)) : -INFINITY);
        s2 = fmaxf(s2, cand);
    }
    out_keys[q] = best;
    out_sec[q] = s2;
}

// one wave per query: the exact score (fp32, hi + lo parts of both operands) of the pair (query q, row named by keys[q])
// replaces the approximate score inside the key
template <int QSPLIT, int BSPLIT>
__global__ __launch_bounds__(256) void rescore_keys_kernel(const _Float16* __restrict__ xb, long long ldb,
                                                           const _Float16* __restrict__ xq, long long ldq, int dpad,
                                                           int metric, const float* __restrict__ bn,
                                                           const float* __restrict__ qn, long long id_offset, long long nq,
                                                           int k, u64* __restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const long long slot = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // one wave per (query, rank)
    if (slot >= nq * k) return;
    const long long q = slot / k;
    const u64 key = keys[slot];
    if (key == 0) return;
    const uint32_t id = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    const long long row = (long long)id - id_offset;
    const _Float16* qr = xq + q * ldq;
    const _Float16* br = xb + row * ldb;
    const float acc = lvs_exact_dots<QSPLIT, BSPLIT, 1>(qr, br, nullptr, dpad, lane).a;
    if (lane == 0) {
        float better = acc;
        if (metric == LVS_METRIC_L2) better = lvs_l2_score(qn[q], bn[row], acc);
        keys[slot] = lvs_pack_key(better, id);
    }
}

// one wave per query: keys[q][0..k) sorted descending in place (k <= 64)
__global__ __launch_bounds__(256) void sort_keys_kernel(u64* __restrict__ keys, long long nq, int k) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;
    u64 v = lane < k ? keys[q * k + lane] : 0ull;
    v = lvs_wave_sort_desc(v, lane);
    if (lane < k) keys[q * k + lane] = v;
}

// Certificate of a one-pass ("hi" parts only) top-k search with k1 > k list slots:
//   approx [nq][k1]: the one-pass keys, best first;  exact [nq][k1]: the same candidates rescored exactly and re-sorted.
// A row outside the candidate list has a one-pass score <= the list's last one-pass score s_min, hence an exact score
// <= s_min + bound(q); if the k-th exact score of the candidates is STRICTLY above that, the candidates' exact top k is the
// exact top k.  Queries that fail the test are appended to out_idx.  An unfilled list (fewer than k1 rows) holds every row.
__global__ __launch_bounds__(256) void certify_topk_kernel(const u64* __restrict__ approx, const u64* __restrict__ exact,
                                                           const float* __restrict__ qn, long long nq, int k1, int k,
                                                           float scale, float slack, float band,
                                                           long long* __restrict__ out_idx,
                                                           unsigned long long* __restrict__ out_count) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool open = false;
    if (q < nq) {
        const u64 last = approx[q * k1 + k1 - 1];
        const u64 kth = exact[q * k1 + k - 1];
        const float bound = scale * sqrtf(qn ? qn[q] : 1.0f) + slack;
        if (band > 0.f) {
            // banded list: a row outside it scored below max(last slot, k-th one-pass score - band * bound) when it was
            // turned away (both only rise during the search); an unfilled list no longer means "every row is here"
            const u64 akth = approx[q * k1 + k - 1];
            if (kth != 0 && akth != 0) {
                float s_min = lvs_unord32((uint32_t)(akth >> 32)) - band * bound;
                if (last != 0) s_min = fmaxf(s_min, lvs_unord32((uint32_t)(last >> 32)));
                open = !(lvs_unord32((uint32_t)(kth >> 32)) > s_min + bound);
            }
        } else if (last != 0 && kth != 0) {
            const float s_min = lvs_unord32((uint32_t)(last >> 32));
            const float s_k = lvs_unord32((uint32_t)(kth >> 32));
            open = !(s_k > s_min + bound);
        }
    }
    const unsigned long long m = __ballot(open);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(out_count, (unsigned long long)__popcll(m));
    base = lvs_shfl_u64(base, 0);
    if (open) out_idx[base + __popcll(m & ((1ull << lane) - 1ull))] = q;
}

// queries whose winner is NOT certified by its margin: (best score - runner-up score) <= scale * |q| + slack.
// Their indices are appended to out_idx (order unspecified), *out_count counts them.
// With `stats` (device: [0] = R^2 largest squared row norm, [1] = E^2 largest squared lo-part norm of the corpus rows) the
// bound is (coef[0] E + coef[1] R) |q| + coef[2] + coef[3] R + coef[4] R^2 - the k-means loop keeps those statistics on the
// device (lvs_kmeans_update_centroids) so that no iteration waits for the host; without it: scale |q| + slack.
// One workgroup owns `per_block` consecutive queries (lvs_append_lists).
__global__ __launch_bounds__(256) void margin_select_kernel(const u64* __restrict__ keys, const float* __restrict__ sec,
                                                            const float* __restrict__ qn, long long nq, float scale,
                                                            float slack, const float* __restrict__ stats, LvsBoundCoef coef,
                                                            long long per_block, long long* __restrict__ out_idx,
                                                            unsigned long long* __restrict__ out_count) {
    if (stats) {
        const LvsBound b(coef, stats);
        scale = b.scale();
        slack = b.slack();
    }
    auto is_open = [&](long long q) -> int {
        const u64 kq = keys[q];
        if (!kq) return 0;
        const float best = lvs_unord32((uint32_t)(kq >> 32));
        const float bound = scale * sqrtf(qn ? qn[q] : 1.0f) + slack;
        return !((best - sec[q]) > bound);  // also true for NaN / inf - inf: never certify what cannot be compared
    };
    long long* const out[1] = {out_idx};
    lvs_append_lists<1>(per_block, nq, is_open, is_open, out, out_count);
}

}  // namespace

extern "C" int32_t lvs_pack_rows(const void* src, int32_t src_dtype, int64_t n, int32_t d, int32_t pack_mode,
                                 int32_t normalize, void* dst, float* out_norms_sq, void* stream) {
    return lvs_pack_rows_checked(src, src_dtype, n, d, pack_mode, normalize, 0, dst, out_norms_sq, nullptr, stream);
}

extern "C" int32_t lvs_pack_rows_checked(const void* src, int32_t src_dtype, int64_t n, int32_t d, int32_t pack_mode,
                                         int32_t normalize, int32_t scale_exp, void* dst, float* out_norms_sq,
                                         uint32_t* out_flags, void* stream) {
    LVS_REQUIRE(scale_exp >= -100 && scale_exp <= 100, "scale_exp %d out of range", scale_exp);
    const float pw = ldexpf(1.0f, scale_exp);
    LVS_REQUIRE(n >= 0 && d > 0, "bad shape n=%lld d=%d", (long long)n, d);
    LvsLayout l;
    LVS_REQUIRE(lvs_layout(d, pack_mode, pack_mode, false, l) == LVS_OK, "bad pack_mode %d", pack_mode);
    LVS_REQUIRE(src_dtype == LVS_DTYPE_F32 || src_dtype == LVS_DTYPE_F16, "bad src_dtype %d", src_dtype);
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(src && dst, "NULL buffer");
    const int dpad = l.dpad;
    LVS_DEVICE_GUARD(stream);
    dim3 block(256), grid((unsigned)lvs_ceil_div(n, 4));
    hipStream_t st = (hipStream_t)stream;
    const bool split = pack_mode == LVS_PACK_SPLIT;
    const bool vec = d % 8 == 0 && ((uintptr_t)src & 15) == 0;  // every source row 16-byte aligned
    _Float16* o = (_Float16*)dst;
    if (vec && src_dtype == LVS_DTYPE_F32 && split)
        hipLaunchKernelGGL((pack_rows_vec_kernel<float, 1>), grid, block, 0, st, (const float*)src, (long long)n, d,
                           dpad, normalize, pw, o, out_norms_sq, out_flags);
    else if (vec && src_dtype == LVS_DTYPE_F32)
        hipLaunchKernelGGL((pack_rows_vec_kernel<float, 0>), grid, block, 0, st, (const float*)src, (long long)n, d,
                           dpad, normalize, pw, o, out_norms_sq, out_flags);
    else if (vec && split)
        hipLaunchKernelGGL((pack_rows_vec_kernel<_Float16, 1>), grid, block, 0, st, (const _Float16*)src, (long long)n,
                           d, dpad, normalize, pw, o, out_norms_sq, out_flags);
    else if (vec)
        hipLaunchKernelGGL((pack_rows_vec_kernel<_Float16, 0>), grid, block, 0, st, (const _Float16*)src, (long long)n,
                           d, dpad, normalize, pw, o, out_norms_sq, out_flags);
    else if (src_dtype == LVS_DTYPE_F32)
        hipLaunchKernelGGL(pack_rows_kernel<float>, grid, block, 0, st, (const float*)src, (long long)n, d, dpad,
                           split, normalize, pw, o, out_norms_sq, out_flags);
    else
        hipLaunchKernelGGL(pack_rows_kernel<_Float16>, grid, block, 0, st, (const _Float16*)src, (long long)n, d,
                           dpad, split, normalize, pw, o, out_norms_sq, out_flags);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_absmax(const void* src, int32_t src_dtype, int64_t n, int32_t d, uint32_t* inout_bits, void* stream) {
    LVS_REQUIRE(n >= 0 && d > 0 && inout_bits, "bad arguments");
    LVS_REQUIRE(src_dtype == LVS_DTYPE_F32 || src_dtype == LVS_DTYPE_F16, "bad src_dtype %d", src_dtype);
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(src, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    const long long total = (long long)n * d;
    const unsigned grid = (unsigned)(lvs_ceil_div(total, 256 * 8) < 4096 ? lvs_ceil_div(total, 256 * 8) : 4096);
    if (src_dtype == LVS_DTYPE_F32)
        hipLaunchKernelGGL(absmax_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)src, total, inout_bits);
    else
        hipLaunchKernelGGL(absmax_kernel<_Float16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)src, total,
                           inout_bits);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_gather_rows(const void* src, int32_t ld, const int64_t* ids, int64_t n_ids, void* dst,
                                   void* stream) {
    LVS_REQUIRE(ld > 0 && ld % 8 == 0, "ld must be a positive multiple of 8 halfs");
    if (n_ids == 0) return LVS_OK;
    LVS_REQUIRE(src && ids && dst && n_ids > 0, "bad arguments");
    LVS_DEVICE_GUARD(stream);
    long long ld16 = ld / 8;
    long long total = n_ids * ld16;
    unsigned grid = (unsigned)(lvs_ceil_div(total, 256) < 16384 ? lvs_ceil_div(total, 256) : 16384);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, ld16,
                       (const long long*)ids, (long long)n_ids, (uint4*)dst);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_gather_f32(const float* src, const int64_t* ids, int64_t n_ids, float* dst, void* stream) {
    if (n_ids == 0) return LVS_OK;
    LVS_REQUIRE(src && ids && dst && n_ids > 0, "bad arguments");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)lvs_ceil_div(n_ids, 256)), dim3(256), 0,
                       (hipStream_t)stream, src, (const long long*)ids, (long long)n_ids, dst);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------------------------------
namespace {
// (layout, tile geometry, route and workspace of a call: lvs_plan.h)
// The plan-derived fields of a tile-kernel launch over rows xb[0, nb) and queries xq[0, nq); every other field is zero, for
// the caller to set those of its mode (outputs, k, thresholds, pairs).
void tile_args(LvsTileArgs& a, const LvsLayout& l, const LvsTileGeom& g, const void* xb, const void* xq, const float* bn, const float* qn, int64_t nb,
               int64_t nq, int32_t metric, int64_t id_offset) {
    memset(&a, 0, sizeof(a));
    a.xb = xb;
    a.xq = xq;
    a.bn = bn;
    a.qn = qn;
    a.nb = nb;
    a.nq = nq;
    a.ldb = l.ldb;
    a.ldq = l.ldq;
    a.nseg = l.nseg;
    for (int i = 0; i < 3; ++i) {
        a.seg_q[i] = l.seg_q[i];
        a.seg_c[i] = l.seg_c[i];
    }
    a.nkd = l.nkd;
    a.nk = l.nk;
    a.metric = metric;
    a.ntiles = g.ntiles;
    a.tiles_per_slab = g.tiles_per_slab;
    a.nslab = g.nslab;
    a.nqt = g.nqt;
    a.bq = g.v2 ? LVS2_BQ : LVS3_BQ;
    a.gq = g.gq;
    a.lead_slabs = g.lead_slabs;
    a.id_offset = id_offset;
}

// LVS_MODE_SEED over the corpus' first `tiles` tiles: one tile per slab, 256-query tiles, whatever the plan said
void seed_tile_geometry(LvsTileArgs& a, int tiles) {
    a.nb = (int64_t)tiles * LVS_BC;
    a.ntiles = a.nslab = tiles;
    a.tiles_per_slab = 1;
    a.nqt = (int)lvs_ceil_div(a.nq, LVS2_BQ);
    a.bq = LVS2_BQ;
    a.gq = 1;
    a.lead_slabs = 0;
    a.k = 1;
}

// One workgroup per query: n candidate keys src[q * stride_q + (i / inner) * stride_outer + (i % inner)], i < n, are
// sorted descending (bitonic, in LDS, P2 = power of two >= n slots) and the k-th largest (kth_out[q]; 0 when n < k)
// and/or the k largest (topk_out[q * out_ld + 0..k)) are written.  With counts != NULL, n = min(counts[q], n_max) and
// *overflow is set when some counts[q] > n_max (candidates were dropped by the producer).
__global__ __launch_bounds__(256) void select_keys_kernel(const u64* __restrict__ src, long long stride_q, int inner,
                                                          long long stride_outer, int n_max,
                                                          const uint32_t* __restrict__ counts, int k, int P2,
                                                          u64* __restrict__ kth_out, u64* __restrict__ topk_out,
                                                          long long out_ld, uint32_t* __restrict__ overflow) {
    extern __shared__ __attribute__((aligned(16))) char sel_smem[];
    u64* sk = (u64*)sel_smem;
    const long long q = blockIdx.x;
    int n = n_max;
    if (counts) {
        uint32_t c = counts[q];
        if (c > (uint32_t)n_max) {
            if (threadIdx.x == 0 && overflow) atomicOr(overflow, 1u);
            c = (uint32_t)n_max;
        }
        n = (int)c;
    }
    const u64* base = src + q * stride_q;
    for (int i = threadIdx.x; i < P2; i += 256) {
        u64 v = 0;
        if (i < n) v = base[(long long)(i / inner) * stride_outer + (i % inner)];
        sk[i] = v;
    }
    __syncthreads();
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < P2; i += 256) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool desc = (i & size) == 0;  // the last merge (size == P2) is descending everywhere
                    const u64 x = sk[i], y = sk[j];
                    if ((x < y) == desc) {
                        sk[i] = y;
                        sk[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (kth_out && threadIdx.x == 0) kth_out[q] = k <= P2 ? sk[k - 1] : 0;
    if (topk_out)
        for (int j = threadIdx.x; j < k; j += 256) topk_out[q * out_ld + j] = j < P2 ? sk[j] : 0;
}

hipError_t launch_select(const u64* src, long long stride_q, int inner, long long stride_outer, int n_max,
                         const uint32_t* counts, int k, u64* kth_out, u64* topk_out, long long out_ld, uint32_t* overflow,
                         int64_t nq, hipStream_t st) {
    const int P2 = pow2_ceil(n_max < 2 ? 2 : n_max);
    hipLaunchKernelGGL(select_keys_kernel, dim3((unsigned)nq), dim3(256), (size_t)P2 * 8, st, src, stride_q, inner,
                       stride_outer, n_max, counts, k, P2, kth_out, topk_out, out_ld, overflow);
    return hipGetLastError();
}

// One workgroup per query: out[q][0..k) = the k largest of {acc[q][0..k) if acc} U {parts[p][q][0..k) : p0 <= p < p0 + np}
// (bitonic sort of P2 >= (np + (acc != 0)) * k slots in LDS).  acc may alias out: every input of the query is in LDS
// before the first result is written.
__global__ __launch_bounds__(256) void merge_long_kernel(const u64* __restrict__ parts, int p0, int np,
                                                         const u64* acc, long long nq, int k, int P2, u64* out) {
    extern __shared__ __attribute__((aligned(16))) char sel_smem[];
    u64* sk = (u64*)sel_smem;
    const long long q = blockIdx.x;
    const int nacc = acc ? k : 0;
    const int n = nacc + np * k;
    for (int i = threadIdx.x; i < P2; i += 256) {
        u64 v = 0;
        if (i < nacc) {
            v = acc[q * k + i];
        } else if (i < n) {
            const int c = i - nacc, p = c / k, j = c - p * k;
            v = parts[((long long)(p0 + p) * nq + q) * k + j];
        }
        sk[i] = v;
    }
    __syncthreads();
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < P2; i += 256) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool desc = (i & size) == 0;
                    const u64 x = sk[i], y = sk[j];
                    if ((x < y) == desc) {
                        sk[i] = y;
                        sk[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int j = threadIdx.x; j < k; j += 256) out[q * k + j] = sk[j];
}

hipError_t launch_merge_long(const u64* parts, int p0, int np, const u64* acc, int64_t nq, int k, u64* out,
                             hipStream_t st) {
    const int n = (np + (acc ? 1 : 0)) * k;
    const int P2 = pow2_ceil(n < 2 ? 2 : n);
    if (P2 > LVS_SELECT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(merge_long_kernel, dim3((unsigned)nq), dim3(256), (size_t)P2 * 8, st, parts, p0, np, acc,
                       (long long)nq, k, P2, out);
    return hipGetLastError();
}

// Seed of the small-batch kernel's shared thresholds: gtau[q] = order key of the k-th largest of the nparts values
// seeds[p][q] (the best score of query q over the sample rows of corpus range p; lvs_stream_kernel<.., SEED>), 0 when fewer
// than k ranges saw a row.  One wave per query: 64 values at a time are sorted across the lanes and folded into the running
// top 64 (k <= 56).  Every value is a real row's score, and the k-th largest of a subset never exceeds the k-th largest of
// all rows: a valid lower bound of the final k-th best score, so the seeded search stays exact.
// Banded lists (kc > 0, qn given): the larger of that and (kc-th largest - the query's band) - equally a lower bound of what
// the kernel's own admission rule ends at.
__global__ __launch_bounds__(256) void seed_kth_kernel(const float* __restrict__ seeds, int nparts, long long nq, int k,
                                                       uint32_t* __restrict__ gtau, int kc = 0, const float* __restrict__ qn = nullptr,
                                                       float bscale = 0.f, float bslack = 0.f) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;
    u64 best = 0;
    for (int p0 = 0; p0 < nparts; p0 += 64) {
        const int p = p0 + lane;
        u64 v = 0;
        if (p < nparts) {
            const float sc = seeds[(long long)p * nq + q];
            if (sc > -INFINITY) v = (u64)lvs_ord32(sc) << 32;  // -inf: that range saw no row
        }
        v = lvs_wave_sort_desc(v, lane);
        if (p0 == 0) {
            best = v;
        } else {
            const u64 w = lvs_shfl_u64(v, 63 - lane);
            best = best > w ? best : w;
            best = lvs_wave_bitonic_merge_desc(best, lane);
        }
    }
    uint32_t kth = (uint32_t)(lvs_shfl_u64(best, k - 1) >> 32);
    if (kc > 0 && qn) {
        const uint32_t kcth = (uint32_t)(lvs_shfl_u64(best, kc - 1) >> 32);
        if (kcth) {
            const uint32_t ob = lvs_ord32(lvs_unord32(kcth) - (bscale * sqrtf(qn[q]) + bslack));
            kth = ob > kth ? ob : kth;
        }
    }
    if (lane == 0) gtau[q] = kth;
}

__global__ __launch_bounds__(256) void fill_f32_kernel(float* __restrict__ dst, long long n, float v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}

__global__ void copy_pass_kernel(const u64* __restrict__ src, long long nq, int kp, u64* __restrict__ dst, int k,
                                 int col0, const uint32_t* __restrict__ pred) {
    if (pred && *pred == 0u) return;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * kp) return;
    long long q = i / kp;
    int j = (int)(i - q * kp);
    if (col0 + j < k) dst[q * k + col0 + j] = src[i];
}

// gtau[q] = order key of the k-th largest of seeds[p][q], p < nparts, for every query q < nq (seed_kth_kernel)
hipError_t launch_seed_kth(const float* seeds, int nparts, int64_t nq, int k, uint32_t* gtau, hipStream_t st, int kc = 0,
                           const float* qn = nullptr, float bscale = 0.f, float bslack = 0.f) {
    hipLaunchKernelGGL(seed_kth_kernel, dim3((unsigned)lvs_ceil_div(nq, 4)), dim3(256), 0, st, seeds, nparts, (long long)nq, k,
                       gtau, kc, qn, bscale, bslack);
    return hipGetLastError();
}

// out[q * out_ld + 0..k) = the best k keys of the nparts partial lists [nparts][nq][k] of every query q < nq.  wide: one
// workgroup of 16 waves per query (merge_keys_wide_kernel, never predicated); else one wave per query (merge_keys_kernel).
hipError_t launch_merge(bool wide, const u64* parts, int nparts, int64_t nq, int k, u64* out, long long out_ld,
                        const uint32_t* pred, hipStream_t st) {
    if (wide)
        hipLaunchKernelGGL(merge_keys_wide_kernel, dim3((unsigned)nq), dim3(1024), 0, st, parts, nparts, (long long)nq, k, out,
                           out_ld);
    else
        hipLaunchKernelGGL(merge_keys_kernel, dim3((unsigned)lvs_ceil_div(nq, 4)), dim3(256), 0, st, parts, nparts,
                           (long long)nq, k, out, out_ld, pred);
    return hipGetLastError();
}

// What a flat search does beyond its operands (the lvs_flat_search_keys variants)
struct SearchOpts {
    bool hi_only = false;  // lvs_flat_search_keys_hi: planned over the fp16 "hi" parts only (one K segment whatever the pack modes)
    // lvs_flat_search_keys_hi_banded: list slots beyond a per-query band below the kc-th best stay empty (LvsTileArgs::kc)
    int kc = 0;
    float bscale = 0.f, bslack = 0.f;
    // lvs_flat_search_keys_seeded (nullable): [ext_rows][nq] scores of real rows of the SEARCHED SET (any shard of it, e.g. the
    // all-gathered sample maxima of every corpus shard of a multi-GPU join, lvs_flat_search_seed_scores): the k-th largest per
    // query replaces the launch's own sample pass as its starting threshold.
    const float* ext_seeds = nullptr;
    int32_t ext_rows = 0;
};

// One flat-search call as its paths see it: the checked arguments, the plan and the workspace carved by it
struct SearchCall {
    const void* xb;
    const void* xq;
    const float* bn;  // [nb] |y|^2 (L2 only)
    const float* qn;  // [nq] |q|^2 (L2 only)
    int64_t nb, nq, id_offset;
    int32_t d, metric, k, xb_pack, xq_pack;
    const uint32_t* row_ids;
    u64* out_keys;  // [nq][k]
    hipStream_t st;
    SearchOpts o;
    LvsFlatPlan p;
    char* ws;  // laid out by p.w
    int64_t ws_bytes;
    uint32_t* gtau;  // ws + p.w.off_gtau
};

// a tile launch of the search over its whole corpus and all its queries, on geometry g
void search_tile_args(LvsTileArgs& a, const SearchCall& sc, const LvsTileGeom& g, uint32_t* gtau, u64* out) {
    tile_args(a, sc.p.l, g, sc.xb, sc.xq, sc.bn, sc.qn, sc.nb, sc.nq, sc.metric, sc.id_offset);
    a.row_ids = sc.row_ids;
    a.gtau = gtau;
    a.out = out;
    a.debug_hot = (int)lvs_tune("LVS_DEBUG_HOT", 0);
}

// ---- k > LVS_KPASS: two corpus passes whatever k is (see make_two_phase_plan).  A bucket overflow (mass ties, or the top k
// clustered in one slab) sets a device-side flag; the selection passes then run PREDICATED on that flag (their kernels return
// at once when it is clear), so the call never synchronises the stream.  *pred = that flag, or NULL when the two phases did
// not run (no two-phase plan, or a workspace too small for it).
int32_t search_two_phase(const SearchCall& sc, const uint32_t** pred) {
    *pred = nullptr;
    const int64_t nq = sc.nq;
    const int k = sc.k;
    hipStream_t st = sc.st;
    TwoPhasePlan tp;
    if (!make_two_phase_plan(nq, sc.nb, k, tp) || tp.total > sc.ws_bytes)
        return LVS_OK;
    char* ws = sc.ws;
    uint32_t* gtau2 = (uint32_t*)(ws + tp.off_gtau);
    u64* lists = (u64*)(ws + tp.off_lists);        // [nslab][nq][slots]
    u64* thr = (u64*)(ws + tp.off_thr);            // [nq]
    uint32_t* cnt = (uint32_t*)(ws + tp.off_cnt);  // [nq]
    uint32_t* flag = (uint32_t*)ws;                // status word 0: some bucket overflowed
    u64* bucket = (u64*)(ws + tp.off_bucket);      // [nq][capacity]
    LvsTileArgs ta;
    search_tile_args(ta, sc, tp.a, gtau2, lists);
    ta.k = tp.slots;
    ta.no_share = 1;  // the bound needs every slab's own top list, not lists pruned by other slabs' thresholds
    LVS_HIP_CHECK(lvs_zero_async(gtau2, (size_t)nq * 4, st));
    LVS_HIP_CHECK(lvs_zero_async(cnt, (size_t)nq * 4, st));
    LVS_HIP_CHECK(lvs_zero_async(flag, 4, st));
    {
        ScopedKernelTimer timer(st);
        LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_TOPK, ta, st));
    }
    // T[q] = k-th largest of the nslab * slots listed keys (element (slab, j) of query q at (slab * nq + q) * slots + j)
    LVS_HIP_CHECK(launch_select(lists, tp.slots, tp.slots, (long long)nq * tp.slots, tp.a.nslab * tp.slots, nullptr, k, thr,
                                nullptr, 0, nullptr, nq, st));
    LvsTileArgs tb;
    search_tile_args(tb, sc, tp.b, gtau2, lists);
    tb.k = 1;
    tb.thr_key = thr;
    tb.bucket_count = cnt;
    tb.bucket = bucket;
    tb.bucket_capacity = tp.capacity;
    LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_COLLECT, tb, st));
    LVS_HIP_CHECK(launch_select(bucket, tp.capacity, tp.capacity, 0, tp.capacity, cnt, k, nullptr, sc.out_keys, k, flag, nq, st));
    *pred = flag;
#ifdef LVS_TUNING
    if (lvs_tune_set("LVS_TWO_PHASE_DEBUG")) {  // bucket statistics of this call (synchronises)
        std::vector<uint32_t> h((size_t)nq);
        uint32_t overflowed = 0;
        LVS_HIP_CHECK(hipStreamSynchronize(st));
        LVS_HIP_CHECK(hipMemcpy(&overflowed, flag, 4, hipMemcpyDeviceToHost));
        LVS_HIP_CHECK(hipMemcpy(h.data(), cnt, (size_t)nq * 4, hipMemcpyDeviceToHost));
        uint32_t mn = ~0u, mx = 0;
        double sum = 0;
        for (uint32_t v : h) {
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            sum += v;
        }
        fprintf(stderr, "[lvs] two-phase k=%d slots=%d slabs=%d capacity=%d: bucket counts min %u mean %.1f max %u overflow=%u\n",
                k, tp.slots, tp.a.nslab, tp.capacity, mn, sum / (double)nq, mx, overflowed);
    }
#endif
    return LVS_OK;
}

// ---- lvs_rq_kernel / lvs_rj_kernel, one launch per chunk of queries (rq_chunk_size): a query belongs to one chunk, so every
// chunk is a complete search of its own (own seeds, own lists, own merge - or, with one list per query, no merge: a launch of
// lvs_rj_kernel with ONE corpus range and no nb % 32 tail rows writes [1][cn][k] = the chunk's [cn][k] of out_keys itself; a
// one-part merge_keys_kernel is a plain copy of a sorted, zero-padded list) ----
int32_t search_rq_chunks(const SearchCall& sc, bool rq_join) {
    const LvsLayout& p = sc.p.l;
    const int64_t nq = sc.nq, nb = sc.nb;
    const int k = sc.k;
    hipStream_t st = sc.st;
    uint32_t* gtau = sc.gtau;
    u64* partial = (u64*)(sc.ws + sc.p.w.off_parts);
    float* seeds = (float*)(sc.ws + sc.p.w.off_seeds);  // [ranges][<= 4 096]
    const bool rq_ext_seeds = sc.o.ext_seeds && sc.o.ext_rows >= k;
    if (rq_join && rq_ext_seeds)  // the k-th largest of the caller's sample scores, for every query of the call at once
        LVS_HIP_CHECK(launch_seed_kth(sc.o.ext_seeds, (int)sc.o.ext_rows, nq, k, gtau, st));
    const int64_t chunk = rq_chunk_size(lvs_tune("LVS_RQ_CHUNK", LVS_RQ_CHUNK_DEFAULT));
    for (int64_t c0 = 0, cn = 0; c0 < nq; c0 += cn) {
        cn = rq_chunk_len(nq - c0, chunk);
        LvsRqArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.xb = sc.xb;
        ra.xq = (const _Float16*)sc.xq + c0 * p.ldq;
        ra.bn = sc.bn;
        ra.qn = sc.qn ? sc.qn + c0 : nullptr;
        ra.row_ids = sc.row_ids;
        ra.gtau = gtau + c0;
        ra.out = partial;
        ra.nb = nb;
        ra.ldb = p.ldb;
        ra.ldq = p.ldq;
        ra.id_offset = sc.id_offset;
        ra.nq = (int)cn;
        ra.k = k;
        ra.metric = sc.metric;
        const int64_t sample = lvs_rq_sample_rows(nb, cn);  // thresholds seeded from the kernel's own SEED mode over these rows
        if (rq_join && rq_ext_seeds) {
            // seeded above
        } else if (sample > 0) {
            // (the k-th largest of one maximum per corpus range needs >= k ranges: the sample pass keeps launches of <= 16 groups)
            for (int64_t s0 = 0; s0 < cn; s0 += LVS_RQ_MAXQ) {
                const int64_t sn = cn - s0 < LVS_RQ_MAXQ ? cn - s0 : LVS_RQ_MAXQ;
                LvsRqArgs rs = ra;
                rs.xq = (const _Float16*)ra.xq + s0 * p.ldq;
                rs.qn = ra.qn ? ra.qn + s0 : nullptr;
                rs.gtau = ra.gtau + s0;
                rs.nq = (int)sn;
                rs.nb = sample;
                rs.seed_out = seeds;
                LVS_HIP_CHECK(lvs_rq_launch(rs, p.dpad, st));
                LVS_HIP_CHECK(launch_seed_kth(seeds, rs.nparts, sn, k, gtau + c0 + s0, st));  // writes every gtau[q] of the piece
            }
        } else {
            LVS_HIP_CHECK(lvs_zero_async(gtau + c0, (size_t)cn * 4, st));
        }
        const int kernel = lvs_rq_chunk_kernel(cn, nb, p.dpad, k, sc.row_ids != nullptr);
        if (kernel != LVS_CHUNK_RQ) {
            if (kernel == LVS_CHUNK_RJ_SOLO) {
                ra.out = sc.out_keys + c0 * k;
                ScopedKernelTimer timer(st, LVS_KERNEL_RJ, c0 > 0);
                LVS_HIP_CHECK(lvs_rj_launch(ra, p.dpad, st));
                continue;
            }
            {
                ScopedKernelTimer timer(st, LVS_KERNEL_RJ, c0 > 0);
                LVS_HIP_CHECK(lvs_rj_launch(ra, p.dpad, st));
            }
            const int64_t nb_full = nb / 32 * 32;
            if (nb_full < nb) {
                LvsRqArgs rt = ra;
                rt.xb = (const char*)sc.xb + nb_full * p.ldb * 2;
                rt.bn = sc.bn ? sc.bn + nb_full : nullptr;
                rt.nb = nb - nb_full;
                rt.id_offset = sc.id_offset + nb_full;
                rt.out = partial + (int64_t)ra.nparts * cn * k;
                LVS_HIP_CHECK(lvs_rq_launch(rt, p.dpad, st));
                ra.nparts += rt.nparts;
            }
        } else {
            ScopedKernelTimer timer(st, LVS_KERNEL_RQ, c0 > 0);
            LVS_HIP_CHECK(lvs_rq_launch(ra, p.dpad, st));
        }
        LVS_HIP_CHECK(launch_merge(ra.nparts >= 16, partial, ra.nparts, cn, k, sc.out_keys + c0 * k, k, nullptr, st));
    }
    return LVS_OK;
}

// ---- lvs_stream_kernel: stream the corpus once, queries resident in LDS ----
int32_t search_stream(const SearchCall& sc, const LvsStreamShape& sh) {
    const LvsLayout& p = sc.p.l;
    const int64_t nq = sc.nq, nb = sc.nb;
    const int k = sc.k;
    hipStream_t st = sc.st;
    uint32_t* gtau = sc.gtau;
    u64* partial = (u64*)(sc.ws + sc.p.w.off_parts);
    const int jper = p.dpad / 16;
    LvsStreamArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.xb = sc.xb;
    sa.xq = sc.xq;
    sa.bn = sc.bn;
    sa.qn = sc.qn;
    sa.row_ids = sc.row_ids;
    sa.gtau = gtau;
    sa.out = partial;
    sa.nb = nb;
    sa.ldb = p.ldb;
    sa.ldq = p.ldq;
    sa.id_offset = sc.id_offset;
    sa.nq = (int)nq;
    sa.k = k;
    sa.metric = sc.metric;
    sa.jper = jper;
    sa.nseg = p.nseg;
    sa.nj = p.nseg * jper;
    sa.nbfrag = sh.nbfrag;
    sa.kcap = sh.kcap;
    sa.nqb = sh.nqb;
    sa.groups = sh.groups;
    for (int i = 0; i < 3; ++i) {
        sa.seg_q[i] = p.seg_q[i];
        sa.seg_c[i] = p.seg_c[i];
        sa.seg_b[i] = p.seg_q[i] == 0 ? 0 : jper;
    }
    const int64_t sample = lvs_stream_sample_rows(nq, nb);  // seeded thresholds: the kernel's own SEED mode over these rows
    if (sample > 0) {
        float* seeds = (float*)(sc.ws + sc.p.w.off_seeds);  // [ranges][nq]
        LvsStreamArgs ss = sa;
        ss.nb = sample;
        ss.seed_out = seeds;
        LVS_HIP_CHECK(lvs_stream_launch(ss, st));
        LVS_HIP_CHECK(launch_seed_kth(seeds, ss.nparts, nq, k, gtau, st));  // writes every gtau[q]
    } else {
        LVS_HIP_CHECK(lvs_zero_async(gtau, (size_t)nq * 4, st));
    }
    {
        ScopedKernelTimer timer(st, LVS_KERNEL_STREAM);
        LVS_HIP_CHECK(lvs_stream_launch(sa, st));
    }
    LVS_HIP_CHECK(launch_merge(sa.nparts >= 16 && k <= 64, partial, sa.nparts, nq, k, sc.out_keys, k, nullptr, st));
    return LVS_OK;
}

// ---- the list kernel (lvs_tile.hip): ceil(k / LVS_KPASS) passes of per-slab lists and their merge; pred (nullable): every
// launch is a no-op unless *pred != 0 (the fallback of the two-phase search) ----
int32_t search_list_passes(const SearchCall& sc, const uint32_t* pred) {
    const LvsTileGeom& p = sc.p.g;
    const LvsWorkspace& w = sc.p.w;
    const int64_t nq = sc.nq;
    const int k = sc.k;
    hipStream_t st = sc.st;
    uint32_t* gtau = sc.gtau;
    u64* partial = (u64*)(sc.ws + w.off_partial);
    u64* passbuf = (u64*)(sc.ws + w.off_pass);
    LvsTileArgs a;
    search_tile_args(a, sc, p, gtau, partial);
    a.pred = pred;
    unsigned long long* dbg_counters = nullptr;
#if defined(LVS_COUNT_EVENTS) && defined(LVS_TUNING)
    if (lvs_tune("LVS_COUNT", 0)) {  // tuning build only: count slow-path events of this call (allocates, synchronises)
        LVS_HIP_CHECK(hipMalloc((void**)&dbg_counters, 8 * sizeof(unsigned long long)));
        LVS_HIP_CHECK(hipMemsetAsync(dbg_counters, 0, 8 * sizeof(unsigned long long), st));
        a.dbg = dbg_counters;
    }
#endif
    // k == 1: the list-free per-lane running best (TOP1) wins on short streams (k-means assignment: a few corpus tiles
    // per query, nearly every block improves some lane's best); on long streams the threshold filter of the list
    // kernel skips almost every block, so k = 1 goes through it like any other k.  Same winner either way
    // (best score, lowest row among equals).
    bool use_top1 = k == 1 && !sc.row_ids && p.tiles_per_slab <= 64;
    if (lvs_tune_set("LVS_TOP1")) use_top1 = k == 1 && !sc.row_ids && lvs_tune("LVS_TOP1", 0) != 0;  // -DLVS_TUNING only
    for (int pass = 0; pass < w.npass; ++pass) {
        const int col0 = pass * w.kpass;
        const int kp = (k - col0) < w.kpass ? (k - col0) : w.kpass;
        a.k = kp;
        // pass > 0: only keys strictly below the last key of the previous pass take part
        a.ub = pass == 0 ? nullptr : sc.out_keys + (col0 - 1);
        a.ub_stride = k;
        const bool banded = sc.o.kc > 0 && sc.o.kc < kp && w.npass == 1 && !pred && !use_top1 && sc.qn;
        a.kc = banded ? sc.o.kc : 0;
        a.bscale = banded ? sc.o.bscale : 0.f;
        a.bslack = banded ? sc.o.bslack : 0.f;
        const bool seedable = pass == 0 && w.npass == 1 && !pred && !use_top1;
        const int seed_tiles = seedable ? tile_seed_tiles(nq, sc.nb, kp) : 0;
        if (seedable && sc.o.ext_seeds && sc.o.ext_rows >= kp) {  // the caller's pooled sample scores (every shard's sample)
            LVS_HIP_CHECK(launch_seed_kth(sc.o.ext_seeds, (int)sc.o.ext_rows, nq, kp, gtau, st, a.kc, sc.qn, a.bscale,
                                          a.bslack));  // writes every gtau[q]
        } else if (seed_tiles > 0) {  // thresholds seeded from a sample instead of cold starts (tile_seed_tiles)
            float* seeds = (float*)(sc.ws + w.off_tile_seeds);
            LvsTileArgs sd = a;
            seed_tile_geometry(sd, seed_tiles);
            sd.kc = 0;
            sd.ub = nullptr;
            sd.seed_out = seeds;
            LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_SEED, sd, st));
            LVS_HIP_CHECK(launch_seed_kth(seeds, sd.nslab, nq, kp, gtau, st, a.kc, sc.qn, a.bscale, a.bslack));  // writes every gtau[q]
        } else {
            LVS_HIP_CHECK(lvs_zero_async(gtau, (size_t)nq * 4, st));
        }
        if (pred) {  // predicated fallback pass: not a measurement of the dominant kernel
            LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_TOPK, a, st));
        } else {
            ScopedKernelTimer timer(st);
            LVS_HIP_CHECK(lvs_tile_launch(use_top1 ? LVS_MODE_TOP1 : LVS_MODE_TOPK, a, st));
        }
        if (w.npass == 1 && kp == 1) {
            hipLaunchKernelGGL(merge_top1_kernel, dim3((unsigned)lvs_ceil_div(nq, 256)), dim3(256), 0, st, partial, p.nslab,
                               (long long)nq, sc.out_keys, (long long)k);
        } else if (w.npass == 1) {
            // few queries, many slabs: one workgroup of 16 waves per query (one wave per query walks hundreds of partial
            // lists as a chain of dependent loads: 150 us of a 0.5 ms call at 256 queries x 489 slabs)
            const bool wide = !pred && p.nslab >= 16 && nq <= 4096;
            LVS_HIP_CHECK(launch_merge(wide, partial, p.nslab, nq, kp, sc.out_keys, k, pred, st));
        } else {
            // the upper bounds of this pass live in out_keys, so merge into a side buffer first
            LVS_HIP_CHECK(launch_merge(false, partial, p.nslab, nq, kp, passbuf, kp, pred, st));
            hipLaunchKernelGGL(copy_pass_kernel, dim3((unsigned)lvs_ceil_div(nq * kp, 256)), dim3(256), 0, st, passbuf,
                               (long long)nq, kp, sc.out_keys, k, col0, pred);
        }
        LVS_HIP_CHECK(hipGetLastError());
    }
    if (dbg_counters) {
        unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        LVS_HIP_CHECK(hipStreamSynchronize(st));
        LVS_HIP_CHECK(hipMemcpy(h, dbg_counters, sizeof(h), hipMemcpyDeviceToHost));
        (void)hipFree(dbg_counters);
        fprintf(stderr,
                "[lvs] nq=%lld nb=%lld k=%d nslab=%d: wave-tiles %llu, block visits %llu, insertions %llu (%.1f per query); "
                "cycles per wave-tile: filter %.0f, visit loop %.0f (of which insertions %.0f); per visit %.0f, per insertion %.0f\n",
                (long long)nq, (long long)sc.nb, k, p.nslab, h[2], h[0], h[1], (double)h[1] / (double)(nq > 0 ? nq : 1),
                (double)h[3] / (double)(h[2] ? h[2] : 1), (double)h[4] / (double)(h[2] ? h[2] : 1),
                (double)h[5] / (double)(h[2] ? h[2] : 1), (double)(h[4] - h[5]) / (double)(h[0] ? h[0] : 1),
                (double)h[5] / (double)(h[1] ? h[1] : 1));
    }
    return LVS_OK;
}
}  // namespace

extern "C" int64_t lvs_flat_search_workspace_bytes(int64_t nq, int64_t nb, int32_t d, int32_t k, int32_t xb_pack,
                                                   int32_t xq_pack) {
    return lvs_flat_workspace_bytes(nq, nb, d, k, xb_pack, xq_pack);
}

static int32_t flat_search_impl(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack,
                                int64_t nq, int32_t d, int32_t metric, int32_t k, const float* xb_norms_sq,
                                const float* xq_norms_sq, int64_t id_offset, const uint32_t* row_ids,
                                uint64_t* out_keys, void* workspace, int64_t workspace_bytes, void* stream,
                                const SearchOpts& o) {
    LvsFlatPlan p;
    LVS_REQUIRE(lvs_flat_plan(nq, nb, d, xb_pack, xq_pack, o.hi_only, k, p) == LVS_OK,
                "bad shape nq=%lld nb=%lld d=%d k=%d pack=%d/%d", (long long)nq, (long long)nb, d, k, xb_pack, xq_pack);
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LVS_REQUIRE(k <= LVS_MAX_K, "k=%d exceeds LVS_MAX_K", k);
    LVS_REQUIRE(id_offset >= 0 && id_offset + nb <= 0xFFFFFFFFll, "ids must stay below 2^32-1");  // the last id is id_offset + nb - 1
    if (nq == 0 || k == 0) return LVS_OK;
    LVS_REQUIRE(out_keys, "out_keys is NULL");
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nb == 0) {
        LVS_HIP_CHECK(lvs_zero_async(out_keys, (size_t)nq * k * 8, st));
        return LVS_OK;
    }
    LVS_REQUIRE(xb && xq, "NULL rows");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && xq_norms_sq), "L2 needs both norm vectors");
    // the declared size: the larger of the call's own layout and its two-phase plan's (lvs_flat_search_workspace_bytes).  A call
    // short of it is refused even where the selection passes' layout would fit: it must not quietly run ceil(k / 56) passes
    TwoPhasePlan tp;
    const int64_t need = make_two_phase_plan(nq, nb, k, tp) && tp.total > p.w.total ? tp.total : p.w.total;
    if (workspace_bytes < need || !workspace) {
        lvs_set_error("workspace too small: need %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
        return LVS_ENOMEM;
    }
    LVS_REQUIRE_WS_ALIGNED(workspace);
    char* ws = (char*)workspace;
    const SearchCall sc = {xb, xq, xb_norms_sq, xq_norms_sq, nb, nq, id_offset, d, metric, k, xb_pack, xq_pack, row_ids,
                           (u64*)out_keys, st, o, p, ws, workspace_bytes, (uint32_t*)(ws + p.w.off_gtau)};

    const uint32_t* pred = nullptr;
    const int32_t rc = search_two_phase(sc, &pred);
    if (rc != LVS_OK) return rc;

    // one path serves the (rest of the) call; the list kernel is also the predicated fallback of the two-phase search
    const LvsRoute route = lvs_flat_route(nq, nb, p.l, k, p.w.npass, o.kc, pred != nullptr);
    switch (route.kind) {
        case LVS_ROUTE_RQ: return search_rq_chunks(sc, false);
        case LVS_ROUTE_RQ_JOIN: return search_rq_chunks(sc, true);
        case LVS_ROUTE_STREAM: return search_stream(sc, route.stream);
        default: return search_list_passes(sc, pred);
    }
}

extern "C" int32_t lvs_flat_search_keys(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack,
                                        int64_t nq, int32_t d, int32_t metric, int32_t k, const float* xb_norms_sq,
                                        const float* xq_norms_sq, int64_t id_offset, const uint32_t* row_ids,
                                        uint64_t* out_keys, void* workspace, int64_t workspace_bytes, void* stream) {
    return flat_search_impl(xb, xb_pack, nb, xq, xq_pack, nq, d, metric, k, xb_norms_sq, xq_norms_sq, id_offset, row_ids,
                            out_keys, workspace, workspace_bytes, stream, SearchOpts{});
}

extern "C" int32_t lvs_flat_search_keys_seeded(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack,
                                               int64_t nq, int32_t d, int32_t metric, int32_t k, const float* xb_norms_sq,
                                               const float* xq_norms_sq, int64_t id_offset, const uint32_t* row_ids,
                                               const float* seed_scores, int32_t seed_rows, uint64_t* out_keys,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
    LVS_REQUIRE(seed_rows >= 0 && (seed_rows == 0 || seed_scores), "bad seed scores");
    SearchOpts o;
    o.ext_seeds = seed_rows > 0 ? seed_scores : nullptr;
    o.ext_rows = seed_rows;
    return flat_search_impl(xb, xb_pack, nb, xq, xq_pack, nq, d, metric, k, xb_norms_sq, xq_norms_sq, id_offset, row_ids,
                            out_keys, workspace, workspace_bytes, stream, o);
}

extern "C" int32_t lvs_flat_search_seed_tiles(int64_t nq, int64_t nb, int32_t k) {
    if (nq < 0 || nb < 0 || k < 1) return LVS_EINVAL;
    int tiles = tile_seed_tiles(nq, nb, k);
    // A shard of a sharded join pools its sample with the other shards', so a larger sample per shard pays: 100 k x 8 x 125 k
    // rows, same box, sample pass + search per shard (profiles/r05y_seed_pool_sweep.log): 10 tiles 0.42 + 19.94 ms, 20 tiles
    // 0.76 + 19.06, 40 tiles 1.51 + 18.22, 61 tiles 2.29 + 17.71 - a twenty-fourth of the shard, at most 24 tiles.
    if (tiles > 0 && lvs_ceil_div(nq, LVS2_BQ) > 64) {
        int64_t t = nb / LVS_BC / 24;
        t = t > 24 ? 24 : t;
        if (t > tiles) tiles = (int)t;
    }
    return tiles;
}

extern "C" int32_t lvs_flat_search_seed_scores(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack,
                                               int64_t nq, int32_t d, int32_t metric, const float* xb_norms_sq,
                                               const float* xq_norms_sq, int32_t tiles, float* out_scores, void* stream) {
    LvsTilePlan p;
    LVS_REQUIRE(lvs_plain_tile_plan(nq, nb, d, xb_pack, xq_pack, p) == LVS_OK, "bad shape nq=%lld nb=%lld d=%d pack=%d/%d",
                (long long)nq, (long long)nb, d, xb_pack, xq_pack);
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LVS_REQUIRE(tiles >= 0, "bad tile count %d", tiles);
    if (nq == 0 || tiles == 0) return LVS_OK;
    LVS_REQUIRE(out_scores, "out_scores is NULL");
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    const int have = (int)(nb / LVS_BC < tiles ? nb / LVS_BC : tiles);  // whole tiles of real rows only
    if (have < tiles) {  // -inf: "that tile saw no row" (seed_kth_kernel skips it)
        const long long cnt = (long long)(tiles - have) * nq;
        float* dst = out_scores + (long long)have * nq;
        hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)lvs_ceil_div(cnt, 256)), dim3(256), 0, st, dst, cnt, -INFINITY);
        LVS_HIP_CHECK(hipGetLastError());
    }
    if (have == 0) return LVS_OK;  // an empty or shorter-than-a-tile shard (its buffers may be NULL) still fills its block
    LVS_REQUIRE(xb && xq, "NULL rows");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && xq_norms_sq), "L2 needs both norm vectors");
    LvsTileArgs a;
    tile_args(a, p.l, p.g, xb, xq, xb_norms_sq, xq_norms_sq, nb, nq, metric, 0);
    seed_tile_geometry(a, have);
    a.seed_out = out_scores;
    LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_SEED, a, st));
    return LVS_OK;
}

extern "C" int64_t lvs_nearest_hi_workspace_bytes(int64_t nq, int64_t nb, int32_t d) {
    LvsTilePlan p;
    if (lvs_plain_tile_plan(nq, nb, d, LVS_PACK_F16, LVS_PACK_F16, p) != LVS_OK) return LVS_EINVAL;
    return 256 + lvs_round_up((int64_t)p.g.nslab * nq * 8, 256) + lvs_round_up((int64_t)p.g.nslab * nq * 4, 256);
}

extern "C" int32_t lvs_nearest_hi(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack, int64_t nq,
                                  int32_t d, int32_t metric, const float* xb_norms_sq, const float* xq_norms_sq,
                                  int64_t id_offset, uint64_t* out_keys, float* out_second, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    LvsTilePlan p;
    LVS_REQUIRE(lvs_plain_tile_plan(nq, nb, d, xb_pack, xq_pack, p) == LVS_OK, "bad shape nq=%lld nb=%lld d=%d pack=%d/%d",
                (long long)nq, (long long)nb, d, xb_pack, xq_pack);
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LVS_REQUIRE(id_offset >= 0 && id_offset + nb < 0xFFFFFFFFll, "ids must stay below 2^32-1");
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(out_keys && out_second, "NULL output");
    LVS_REQUIRE(nb > 0 && xb && xq, "NULL rows / empty corpus");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && xq_norms_sq), "L2 needs both norm vectors");
    const int64_t need = lvs_nearest_hi_workspace_bytes(nq, nb, d);
    if (!workspace || workspace_bytes < need) {
        lvs_set_error("workspace too small: need %lld bytes, got %lld", (long long)need, (long long)workspace_bytes);
        return LVS_ENOMEM;
    }
    LVS_REQUIRE_WS_ALIGNED(workspace);
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace + 256;
    u64* pk = (u64*)ws;
    float* ps = (float*)(ws + lvs_round_up((int64_t)p.g.nslab * nq * 8, 256));
    LvsTileArgs a;
    tile_args(a, p.l, p.g, xb, xq, xb_norms_sq, xq_norms_sq, nb, nq, metric, id_offset);
    // SPLIT rows keep their leading dimension; only the fp16 "hi" half (columns [0, dpad)) is read
    a.nseg = 1;
    a.nk = p.l.nkd;
    a.bq = LVS2_BQ;
    a.k = 1;
    a.out = p.g.nslab == 1 ? (u64*)out_keys : pk;
    a.out_second = p.g.nslab == 1 ? out_second : ps;
    {
        ScopedKernelTimer timer(st);
        LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_TOP2, a, st));
    }
    if (p.g.nslab > 1) {
        hipLaunchKernelGGL(merge_top2_kernel, dim3((unsigned)lvs_ceil_div(nq, 256)), dim3(256), 0, st, pk, ps, p.g.nslab,
                           (long long)nq, (u64*)out_keys, out_second);
        LVS_HIP_CHECK(hipGetLastError());
    }
    return LVS_OK;
}

extern "C" int32_t lvs_rescore_keys(const void* xb, int32_t xb_pack, const void* xq, int32_t xq_pack, int64_t nq, int32_t d,
                                    int32_t metric, const float* xb_norms_sq, const float* xq_norms_sq, int64_t id_offset,
                                    int32_t k, uint64_t* keys, void* stream) {
    LVS_REQUIRE(nq >= 0 && d > 0 && k >= 0, "bad shape");
    if (k == 0) return LVS_OK;
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LvsLayout l;
    LVS_REQUIRE(lvs_layout(d, xb_pack, xq_pack, false, l) == LVS_OK, "bad pack mode %d/%d", xb_pack, xq_pack);
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(xb && xq && keys, "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && xq_norms_sq), "L2 needs both norm vectors");
    LVS_DEVICE_GUARD(stream);
    const dim3 grid((unsigned)lvs_ceil_div(nq * k, 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    lvs_split_dispatch(xq_pack, xb_pack, [&](auto qs, auto bs) {
        hipLaunchKernelGGL((rescore_keys_kernel<qs(), bs()>), grid, block, 0, st, (const _Float16*)xb, (long long)l.ldb,
                           (const _Float16*)xq, (long long)l.ldq, l.dpad, metric, xb_norms_sq, xq_norms_sq, (long long)id_offset,
                           (long long)nq, (int)k, (u64*)keys);
    });
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_flat_search_keys_hi(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack,
                                           int64_t nq, int32_t d, int32_t metric, int32_t k, const float* xb_norms_sq,
                                           const float* xq_norms_sq, int64_t id_offset, const uint32_t* row_ids,
                                           uint64_t* out_keys, void* workspace, int64_t workspace_bytes, void* stream) {
    SearchOpts o;
    o.hi_only = true;
    return flat_search_impl(xb, xb_pack, nb, xq, xq_pack, nq, d, metric, k, xb_norms_sq, xq_norms_sq, id_offset, row_ids,
                            out_keys, workspace, workspace_bytes, stream, o);
}

extern "C" int32_t lvs_flat_search_keys_hi_banded(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack,
                                                  int64_t nq, int32_t d, int32_t metric, int32_t k, int32_t kc,
                                                  float band_scale, float band_slack, const float* xb_norms_sq,
                                                  const float* xq_norms_sq, int64_t id_offset, const uint32_t* row_ids,
                                                  uint64_t* out_keys, void* workspace, int64_t workspace_bytes,
                                                  void* stream) {
    LVS_REQUIRE(kc >= 1 && kc <= k, "banded search: 1 <= kc <= k (got kc=%d, k=%d)", kc, k);
    LVS_REQUIRE(band_scale >= 0.f && band_slack >= 0.f, "negative band");
    LVS_REQUIRE(nq == 0 || xq_norms_sq, "banded search needs the query norms");
    SearchOpts o;
    o.hi_only = true;
    o.kc = kc;
    o.bscale = band_scale;
    o.bslack = band_slack;
    return flat_search_impl(xb, xb_pack, nb, xq, xq_pack, nq, d, metric, k, xb_norms_sq, xq_norms_sq, id_offset, row_ids,
                            out_keys, workspace, workspace_bytes, stream, o);
}

extern "C" int32_t lvs_sort_keys_desc(uint64_t* keys, int64_t nq, int32_t k, void* stream) {
    LVS_REQUIRE(nq >= 0 && k >= 0 && k <= 64, "lvs_sort_keys_desc: k must be at most 64 (got %d)", k);
    if (nq == 0 || k <= 1) return LVS_OK;
    LVS_REQUIRE(keys, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(sort_keys_kernel, dim3((unsigned)lvs_ceil_div(nq, 4)), dim3(256), 0, (hipStream_t)stream, (u64*)keys,
                       (long long)nq, (int)k);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_certify_topk_banded(const uint64_t* approx_keys, const uint64_t* exact_keys, const float* q_norms_sq,
                                           int64_t nq, int32_t k1, int32_t k, float scale, float slack, float band,
                                           int64_t* out_idx, uint64_t* out_count, void* stream) {
    LVS_REQUIRE(nq >= 0 && k >= 1 && k1 >= k && scale >= 0.f && slack >= 0.f && band >= 0.f, "bad arguments");
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(approx_keys && exact_keys && out_idx && out_count, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(certify_topk_kernel, dim3((unsigned)lvs_ceil_div(nq, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)approx_keys, (const u64*)exact_keys, q_norms_sq, (long long)nq, (int)k1, (int)k, scale, slack,
                       band, (long long*)out_idx, (unsigned long long*)out_count);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_certify_topk(const uint64_t* approx_keys, const uint64_t* exact_keys, const float* q_norms_sq,
                                    int64_t nq, int32_t k1, int32_t k, float scale, float slack, int64_t* out_idx,
                                    uint64_t* out_count, void* stream) {
    return lvs_certify_topk_banded(approx_keys, exact_keys, q_norms_sq, nq, k1, k, scale, slack, 0.f, out_idx, out_count, stream);
}

static int32_t margin_select_launch(const uint64_t* keys, const float* second, const float* q_norms_sq, int64_t nq, float scale,
                                    float slack, const float* stats, const LvsBoundCoef& coef, int64_t* out_idx,
                                    uint64_t* out_count, void* stream) {
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(keys && second && out_idx && out_count, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    const long long per_block = lvs_append_per_block(nq);
    hipLaunchKernelGGL(margin_select_kernel, dim3((unsigned)lvs_ceil_div(nq, per_block)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)keys, second, q_norms_sq, (long long)nq, scale, slack, stats, coef, per_block,
                       (long long*)out_idx, (unsigned long long*)out_count);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_margin_select(const uint64_t* keys, const float* second, const float* q_norms_sq, int64_t nq,
                                     float scale, float slack, int64_t* out_idx, uint64_t* out_count, void* stream) {
    LVS_REQUIRE(nq >= 0 && scale >= 0.f && slack >= 0.f, "bad arguments");
    return margin_select_launch(keys, second, q_norms_sq, nq, scale, slack, nullptr, LvsBoundCoef{{0, 0, 0, 0, 0}}, out_idx,
                                out_count, stream);
}

extern "C" int32_t lvs_margin_select_stats(const uint64_t* keys, const float* second, const float* q_norms_sq, int64_t nq,
                                           const float* corpus_stats, const float* coef5, int64_t* out_idx,
                                           uint64_t* out_count, void* stream) {
    LVS_REQUIRE(nq >= 0 && corpus_stats && coef5, "bad arguments");
    LvsBoundCoef c;
    for (int i = 0; i < 5; ++i) {
        LVS_REQUIRE(coef5[i] >= 0.f, "negative coefficient");
        c.c[i] = coef5[i];
    }
    return margin_select_launch(keys, second, q_norms_sq, nq, 0.f, 0.f, corpus_stats, c, out_idx, out_count, stream);
}

extern "C" int32_t lvs_nearest_bound_coef(int32_t metric, int32_t xq_pack, int32_t d, int32_t exp_sum, float* out_coef5) {
    LVS_REQUIRE(out_coef5 && lvs_nearest_bound_coef(metric, xq_pack, d, exp_sum, *(LvsBoundCoef*)out_coef5) == LVS_OK,
                "bad arguments metric=%d pack=%d d=%d (or a NULL output)", metric, xq_pack, d);
    return LVS_OK;
}

extern "C" int32_t lvs_merge_keys(const uint64_t* parts, int32_t nparts, int64_t nq, int32_t k, uint64_t* out_keys,
                                  void* stream) {
    LVS_REQUIRE(nparts >= 1 && nq >= 0 && k >= 0, "bad arguments");
    if (nq == 0 || k == 0) return LVS_OK;
    LVS_REQUIRE(parts && out_keys, "NULL buffer");
    LVS_REQUIRE(k <= LVS_MAX_K, "k=%d exceeds LVS_MAX_K", k);
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    if (k > 64) {
        // long lists: sort the candidates of a query in LDS, at most LVS_SELECT_MAX at a time.  More than that (e.g. 8
        // shards x k = 1000) is folded in rounds: out = top k of (out U the next group of parts); one workgroup owns a
        // query and reads everything it needs before it writes, so `out` is updated in place and no scratch is needed.
        const int per_round0 = LVS_SELECT_MAX / k;            // parts in the first round (>= 2 because k <= 2048)
        const int per_round = per_round0 - 1;                 // later rounds: one slot goes to the running result
        int done = nparts < per_round0 ? nparts : per_round0;
        LVS_HIP_CHECK(launch_merge_long((const u64*)parts, 0, done, nullptr, nq, k, (u64*)out_keys, st));
        while (done < nparts) {
            const int take = nparts - done < per_round ? nparts - done : per_round;
            LVS_HIP_CHECK(launch_merge_long((const u64*)parts, done, take, (const u64*)out_keys, nq, k, (u64*)out_keys, st));
            done += take;
        }
        return LVS_OK;
    }
    LVS_HIP_CHECK(launch_merge(false, (const u64*)parts, nparts, nq, k, (u64*)out_keys, k, nullptr, st));
    return LVS_OK;
}

extern "C" int32_t lvs_keys_to_result(const uint64_t* keys, int64_t nq, int32_t k, int32_t metric,
                                      const int64_t* id_map, int32_t score_exp, float* out_D, int64_t* out_I, void* stream) {
    LVS_REQUIRE(nq >= 0 && k >= 0, "bad shape");
    LVS_REQUIRE(score_exp >= -120 && score_exp <= 120, "score_exp %d out of range", score_exp);
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    long long n = (long long)nq * k;
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(keys && out_D && out_I, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(keys_to_result_kernel, dim3((unsigned)lvs_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)keys, n, metric, (const long long*)id_map, ldexpf(1.0f, -score_exp), out_D,
                       (long long*)out_I);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_scores(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack, int64_t nq,
                              int32_t d, int32_t metric, const float* xb_norms_sq, const float* xq_norms_sq,
                              int32_t score_exp, float* out, int64_t ld_out, void* stream) {
    LvsTilePlan p;
    LVS_REQUIRE(score_exp >= -120 && score_exp <= 120, "score_exp %d out of range", score_exp);
    LVS_REQUIRE(lvs_plain_tile_plan(nq, nb, d, xb_pack, xq_pack, p) == LVS_OK, "bad shape");
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    if (nq == 0 || nb == 0) return LVS_OK;
    LVS_REQUIRE(xb && xq && out && ld_out >= nb, "bad buffers");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && xq_norms_sq), "L2 needs both norm vectors");
    LVS_DEVICE_GUARD(stream);
    LvsTileArgs a;
    tile_args(a, p.l, p.g, xb, xq, xb_norms_sq, xq_norms_sq, nb, nq, metric, 0);
    a.scores = out;
    a.ld_scores = ld_out;
    a.out_scale = ldexpf(1.0f, -score_exp);
    a.k = 1;
    LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_SCORES, a, (hipStream_t)stream));
    return LVS_OK;
}

extern "C" int32_t lvs_range_join(const void* xb, int32_t xb_pack, int64_t nb, const void* xq, int32_t xq_pack, int64_t nq,
                                  int32_t d, int32_t metric, const float* xb_norms_sq, const float* xq_norms_sq,
                                  float threshold, int32_t score_exp, int64_t q_row0, int64_t id_offset,
                                  int32_t qt_stride, int32_t qt_phase, int64_t capacity, int64_t* out_q, int64_t* out_j,
                                  float* out_s, uint64_t* out_count, void* stream) {
    LvsTilePlan p;
    LVS_REQUIRE(score_exp >= -120 && score_exp <= 120, "score_exp %d out of range", score_exp);
    LVS_REQUIRE(lvs_plain_tile_plan(nq, nb, d, xb_pack, xq_pack, p) == LVS_OK, "bad shape");
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LVS_REQUIRE(capacity >= 0 && out_count, "bad output buffers");
    LVS_REQUIRE(qt_stride >= 1 && qt_phase >= 0 && qt_phase < qt_stride, "bad tile dealing %d/%d", qt_phase, qt_stride);
    if (nq == 0 || nb == 0) return LVS_OK;
    LVS_REQUIRE(xb && xq && (capacity == 0 || (out_q && out_j && out_s)), "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && xq_norms_sq), "L2 needs both norm vectors");
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    const float thr = threshold * ldexpf(1.0f, score_exp);  // the device scores are 2^score_exp x the caller's (exact)
    const float out_scale = ldexpf(1.0f, -score_exp);
    // one launch of the list kernel over queries [c0, c0 + cn) x rows [r0, r0 + rn), query tiles dealt stride / phase
    auto tile_launch = [&](int64_t c0, int64_t cn, int64_t r0, int64_t rn, int32_t stride, int32_t phase,
                           bool continuation) -> int32_t {
        LvsTileArgs a;
        tile_args(a, p.l, lvs_tile_geometry(lvs_tile_request_plain(cn, rn)), (const char*)xb + r0 * p.l.ldb * 2, (const char*)xq + c0 * p.l.ldq * 2,
                  xb_norms_sq ? xb_norms_sq + r0 : nullptr, xq_norms_sq ? xq_norms_sq + c0 : nullptr, rn, cn, metric,
                  id_offset + r0);
        a.k = 1;
        a.pair_q = (long long*)out_q;
        a.pair_j = (long long*)out_j;
        a.pair_s = out_s;
        a.pair_count = (unsigned long long*)out_count;
        a.pair_capacity = capacity;
        a.q_row0 = q_row0 >= 0 ? q_row0 + c0 : -1;
        a.q_base = c0;
        a.threshold = thr;
        a.out_scale = out_scale;
        a.qt_stride = stride;
        a.qt_phase = phase;
        ScopedKernelTimer timer(st, LVS_KERNEL_TILE, continuation);
        LVS_HIP_CHECK(lvs_tile_launch(LVS_MODE_RANGE, a, st));
        return LVS_OK;
    };
    // one launch of lvs_rj_kernel in RANGE mode over the same rectangle (whole 32-row blocks)
    auto rj_launch = [&](int64_t c0, int64_t cn, int64_t r0, int64_t rn, bool continuation) -> int32_t {
        LvsRqArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.xb = (const char*)xb + r0 * p.l.ldb * 2;
        ra.xq = (const _Float16*)xq + c0 * p.l.ldq;
        ra.nb = rn;
        ra.ldb = p.l.ldb;
        ra.ldq = p.l.ldq;
        ra.id_offset = id_offset + r0;
        ra.nq = (int)cn;
        ra.k = 1;
        ra.metric = metric;
        ra.pair_q = (long long*)out_q;
        ra.pair_j = (long long*)out_j;
        ra.pair_s = out_s;
        ra.pair_count = (unsigned long long*)out_count;
        ra.pair_capacity = capacity;
        ra.q_row0 = q_row0 >= 0 ? q_row0 + c0 : -1;
        ra.q_base = c0;
        ra.threshold = thr;
        ra.out_scale = out_scale;
        ScopedKernelTimer timer(st, LVS_KERNEL_RJ, continuation);
        LVS_HIP_CHECK(lvs_rj_range_launch(ra, p.l.dpad, st));
        return LVS_OK;
    };
    // the plan (lvs_plan.h): one launch of the list kernel, or chunks of queries, each against the rows that can still pair with
    // it.  Same pairs whichever kernel finds them (keys are scores of the same MFMA sequence), one shared counter.
    if (!lvs_range_rj_ok(nq, p.l.dpad, xb_pack, xq_pack, metric, qt_stride)) return tile_launch(0, nq, 0, nb, qt_stride, qt_phase, false);
    bool first = true;
    for (int64_t c0 = 0, cn = 0; c0 < nq; c0 += cn) {
        cn = range_chunk_len(nq - c0);
        const LvsRangeChunk c = lvs_range_chunk_plan(c0, cn, nb, q_row0, id_offset);
        if (c.rn <= 0) continue;
        int32_t rc = c.kernel == LVS_RANGE_RJ ? rj_launch(c0, cn, c.r0, c.rn, !first) : tile_launch(c0, cn, c.r0, c.rn, 1, 0, !first);
        if (rc != LVS_OK) return rc;
        first = false;
        if (c.tn > 0 && (rc = tile_launch(c0, cn, c.t0, c.tn, 1, 0, true)) != LVS_OK) return rc;  // the corpus' last nb % 32 rows
    }
    return LVS_OK;
}


// ---------------------------------------------------------------------------------------------------------------
// IVF: inverted lists over the flat packed image, searched by probing nprobe lists per query.  Three modes share the lists,
// the coarse step and the host driver below and differ in how a list's rows are scored: IVF-Flat (lvs_ivf.hip) from the
// rows themselves, IVF-SQ8 (lvs_ivf_sq8.hip) from 8-bit residual codes, IVF-PQ (lvs_ivf_pq.hip) from product-quantizer codes
// ---------------------------------------------------------------------------------------------------------------
namespace {
// the timing hook reports the list scan: the coarse step's own flat search is not timed
struct TimingPause {
    bool was;
    TimingPause() {
        std::lock_guard<std::mutex> lk(g_timing.mu);
        was = g_timing.on;
        g_timing.on = false;
    }
    ~TimingPause() {
        std::lock_guard<std::mutex> lk(g_timing.mu);
        g_timing.on = was;
    }
};

// the argument checks of the searches through the lists, in the order they are reported.  A mode without rows of its own passes
// xb_pack = LVS_PACK_F16, a mode without a product quantizer M = ksub = 1: those checks then always hold
int32_t ivf_check_search(int32_t metric, int64_t nb, int64_t nq, int32_t d, int32_t nlist, int32_t M, int32_t ksub,
                         int32_t nprobe, int32_t k, int32_t xb_pack, int32_t xq_pack, int32_t c_pack) {
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LVS_REQUIRE(nb >= 0 && nb < 0xFFFFFFFFll && nq >= 0 && d > 0, "bad shape nb=%lld nq=%lld d=%d", (long long)nb,
                (long long)nq, d);
    LVS_REQUIRE(nlist >= 1, "nlist=%d must be >= 1", nlist);
    LVS_REQUIRE(M >= 1 && d % M == 0, "M=%d must be >= 1 and divide d=%d", M, d);
    LVS_REQUIRE(ksub >= 1 && ksub <= LVS_PQ_KSUB, "ksub=%d must be in [1, %d]", ksub, LVS_PQ_KSUB);
    LVS_REQUIRE(nprobe >= 1 && nprobe <= nlist && nprobe <= LVS_MAX_K, "nprobe=%d must be in [1, min(nlist=%d, %d)]", nprobe,
                nlist, LVS_MAX_K);
    LVS_REQUIRE(k >= 1 && k <= LVS_KPASS, "k=%d must be in [1, %d] (one pass of the list scan)", k, LVS_KPASS);
    LVS_REQUIRE(xb_pack == LVS_PACK_F16 || xb_pack == LVS_PACK_SPLIT, "bad xb_pack");
    LVS_REQUIRE(xq_pack == LVS_PACK_F16 || xq_pack == LVS_PACK_SPLIT, "bad xq_pack");
    LVS_REQUIRE(c_pack == LVS_PACK_F16 || c_pack == LVS_PACK_SPLIT, "bad c_pack");
    return LVS_OK;
}

// the arguments the searches hand to the driver unchanged (the threshold search: k = 0, no out_keys)
struct IvfSearch {
    int32_t nlist;
    const void* centroids;
    int32_t c_pack;
    const float* c_norms_sq;
    const void* xq;
    int32_t xq_pack;
    int64_t nq;
    const float* xq_norms_sq;
    int32_t d, metric, nprobe, k;
    uint64_t* out_keys;
    int32_t* out_probe;
    void* workspace;
    int64_t workspace_bytes;
    void* stream;
    const uint32_t* sel_bits;  // the *_sel entry points' row selector for the mode's scan (NULL: every row)
};

// The host driver of the four searches through the lists (top-k over the rows, the SQ8 codes and the PQ codes; the threshold
// search): plan the scratch, then per chunk of queries the coarse step (the nprobe best centroids of every query under the
// index's metric), the probe ids, the mode's scan and the merge of its parts.
// scan(L, w, q0, cn, xq_c, qn_c, coarse, parts, nparts) launches the scan of queries [q0, q0 + cn) under its own
// ScopedKernelTimer (q0 > 0: a continuation) and may lower nparts, the lists per query that it fills (nprobe on entry).
// s.k = 0 (the threshold search): the scan appends to the caller's own buffers - no parts region and nothing to merge.
// A row selector (s.sel_bits) concerns the scan alone: the coarse step, the pair grouping, the tiling and the merge see none.
// mode: LVS_IVF_*, M: PQ's subspaces (1 otherwise) - the plan (lvs_ivf_plan.h) is the one *_workspace_bytes declared.
template <class Scan>
int32_t ivf_search_chunks(const IvfSearch& s, int mode, int32_t M, Scan scan) {
    LvsIvfPlan L;
    const int planned = lvs_ivf_plan(mode, s.nq, s.nlist, s.nprobe, s.d, M, s.k, s.c_pack, s.xq_pack, L);
    if (planned == LVS_EUNSUPPORTED) {
        if (mode == LVS_IVF_FLAT)
            lvs_set_error("d=%d with k=%d does not fit the list scan's LDS (see lvs_ivf_search_workspace_bytes)", s.d, s.k);
        else if (mode == LVS_IVF_RANGE)
            lvs_set_error("d=%d does not fit the threshold scan's LDS (see lvs_ivf_range_workspace_bytes)", s.d);
        else if (mode == LVS_IVF_SQ8)
            lvs_set_error("d=%d with k=%d does not fit the SQ8 list scan's LDS (see lvs_ivf_sq8_search_workspace_bytes)", s.d, s.k);
        else
            lvs_set_error("M=%d with k=%d does not fit the PQ list scan's LDS (see lvs_ivf_pq_search_workspace_bytes)", M, s.k);
        return LVS_EUNSUPPORTED;
    }
    LVS_REQUIRE(planned == LVS_OK, "shape beyond the IVF search");
    if (s.workspace_bytes < L.total) {
        lvs_set_error("workspace too small: need %lld bytes", (long long)L.total);
        return LVS_ENOMEM;
    }
    LVS_REQUIRE_WS_ALIGNED(s.workspace);
    LVS_DEVICE_GUARD(s.stream);
    hipStream_t st = (hipStream_t)s.stream;
    char* w = (char*)s.workspace;
    uint64_t* coarse = (uint64_t*)(w + L.off_coarse);
    u64* parts = (u64*)(w + L.off_parts);
    const size_t qrow_bytes = (size_t)lvs_packed_ld(s.d, s.xq_pack) * 2;
    for (int64_t q0 = 0; q0 < s.nq; q0 += L.chunk) {
        const int64_t cn = s.nq - q0 < L.chunk ? s.nq - q0 : L.chunk;
        const void* xq_c = (const char*)s.xq + (size_t)q0 * qrow_bytes;
        const float* qn_c = s.xq_norms_sq ? s.xq_norms_sq + q0 : nullptr;
        {
            TimingPause pause;
            const int32_t rc = lvs_flat_search_keys(s.centroids, s.c_pack, s.nlist, xq_c, s.xq_pack, cn, s.d, s.metric, s.nprobe,
                                                    s.c_norms_sq, qn_c, 0, nullptr, coarse, w, L.flat_bytes, s.stream);
            if (rc != LVS_OK) return rc;
        }
        if (s.out_probe)
            LVS_HIP_CHECK(lvs_ivf_probe_ids_launch((const u64*)coarse, cn * s.nprobe, s.out_probe + q0 * s.nprobe, st));
        int32_t nparts = s.nprobe;
        int32_t rc = scan(L, w, q0, cn, xq_c, qn_c, coarse, parts, nparts);
        if (rc != LVS_OK) return rc;
        if (s.k == 0) continue;
        rc = lvs_merge_keys((const uint64_t*)parts, nparts, cn, s.k, s.out_keys + q0 * s.k, s.stream);
        if (rc != LVS_OK) return rc;
    }
    return LVS_OK;
}

// Flat and SQ8: invert a chunk's (query, probe) pairs - pair numbers q * nprobe + p grouped by list (the bucket sort of
// lvs_count_sort.hip) -, cut every list's pairs into work items of 32 (the SQ8 scan halves them) and zero the parts (a pair
// whose probe named no list - never with nprobe <= nlist - keeps empty slots; k = 0: there are none)
int32_t ivf_group_pairs(const LvsIvfPlan& L, char* w, const uint64_t* coarse, int64_t npairs, int32_t nlist, int32_t k, u64* parts,
                        hipStream_t st, const uint32_t** pairs, const uint32_t** pair_offs) {
    const int32_t rc = lvs_bucket_positions(coarse, nullptr, npairs, nlist, 0, w + L.off_sort, L.sort_bytes, st, pairs, pair_offs);
    if (rc != LVS_OK) return rc;
    LVS_HIP_CHECK(lvs_ivf_tiles_launch(*pair_offs, nlist, (uint32_t*)(w + L.off_tiles), (uint32_t*)(w + L.off_items), st));
    if (k > 0) LVS_HIP_CHECK(lvs_zero_async(parts, (size_t)npairs * k * 8, st));
    return LVS_OK;
}

// the gathered-row scans' shared arguments (lvs_ivf_scan_kernel, lvs_ivf_range_kernel) that do not change from chunk to chunk
void ivf_gather_args(LvsIvfGatherArgs& g, const LvsLayout& p, const void* xb, const float* xb_norms_sq,
                     const int64_t* offsets, const uint32_t* rows, const uint32_t* sel_bits, int32_t nlist, int32_t nprobe,
                     int32_t metric) {
    g.xb = xb;
    g.bn = xb_norms_sq;
    g.rows = rows;
    g.offsets = offsets;
    g.sel = sel_bits;
    g.ldb = p.ldb;
    g.ldq = p.ldq;
    g.nlist = nlist;
    g.nprobe = nprobe;
    g.metric = metric;
    g.jper = p.dpad / 16;
    g.nseg = p.nseg;
    g.nbfrag = p.nbfrag;
    for (int i = 0; i < 3; ++i) {
        g.seg_c[i] = p.seg_c[i];
        g.seg_b[i] = p.seg_q[i] == 0 ? 0 : g.jper;
    }
}
// ... and those that do: the chunk's queries and its work items (ivf_group_pairs)
int32_t ivf_gather_chunk(LvsIvfGatherArgs& g, const LvsIvfPlan& L, char* w, const uint64_t* coarse, int64_t npairs, int32_t k,
                         u64* parts, hipStream_t st, const void* xq_c, const float* qn_c) {
    const int32_t rc = ivf_group_pairs(L, w, coarse, npairs, g.nlist, k, parts, st, &g.pairs, &g.pair_offs);
    if (rc != LVS_OK) return rc;
    g.tile_offs = (const uint32_t*)(w + L.off_tiles);
    g.item_list = (const uint32_t*)(w + L.off_items);
    g.xq = xq_c;
    g.qn = qn_c;
    return LVS_OK;
}

// what the two encoders share: the checks up to the pack mode; ldb and dpad of the packed rows
int32_t ivf_check_encode(int64_t n, int32_t d, int32_t nlist, int32_t M, int32_t ksub, int32_t xb_pack, int64_t& ldb,
                         int& dpad) {
    LVS_REQUIRE(n >= 0 && n < 0xFFFFFFFFll && d > 0, "bad shape n=%lld d=%d", (long long)n, d);
    LVS_REQUIRE(nlist >= 1, "nlist=%d must be >= 1", nlist);
    LVS_REQUIRE(M >= 1 && d % M == 0, "M=%d must be >= 1 and divide d=%d", M, d);
    LVS_REQUIRE(ksub >= 1 && ksub <= LVS_PQ_KSUB, "ksub=%d must be in [1, %d]", ksub, LVS_PQ_KSUB);
    LvsLayout l;
    LVS_REQUIRE(lvs_layout(d, xb_pack, xb_pack, false, l) == LVS_OK, "bad xb_pack");
    dpad = l.dpad;
    ldb = l.ldb;
    return LVS_OK;
}
}  // namespace

extern "C" int64_t lvs_ivf_build_workspace_bytes(int64_t n, int32_t nlist) {
    if (n < 0 || nlist < 1 || n >= 0xFFFFFFFFll) return LVS_EINVAL;
    const int64_t b = lvs_bucket_workspace_bytes(n > 0 ? n : 1, nlist);
    return b < 0 ? LVS_EINVAL : b;
}

extern "C" int32_t lvs_ivf_build_lists(const int64_t* assign, int64_t n, int32_t nlist, int64_t* out_offsets, uint32_t* out_rows,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    LVS_REQUIRE(n >= 0 && n < 0xFFFFFFFFll, "n=%lld out of range", (long long)n);
    LVS_REQUIRE(nlist >= 1, "nlist=%d must be >= 1", nlist);
    LVS_REQUIRE(out_offsets, "NULL offsets");
    LVS_REQUIRE(n == 0 || (assign && out_rows && workspace), "NULL buffer");
    const int64_t need = lvs_ivf_build_workspace_bytes(n, nlist);
    LVS_REQUIRE(need >= 0, "nlist=%d is beyond the bucket sort", nlist);
    if (n > 0 && workspace_bytes < need) {
        lvs_set_error("workspace too small: need %lld bytes", (long long)need);
        return LVS_ENOMEM;
    }
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        LVS_HIP_CHECK(lvs_zero_async(out_offsets, (size_t)(nlist + 1) * 8, st));
        return LVS_OK;
    }
    const uint32_t *rows = nullptr, *offs = nullptr;
    const int32_t rc = lvs_bucket_positions(nullptr, assign, n, nlist, 0, workspace, workspace_bytes, st, &rows, &offs);
    if (rc != LVS_OK) return rc;
    LVS_HIP_CHECK(hipMemcpyAsync(out_rows, rows, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    LVS_HIP_CHECK(lvs_ivf_offsets_launch(offs, nlist, out_offsets, st));
    return LVS_OK;
}

// ---- IVF-Flat
extern "C" int64_t lvs_ivf_search_workspace_bytes(int64_t nq, int32_t nlist, int32_t nprobe, int32_t d, int32_t k, int32_t pack) {
    return lvs_ivf_plan_bytes(LVS_IVF_FLAT, nq, nlist, nprobe, d, 1, k, pack);
}

extern "C" int32_t lvs_ivf_search_keys_sel(const void* xb, int32_t xb_pack, int64_t nb, const float* xb_norms_sq,
                                           const int64_t* offsets, const uint32_t* rows, const uint32_t* sel_bits,
                                           int32_t nlist, const void* centroids, int32_t c_pack, const float* c_norms_sq,
                                           const void* xq, int32_t xq_pack, int64_t nq, const float* xq_norms_sq, int32_t d,
                                           int32_t metric, int32_t nprobe, int32_t k, uint64_t* out_keys, int32_t* out_probe,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    const int32_t ok = ivf_check_search(metric, nb, nq, d, nlist, 1, 1, nprobe, k, xb_pack, xq_pack, c_pack);
    if (ok != LVS_OK) return ok;
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(xb && offsets && rows && centroids && xq && out_keys && workspace, "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && c_norms_sq && xq_norms_sq), "squared L2 needs the norms");
    LvsLayout p;
    LVS_REQUIRE(lvs_layout(d, xb_pack, xq_pack, false, p) == LVS_OK, "bad plan");
    LvsIvfArgs a;
    memset(&a, 0, sizeof(a));
    ivf_gather_args(a.g, p, xb, xb_norms_sq, offsets, rows, sel_bits, nlist, nprobe, metric);
    a.k = k;
    a.kcap = lvs_ivf_kcap(k);
    const IvfSearch s = {nlist, centroids, c_pack, c_norms_sq, xq, xq_pack, nq, xq_norms_sq, d,
                         metric, nprobe, k, out_keys, out_probe, workspace, workspace_bytes, stream, sel_bits};
    return ivf_search_chunks(s, LVS_IVF_FLAT, 1, [&](const LvsIvfPlan& L, char* w, int64_t q0, int64_t cn, const void* xq_c,
                                                     const float* qn_c, const uint64_t* coarse, u64* parts, int32_t&) -> int32_t {
        hipStream_t st = (hipStream_t)stream;
        const int32_t rc = ivf_gather_chunk(a.g, L, w, coarse, cn * nprobe, k, parts, st, xq_c, qn_c);
        if (rc != LVS_OK) return rc;
        a.out = parts;
        a.nq = (int)cn;
        ScopedKernelTimer timer(st, LVS_KERNEL_IVF, q0 > 0);
        LVS_HIP_CHECK(lvs_ivf_scan_launch(a, lvs_ivf_max_items(cn * nprobe, nlist), st));
        return LVS_OK;
    });
}

extern "C" int32_t lvs_ivf_search_keys(const void* xb, int32_t xb_pack, int64_t nb, const float* xb_norms_sq,
                                       const int64_t* offsets, const uint32_t* rows, int32_t nlist, const void* centroids,
                                       int32_t c_pack, const float* c_norms_sq, const void* xq, int32_t xq_pack, int64_t nq,
                                       const float* xq_norms_sq, int32_t d, int32_t metric, int32_t nprobe, int32_t k,
                                       uint64_t* out_keys, int32_t* out_probe, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
    return lvs_ivf_search_keys_sel(xb, xb_pack, nb, xb_norms_sq, offsets, rows, nullptr, nlist, centroids, c_pack, c_norms_sq, xq,
                                   xq_pack, nq, xq_norms_sq, d, metric, nprobe, k, out_keys, out_probe, workspace, workspace_bytes,
                                   stream);
}

// ---- threshold search through the lists (faiss IndexIVF::range_search): lvs_ivf_range_kernel over the full-precision rows
extern "C" int64_t lvs_ivf_range_workspace_bytes(int64_t nq, int32_t nlist, int32_t nprobe, int32_t d, int32_t pack) {
    return lvs_ivf_plan_bytes(LVS_IVF_RANGE, nq, nlist, nprobe, d, 1, 0, pack);
}

// Where the top-k searches scan into parts that the driver merges, every chunk's launch appends to the call's one pair list.
extern "C" int32_t lvs_ivf_range_search(const void* xb, int32_t xb_pack, int64_t nb, const float* xb_norms_sq,
                                        const int64_t* offsets, const uint32_t* rows, const uint32_t* sel_bits, int32_t nlist,
                                        const void* centroids, int32_t c_pack, const float* c_norms_sq, const void* xq,
                                        int32_t xq_pack, int64_t nq, const float* xq_norms_sq, const uint32_t* q_rows, int32_t d,
                                        int32_t metric, int32_t nprobe, float threshold, int32_t score_exp, int64_t capacity,
                                        int64_t* out_q, int64_t* out_j, float* out_s, uint64_t* out_count, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    const int32_t ok = ivf_check_search(metric, nb, nq, d, nlist, 1, 1, nprobe, 1, xb_pack, xq_pack, c_pack);
    if (ok != LVS_OK) return ok;
    LVS_REQUIRE(score_exp >= -120 && score_exp <= 120, "score_exp %d out of range", score_exp);
    LVS_REQUIRE(capacity >= 0 && out_count, "bad output buffers");
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(xb && offsets && rows && centroids && xq && workspace && (capacity == 0 || (out_q && out_j && out_s)), "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xb_norms_sq && c_norms_sq && xq_norms_sq), "squared L2 needs the norms");
    LvsLayout p;
    LVS_REQUIRE(lvs_layout(d, xb_pack, xq_pack, false, p) == LVS_OK, "bad plan");
    LvsIvfRangeArgs a;
    memset(&a, 0, sizeof(a));
    ivf_gather_args(a.g, p, xb, xb_norms_sq, offsets, rows, sel_bits, nlist, nprobe, metric);
    a.out_q = (long long*)out_q;
    a.out_j = (long long*)out_j;
    a.out_s = out_s;
    a.out_count = (unsigned long long*)out_count;
    a.capacity = capacity;
    a.threshold = threshold * ldexpf(1.0f, score_exp);  // the device scores are 2^score_exp x the caller's (exact)
    a.out_scale = ldexpf(1.0f, -score_exp);
    const IvfSearch s = {nlist, centroids, c_pack, c_norms_sq, xq, xq_pack, nq, xq_norms_sq, d,
                         metric, nprobe, 0, nullptr, nullptr, workspace, workspace_bytes, stream, sel_bits};
    return ivf_search_chunks(s, LVS_IVF_RANGE, 1, [&](const LvsIvfPlan& L, char* w, int64_t q0, int64_t cn, const void* xq_c,
                                                      const float* qn_c, const uint64_t* coarse, u64* parts, int32_t&) -> int32_t {
        hipStream_t st = (hipStream_t)stream;
        const int32_t rc = ivf_gather_chunk(a.g, L, w, coarse, cn * nprobe, 0, parts, st, xq_c, qn_c);
        if (rc != LVS_OK) return rc;
        a.q_rows = q_rows ? q_rows + q0 : nullptr;
        a.q_base = q0;
        ScopedKernelTimer timer(st, LVS_KERNEL_IVF_RANGE, q0 > 0);
        LVS_HIP_CHECK(lvs_ivf_range_launch(a, lvs_ivf_max_items(cn * nprobe, nlist), st));
        return LVS_OK;
    });
}

// ---- IVF-SQ8: the rows scored from 8-bit residual codes
extern "C" int32_t lvs_ivf_sq8_encode(const void* xb, int32_t xb_pack, int64_t n, int32_t d, const int64_t* offsets,
                                      const uint32_t* rows, int32_t nlist, const float* centroids, const float* vmin,
                                      const float* vdiff, uint8_t* out_codes, float* out_residual_norms_sq, void* stream) {
    int64_t ldb;
    int dpad;
    const int32_t ok = ivf_check_encode(n, d, nlist, 1, 1, xb_pack, ldb, dpad);
    if (ok != LVS_OK) return ok;
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(xb && offsets && rows && centroids && vmin && vdiff && out_codes && out_residual_norms_sq, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    LVS_HIP_CHECK(lvs_ivf_sq8_encode_launch(xb, ldb, xb_pack == LVS_PACK_SPLIT, dpad, n, d, offsets, nlist, rows, centroids, vmin,
                                            vdiff, out_codes, out_residual_norms_sq, (hipStream_t)stream));
    return LVS_OK;
}

extern "C" int64_t lvs_ivf_sq8_search_workspace_bytes(int64_t nq, int32_t nlist, int32_t nprobe, int32_t d, int32_t k,
                                                      int32_t pack) {
    return lvs_ivf_plan_bytes(LVS_IVF_SQ8, nq, nlist, nprobe, d, 1, k, pack);
}

extern "C" int32_t lvs_ivf_sq8_search_keys_sel(const uint8_t* codes, const float* residual_norms_sq, const float* vmin,
                                               const float* vdiff, const int64_t* offsets, const uint32_t* rows,
                                               const uint32_t* sel_bits, int64_t nb, int32_t nlist, const void* centroids,
                                               int32_t c_pack, const float* c_norms_sq, const float* centroids_f32,
                                               const void* xq, int32_t xq_pack, int64_t nq, const float* xq_norms_sq, int32_t d,
                                               int32_t metric, int32_t nprobe, int32_t k, uint64_t* out_keys,
                                               int32_t* out_probe, void* workspace, int64_t workspace_bytes, void* stream) {
    const int32_t ok = ivf_check_search(metric, nb, nq, d, nlist, 1, 1, nprobe, k, LVS_PACK_F16, xq_pack, c_pack);
    if (ok != LVS_OK) return ok;
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(codes && vmin && vdiff && offsets && rows && centroids && centroids_f32 && xq && out_keys && workspace,
                "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (residual_norms_sq && c_norms_sq && xq_norms_sq), "squared L2 needs the norms");
    LvsIvfSq8Args a;
    memset(&a, 0, sizeof(a));
    a.codes = codes;
    a.rnorm = residual_norms_sq;
    a.vmin = vmin;
    a.vdiff = vdiff;
    a.cent = centroids_f32;
    a.rows = rows;
    a.offsets = offsets;
    a.nlist = nlist;
    a.nprobe = nprobe;
    a.k = k;
    a.metric = metric;
    a.d = d;
    a.ldc = lvs_ivf_sq8_ldc(d);
    LvsLayout l;
    lvs_layout(d, xq_pack, xq_pack, false, l);  // (d and xq_pack passed ivf_check_search)
    a.qsplit = xq_pack == LVS_PACK_SPLIT;
    a.qdpad = l.dpad;
    a.ldq = l.ldq;
    a.kcap = lvs_ivf_kcap(k);
    const IvfSearch s = {nlist, centroids, c_pack, c_norms_sq, xq, xq_pack, nq, xq_norms_sq, d,
                         metric, nprobe, k, out_keys, out_probe, workspace, workspace_bytes, stream, sel_bits};
    return ivf_search_chunks(s, LVS_IVF_SQ8, 1, [&](const LvsIvfPlan& L, char* w, int64_t q0, int64_t cn, const void* xq_c,
                                                    const float*, const uint64_t* coarse, u64* parts, int32_t&) -> int32_t {
        hipStream_t st = (hipStream_t)stream;
        const int32_t rc = ivf_group_pairs(L, w, coarse, cn * nprobe, nlist, k, parts, st, &a.pairs, &a.pair_offs);
        if (rc != LVS_OK) return rc;
        a.tile_offs = (const uint32_t*)(w + L.off_tiles);
        a.item_list = (const uint32_t*)(w + L.off_items);
        a.out = parts;
        a.xq = xq_c;
        a.nq = (int)cn;
        a.sel = s.sel_bits;
        ScopedKernelTimer timer(st, LVS_KERNEL_IVF_SQ8, q0 > 0);
        LVS_HIP_CHECK(lvs_ivf_sq8_scan_launch(a, lvs_ivf_max_items(cn * nprobe, nlist), st));
        return LVS_OK;
    });
}

extern "C" int32_t lvs_ivf_sq8_search_keys(const uint8_t* codes, const float* residual_norms_sq, const float* vmin,
                                           const float* vdiff, const int64_t* offsets, const uint32_t* rows, int64_t nb,
                                           int32_t nlist, const void* centroids, int32_t c_pack, const float* c_norms_sq,
                                           const float* centroids_f32, const void* xq, int32_t xq_pack, int64_t nq,
                                           const float* xq_norms_sq, int32_t d, int32_t metric, int32_t nprobe, int32_t k,
                                           uint64_t* out_keys, int32_t* out_probe, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
    return lvs_ivf_sq8_search_keys_sel(codes, residual_norms_sq, vmin, vdiff, offsets, rows, nullptr, nb, nlist, centroids, c_pack,
                                       c_norms_sq, centroids_f32, xq, xq_pack, nq, xq_norms_sq, d, metric, nprobe, k, out_keys,
                                       out_probe, workspace, workspace_bytes, stream);
}

// ---- IVF-PQ: the rows scored from product-quantizer codes
extern "C" int32_t lvs_ivf_pq_encode(const void* xb, int32_t xb_pack, int64_t n, int32_t d, const int64_t* offsets,
                                     const uint32_t* rows, int32_t nlist, const float* centroids, int32_t M, int32_t ksub,
                                     const float* codebooks, uint8_t* out_codes, float* out_beta, void* stream) {
    int64_t ldb;
    int dpad;
    const int32_t ok = ivf_check_encode(n, d, nlist, M, ksub, xb_pack, ldb, dpad);
    if (ok != LVS_OK) return ok;
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(xb && offsets && rows && centroids && codebooks && out_codes && out_beta, "NULL buffer");
    LVS_DEVICE_GUARD(stream);
    LVS_HIP_CHECK(lvs_ivf_pq_encode_launch(xb, ldb, xb_pack == LVS_PACK_SPLIT, dpad, n, d, M, ksub, offsets, nlist, rows,
                                           centroids, codebooks, out_codes, out_beta, (hipStream_t)stream));
    return LVS_OK;
}

extern "C" int64_t lvs_ivf_pq_search_workspace_bytes(int64_t nq, int32_t nlist, int32_t nprobe, int32_t d, int32_t M, int32_t k,
                                                     int32_t pack) {
    return lvs_ivf_plan_bytes(LVS_IVF_PQ, nq, nlist, nprobe, d, M, k, pack);
}

extern "C" int32_t lvs_ivf_pq_search_keys_sel(const uint8_t* codes, const float* beta, const float* codebooks, int32_t M,
                                              int32_t ksub, const int64_t* offsets, const uint32_t* rows,
                                              const uint32_t* sel_bits, int64_t nb, int32_t nlist, const void* centroids,
                                              int32_t c_pack, const float* c_norms_sq, const float* centroids_f32,
                                              const void* xq, int32_t xq_pack, int64_t nq, const float* xq_norms_sq, int32_t d,
                                              int32_t metric, int32_t nprobe, int32_t k, uint64_t* out_keys, int32_t* out_probe,
                                              void* workspace, int64_t workspace_bytes, void* stream) {
    const int32_t ok = ivf_check_search(metric, nb, nq, d, nlist, M, ksub, nprobe, k, LVS_PACK_F16, xq_pack, c_pack);
    if (ok != LVS_OK) return ok;
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(codes && codebooks && offsets && rows && centroids && centroids_f32 && xq && out_keys && workspace,
                "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (beta && c_norms_sq && xq_norms_sq), "squared L2 needs the norms");
    LvsIvfPqArgs a;
    memset(&a, 0, sizeof(a));
    a.codes = codes;
    a.beta = beta;
    a.cent = centroids_f32;
    a.rows = rows;
    a.offsets = offsets;
    a.nlist = nlist;
    a.nprobe = nprobe;
    a.k = k;
    a.metric = metric;
    a.d = d;
    a.M = M;
    a.ldc = lvs_ivf_pq_ldc(M);
    LvsLayout l;
    lvs_layout(d, xq_pack, xq_pack, false, l);  // (d and xq_pack passed ivf_check_search)
    a.qsplit = xq_pack == LVS_PACK_SPLIT;
    a.qdpad = l.dpad;
    a.ldq = l.ldq;
    a.kcap = lvs_ivf_kcap(k);
    const IvfSearch s = {nlist, centroids, c_pack, c_norms_sq, xq, xq_pack, nq, xq_norms_sq, d,
                         metric, nprobe, k, out_keys, out_probe, workspace, workspace_bytes, stream, sel_bits};
    // the queries' tables, then the query-major scan: one part per range of probes
    return ivf_search_chunks(s, LVS_IVF_PQ, M,
                             [&](const LvsIvfPlan& L, char* w, int64_t q0, int64_t cn, const void* xq_c, const float*,
                                 const uint64_t* coarse, u64* parts, int32_t& nparts) -> int32_t {
        hipStream_t st = (hipStream_t)stream;
        float* lut = (float*)(w + L.off_extra);
        a.prange = lvs_ivf_pq_prange(nb, nlist, cn, nprobe);
        nparts = (nprobe + a.prange - 1) / a.prange;
        a.lut = lut;
        a.coarse = (const u64*)coarse;
        a.out = parts;
        a.xq = xq_c;
        a.nq = (int)cn;
        a.sel = s.sel_bits;
        ScopedKernelTimer timer(st, LVS_KERNEL_IVF_PQ, q0 > 0);
        LVS_HIP_CHECK(lvs_ivf_pq_lut_launch(xq_c, a.ldq, a.qsplit, a.qdpad, cn, d, M, ksub, codebooks, lut, st));
        LVS_HIP_CHECK(lvs_ivf_pq_scan_launch(a, st));
        return LVS_OK;
    });
}

extern "C" int32_t lvs_ivf_pq_search_keys(const uint8_t* codes, const float* beta, const float* codebooks, int32_t M,
                                          int32_t ksub, const int64_t* offsets, const uint32_t* rows, int64_t nb, int32_t nlist,
                                          const void* centroids, int32_t c_pack, const float* c_norms_sq,
                                          const float* centroids_f32, const void* xq, int32_t xq_pack, int64_t nq,
                                          const float* xq_norms_sq, int32_t d, int32_t metric, int32_t nprobe, int32_t k,
                                          uint64_t* out_keys, int32_t* out_probe, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
    return lvs_ivf_pq_search_keys_sel(codes, beta, codebooks, M, ksub, offsets, rows, nullptr, nb, nlist, centroids, c_pack,
                                      c_norms_sq, centroids_f32, xq, xq_pack, nq, xq_norms_sq, d, metric, nprobe, k, out_keys,
                                      out_probe, workspace, workspace_bytes, stream);
}

// ---- exact re-ranking of a first stage's candidates ("...,Refine(Flat)"): every check ahead of the first device call
extern "C" int32_t lvs_refine_keys(const void* xb, int32_t xb_pack, int64_t nb, const float* xb_norms_sq, const void* xq,
                                   int32_t xq_pack, int64_t nq, const float* xq_norms_sq, int32_t d, int32_t metric,
                                   const uint64_t* cand_keys, int32_t kc, int32_t k, uint64_t* out_keys, void* stream) {
    LVS_REQUIRE(metric == LVS_METRIC_IP || metric == LVS_METRIC_L2, "bad metric %d", metric);
    LVS_REQUIRE(nb >= 0 && nb < 0xFFFFFFFFll && nq >= 0 && nq < (1ll << 32) && d > 0 && d <= (1 << 24),
                "bad shape nb=%lld nq=%lld d=%d", (long long)nb, (long long)nq, d);
    LVS_REQUIRE(xb_pack == LVS_PACK_F16 || xb_pack == LVS_PACK_SPLIT, "bad xb_pack");
    LVS_REQUIRE(xq_pack == LVS_PACK_F16 || xq_pack == LVS_PACK_SPLIT, "bad xq_pack");
    LVS_REQUIRE(kc >= 1 && kc <= LVS_REFINE_MAXKC, "kc=%d must be in [1, %d] (one candidate per lane)", kc, LVS_REFINE_MAXKC);
    LVS_REQUIRE(k >= 1 && k <= kc, "k=%d must be in [1, kc=%d]", k, kc);
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(xq && cand_keys && out_keys && (xb || nb == 0), "NULL buffer");
    LVS_REQUIRE(metric != LVS_METRIC_L2 || (xq_norms_sq && (xb_norms_sq || nb == 0)), "squared L2 needs the norms");
    LvsRefineArgs a;
    memset(&a, 0, sizeof(a));
    a.xb = xb;
    a.bn = xb_norms_sq;
    a.xq = xq;
    a.qn = xq_norms_sq;
    a.cand = (const u64*)cand_keys;
    a.out = (u64*)out_keys;
    a.nb = nb;
    a.nq = nq;
    LvsLayout l;
    lvs_layout(d, xb_pack, xq_pack, false, l);  // (checked above)
    a.dpad = l.dpad;
    a.bsplit = xb_pack == LVS_PACK_SPLIT;
    a.qsplit = xq_pack == LVS_PACK_SPLIT;
    a.ldb = l.ldb;
    a.ldq = l.ldq;
    a.kc = kc;
    a.k = k;
    a.metric = metric;
    LVS_DEVICE_GUARD(stream);
    hipStream_t st = (hipStream_t)stream;
    ScopedKernelTimer timer(st, LVS_KERNEL_REFINE);
    LVS_HIP_CHECK(lvs_refine_launch(a, st));
    return LVS_OK;
}
