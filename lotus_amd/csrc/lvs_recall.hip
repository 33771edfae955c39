// Recall measurement on the device: three small kernels and their entry points (lvs_keys_overlap, lvs_ivf_row_lists,
// lvs_ivf_probe_ranks) behind HipVS.recall / probe_recall_curve / tune_nprobe.  They compare result keys that are already
// resident - the exact search's and an approximate search's - so that only counts travel to the host.
//
// Only the ROW NUMBER of a key is read (its low half, 0xFFFFFFFF - row): the two lists of a comparison may carry scores from
// different arithmetic (fp16 rows against decoded codes).  A key is EMPTY when it is 0; so is one whose low half is 0 - it
// would name row 2^32 - 1, which no image has (every entry point keeps nb below 2^32 - 1) - and that lets the staged 32-bit
// halves use 0 for "nothing here".
//   * lvs_keys_overlap_kernel / lvs_ivf_probe_ranks_kernel: one wave per query, RC_WAVES waves per workgroup.  The wave
//     stages the list it searches IN - the low halves of got_keys[q], or probe[q] - in its own stretch of LDS, padded to a
//     multiple of four with a value no needle equals; then lane v takes needles v, v + 64, ... (truth entries) and walks
//     the staged list four entries per 16-byte LDS read (all lanes read one address: a broadcast).  kt kg / 256 reads per
//     lane at the most, 16 K at kt = kg = 2 048; at the K = 10 of a search it is three.
//   * lvs_ivf_row_lists_kernel: one thread per list position p; the list of p is the last l with offsets[l] <= p, found by
//     bisection over offsets[1 .. nlist] (runs of equal offsets - empty lists - are stepped over by the strict compare).
// No kernel here needs scratch, a lock or more than one barrier.
#include "lvs_common.h"

namespace {

constexpr int RC_WAVES = 4;
constexpr int RC_THREADS = 256;  // lvs_ivf_row_lists_kernel

__host__ __device__ inline int rc_pad4(int n) { return (n + 3) & ~3; }

// position of the first entry of hay[0 .. npad) equal to `needle`, npad when there is none (npad % 4 == 0; hay is wave-uniform)
__device__ __forceinline__ int rc_find(const uint32_t* hay, int npad, uint32_t needle) {
    int at = npad;
    for (int i = npad - 4; i >= 0; i -= 4) {
        const uint4 h = *(const uint4*)(hay + i);
        at = h.w == needle ? i + 3 : at;
        at = h.z == needle ? i + 2 : at;
        at = h.y == needle ? i + 1 : at;
        at = h.x == needle ? i : at;
    }
    return at;
}

__global__ __launch_bounds__(RC_WAVES * 64) void lvs_keys_overlap_kernel(const u64* truth, int kt, const u64* got, int kg,
                                                                         long long nq, int32_t* out_hits, int32_t* out_first) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rc_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long q = (long long)blockIdx.x * RC_WAVES + wave;
    const bool live = q < nq;
    const int kgpad = rc_pad4(kg);
    uint32_t* hay = rc_lds + wave * kgpad;
    if (live) {
        const u64* g = got + q * kg;
        for (int i = lane; i < kgpad; i += 64) {
            const u64 key = i < kg ? g[i] : 0ull;
            hay[i] = key ? (uint32_t)key : 0u;  // (an empty slot and a row past every image both stage as 0)
        }
    }
    __syncthreads();
    if (!live) return;
    const u64* t = truth + q * kt;
    int hits = 0, first = 0;
    for (int j0 = 0; j0 < kt; j0 += 64) {
        const u64 key = j0 + lane < kt ? t[j0 + lane] : 0ull;
        const uint32_t lo = (uint32_t)key;
        const bool have = key != 0 && lo != 0;
        const bool found = have && rc_find(hay, kgpad, lo) < kgpad;
        const unsigned long long m = __ballot(found);
        hits += __popcll(m);
        if (j0 == 0) first = (int)(m & 1ull);
    }
    if (lane == 0) {
        out_hits[q] = hits;
        out_first[q] = first;
    }
}

__global__ __launch_bounds__(RC_THREADS) void lvs_ivf_row_lists_kernel(const long long* offsets, const uint32_t* rows, long long n,
                                                                       int nlist, int32_t* out_row_list) {
    const long long p = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    if (p >= n) return;
    // the smallest i in [1, nlist] with offsets[i] > p (offsets[nlist] = n > p); the list is i - 1
    int lo = 1, hi = nlist;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] > p) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t r = rows[p];
    if ((long long)r < n) out_row_list[r] = lo - 1;  // (a row number past the image is never written through)
}

__global__ __launch_bounds__(RC_WAVES * 64) void lvs_ivf_probe_ranks_kernel(const u64* truth, int kt, const int32_t* row_list,
                                                                            long long n, const int32_t* probe, int P, long long nq,
                                                                            int32_t* out_rank, u64* out_hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rc_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long q = (long long)blockIdx.x * RC_WAVES + wave;
    const bool live = q < nq;
    const int ppad = rc_pad4(P);
    uint32_t* hay = rc_lds + wave * ppad;
    if (live) {
        const int32_t* pr = probe + q * P;
        for (int i = lane; i < ppad; i += 64) hay[i] = i < P ? (uint32_t)pr[i] : 0xFFFFFFFFu;  // -1: no list
    }
    __syncthreads();
    if (!live) return;
    const u64* t = truth + q * kt;
    for (int j = lane; j < kt; j += 64) {
        const u64 key = t[j];
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)key;
        int rank = -1;
        if (key != 0 && (long long)row < n) {
            const int32_t l = row_list[row];
            const int at = l >= 0 ? rc_find(hay, ppad, (uint32_t)l) : ppad;  // a row in no list (-1) equals the padding: skip
            rank = at < P ? at : P;
            atomicAdd((unsigned long long*)&out_hist[rank], 1ull);
        }
        out_rank[q * kt + j] = rank;
    }
}

}  // namespace

extern "C" int32_t lvs_keys_overlap(const uint64_t* truth_keys, int32_t kt, const uint64_t* got_keys, int32_t kg, int64_t nq,
                                    int32_t* out_hits, int32_t* out_first, void* stream) {
    LVS_REQUIRE(kt >= 1 && kt <= LVS_MAX_K, "lvs_keys_overlap: kt=%d must be in [1, %d]", kt, LVS_MAX_K);
    LVS_REQUIRE(kg >= 1 && kg <= LVS_MAX_K, "lvs_keys_overlap: kg=%d must be in [1, %d]", kg, LVS_MAX_K);
    LVS_REQUIRE(nq >= 0 && nq < (1ll << 32), "lvs_keys_overlap: bad nq=%lld", (long long)nq);
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(truth_keys && got_keys && out_hits && out_first, "lvs_keys_overlap: NULL buffer");
    LVS_DEVICE_GUARD(stream);
    const size_t lds = (size_t)RC_WAVES * rc_pad4(kg) * sizeof(uint32_t);
    LVS_HIP_CHECK(lvs_launch_lds<lvs_keys_overlap_kernel>(dim3((unsigned)lvs_ceil_div(nq, RC_WAVES)), dim3(RC_WAVES * 64), lds,
                                                          (hipStream_t)stream, (const u64*)truth_keys, (int)kt,
                                                          (const u64*)got_keys, (int)kg, (long long)nq, out_hits, out_first));
    return LVS_OK;
}

extern "C" int32_t lvs_ivf_row_lists(const int64_t* offsets, const uint32_t* rows, int64_t n, int32_t nlist,
                                     int32_t* out_row_list, void* stream) {
    LVS_REQUIRE(nlist >= 1, "lvs_ivf_row_lists: nlist=%d must be at least 1", nlist);
    LVS_REQUIRE(n >= 0 && n < 0xFFFFFFFFll, "lvs_ivf_row_lists: bad n=%lld", (long long)n);
    if (n == 0) return LVS_OK;
    LVS_REQUIRE(offsets && rows && out_row_list, "lvs_ivf_row_lists: NULL buffer");
    LVS_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(lvs_ivf_row_lists_kernel, dim3((unsigned)lvs_ceil_div(n, RC_THREADS)), dim3(RC_THREADS), 0,
                       (hipStream_t)stream, (const long long*)offsets, rows, (long long)n, (int)nlist, out_row_list);
    LVS_HIP_CHECK(hipGetLastError());
    return LVS_OK;
}

extern "C" int32_t lvs_ivf_probe_ranks(const uint64_t* truth_keys, int32_t kt, const int32_t* row_list, int64_t n,
                                       const int32_t* probe, int32_t P, int64_t nq, int32_t* out_rank, uint64_t* out_hist,
                                       void* stream) {
    LVS_REQUIRE(kt >= 1 && kt <= LVS_MAX_K, "lvs_ivf_probe_ranks: kt=%d must be in [1, %d]", kt, LVS_MAX_K);
    LVS_REQUIRE(P >= 1 && P <= LVS_MAX_K, "lvs_ivf_probe_ranks: P=%d must be in [1, %d]", P, LVS_MAX_K);
    LVS_REQUIRE(n >= 0 && n < 0xFFFFFFFFll, "lvs_ivf_probe_ranks: bad n=%lld", (long long)n);
    LVS_REQUIRE(nq >= 0 && nq < (1ll << 32), "lvs_ivf_probe_ranks: bad nq=%lld", (long long)nq);
    if (nq == 0) return LVS_OK;
    LVS_REQUIRE(truth_keys && probe && out_rank && out_hist && (row_list || n == 0), "lvs_ivf_probe_ranks: NULL buffer");
    LVS_DEVICE_GUARD(stream);
    const size_t lds = (size_t)RC_WAVES * rc_pad4(P) * sizeof(uint32_t);
    LVS_HIP_CHECK(lvs_launch_lds<lvs_ivf_probe_ranks_kernel>(dim3((unsigned)lvs_ceil_div(nq, RC_WAVES)), dim3(RC_WAVES * 64), lds,
                                                             (hipStream_t)stream, (const u64*)truth_keys, (int)kt, row_list,
                                                             (long long)n, probe, (int)P, (long long)nq, out_rank,
                                                             (u64*)out_hist));
    return LVS_OK;
}
