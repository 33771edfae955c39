// The exclusive scan of the counting sorts, and the bucket sort: a STABLE counting sort of positions by an id.
//
// lvs_bucket_positions groups the rows of a k-means iteration by centroid (lvs_kmeans.hip), the corpus rows by inverted list
// (lvs_ivf_build_lists) and a search chunk's (query, probe) pairs by list (ivf_group_pairs, lvs_capi.hip).  Hand-written -
// round 2 used rocPRIM's radix sort.
// bins = k + 1 (the last one collects ids outside [0, k): ignored rows).  A launch works on chunks of BUCKET_CHUNK
// consecutive rows, one workgroup each:
//   lvs_bucket_count_kernel    counts[bin][chunk] = rows of the chunk that go to `bin`          (histogram in LDS)
//   lvs_scan_excl_launch       exclusive scan over counts in (bin-major, chunk-minor) order = first output position of every
//                              (bin, chunk) run; offsets[c] = start of bucket c, c = 0 .. k
//   lvs_bucket_scatter_kernel  rows_out[position] = row, in row order inside a chunk (waves of a tile take turns,
//                              lanes rank themselves among the lanes with the same bin by ballots over the bin's bits)
// Rows keep their order inside a bucket, which is what makes the centroid sums independent of the launch shape.
#include "lvs_count_sort.h"

namespace {
// ---- exclusive scan, three launches: per-segment scan + segment totals, scan of the totals (one workgroup), add --------
__global__ __launch_bounds__(256) void lvs_scan1_kernel(uint32_t* __restrict__ v, long long total, uint32_t* __restrict__ seg_sum) {
    __shared__ uint32_t part[256];
    const long long base = (long long)blockIdx.x * LVS_SCAN_SEG + (long long)threadIdx.x * (LVS_SCAN_SEG / 256);
    uint32_t loc[LVS_SCAN_SEG / 256], sum = 0;
#pragma unroll
    for (int i = 0; i < LVS_SCAN_SEG / 256; ++i) {
        loc[i] = base + i < total ? v[base + i] : 0u;
        sum += loc[i];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // Hillis-Steele inclusive scan of the 256 thread sums
        const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;  // exclusive prefix of this thread inside the segment
#pragma unroll
    for (int i = 0; i < LVS_SCAN_SEG / 256; ++i) {
        if (base + i < total) v[base + i] = run;
        run += loc[i];
    }
    if (threadIdx.x == 255) seg_sum[blockIdx.x] = part[255];
}
__global__ __launch_bounds__(256) void lvs_scan2_kernel(uint32_t* __restrict__ seg_sum, long long nseg) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long s0 = 0; s0 < nseg; s0 += 256) {
        const long long i = s0 + threadIdx.x;
        const uint32_t mine = i < nseg ? seg_sum[i] : 0u;
        part[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t add = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nseg) seg_sum[i] = carry + part[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 255) carry += part[255];
        __syncthreads();
    }
}
// v += its segment's offset; offsets[b] = v[b * nchunks] for b = 0 .. nbuckets, written only when `offsets` is given
__global__ __launch_bounds__(256) void lvs_scan3_kernel(uint32_t* __restrict__ v, long long total,
                                                        const uint32_t* __restrict__ seg_sum, int nchunks,
                                                        uint32_t* __restrict__ offsets, int nbuckets) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        const uint32_t val = v[i] + seg_sum[i / LVS_SCAN_SEG];
        v[i] = val;
        if (offsets && i % nchunks == 0 && i / nchunks <= nbuckets) offsets[i / nchunks] = val;
    }
}

// ---- bucket sort -----------------------------------------------------------------------------------------------
// (BucketPlan, BUCKET_CHUNK, BUCKET_MAX_BINS: lvs_ivf_plan.h)
template <typename KeyT>
__device__ inline uint32_t lvs_bucket_bin_of(KeyT v, long long id_offset, int k);
template <>
__device__ inline uint32_t lvs_bucket_bin_of<long long>(long long c, long long, int k) {
    return (c < 0 || c >= k) ? (uint32_t)k : (uint32_t)c;
}
template <>
__device__ inline uint32_t lvs_bucket_bin_of<u64>(u64 key, long long id_offset, int k) {  // a result key: id in the low word
    if (key == 0) return (uint32_t)k;
    const long long c = (long long)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) - id_offset;
    return (c < 0 || c >= k) ? (uint32_t)k : (uint32_t)c;
}

// digit of a row: ((bin >> shift) & mask); rows are read through `order` (nullable: identity) so that a second pass can
// sort the output of the first
template <typename KeyT>
__global__ __launch_bounds__(256) void lvs_bucket_count_kernel(const KeyT* __restrict__ assign, const uint32_t* __restrict__ order,
                                                               long long n, int k, long long id_offset, int shift,
                                                               uint32_t mask, int nbins, int nchunks,
                                                               uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t lvs_bucket_hist[];
    for (int b = threadIdx.x; b < nbins; b += 256) lvs_bucket_hist[b] = 0;
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * BUCKET_CHUNK;
    const long long r1 = r0 + BUCKET_CHUNK < n ? r0 + BUCKET_CHUNK : n;
    for (long long i = r0 + threadIdx.x; i < r1; i += 256) {
        const long long row = order ? (long long)order[i] : i;
        atomicAdd(&lvs_bucket_hist[(lvs_bucket_bin_of<KeyT>(assign[row], id_offset, k) >> shift) & mask], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += 256) counts[(long long)b * nchunks + blockIdx.x] = lvs_bucket_hist[b];
}

// bucket boundaries from the SORTED rows (two-digit sorts only): offsets[c] = first position whose bin is >= c, c = 0..k
// (no atomics: position i writes the offsets of every bucket that starts there; k + 1 writes in total)
template <typename KeyT>
__global__ __launch_bounds__(256) void lvs_bucket_bounds_kernel(const KeyT* __restrict__ assign, const uint32_t* __restrict__ rows,
                                                                long long n, int k, long long id_offset,
                                                                uint32_t* __restrict__ offsets) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const long long lo = i == 0 ? 0 : (long long)lvs_bucket_bin_of<KeyT>(assign[rows[i - 1]], id_offset, k) + 1;
    const long long hi = i == n ? (long long)k : (long long)lvs_bucket_bin_of<KeyT>(assign[rows[i]], id_offset, k);
    for (long long c = lo; c <= hi && c <= k; ++c) offsets[c] = (uint32_t)i;
}

template <typename KeyT>
__global__ __launch_bounds__(256) void lvs_bucket_scatter_kernel(const KeyT* __restrict__ assign, const uint32_t* __restrict__ order,
                                                                 long long n, int k, long long id_offset, int shift,
                                                                 uint32_t mask, int nbins, int nbits, int nchunks,
                                                                 const uint32_t* __restrict__ counts,
                                                                 uint32_t* __restrict__ rows_out) {
    extern __shared__ uint32_t lvs_bucket_pos[];  // next output position of every bin for this chunk
    for (int b = threadIdx.x; b < nbins; b += 256) lvs_bucket_pos[b] = counts[(long long)b * nchunks + blockIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * BUCKET_CHUNK;
    const long long r1 = r0 + BUCKET_CHUNK < n ? r0 + BUCKET_CHUNK : n;
    for (long long t0 = r0; t0 < r1; t0 += 256) {
        const long long i = t0 + threadIdx.x;
        const bool live = i < r1;
        uint32_t row = 0, bin = 0;
        if (live) {
            row = order ? order[i] : (uint32_t)i;
            bin = (lvs_bucket_bin_of<KeyT>(assign[row], id_offset, k) >> shift) & mask;
        }
        // lanes of this wave holding the same bin (dead lanes match nobody)
        u64 peers = __builtin_amdgcn_ballot_w64(live);
        for (int b = 0; b < nbits; ++b) {
            const u64 m = __builtin_amdgcn_ballot_w64(live && ((bin >> b) & 1u));
            peers &= ((bin >> b) & 1u) ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        const int cnt = __popcll(peers);
        uint32_t base = 0;
        for (int w = 0; w < 4; ++w) {  // waves take turns: rows of wave w come before those of wave w + 1
            if (wave == w && live && rank == 0) {
                base = lvs_bucket_pos[bin];
                lvs_bucket_pos[bin] = base + (uint32_t)cnt;
            }
            __syncthreads();
        }
        // the leader's base -> its peers
        const int leader = live ? __ffsll((long long)peers) - 1 : lane;
        base = __shfl(base, leader, 64);
        if (live) rows_out[base + (uint32_t)rank] = row;
    }
}

int bucket_bits(int nbins) {
    int b = 1;
    while ((1 << b) < nbins) ++b;
    return b;
}
template <typename KeyT>
int32_t bucket_rows(const KeyT* assign, int64_t n, int32_t k, int64_t id_offset, const BucketPlan& p, char* w, hipStream_t st,
                    const uint32_t** rows_out, const uint32_t** offs_out) {
    uint32_t* counts = (uint32_t*)(w + p.off_counts);
    uint32_t* seg = (uint32_t*)(w + p.off_seg);
    uint32_t* rows[2] = {(uint32_t*)(w + p.off_rows_a), (uint32_t*)(w + p.off_rows_b)};
    uint32_t* offs = (uint32_t*)(w + p.off_offs);
    const uint32_t* order = nullptr;
    // a pass may use BUCKET_MAX_BINS counters: > 64 KB of dynamic LDS needs the attribute
    LVS_HIP_CHECK(lvs_arm_lds<lvs_bucket_count_kernel<KeyT>>((size_t)BUCKET_MAX_BINS * 4));
    LVS_HIP_CHECK(lvs_arm_lds<lvs_bucket_scatter_kernel<KeyT>>((size_t)BUCKET_MAX_BINS * 4));
    for (int ps = 0; ps < p.passes; ++ps) {
        const int nbins = p.nbins[ps];
        const size_t lds = (size_t)nbins * 4;
        hipLaunchKernelGGL((lvs_bucket_count_kernel<KeyT>), dim3((unsigned)p.nchunks), dim3(256), lds, st, assign, order,
                           (long long)n, k, (long long)id_offset, p.shift[ps], p.mask[ps], nbins, p.nchunks, counts);
        // a one-digit sort reads the buckets' starts off the scanned counters; two digits: lvs_bucket_bounds_kernel below
        lvs_scan_excl_launch(counts, (long long)nbins * p.nchunks, seg, st, p.passes == 1 ? offs : nullptr, p.nchunks, k);
        hipLaunchKernelGGL((lvs_bucket_scatter_kernel<KeyT>), dim3((unsigned)p.nchunks), dim3(256), lds, st, assign, order,
                           (long long)n, k, (long long)id_offset, p.shift[ps], p.mask[ps], nbins, bucket_bits(nbins),
                           p.nchunks, (const uint32_t*)counts, rows[ps]);
        order = rows[ps];
    }
    if (p.passes > 1)
        hipLaunchKernelGGL((lvs_bucket_bounds_kernel<KeyT>), dim3((unsigned)lvs_ceil_div(n + 1, 256)), dim3(256), 0, st, assign,
                           order, (long long)n, k, (long long)id_offset, offs);
    LVS_HIP_CHECK(hipGetLastError());
    *rows_out = order;
    *offs_out = offs;
    return LVS_OK;
}
}  // namespace

void lvs_scan_excl_launch(uint32_t* v, long long total, uint32_t* seg, hipStream_t stream, uint32_t* offsets, int nchunks,
                          int nbuckets) {
    const long long nseg = lvs_ceil_div(total, LVS_SCAN_SEG);
    hipLaunchKernelGGL(lvs_scan1_kernel, dim3((unsigned)nseg), dim3(256), 0, stream, v, total, seg);
    hipLaunchKernelGGL(lvs_scan2_kernel, dim3(1), dim3(256), 0, stream, seg, nseg);
    hipLaunchKernelGGL(lvs_scan3_kernel, dim3((unsigned)lvs_ceil_div(total, 256)), dim3(256), 0, stream, v, total,
                       (const uint32_t*)seg, nchunks, offsets, nbuckets);
}

int32_t lvs_bucket_positions(const uint64_t* keys, const int64_t* assign, int64_t n, int32_t k, int64_t id_offset, void* ws,
                             int64_t ws_bytes, hipStream_t stream, const uint32_t** rows_out, const uint32_t** offs_out) {
    LVS_REQUIRE(n > 0 && k > 0 && (keys == nullptr) != (assign == nullptr) && ws, "bad arguments");
    BucketPlan p;
    LVS_REQUIRE(bucket_plan(n, k, p), "k=%d is beyond the bucket sort", k);
    if (ws_bytes < p.total) {
        lvs_set_error("workspace too small: need %lld bytes", (long long)p.total);
        return LVS_ENOMEM;
    }
    LVS_REQUIRE_WS_ALIGNED(ws);
    LVS_DEVICE_GUARD(stream);  // after the checks: a caller that holds no guard yet (k-means) reports these errors first
    if (keys) return bucket_rows<u64>((const u64*)keys, n, k, id_offset, p, (char*)ws, stream, rows_out, offs_out);
    return bucket_rows<long long>((const long long*)assign, n, k, id_offset, p, (char*)ws, stream, rows_out, offs_out);
}
