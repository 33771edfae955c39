// IVF-Flat list scan: the hot kernel of lvs_ivf_search_keys (lvs_capi.hip).
//
// An IVF search probes nprobe of nlist inverted lists per query.  The (query, probe rank) pairs are grouped by list
// (the bucket sort of lvs_count_sort.hip), and one work item is one list together with a tile of up to 32 of the pairs that
// probe it.  The work item, the tile's queries in LDS, the gathered rows and the MFMA loop that scores a 32-row block against
// the tile are lvs_ivf_gather.h's.  This kernel's own part is what happens to a score:
//   * hits go through the wave-cooperative sorted insertion (lvs_list_insert, lvs_common.h) into per-query lists in LDS (one
//     lock per query: the four waves share the tile).  Keys carry the GLOBAL row number, so ties between rows of different
//     lists keep the oracle's total order when the per-probe lists are merged (lvs_merge_keys);
//   * the work item writes its k keys per pair to the part of the pair's probe rank: parts [nprobe][nq][k].
//
// Rooflines (1 M x 768 fp16, nlist 4 096, nprobe 32 -> ~7 800 rows per query): one query is HBM-bound, 12 MB of rows over
// 8 TB/s = 1.5 us, in practice bounded by the latency of a few dozen workgroups; 10 000 queries are 120 GFLOP (48 us at
// 2.5 PFLOP/s), but every work item reads its whole list and a list serves ~3 tiles, so ~4.6 GB of row reads make this
// tiling bandwidth-bound at ~0.58 ms.  The LDS image bounds d: lvs_ivf_search_workspace_bytes.
#include "lvs_ivf_gather.h"

namespace {

// SEL: only the rows whose bit is set in a.g.sel (bit r & 31 of word r >> 5 for row r of the flat image) take part.
template <int U, bool SEL>
__global__ __launch_bounds__(LVS_IVF_WAVES * 64) void lvs_ivf_scan_kernel(const LvsIvfArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TQ = LVS_IVF_TILEQ;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KCAP = a.kcap;
    half8* bfrag = (half8*)smem;                                            // [nbfrag][64]
    u64* lists = (u64*)(smem + (size_t)a.g.nbfrag * 1024);                  // [TQ][KCAP]
    uint32_t* locks = (uint32_t*)((char*)lists + (size_t)TQ * KCAP * 8);    // [TQ]
    int* slot_q = (int*)(locks + TQ);                                       // [TQ] query of every pair slot
    int* slot_p = slot_q + TQ;                                              // [TQ] its probe rank

    const LvsIvfItem it = lvs_ivf_work_item(a.g, blockIdx.x);
    if (!it.ok) return;
    const int npair = it.npair;
    lvs_ivf_tile_begin<TQ, LVS_IVF_WAVES * 64>(a.g.pairs, it.p0, npair, a.g.nprobe, tid, lists, KCAP, locks, slot_q, slot_p);
    lvs_ivf_stage_queries(a.g, slot_q, bfrag, tid);

    const int qs = lane & 31;  // this lane's pair slot (lanes l and l + 32 share it)
    const bool qvalid = qs < npair;
    const float qnv = a.g.metric == LVS_METRIC_L2 ? a.g.qn[slot_q[qs]] : 0.f;
    float tauf = -INFINITY;
    const int k = a.k;

    const LvsIvfList L = lvs_ivf_list(a.g, it.list);
    for (int blk = wave; blk < L.nblk; blk += LVS_IVF_WAVES) {
        const LvsIvfRows b = lvs_ivf_block_rows<SEL>(a.g, L, blk, lane);
        if (SEL && b.mask == 0) continue;  // wave-uniform; the block loop has no workgroup barrier
        const uint32_t rid = b.rid;
        const f32x16 acc = lvs_ivf_block_scores<U, true>(a.g, L, bfrag, rid, qnv, lane);
        // ---- block epilogue: lane holds pair slot qs, block rows lvs_ivf_acc_row(r) + 4 (lane >> 5)
        const uint32_t selw = b.mask >> (4 * (lane >> 5));  // bit j = this lane's block row 4 (lane >> 5) + j takes part
        const int brow0 = blk * 32 + 4 * (lane >> 5);
        // does the row of acc[r] take part?  Without a selector `< len` says the same as the mask's bit, and the 768-wide
        // scan is 0.5-1.5 % faster with the compare (profiles/ivf_gather_refactor_ab.json)
        auto on = [&](int r) -> bool {
            if constexpr (SEL) return (selw >> lvs_ivf_acc_row(r)) & 1u;
            else return brow0 + lvs_ivf_acc_row(r) < L.len;
        };
        {
            const uint32_t lo = (uint32_t)(lists[qs * KCAP + k - 1] >> 32);
            tauf = fmaxf(tauf, lvs_tau(lo));
        }
        float best = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) best = on(r) ? fmaxf(best, acc[r]) : best;
        const bool th = qvalid && best >= tauf;
        if (!__any(th)) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = (uint32_t)__shfl((int)rid, lvs_ivf_acc_row(r) + 4 * (lane >> 5), 64);
            const bool pending = th && on(r) && acc[r] >= tauf;
            const u64 key = pending ? lvs_pack_key(acc[r], id) : 0ull;
            lvs_list_insert(__ballot(pending), key, qs, lists, KCAP, locks, k, lane, tauf);
        }
    }
    lvs_ivf_write_parts<LVS_IVF_WAVES * 64>(lists, KCAP, slot_q, slot_p, npair, k, a.nq, tid, a.out);
}

// tile_offs[l] = first work item of list l (exclusive scan of ceil(pairs / 32)), tile_offs[nlist] = work items;
// item_list[w] = list of work item w.  One workgroup of 1024 threads, four lists per thread per round.
__global__ __launch_bounds__(1024) void lvs_ivf_tiles_kernel(const uint32_t* __restrict__ pair_offs, int nlist,
                                                             uint32_t* __restrict__ tile_offs, uint32_t* __restrict__ item_list) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nlist; base += 4096) {
        uint32_t t[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + tid * 4 + u;
            t[u] = i < nlist ? (pair_offs[i + 1] - pair_offs[i] + LVS_IVF_TILEQ - 1) / LVS_IVF_TILEQ : 0u;
            sum += t[u];
        }
        part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
            const uint32_t add = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        uint32_t run = carry + part[tid] - sum;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + tid * 4 + u;
            if (i < nlist) {
                tile_offs[i] = run;
                for (uint32_t w = 0; w < t[u]; ++w) item_list[run + w] = (uint32_t)i;
            }
            run += t[u];
        }
        __syncthreads();
        if (tid == 1023) carry += part[1023];
        __syncthreads();
    }
    if (tid == 0) tile_offs[nlist] = carry;
}

__global__ __launch_bounds__(256) void lvs_ivf_probe_ids_kernel(const u64* __restrict__ keys, long long n,
                                                                int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    out[i] = key == 0 ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
}

__global__ __launch_bounds__(256) void lvs_ivf_offsets_kernel(const uint32_t* __restrict__ offs, int n, int64_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n) out[i] = (int64_t)offs[i];
}

template <int U, bool SEL>
hipError_t ivf_scan_launch_u(const LvsIvfArgs& a, int64_t max_items, hipStream_t stream) {
    return lvs_launch_lds<lvs_ivf_scan_kernel<U, SEL>>(dim3((unsigned)max_items), dim3(LVS_IVF_WAVES * 64),
                                                       lvs_ivf_lds_bytes(a.g.nbfrag, a.kcap), stream, a);
}

}  // namespace

hipError_t lvs_ivf_tiles_launch(const uint32_t* pair_offs, int nlist, uint32_t* tile_offs, uint32_t* item_list,
                                hipStream_t stream) {
    hipLaunchKernelGGL(lvs_ivf_tiles_kernel, dim3(1), dim3(1024), 0, stream, pair_offs, nlist, tile_offs, item_list);
    return hipGetLastError();
}

// jper = dpad / 16 is a multiple of 4 (dpad is a multiple of 64): batches of 8 fragments where they divide it, else 4
hipError_t lvs_ivf_scan_launch(const LvsIvfArgs& a, int64_t max_items, hipStream_t stream) {
    if (a.g.jper % 4 != 0 || a.k < 1 || a.k > a.kcap || a.kcap > 64 || a.g.nseg < 1 || a.g.nseg > 3) return hipErrorInvalidValue;
    if (max_items <= 0) return hipSuccess;
    if (a.g.sel) return a.g.jper % 8 == 0 ? ivf_scan_launch_u<8, true>(a, max_items, stream) : ivf_scan_launch_u<4, true>(a, max_items, stream);
    if (a.g.jper % 8 == 0) return ivf_scan_launch_u<8, false>(a, max_items, stream);
    return ivf_scan_launch_u<4, false>(a, max_items, stream);
}

hipError_t lvs_ivf_probe_ids_launch(const u64* keys, int64_t n, int32_t* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lvs_ivf_probe_ids_kernel, dim3((unsigned)lvs_ceil_div(n, 256)), dim3(256), 0, stream, keys, (long long)n, out);
    return hipGetLastError();
}

hipError_t lvs_ivf_offsets_launch(const uint32_t* offs, int nlist, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(lvs_ivf_offsets_kernel, dim3((unsigned)lvs_ceil_div(nlist + 1, 256)), dim3(256), 0, stream, offs, nlist, out);
    return hipGetLastError();
}
