// IVF-Flat list scan: the hot kernel of lvs_ivf_search_keys (lvs_capi.hip).
//
// An IVF search probes nprobe of nlist inverted lists per query.  The (query, probe rank) pairs are grouped by list
// (the bucket sort of lvs_count_sort.hip), and one work item is one list together with a tile of up to 32 of the pairs that
// probe it:
//   * the tile's queries live in LDS as ready-made MFMA B fragments, laid out as in lvs_stream_kernel
//     ([nbfrag][64 lanes][16 B], lane-linear -> conflict-free ds_read_b128);
//   * the list's rows are GATHERED by number from the flat packed image: lane (r, h) of a wave reads 16 B of row
//     rows[offsets[l] + 32 b + r] per fragment - lvs_stream_kernel's lane-to-row load with an indexed row base instead of a
//     linear one.  A gathered row is 1-3 KB read in 128-B lines, which HBM serves at the rate of a sweep, so the corpus is
//     never copied into list order;
//   * each wave takes every fourth 32-row block of the list: v_mfma_f32_32x32x16_f16 on 32 rows x 32 queries per K step,
//     hi|lo operands as the K segments hi.hi + hi.lo + lo.hi (fp32-accurate, like the flat path); the fragments of the next
//     K step are loaded while the current ones are multiplied;
//   * hits go through the wave-cooperative sorted insertion (lvs_list_insert, lvs_common.h) into per-query lists in LDS (one
//     lock per query: the four waves share the tile).  Keys carry the GLOBAL row number, so ties between rows of different
//     lists keep the oracle's total order when the per-probe lists are merged (lvs_merge_keys);
//   * the work item writes its k keys per pair to the part of the pair's probe rank: parts [nprobe][nq][k].
//
// Rooflines (1 M x 768 fp16, nlist 4 096, nprobe 32 -> ~7 800 rows per query): one query is HBM-bound, 12 MB of rows over
// 8 TB/s = 1.5 us, in practice bounded by the latency of a few dozen workgroups; 10 000 queries are 120 GFLOP (48 us at
// 2.5 PFLOP/s), but every work item reads its whole list and a list serves ~3 tiles, so ~4.6 GB of row reads make this
// tiling bandwidth-bound at ~0.58 ms.  The LDS image bounds d: lvs_ivf_search_workspace_bytes.
#include "lvs_common.h"
#include "lvs_tile.h"

namespace {

// SEL: only the rows whose bit is set in a.sel (bit r & 31 of word r >> 5 for row r of the flat image) take part.  A wave
// looks its 32 rows' bits up right after their numbers and skips the block before any row data when none is selected; the
// 32-bit ballot of (inside the list and selected), indexed by the block row, masks the epilogue in place of the `< len` test.
template <int U, bool SEL>
__global__ __launch_bounds__(LVS_IVF_WAVES * 64) void lvs_ivf_scan_kernel(const LvsIvfArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TQ = LVS_IVF_TILEQ;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KCAP = a.kcap;
    half8* bfrag = (half8*)smem;                                            // [nbfrag][64]
    u64* lists = (u64*)(smem + (size_t)a.nbfrag * 1024);                    // [TQ][KCAP]
    uint32_t* locks = (uint32_t*)((char*)lists + (size_t)TQ * KCAP * 8);    // [TQ]
    int* slot_q = (int*)(locks + TQ);                                       // [TQ] query of every pair slot
    int* slot_p = slot_q + TQ;                                              // [TQ] its probe rank

    // ---- work item -> (list, tile of pairs)
    const uint32_t wi = blockIdx.x;
    if (wi >= a.tile_offs[a.nlist]) return;  // the grid is an upper bound of the work items
    const int l = (int)a.item_list[wi];
    const uint32_t p0 = a.pair_offs[l] + (wi - a.tile_offs[l]) * TQ;
    const uint32_t pend = a.pair_offs[l + 1];
    const int npair = (int)(pend - p0 < (uint32_t)TQ ? pend - p0 : (uint32_t)TQ);  // >= 1
    lvs_ivf_tile_begin<TQ, LVS_IVF_WAVES * 64>(a.pairs, p0, npair, a.nprobe, tid, lists, KCAP, locks, slot_q, slot_p);
    // ---- queries -> LDS as B fragments: fragment f, lane v = pair slot (v & 31), halfs (v >> 5) * 8 .. + 8
    const _Float16* xq = (const _Float16*)a.xq;
    for (int idx = tid; idx < a.nbfrag * 64; idx += LVS_IVF_WAVES * 64) {
        const int v = idx & 63, f = idx >> 6;
        const int part = f / a.jper, jj = f - part * a.jper;  // part 0: columns [0, dpad), part 1: [dpad, 2 dpad)
        const long long q = slot_q[v & 31];
        bfrag[idx] = *(const half8*)(xq + q * a.ldq + part * a.jper * 16 + jj * 16 + (v >> 5) * 8);
    }
    __syncthreads();

    const int qs = lane & 31;  // this lane's pair slot (lanes l and l + 32 share it)
    const bool qvalid = qs < npair;
    const float qnv = a.metric == LVS_METRIC_L2 ? a.qn[slot_q[qs]] : 0.f;
    float tauf = -INFINITY;
    const int k = a.k;

    const _Float16* xb = (const _Float16*)a.xb;
    const long long r0 = a.offsets[l];
    const int len = (int)(a.offsets[l + 1] - r0);
    const int nblk = (len + 31) / 32;
    const int jper = a.jper, nj = a.nseg * jper;
    const int segc0 = a.seg_c[0], segc1 = a.seg_c[1], segc2 = a.seg_c[2];
    const int segb0 = a.seg_b[0], segb1 = a.seg_b[1], segb2 = a.seg_b[2];

    for (int blk = wave; blk < nblk; blk += LVS_IVF_WAVES) {
        // the row this lane loads: row (lane & 31) of the block; past the list's end the last row is repeated (masked below)
        int rr = blk * 32 + (lane & 31);
        if (rr > len - 1) rr = len - 1;
        const uint32_t rid = a.rows[r0 + rr];
        uint32_t selm = 0;  // SEL: bit j = block row j is inside the list and selected (lanes j and j + 32 hold the same row)
        if constexpr (SEL) {
            const bool on = blk * 32 + (lane & 31) < len && ((a.sel[rid >> 5] >> (rid & 31)) & 1u);
            selm = (uint32_t)__ballot(on);
            if (selm == 0) continue;  // wave-uniform; the block loop has no workgroup barrier
        }
        const float bnv = a.metric == LVS_METRIC_L2 ? a.bn[rid] : 0.f;
        const _Float16* ap = xb + (long long)rid * a.ldb + (lane >> 5) * 8;
        // fragments f = seg * jper + jj; U divides jper, so a batch of U never crosses a K segment.  The batch after the
        // current one is in flight while the current one is multiplied.
        half8 cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = *(const half8*)(ap + segc0 + u * 16);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int f0 = 0; f0 < nj; f0 += U) {
            const int seg = f0 / jper, jj = f0 - seg * jper;
            if (f0 + U < nj) {
                const int nseg_ = (f0 + U) / jper, njj = f0 + U - nseg_ * jper;
                const int coff = nseg_ == 0 ? segc0 : (nseg_ == 1 ? segc1 : segc2);
                const _Float16* sp = ap + coff + njj * 16;
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = *(const half8*)(sp + u * 16);
            }
            const int boff = seg == 0 ? segb0 : (seg == 1 ? segb1 : segb2);
            const half8* bp = bfrag + (long long)(boff + jj) * 64 + lane;
#pragma unroll
            for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[u], bp[u * 64], acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
        // ---- block epilogue: lane holds pair slot qs, block rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int brow0 = blk * 32 + 4 * (lane >> 5);
        const uint32_t selw = selm >> (4 * (lane >> 5));  // SEL: bit j = this lane's block row 4 (lane >> 5) + j takes part
        if (a.metric == LVS_METRIC_L2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float bv = __shfl(bnv, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), 64);
                acc[r] = -fmaxf((qnv + bv) - 2.0f * acc[r], 0.f);
            }
        }
        {
            const uint32_t lo = (uint32_t)(lists[qs * KCAP + k - 1] >> 32);
            tauf = fmaxf(tauf, lvs_tau(lo));
        }
        float best = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (SEL) best = (selw >> ((r & 3) + 8 * (r >> 2))) & 1u ? fmaxf(best, acc[r]) : best;
            else best = brow0 + (r & 3) + 8 * (r >> 2) < len ? fmaxf(best, acc[r]) : best;
        }
        const bool th = qvalid && best >= tauf;
        if (!__any(th)) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = (uint32_t)__shfl((int)rid, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), 64);
            bool pending;
            if constexpr (SEL) pending = th && ((selw >> ((r & 3) + 8 * (r >> 2))) & 1u) && acc[r] >= tauf;
            else pending = th && brow0 + (r & 3) + 8 * (r >> 2) < len && acc[r] >= tauf;
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
                                                       lvs_ivf_lds_bytes(a.nbfrag, a.kcap), stream, a);
}

}  // namespace

size_t lvs_ivf_lds_bytes(int nbfrag, int kcap) {
    return (size_t)nbfrag * 1024 + (size_t)LVS_IVF_TILEQ * kcap * 8 + (size_t)LVS_IVF_TILEQ * 4 * 3;
}

int lvs_ivf_kcap(int k) { return k <= 16 ? 16 : (k <= 32 ? 32 : 64); }

hipError_t lvs_ivf_tiles_launch(const uint32_t* pair_offs, int nlist, uint32_t* tile_offs, uint32_t* item_list,
                                hipStream_t stream) {
    hipLaunchKernelGGL(lvs_ivf_tiles_kernel, dim3(1), dim3(1024), 0, stream, pair_offs, nlist, tile_offs, item_list);
    return hipGetLastError();
}

// jper = dpad / 16 is a multiple of 4 (dpad is a multiple of 64): batches of 8 fragments where they divide it, else 4
hipError_t lvs_ivf_scan_launch(const LvsIvfArgs& a, int64_t max_items, hipStream_t stream) {
    if (a.jper % 4 != 0 || a.k < 1 || a.k > a.kcap || a.kcap > 64 || a.nseg < 1 || a.nseg > 3) return hipErrorInvalidValue;
    if (max_items <= 0) return hipSuccess;
    if (a.sel) return a.jper % 8 == 0 ? ivf_scan_launch_u<8, true>(a, max_items, stream) : ivf_scan_launch_u<4, true>(a, max_items, stream);
    if (a.jper % 8 == 0) return ivf_scan_launch_u<8, false>(a, max_items, stream);
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
