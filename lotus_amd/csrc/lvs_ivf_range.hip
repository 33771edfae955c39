// IVF threshold search: the hot kernel of lvs_ivf_range_search (lvs_capi.hip) - faiss IndexIVF::range_search over the
// full-precision rows.  Every row of a query's probed lists whose score exceeds a threshold is emitted, not the k best.
//
// The work item, the tile's queries in LDS, the gathered rows and the MFMA loop that scores a 32-row block against the tile
// are lvs_ivf_gather.h's, shared with lvs_ivf_scan_kernel.  This kernel's own part is what happens to a score:
//   * there are no per-query lists and no locks: LDS holds the fragments and the slot -> query table only, so the bound on d
//     is this kernel's own (lvs_ivf_range_lds_bytes: d <= 2 496 for fp16 queries, 1 216 for hi|lo);
//   * a lane's accumulator is a hit when its block row is inside the list (and selected), its pair slot is valid, its score is
//     > threshold (strict, in the scaled fp32 domain lvs_range_join compares in) and its row is not the query's own
//     (q_rows).  "Any hit in this block" is one __any - most blocks have none;
//   * a block with hits counts them per lane, prefixes the counts over the wave and takes ONE returning 64-bit atomicAdd per
//     (wave, block) on the call's pair counter; every hit lane then stores (query, row, score) at base + rank while that
//     slot is below the capacity.  Past the capacity hits are counted and never stored (the caller sizes its buffers from
//     the count and runs again).
// Roofline: as the scan's - a work item reads its whole list, so a list is read once per tile of 32
// probing pairs; section 3.12.
#include "lvs_ivf_gather.h"

namespace {

template <int U, bool SEL>
__global__ __launch_bounds__(LVS_IVF_WAVES * 64) void lvs_ivf_range_kernel(const LvsIvfRangeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TQ = LVS_IVF_TILEQ;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    half8* bfrag = (half8*)smem;                                // [nbfrag][64]
    int* slot_q = (int*)(smem + (size_t)a.g.nbfrag * 1024);     // [TQ] query of every pair slot

    const LvsIvfItem it = lvs_ivf_work_item(a.g, blockIdx.x);
    if (!it.ok) return;
    const int npair = it.npair;
    if (tid < TQ) slot_q[tid] = (int)(a.g.pairs[it.p0 + (tid < npair ? tid : 0)] / (uint32_t)a.g.nprobe);  // empty slots repeat the first
    __syncthreads();
    lvs_ivf_stage_queries(a.g, slot_q, bfrag, tid);

    const int qs = lane & 31;  // this lane's pair slot (lanes l and l + 32 share it)
    const bool qvalid = qs < npair;
    const int myq = slot_q[qs];
    const float qnv = a.g.metric == LVS_METRIC_L2 ? a.g.qn[myq] : 0.f;
    const uint32_t own = a.q_rows ? a.q_rows[myq] : 0xFFFFFFFFu;  // the query's own row (row numbers are < 2^32 - 1)
    const float thr = a.threshold;

    const LvsIvfList L = lvs_ivf_list(a.g, it.list);
    for (int blk = wave; blk < L.nblk; blk += LVS_IVF_WAVES) {
        const LvsIvfRows b = lvs_ivf_block_rows<SEL>(a.g, L, blk, lane);
        if (SEL && b.mask == 0) continue;  // wave-uniform; the block loop has no workgroup barrier
        const uint32_t rid = b.rid;
        const f32x16 acc = lvs_ivf_block_scores<U, false>(a.g, L, bfrag, rid, qnv, lane);
        // ---- block epilogue: lane holds pair slot qs, block rows lvs_ivf_acc_row(r) + 4 (lane >> 5)
        const uint32_t selw = b.mask >> (4 * (lane >> 5));  // bit j = this lane's block row 4 (lane >> 5) + j takes part
        float best = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) best = (selw >> lvs_ivf_acc_row(r)) & 1u ? fmaxf(best, acc[r]) : best;
        if (!__any(qvalid && best > thr)) continue;
        // ---- a block with hits: which of this lane's 16 scores, how many, where in the wave's run of slots
        uint32_t hits = 0;  // bit r = acc[r] is a hit
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = (uint32_t)__shfl((int)rid, lvs_ivf_acc_row(r) + 4 * (lane >> 5), 64);
            const bool hit = qvalid && ((selw >> lvs_ivf_acc_row(r)) & 1u) && acc[r] > thr && id != own;
            hits |= hit ? 1u << r : 0u;
        }
        const int cnt = __popc(hits);
        int incl = cnt;  // inclusive prefix of the counts over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            incl += lane >= off ? up : 0;
        }
        const int total = __shfl(incl, 63, 64);
        if (total == 0) continue;  // the only scores above the threshold were the queries' own rows
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.out_count, (unsigned long long)total);  // one per (wave, block)
        base = lvs_shfl_u64(base, 0);
        long long pos = (long long)base + (incl - cnt);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = (uint32_t)__shfl((int)rid, lvs_ivf_acc_row(r) + 4 * (lane >> 5), 64);
            if ((hits >> r) & 1u) {
                if (pos < a.capacity) {
                    a.out_q[pos] = (long long)myq + a.q_base;
                    a.out_j[pos] = (long long)id;
                    a.out_s[pos] = acc[r] * a.out_scale;
                }
                ++pos;
            }
        }
    }
}

template <int U, bool SEL>
hipError_t ivf_range_launch_u(const LvsIvfRangeArgs& a, int64_t max_items, hipStream_t stream) {
    return lvs_launch_lds<lvs_ivf_range_kernel<U, SEL>>(dim3((unsigned)max_items), dim3(LVS_IVF_WAVES * 64),
                                                        lvs_ivf_range_lds_bytes(a.g.nbfrag), stream, a);
}

}  // namespace

// jper = dpad / 16 is a multiple of 4 (dpad is a multiple of 64): batches of 8 fragments where they divide it, else 4
hipError_t lvs_ivf_range_launch(const LvsIvfRangeArgs& a, int64_t max_items, hipStream_t stream) {
    if (a.g.jper % 4 != 0 || a.g.nseg < 1 || a.g.nseg > 3 || a.capacity < 0 || !a.out_count ||
        lvs_ivf_range_lds_bytes(a.g.nbfrag) > LVS_LDS_MAX)
        return hipErrorInvalidValue;
    if (max_items <= 0) return hipSuccess;
    if (a.g.sel) return a.g.jper % 8 == 0 ? ivf_range_launch_u<8, true>(a, max_items, stream) : ivf_range_launch_u<4, true>(a, max_items, stream);
    if (a.g.jper % 8 == 0) return ivf_range_launch_u<8, false>(a, max_items, stream);
    return ivf_range_launch_u<4, false>(a, max_items, stream);
}
