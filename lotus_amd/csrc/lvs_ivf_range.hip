// IVF threshold search: the hot kernel of lvs_ivf_range_search (lvs_capi.hip) - faiss IndexIVF::range_search over the
// full-precision rows.  Every row of a query's probed lists whose score exceeds a threshold is emitted, not the k best.
//
// The work item and the MFMA loop are lvs_ivf_scan_kernel's (lvs_ivf.hip): one list x a tile of up to 32 of the (query, probe
// rank) pairs that probe it; the tile's queries in LDS as B fragments; the list's rows gathered by number into A fragments;
// each of the four waves takes every fourth 32-row block; v_mfma_f32_32x32x16_f16 with hi|lo operands as K segments; the next
// batch of fragments loads while the current one multiplies; squared L2 as -max(qn + bn - 2 acc, 0); the SEL ballot skips
// blocks without a selected row.  What differs is what happens to a score:
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
#include "lvs_common.h"
#include "lvs_tile.h"

namespace {

template <int U, bool SEL>
__global__ __launch_bounds__(LVS_IVF_WAVES * 64) void lvs_ivf_range_kernel(const LvsIvfRangeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TQ = LVS_IVF_TILEQ;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    half8* bfrag = (half8*)smem;                                // [nbfrag][64]
    int* slot_q = (int*)(smem + (size_t)a.nbfrag * 1024);       // [TQ] query of every pair slot

    // ---- work item -> (list, tile of pairs)
    const uint32_t wi = blockIdx.x;
    if (wi >= a.tile_offs[a.nlist]) return;  // the grid is an upper bound of the work items
    const int l = (int)a.item_list[wi];
    const uint32_t p0 = a.pair_offs[l] + (wi - a.tile_offs[l]) * TQ;
    const uint32_t pend = a.pair_offs[l + 1];
    const int npair = (int)(pend - p0 < (uint32_t)TQ ? pend - p0 : (uint32_t)TQ);  // >= 1
    if (tid < TQ) slot_q[tid] = (int)(a.pairs[p0 + (tid < npair ? tid : 0)] / (uint32_t)a.nprobe);  // empty slots repeat the first
    __syncthreads();
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
    const int myq = slot_q[qs];
    const float qnv = a.metric == LVS_METRIC_L2 ? a.qn[myq] : 0.f;
    const uint32_t own = a.q_rows ? a.q_rows[myq] : 0xFFFFFFFFu;  // the query's own row (row numbers are < 2^32 - 1)
    const float thr = a.threshold;

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
        // bit j = block row j takes part: inside the list and (SEL) selected (lanes j and j + 32 hold the same row)
        bool on = blk * 32 + (lane & 31) < len;
        if constexpr (SEL) on = on && ((a.sel[rid >> 5] >> (rid & 31)) & 1u);
        const uint32_t selm = (uint32_t)__ballot(on);
        if constexpr (SEL) {
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
        const uint32_t selw = selm >> (4 * (lane >> 5));  // bit j = this lane's block row 4 (lane >> 5) + j takes part
        if (a.metric == LVS_METRIC_L2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float bv = __shfl(bnv, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), 64);
                acc[r] = -fmaxf((qnv + bv) - 2.0f * acc[r], 0.f);
            }
        }
        float best = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) best = (selw >> ((r & 3) + 8 * (r >> 2))) & 1u ? fmaxf(best, acc[r]) : best;
        if (!__any(qvalid && best > thr)) continue;
        // ---- a block with hits: which of this lane's 16 scores, how many, where in the wave's run of slots
        uint32_t hits = 0;  // bit r = acc[r] is a hit
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t id = (uint32_t)__shfl((int)rid, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), 64);
            const bool hit = qvalid && ((selw >> ((r & 3) + 8 * (r >> 2))) & 1u) && acc[r] > thr && id != own;
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
            const uint32_t id = (uint32_t)__shfl((int)rid, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), 64);
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
                                                        lvs_ivf_range_lds_bytes(a.nbfrag), stream, a);
}

}  // namespace

// the tile's query fragments (1 KB each) + the slot -> query table
size_t lvs_ivf_range_lds_bytes(int nbfrag) { return (size_t)nbfrag * 1024 + (size_t)LVS_IVF_TILEQ * 4; }

// jper = dpad / 16 is a multiple of 4 (dpad is a multiple of 64): batches of 8 fragments where they divide it, else 4
hipError_t lvs_ivf_range_launch(const LvsIvfRangeArgs& a, int64_t max_items, hipStream_t stream) {
    if (a.jper % 4 != 0 || a.nseg < 1 || a.nseg > 3 || a.capacity < 0 || !a.out_count ||
        lvs_ivf_range_lds_bytes(a.nbfrag) > 160 * 1024)
        return hipErrorInvalidValue;
    if (max_items <= 0) return hipSuccess;
    if (a.sel) return a.jper % 8 == 0 ? ivf_range_launch_u<8, true>(a, max_items, stream) : ivf_range_launch_u<4, true>(a, max_items, stream);
    if (a.jper % 8 == 0) return ivf_range_launch_u<8, false>(a, max_items, stream);
    return ivf_range_launch_u<4, false>(a, max_items, stream);
}
