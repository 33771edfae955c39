// The gathered-row block scorer of the IVF scans over full-precision rows: lvs_ivf_scan_kernel (lvs_ivf.hip, the k best per
// pair) and lvs_ivf_range_kernel (lvs_ivf_range.hip, every score above a threshold) differ only in what happens to a score.
//
// A work item is one inverted list and a tile of up to 32 of the (query, probe rank) pairs that probe it (LvsIvfGatherArgs,
// lvs_tile.h):
//   * the tile's queries live in LDS as ready-made MFMA B fragments, laid out as in lvs_stream_kernel
//     ([nbfrag][64 lanes][16 B], lane-linear -> conflict-free ds_read_b128);
//   * the list's rows are GATHERED by number from the flat packed image: lane (r, h) of a wave reads 16 B of row
//     rows[offsets[l] + 32 b + r] per fragment - lvs_stream_kernel's lane-to-row load with an indexed row base instead of a
//     linear one.  A gathered row is 1-3 KB read in 128-B lines, which HBM serves at the rate of a sweep, so the corpus is
//     never copied into list order;
//   * each wave takes every fourth 32-row block of the list: v_mfma_f32_32x32x16_f16 on 32 rows x 32 queries per K step,
//     hi|lo operands as the K segments hi.hi + hi.lo + lo.hi (fp32-accurate, like the flat path); the fragments of the next
//     batch are loaded while the current ones are multiplied; squared L2 is -max(qn + bn - 2 acc, 0);
//   * a 32-bit mask says which of a block's rows take part: inside the list and, under SEL, selected.  A block without one
//     is skipped before any row data is read; the mask then gates the kernel's epilogue (the scan without a selector tests
//     `< len` there, which says the same).
// The helpers hand their results back by value.  What hipcc makes of the K loop depends on how it is written down, not only
// on what it computes (see the notes in lvs_ivf_block_scores): read the listing and measure after a change to it.
#pragma once
#include "lvs_common.h"
#include "lvs_tile.h"

// work item -> (list, first pair, pairs of the tile); !ok: the grid is an upper bound, this workgroup has no work
struct LvsIvfItem {
    bool ok;
    int list, npair;
    uint32_t p0;
};
__device__ __forceinline__ LvsIvfItem lvs_ivf_work_item(const LvsIvfGatherArgs& g, uint32_t wi) {
    LvsIvfItem it = {false, 0, 0, 0};
    if (wi >= g.tile_offs[g.nlist]) return it;
    it.ok = true;
    it.list = (int)g.item_list[wi];
    it.p0 = g.pair_offs[it.list] + (wi - g.tile_offs[it.list]) * LVS_IVF_TILEQ;
    const uint32_t pend = g.pair_offs[it.list + 1];
    it.npair = (int)(pend - it.p0 < (uint32_t)LVS_IVF_TILEQ ? pend - it.p0 : (uint32_t)LVS_IVF_TILEQ);  // >= 1
    return it;
}

// queries -> LDS as B fragments: fragment f, lane v = pair slot (v & 31), halfs (v >> 5) * 8 .. + 8.  slot_q (LDS) is
// visible to the workgroup on entry; the fragments are on return
__device__ __forceinline__ void lvs_ivf_stage_queries(const LvsIvfGatherArgs& g, const int* slot_q, half8* bfrag, int tid) {
    const _Float16* xq = (const _Float16*)g.xq;
    for (int idx = tid; idx < g.nbfrag * 64; idx += LVS_IVF_WAVES * 64) {
        const int v = idx & 63, f = idx >> 6;
        const int part = f / g.jper, jj = f - part * g.jper;  // part 0: columns [0, dpad), part 1: [dpad, 2 dpad)
        const long long q = slot_q[v & 31];
        bfrag[idx] = *(const half8*)(xq + q * g.ldq + part * g.jper * 16 + jj * 16 + (v >> 5) * 8);
    }
    __syncthreads();
}

// what the blocks of one work item share (wave-uniform)
struct LvsIvfList {
    const uint32_t* rows;  // the list's row numbers
    int len, nblk;         // rows, 32-row blocks
    int jper, nj;          // fragments per K segment, in all
    int segc0, segc1, segc2, segb0, segb1, segb2;  // K segment -> first half of a row, first fragment of the queries
};
__device__ __forceinline__ LvsIvfList lvs_ivf_list(const LvsIvfGatherArgs& g, int l) {
    const long long r0 = g.offsets[l];
    const int len = (int)(g.offsets[l + 1] - r0);
    return {g.rows + r0,  len,         (len + 31) / 32, g.jper,      g.nseg * g.jper, g.seg_c[0],
            g.seg_c[1],   g.seg_c[2],  g.seg_b[0],      g.seg_b[1],  g.seg_b[2]};
}

// a block's rows.  rid: the row this lane loads - row (lane & 31) of the block; past the list's end the last row is repeated
// (masked).  mask: bit j = block row j takes part (lanes j and j + 32 hold the same row); 0: skip the block (wave-uniform)
struct LvsIvfRows {
    uint32_t rid, mask;
};
template <bool SEL>
__device__ __forceinline__ LvsIvfRows lvs_ivf_block_rows(const LvsIvfGatherArgs& g, const LvsIvfList& L, int blk, int lane) {
    int rr = blk * 32 + (lane & 31);
    if (rr > L.len - 1) rr = L.len - 1;
    const uint32_t rid = L.rows[rr];
    bool on = blk * 32 + (lane & 31) < L.len;
    if constexpr (SEL) on = on && ((g.sel[rid >> 5] >> (rid & 31)) & 1u);
    return {rid, (uint32_t)__ballot(on)};
}

// Accumulator register r of a lane holds pair slot lane & 31 and block row lvs_ivf_acc_row(r) + 4 (lane >> 5)
__device__ __forceinline__ int lvs_ivf_acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// a block's scores: rows x the tile's queries over all K segments.  fragments f = seg * jper + jj; U divides jper, so a batch
// of U never crosses a K segment.  The batch after the current one is in flight while the current one is multiplied.
// qnv: |q|^2 of this lane's pair slot (L2 only).  PIN is the caller's choice by measurement (profiles/ivf_gather_refactor_ab.json):
// the scan is 1-2 % faster per call with it (one query most of all), the threshold search 0.2-0.7 % slower
template <int U, bool PIN>
__device__ __forceinline__ f32x16 lvs_ivf_block_scores(const LvsIvfGatherArgs& g, const LvsIvfList& L, const half8* bfrag, uint32_t rid,
                                                       float qnv, int lane) {
    const float bnv = g.metric == LVS_METRIC_L2 ? g.bn[rid] : 0.f;
    const _Float16* ap = (const _Float16*)g.xb + (long long)rid * g.ldb + (lane >> 5) * 8;
    // copies, so that the segment choices below are selects between values (through L they compile to branches)
    const int jper = L.jper, nj = L.nj;
    const int segc0 = L.segc0, segc1 = L.segc1, segc2 = L.segc2, segb0 = L.segb0, segb1 = L.segb1, segb2 = L.segb2;
    // a batch is ONE value, copied whole (v_mov_b64 pairs): as two arrays copied fragment by fragment the compiler moves
    // them dword by dword at the end of every K step, which cost lvs_ivf_range_kernel 3-5 % (profiles/ivf_gather_refactor_ab.json)
    struct Batch {
        half8 v[U];
    } cur, nxt;
    // PIN: the first batch is issued in fragment order (hipcc issues it last fragment first): MFMA u then waits for loads
    // 0 .. u alone - the descending s_waitcnt vmcnt ladder under the MFMAs - and not for the whole next batch as well
#pragma unroll
    for (int u = 0; u < U; ++u) {
        cur.v[u] = *(const half8*)(ap + segc0 + u * 16);
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
    }
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
            for (int u = 0; u < U; ++u) nxt.v[u] = *(const half8*)(sp + u * 16);
        }
        const int boff = seg == 0 ? segb0 : (seg == 1 ? segb1 : segb2);
        const half8* bp = bfrag + (long long)(boff + jj) * 64 + lane;
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.v[u], bp[u * 64], acc, 0, 0, 0);
        cur = nxt;
    }
    if (g.metric == LVS_METRIC_L2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float bv = __shfl(bnv, lvs_ivf_acc_row(r) + 4 * (lane >> 5), 64);
            acc[r] = -fmaxf((qnv + bv) - 2.0f * acc[r], 0.f);
        }
    }
    return acc;
}
