// The host planner of the searches through inverted lists (top-k over the rows, the SQ8 codes and the PQ codes; the threshold
// search) and of the bucket sort they invert their probes with: every size, fit and chunk, as pure functions of integers.
// Like lvs_plan.h - the only project header included - a plain C++17 host compiler builds this file
// (tests/native/plan_check.cpp runs it).  lvs_tile.h and lvs_count_sort.h include it.
#pragma once
#include "lvs_plan.h"

// ---- exclusive scan and bucket sort (lvs_count_sort.hip) -------------------------------------------------------------------
constexpr int LVS_SCAN_SEG = 2048;  // counters per workgroup of the scan
inline int64_t lvs_scan_scratch_bytes(int64_t total) { return lvs_ceil_div(total, LVS_SCAN_SEG) * 4 + 4; }

constexpr int BUCKET_CHUNK = 8192;
constexpr int BUCKET_MAX_BINS = 24576;  // (k + 1) * 4 B of LDS per workgroup; larger k sorts by two digits
struct BucketPlan {
    int nchunks, passes, nbins[2], shift[2];
    uint32_t mask[2];
    int64_t off_counts, off_seg, off_rows_a, off_rows_b, off_offs, total;
};
inline bool bucket_plan(int64_t n, int32_t k, BucketPlan& p) {
    if (n < 0 || k <= 0 || n >= 0xFFFFFFFFll) return false;
    p.nchunks = (int)lvs_ceil_div(n > 0 ? n : 1, BUCKET_CHUNK);
    if (k + 1 <= BUCKET_MAX_BINS) {
        p.passes = 1;
        p.nbins[0] = k + 1;
        p.shift[0] = 0;
        p.mask[0] = 0xFFFFFFFFu;
        p.nbins[1] = 0;
        p.shift[1] = 0;
        p.mask[1] = 0;
    } else {  // two stable passes: low 12 bits, then the rest
        p.passes = 2;
        p.nbins[0] = 4096;
        p.shift[0] = 0;
        p.mask[0] = 4095u;
        p.nbins[1] = (k >> 12) + 1;
        p.shift[1] = 12;
        p.mask[1] = 0xFFFFFFFFu;
        if (p.nbins[1] > BUCKET_MAX_BINS) return false;  // k >= 2^26.5: not a k-means anyone runs
    }
    const int64_t maxbins = p.nbins[0] > p.nbins[1] ? p.nbins[0] : p.nbins[1];
    int64_t off = 0;
    p.off_counts = off;
    off += lvs_round_up(maxbins * p.nchunks * 4, 256);
    p.off_seg = off;
    off += lvs_round_up(lvs_scan_scratch_bytes(maxbins * p.nchunks), 256);
    p.off_rows_a = off;
    off += lvs_round_up(n * 4, 256);
    p.off_rows_b = off;
    off += p.passes > 1 ? lvs_round_up(n * 4, 256) : 0;
    p.off_offs = off;
    off += lvs_round_up((int64_t)(k + 2) * 4, 256);
    p.total = off;
    return true;
}
inline int64_t lvs_bucket_workspace_bytes(int64_t n, int32_t k) {
    BucketPlan p;
    return bucket_plan(n, k, p) ? p.total : (int64_t)LVS_EINVAL;
}

// ---- the list scans' shapes ------------------------------------------------------------------------------------------------
#define LVS_IVF_TILEQ 32     // lvs_ivf.hip, lvs_ivf_range.hip: pairs per work item (MFMA N)
#define LVS_SQ8_TILEQ 16     // lvs_ivf_sq8.hip: pairs per work item (MFMA N of v_mfma_f32_16x16x32_f16)
#define LVS_PQ_KSUB 256      // lvs_ivf_pq.hip: lookup-table entries per subspace (8-bit codes; codebooks may hold fewer)
#define LVS_PQ_MAXRANGE 16   //                 probes per workgroup of the scan
enum { LVS_IVF_FLAT = 0, LVS_IVF_SQ8 = 1, LVS_IVF_PQ = 2, LVS_IVF_RANGE = 3 };  // the four searches through the lists

inline int lvs_ivf_kcap(int k) { return k <= 16 ? 16 : (k <= 32 ? 32 : 64); }  // list slots per pair in LDS
inline int lvs_ivf_sq8_ldc(int d) { return (int)lvs_round_up(d, 64); }           // SQ8 code bytes per row
inline int lvs_ivf_pq_ldc(int M) { return (int)lvs_round_up(M, 16); }            // PQ code bytes per row
// work items of a launch can never exceed this bound (sum over lists of ceil(pairs / 32))
inline int64_t lvs_ivf_max_items(int64_t npairs, int32_t nlist) { return npairs / LVS_IVF_TILEQ + nlist + 1; }

// LDS image of a workgroup.  Flat: the tile's query fragments (1 KB each) + its lists, locks and slot tables; threshold scan:
// the fragments + the slot -> query table; SQ8: the tile's w fragments, hi|lo whatever the query's pack mode, + its lists and
// five per-slot tables; PQ: one query's fp32 table of M x 256 entries + its list and the probe range's tables
inline size_t lvs_ivf_lds_bytes(int nbfrag, int kcap) {
    return (size_t)nbfrag * 1024 + (size_t)LVS_IVF_TILEQ * kcap * 8 + (size_t)LVS_IVF_TILEQ * 4 * 3;
}
inline size_t lvs_ivf_range_lds_bytes(int nbfrag) { return (size_t)nbfrag * 1024 + (size_t)LVS_IVF_TILEQ * 4; }
inline size_t lvs_ivf_sq8_lds_bytes(int ldc, int kcap) {
    return (size_t)(ldc / 32) * 2 * 1024 + (size_t)LVS_SQ8_TILEQ * kcap * 8 + (size_t)LVS_SQ8_TILEQ * 4 * 5;
}
inline size_t lvs_ivf_pq_lds_bytes(int M, int kcap) {
    return (size_t)M * LVS_PQ_KSUB * 4 + (size_t)kcap * 8 + 16 + (size_t)LVS_PQ_MAXRANGE * 4 * 3 + 4;
}
// Does the mode's LDS image fit a workgroup for queries of dimension d packed with xq_pack?  Flat, hi|lo queries: d <= 1088
// (k <= 16: 1216), fp16 queries: d <= 2240 (2432); threshold scan: d <= 1216 / 2496; SQ8: d <= 2368 (k <= 32: 2432) whatever
// the pack mode; PQ: M <= 159, whatever d and k.  Larger shapes are not served: the caller searches (joins) them exactly
inline bool lvs_ivf_fits(int mode, int32_t d, int32_t M, int32_t k, int32_t xq_pack) {
    if (mode == LVS_IVF_SQ8) return lvs_ivf_sq8_lds_bytes(lvs_ivf_sq8_ldc(d), lvs_ivf_kcap(k)) <= LVS_LDS_MAX;
    if (mode == LVS_IVF_PQ) return lvs_ivf_pq_lds_bytes(M, lvs_ivf_kcap(k)) <= LVS_LDS_MAX;
    LvsLayout l;
    if (lvs_layout(d, xq_pack, xq_pack, false, l) != LVS_OK) return false;
    return (mode == LVS_IVF_RANGE ? lvs_ivf_range_lds_bytes(l.nbfrag) : lvs_ivf_lds_bytes(l.nbfrag, lvs_ivf_kcap(k))) <= LVS_LDS_MAX;
}

// probes per PQ scan workgroup: enough for ~2 048 rows of the average list (the table's staging and the first insertions
// are paid once per workgroup), but no fewer than ~512 workgroups per chunk while the probes allow it; at most LVS_PQ_MAXRANGE
inline int32_t lvs_ivf_pq_prange(int64_t nb, int32_t nlist, int64_t cn, int32_t nprobe) {
    const int64_t avg = nb / nlist > 0 ? nb / nlist : 1;
    int64_t pr = (2048 + avg - 1) / avg;
    const int64_t by_blocks = cn * nprobe / 512;
    if (pr > by_blocks) pr = by_blocks;
    if (pr > LVS_PQ_MAXRANGE) pr = LVS_PQ_MAXRANGE;
    if (pr > nprobe) pr = nprobe;
    return pr < 1 ? 1 : (int32_t)pr;
}

// ---- scratch of a search and its chunk of queries -----------------------------------------------------------------------
constexpr int64_t IVF_WS_BUDGET = 512ll << 20;  // scratch of one call; more queries go through in chunks
constexpr int64_t IVF_CHUNK_MAX = 16384;

struct LvsIvfPlan {
    int64_t chunk;  // queries per chunk
    int64_t off_coarse, off_extra, off_sort, off_tiles, off_items, off_parts, flat_bytes, sort_bytes, max_items, total;
};
// scratch of a call in chunks of `c` queries and a shorter last chunk of `tail` (0: none): [flat search scratch | coarse keys
// [c][nprobe] | the mode's own region, extra_per_q bytes per query (PQ: tables [c][M][256] fp32) | tiled modes (all but PQ):
// bucket sort | tile offsets | work items | parts [<= nprobe][c][k] (the threshold search, k = 0: none - its pairs go to the
// caller's buffers)].  The flat search's declared size is not monotone in its query count (fewer queries can take a path with
// more lists per query, or gain a two-phase plan), so the coarse step's region holds the larger of the two chunk lengths'
// sizes; every other region grows with the chunk.
inline bool lvs_ivf_layout(int64_t c, int64_t tail, int32_t nlist, int32_t nprobe, int32_t d, int32_t k, int32_t c_pack,
                           int32_t xq_pack, int64_t extra_per_q, bool tiled, LvsIvfPlan& L) {
    L.chunk = c;
    L.flat_bytes = lvs_flat_workspace_bytes(c, nlist, d, nprobe, c_pack, xq_pack);
    if (L.flat_bytes < 0) return false;
    if (tail > 0) {
        const int64_t tail_bytes = lvs_flat_workspace_bytes(tail, nlist, d, nprobe, c_pack, xq_pack);
        if (tail_bytes < 0) return false;
        if (tail_bytes > L.flat_bytes) L.flat_bytes = tail_bytes;
    }
    const int64_t npairs = c * nprobe;
    int64_t off = lvs_round_up(L.flat_bytes, 256);
    L.off_coarse = off;
    off += lvs_round_up(npairs * 8, 256);
    L.off_extra = off;
    off += lvs_round_up(c * extra_per_q, 256);
    L.off_sort = L.off_tiles = L.off_items = off;
    L.sort_bytes = L.max_items = 0;
    if (tiled) {
        L.sort_bytes = lvs_bucket_workspace_bytes(npairs, nlist);
        if (L.sort_bytes < 0) return false;
        L.max_items = lvs_ivf_max_items(npairs, nlist);
        off += lvs_round_up(L.sort_bytes, 256);
        L.off_tiles = off;
        off += lvs_round_up((int64_t)(nlist + 1) * 4, 256);
        L.off_items = off;
        off += lvs_round_up(L.max_items * 4, 256);
    }
    L.off_parts = off;
    off += lvs_round_up(npairs * k * 8, 256);
    L.total = off;
    return true;
}
// The plan of one search: the argument checks the four searches share, the mode's fit, then the chunk - it depends on the
// arguments only: the largest of min(nq, 16 384) halved (rounding up) whose scratch fits the budget - and its layout.  The chunks
// a call runs have two lengths at most: c, and nq % c for the last one.  M: PQ's subspaces (1 otherwise); k: 0 for the threshold
// search.  LVS_EUNSUPPORTED: a valid shape beyond the mode's scan
inline int lvs_ivf_plan(int mode, int64_t nq, int32_t nlist, int32_t nprobe, int32_t d, int32_t M, int32_t k, int32_t c_pack,
                        int32_t xq_pack, LvsIvfPlan& L) {
    if (nq < 0 || nlist < 1 || nprobe < 1 || nprobe > nlist || nprobe > LVS_MAX_K || d <= 0) return LVS_EINVAL;
    if (mode != LVS_IVF_RANGE && (k < 1 || k > LVS_KPASS || M < 1 || d % M != 0)) return LVS_EINVAL;
    if (!lvs_pack_ok(c_pack) || !lvs_pack_ok(xq_pack)) return LVS_EINVAL;
    if (!lvs_ivf_fits(mode, d, M, k, xq_pack)) return LVS_EUNSUPPORTED;
    const int64_t extra_per_q = mode == LVS_IVF_PQ ? (int64_t)M * LVS_PQ_KSUB * 4 : 0;
    int64_t c = nq < IVF_CHUNK_MAX ? nq : IVF_CHUNK_MAX;
    if (c < 1) c = 1;
    for (;;) {
        if (!lvs_ivf_layout(c, nq % c, nlist, nprobe, d, mode == LVS_IVF_RANGE ? 0 : k, c_pack, xq_pack, extra_per_q,
                            mode != LVS_IVF_PQ, L))
            return LVS_EINVAL;
        if (L.total <= IVF_WS_BUDGET || c == 1) return c * nprobe < 0xFFFFFFFFll ? LVS_OK : LVS_EINVAL;
        c = (c + 1) / 2;
    }
}
inline int64_t lvs_ivf_plan_bytes(int mode, int64_t nq, int32_t nlist, int32_t nprobe, int32_t d, int32_t M, int32_t k,
                                  int32_t pack) {
    LvsIvfPlan L;
    const int rc = lvs_ivf_plan(mode, nq, nlist, nprobe, d, M, k, pack, pack, L);
    return rc == LVS_OK ? L.total : (int64_t)rc;
}
