// The flat search's host planner: every decision a search makes before a kernel starts, as pure functions of integers - operand
// layout, the tile kernel's slab and XCD-group geometry, sample sizes, the two-phase plan, the query chunks, the grouped and
// streaming launch geometry, the route and the workspace layout - and the launches of the threshold join.  No HIP header, no
// stream, no device pointer: a plain C++17 host compiler builds this file (tests/native/plan_check.cpp runs it).  lvs_common.h
// and lvs_ivf_plan.h (the searches through inverted lists) include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lotus_hip.h"

#ifdef __HIP__
#define LVS_HD __host__ __device__  // the deal functions below also run in the kernels' prologues
#else
#define LVS_HD
#endif

static inline int64_t lvs_round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
static inline int64_t lvs_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---- tuning / debug knobs ----------------------------------------------------------------------------------
// The shipped library reads NO environment variable: every knob below is a compile-time constant unless the library is
// built with -DLVS_TUNING (`make tuning` -> liblotus_hip_tuning.so, reported by lvs_build_flags()).  Some knobs skip
// work and produce wrong results on purpose (timing ablations); they exist in the tuning build only.
#ifdef LVS_TUNING
#include <stdio.h>
#include <stdlib.h>
static inline long long lvs_tune(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e ? atoll(e) : dflt;
}
static inline bool lvs_tune_set(const char* name) { return getenv(name) != nullptr; }
#else
#define lvs_tune(name, dflt) ((long long)(dflt))
#define lvs_tune_set(name) (false)
#endif

// ---- geometry constants --------------------------------------------------------------------------------------
#define LVS_BC 256          // corpus rows per score tile (MFMA M)
#define LVS_BK 64           // halfs per K-step

#define LVS2_KCAP 15        // 256 x 256 geometry: list slots per query = largest k per pass
#define LVS2_BQ 256         //                     queries per score tile (MFMA N)
#define LVS3_KCAP 56        // 256 x 128 geometry (k > LVS2_KCAP): list slots per query = largest k per pass
#define LVS3_BQ 128
#define LVS_KPASS LVS3_KCAP // largest k any single pass selects; k up to LVS_MAX_K runs ceil(k / LVS_KPASS) passes
constexpr int LVS_SELECT_MAX = 4096;  // most candidates per query select_keys_kernel sorts (32 KB of LDS)
constexpr size_t LVS_LDS_MAX = 160 * 1024;  // LDS a workgroup may use: all of a CU's

// small-batch streaming kernel (lvs_stream.hip): nq <= 256, k <= LVS_KPASS
#define LVS_STREAM_MAXQ 256
#define LVS_STREAM_MAXWG 768   // most corpus ranges (= partial candidate lists per query) a launch may use
#define LVS_STREAM_SEED_ROWS 32768  // sample rows (the first of the shard) whose scores seed the thresholds of a multi-query call
#define LVS_STREAM_BLOCKQ 32   // queries per query block (MFMA N)

// lvs_rq.hip: 97 .. 256 queries with the queries resident in registers
#define LVS_RQ_GROUPQ 256   // queries of one workgroup (eight waves x 32)
#define LVS_RQ_MAXQ 4096    // most queries of a call lvs_rq_fits takes as ONE launch of up to 16 groups (also the seed pass' chunk)
#define LVS_RQ_CHUNK_MAX 65536  // most queries per launch of a chunked call: 256 groups x 1 range
// Largest chunk of a chunked top-k call (rq_chunk_len cuts greedily: 65 536 / 32 768 / 16 384 / 8 192 <= this and <= what is
// left).  The earlier "32 768 is the fastest of 4 096 .. 65 536" (profiles/r10j_join_variants.log, r12d_knobs.log `d_64k`) compared
// it with a 65 536 whose remainder went out in four 8 192-query launches - the slow ones of that same log: it measured the
// remainder rule, not the geometry.  65 536 = 256 groups x 1 range: lvs_rj_kernel runs its form without threshold sharing and
// writes the result itself (no merge).  Measured, plain bench (100 k x 1 M, 20 steps), parent and three builds alternated three
// times on one box (profiles/rj_solo_bench_ab.jsonl): ms per step, median (spread over the alternations) - parent 120.79 (0.11);
// greedy plan at a maximum of 32 768: 120.82 (0.14); maximum 65 536 with the shared form and the merge: 120.21 (0.05); maximum
// 65 536, unshared form, no merge: 118.80 (0.06).  Gap to the parent 1.99 ms = 1.65 % = 18 x the larger spread; kernel ms per step
// 119.10 -> 117.15.  (Estimated before measuring: about 2 ms, 1.5 to 2 %.)
#ifndef LVS_RQ_CHUNK_DEFAULT  // (an A/B build may set another one on the command line)
#define LVS_RQ_CHUNK_DEFAULT 65536
#endif
#define LVS_RANGE_CHUNK 32768  // rows per chunk of the threshold join (lvs_range_join): its epilogue shares nothing and its j > i skipping favours short chunks
#define LVS_RQ_KMAX 16      // most list slots per query
#define LVS_RQ_JOIN_DEFAULT 1  // calls beyond LVS_RQ_MAXQ queries in chunks through lvs_rq_kernel / lvs_rj_kernel (1) or through the list kernel (0)
#define LVS_RQ_SEED_ROWS 65536  // sample rows (the first of the shard) whose scores seed the thresholds: a workgroup sees ~4 000
                                // rows, its lists never fill, so the seed IS its threshold - 64 k rows beat 32 k by 4 % per call, 128 k tie
#define LVS_RQ_JOIN_MINROWS 32768  // shortest corpus (shard) a chunked call takes (r6: 50 k x 50 k 5.3 -> 4.4 ms; at 20 000 rows the list kernel wins)
// lvs_rj.hip: the same launches with ONE wave per SIMD and 64 queries per wave
#define LVS_RJ_DEFAULT 1    // launches lvs_rj_fits accepts go through lvs_rj_kernel (1) or lvs_rq_kernel (0)
#ifndef LVS_RJ_SOLO_DEFAULT  // (an A/B build may set another one on the command line)
#define LVS_RJ_SOLO_DEFAULT 1  // a top-k launch with ONE corpus range: the kernel's form without threshold sharing, lists written straight
                               // to the caller's [nq][k] (1), or the shared form and a one-part merge (0)
#endif

// ---- operand layout ------------------------------------------------------------------------------------------
// Packed rows: d padded to whole K-steps, fp16 (ld = dpad) or fp16 hi|lo (ld = 2 dpad).  A product is a sum over K segments of
// q[seg_q ..] . y[seg_c ..]: x = hi + lo on either side; keep hi*hi plus the first-order cross terms (lo*lo ~ 2^-22 relative is
// dropped).  hi_only: the fp16 "hi" parts only - one K segment whatever the pack modes (lvs_flat_search_keys_hi).
struct LvsLayout {
    int dpad, nkd;           // padded d, in halfs and in K-steps of LVS_BK
    int ldb, ldq;            // leading dimensions in halfs (corpus / queries)
    int nseg, nk;            // K segments; K-steps per tile = nseg * nkd
    int seg_q[3], seg_c[3];  // column offsets (halfs) of each segment in the query / corpus rows
    int nbfrag;              // 16-half B fragments a query holds: its segments' distinct query columns x dpad / 16
};
inline bool lvs_pack_ok(int32_t pack) { return pack == LVS_PACK_F16 || pack == LVS_PACK_SPLIT; }
inline int lvs_layout(int32_t d, int32_t xb_pack, int32_t xq_pack, bool hi_only, LvsLayout& l) {
    if (d <= 0 || !lvs_pack_ok(xb_pack) || !lvs_pack_ok(xq_pack)) return LVS_EINVAL;
    l.dpad = (int)lvs_round_up(d, LVS_BK);
    l.nkd = l.dpad / LVS_BK;
    l.ldb = xb_pack == LVS_PACK_SPLIT ? 2 * l.dpad : l.dpad;
    l.ldq = xq_pack == LVS_PACK_SPLIT ? 2 * l.dpad : l.dpad;
    l.nseg = 0;
    for (int i = 0; i < 3; ++i) l.seg_q[i] = l.seg_c[i] = 0;
    auto seg = [&](int qo, int co) {
        l.seg_q[l.nseg] = qo;
        l.seg_c[l.nseg] = co;
        ++l.nseg;
    };
    seg(0, 0);
    if (xb_pack == LVS_PACK_SPLIT && !hi_only) seg(0, l.dpad);
    if (xq_pack == LVS_PACK_SPLIT && !hi_only) seg(l.dpad, 0);
    l.nk = l.nseg * l.nkd;
    l.nbfrag = ((xq_pack == LVS_PACK_SPLIT && !hi_only) ? 2 : 1) * (l.dpad / 16);
    return LVS_OK;
}

// ---- the (query tile, slab) items of a launch in XCD groups of 32 slots (see item_of_block in lvs_tile.hip) ----
// Three regions, in launch order:
//   lead       the first lead_slabs slab(s) of every query tile in 32-wide groups (32 query tiles x 1 slab);
//   full       the nqt / gq whole query groups: gq query tiles x 32 / gq slabs per group, walking the query groups first,
//              then the slabs;
//   remainder  the last nqt % gq query tiles.  Dealt like the others they would fill (nqt % gq) / gq of every group's slots
//              (49 tiles with gq = 8: one tile x 4 slabs in a 32-slot group, 28 CUs of an XCD idle for every 7th group), so
//              they get groups of their own shape: gqr = the power of two >= the remainder query tiles x 32 / gqr slabs.
struct LvsTileGroups {
    int nqg32, n0;        // lead region: nqg32 groups per slab, n0 in all
    int nqf, nsg, n1;     // full region: nqf query groups x nsg slab groups = n1 groups
    int rem, gqr, nsgr;   // remainder region: rem query tiles, gqr x (32 / gqr) slots per group, nsgr groups
    int total, full;      // all groups; the largest multiple of 8 below (whole generations: one group per XCD)
};
LVS_HD inline LvsTileGroups lvs_tile_groups(int nqt, int nslab, int gq, int lead_slabs) {
    LvsTileGroups g;
    const int gs = 32 / gq;
    const int rest = nslab - lead_slabs;
    g.nqg32 = (nqt + 31) / 32;
    g.n0 = g.nqg32 * lead_slabs;
    g.nqf = nqt / gq;
    g.nsg = (rest + gs - 1) / gs;
    g.n1 = g.nqf * g.nsg;
    g.rem = nqt - g.nqf * gq;
    g.gqr = 1;
    while (g.gqr < g.rem) g.gqr <<= 1;
    g.nsgr = g.rem ? (rest + 32 / g.gqr - 1) / (32 / g.gqr) : 0;
    g.total = g.n0 + g.n1 + g.nsgr;
    g.full = g.total & ~7;
    return g;
}
// slot r (0..31) of group g -> (query tile, slab); false when the slot is empty
LVS_HD inline bool lvs_tile_group_slot(int nqt, int nslab, int gq, int lead_slabs, const LvsTileGroups& gr,
                                       int g, int r, int& qt, int& slab) {
    if (g < gr.n0) {
        slab = g / gr.nqg32;
        qt = (g % gr.nqg32) * 32 + r;
    } else if (g < gr.n0 + gr.n1) {
        const int h = g - gr.n0;
        qt = (h % gr.nqf) * gq + (r % gq);
        slab = lead_slabs + (h / gr.nqf) * (32 / gq) + (r / gq);
    } else {
        const int h = g - gr.n0 - gr.n1;
        if ((r % gr.gqr) >= gr.rem) return false;
        qt = gr.nqf * gq + (r % gr.gqr);
        slab = lead_slabs + h * (32 / gr.gqr) + (r / gr.gqr);
    }
    return qt < nqt && slab < nslab;
}
// valid slots of group g
LVS_HD inline int lvs_tile_group_items(int nqt, int nslab, int gq, int lead_slabs, const LvsTileGroups& gr, int g) {
    int vq, vs;
    if (g < gr.n0) {
        vq = nqt - (g % gr.nqg32) * 32;
        vq = vq > 32 ? 32 : vq;
        vs = 1;
    } else if (g < gr.n0 + gr.n1) {
        vq = gq;
        vs = nslab - lead_slabs - ((g - gr.n0) / gr.nqf) * (32 / gq);
        vs = vs > 32 / gq ? 32 / gq : vs;
    } else {
        vq = gr.rem;
        vs = nslab - lead_slabs - (g - gr.n0 - gr.n1) * (32 / gr.gqr);
        vs = vs > 32 / gr.gqr ? 32 / gr.gqr : vs;
    }
    return (vq < 0 ? 0 : vq) * (vs < 0 ? 0 : vs);
}
// block b of the launch -> (group, slot).  Whole generations: XCD b % 8 runs slot (b / 8) % 32 of group (b / 256) * 8 + b % 8;
// the last total % 8 groups are dealt slot by slot across all XCDs (slot r on XCD r % 8).  false: b is past the last group.
LVS_HD inline bool lvs_tile_block_slot(const LvsTileGroups& gr, int b, int& g, int& r) {
    if (b < gr.full * 32) {
        const int x = b & 7, j = b >> 3;
        g = (j >> 5) * 8 + x;
        r = j & 31;
        return true;
    }
    const int f = b - gr.full * 32;
    g = gr.full + (f >> 5);
    r = f & 31;
    return g < gr.total;
}
inline int lvs_tile_grid_blocks(int nqt, int nslab, int gq, int lead_slabs) {
    return lvs_tile_groups(nqt, nslab, gq, lead_slabs).total * 32;
}

// Items (valid (query tile, slab) pairs) each XCD receives under item_of_block's deal, in units of rounds: an XCD runs 32
// items at a time (one workgroup per CU), so it needs ceil(items / 32) item-times.  Returns the largest over the 8 XCDs.
inline int lvs_tile_xcd_rounds(int nqt, int nslab, int gq, int lead_slabs) {
    const LvsTileGroups gr = lvs_tile_groups(nqt, nslab, gq, lead_slabs);
    long long items[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < gr.full; ++g) items[g & 7] += lvs_tile_group_items(nqt, nslab, gq, lead_slabs, gr, g);
    for (int g = gr.full; g < gr.total; ++g)
        for (int r = 0; r < 32; ++r) {
            int qt, slab;
            if (lvs_tile_group_slot(nqt, nslab, gq, lead_slabs, gr, g, r, qt, slab)) ++items[r & 7];
        }
    long long worst = 0;
    for (int x = 0; x < 8; ++x) worst = items[x] > worst ? items[x] : worst;
    return (int)((worst + 31) / 32);
}

// ---- tile geometry: how a launch of the list kernel (lvs_tile.hip) cuts corpus and queries --------------------------------
struct LvsTileRequest {
    int64_t nq, nb;
    int k;                           // list slots a pass needs (1 for the modes without lists)
    bool force_v2;                   // 256 x 256 geometry whatever k is
    int64_t min_slabs, max_slabs;    // 0: free.  The two-phase search needs that many per-slab lists (make_two_phase_plan)
};
inline LvsTileRequest lvs_tile_request_topk(int64_t nq, int64_t nb, int k) { return {nq, nb, k, false, 0, 0}; }
// SCORES, RANGE, TOP2 and SEED keep no lists: the 256 x 256 geometry
inline LvsTileRequest lvs_tile_request_plain(int64_t nq, int64_t nb) { return {nq, nb, 1, true, 0, 0}; }

struct LvsTileGeom {
    int v2;  // 1: 256 x 256 geometry (k <= LVS2_KCAP, TOP1 / SCORES / RANGE); 0: 256 x 128 geometry (k > LVS2_KCAP)
    int nqt, ntiles;
    int gq, lead_slabs;  // query tiles per XCD group (slabs per group = 32 / gq); slabs walked first in 32-wide groups (0 or 1)
    int nslab, tiles_per_slab;
};

// XCD group = gq query tiles x (32 / gq) slabs resident on one XCD at a time.  Wide groups (one corpus stream per
// XCD) are fastest (profiles/r01_tuning.md) but must be full: groups are dealt round-robin to the 8 XCDs, so a
// half-empty group idles half an XCD.  Take the widest gq that wastes < 15 % of its query-tile slots.
inline int lvs_tile_widest_gq(int nqt) {
    for (int g = 32; g >= 1; g >>= 1) {
        const double fill = (double)nqt / (double)(lvs_ceil_div(nqt, g) * g);
        if (fill >= 0.85) return g;
    }
    return 1;
}
// enough (query tile, slab) items to load-balance 256 CUs
inline int64_t lvs_tile_want_slabs(int nqt) { return lvs_ceil_div(4096, nqt); }
// Long corpus streams: 8 query tiles x 4 slabs per XCD share BOTH operands through the 4 MB L2 (hit rate 37 % -> 70 %,
// half the fabric traffic, +3 % clock).  Measured against the 32 x 1 groups (profiles/r02_tuning.md): 100 k x 1 M
// +9 % on the main loop, 100 k x 500 k 78.1 -> 72.6 ms, 100 k x 250 k 41.5 -> 38.5 ms, no difference at 100 k x 125 k
// (12 slabs of 40 tiles) - so it is used whenever >= 8 narrow slabs of >= 40 tiles exist.  Returns those slabs, or 0.
inline int64_t lvs_tile_l2_slabs(const LvsTileRequest& r, const LvsTileGeom& g, int64_t want) {
    if (!(g.v2 && g.gq > 8 && g.nqt >= 64 && r.min_slabs == 0)) return 0;
    const int64_t l2_min_slabs = lvs_tune("LVS_L2_MIN_SLABS", 8);
    const int64_t n8 = lvs_round_up(want > l2_min_slabs ? want : l2_min_slabs, 4);
    const int64_t min_tiles = lvs_tune("LVS_L2_MIN_TILES", 40);
    return g.ntiles / n8 >= min_tiles ? n8 : 0;
}
// Tail effect.  A launch is nqt * s (query tile, slab) items of equal length; an XCD (32 CUs, one workgroup each) runs
// 32 of ITS items at a time, so the launch lasts max over the XCDs of ceil(items of that XCD / 32) item-times
// (lvs_tile_xcd_rounds follows item_of_block's deal exactly, incl. the last groups spread over all XCDs).  Measured
// with the slab count swept (profiles/r02_tuning.md): 100 k x 1 M at 21 slabs 142.8-147.6 ms, 17 140.5-142.4,
// 13 139.2-139.6.  So among the slab counts near the heuristic's choice s (same group shape, slabs not shorter than the
// heuristic allows: at most hi_lim) take the one with the smallest estimated time = rounds x (item length + its fixed cost).
// (r3: from one full round of items on - launches of a few query tiles run seeded, so an item's fixed cost is the same
// two tiles there, and e.g. 256 queries x 1 M rows go from 489 slabs x 8 tiles in two rounds to 245 x 16 in one)
inline int64_t lvs_tile_tail_slabs(const LvsTileGeom& g, int64_t s, int64_t hi_lim) {
    const int gs = 32 / g.gq;
    const int64_t lead = g.lead_slabs;
    double best_cost = 1e30;
    int64_t best = s;
    for (int64_t c = lead + gs; c <= s + s / 4 && c <= hi_lim && c <= g.ntiles; c += gs) {
        if (10 * c < 3 * s) continue;  // stay within [0.3 s, 1.25 s]
        const int64_t tps = lvs_ceil_div(g.ntiles, c), ns = lvs_ceil_div(g.ntiles, tps);
        const int rounds = lvs_tile_xcd_rounds(g.nqt, (int)ns, g.gq, (int)lead);
        // an item also pays a list cold start and its candidate write-out: about two tiles' worth.  (Round 4 swept a larger
        // fixed cost - 6, 12, 20 tiles, i.e. fewer and longer slabs - over ten shapes: slower everywhere, by up to 19 % at
        // 100 k x 125 k with 3 x 163 instead of 9 x 55 tiles; fine items balance the XCDs better than the round count
        // says.  profiles/r05d_plan_sweep.log)
        const double cost = (double)rounds * (double)(tps + 2);
        const int64_t dist = c > s ? c - s : s - c, bdist = best > s ? best - s : s - best;
        if (cost < best_cost - 1e-9 || (cost < best_cost + 1e-9 && dist < bdist)) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}
// One evaluation of the steps above, with or without the L2 8 x 4 plan; *used_l2: that plan was taken
inline LvsTileGeom lvs_tile_geometry_eval(const LvsTileRequest& r, bool allow_l2, bool* used_l2) {
    LvsTileGeom g;
    g.ntiles = (int)lvs_ceil_div(r.nb > 0 ? r.nb : 1, LVS_BC);
    // geometry: 256 queries per tile with 15 list slots (k <= 15 and every non-top-k mode), else 128 queries / 56 slots
    g.v2 = r.force_v2 || r.k <= LVS2_KCAP;
    // a single, at most half-full query tile: the 128-query geometry does half the (padding) MFMA work
    if (!r.force_v2 && r.k > 1 && r.nq <= LVS3_BQ && lvs_tune("LVS_SMALLQ", 1) != 0) g.v2 = 0;
    g.nqt = (int)lvs_ceil_div(r.nq > 0 ? r.nq : 1, g.v2 ? LVS2_BQ : LVS3_BQ);
    g.gq = lvs_tile_widest_gq(g.nqt);
    const int64_t want = lvs_tile_want_slabs(g.nqt);
    int64_t slabs_l2 = allow_l2 ? lvs_tile_l2_slabs(r, g, want) : 0;
    if (slabs_l2 > 0) g.gq = 8;
    if (lvs_tune_set("LVS_GQ")) {  // -DLVS_TUNING builds only
        const int v = (int)lvs_tune("LVS_GQ", 0);
        if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32) {
            g.gq = v;
            slabs_l2 = 0;
        }
    }
    const int gs = 32 / g.gq;
    // slabs kept >= 32 tiles, a multiple of gs slabs; few query tiles: allow slabs down to 8 tiles so that every CU gets
    // work (cold starts are cheap)
    const int64_t max_slabs = lvs_ceil_div(g.ntiles, g.nqt >= 8 ? 32 : (g.nqt >= 2 ? 16 : 8));
    int64_t s = want < 1 ? 1 : want;
    if (s > max_slabs) s = max_slabs;
    s = lvs_round_up(s, gs);
    if (s > g.ntiles) s = g.ntiles;
    if (s < 1) s = 1;
    g.lead_slabs = 0;
    if (slabs_l2 > 0) {  // one leading slab per query tile in wide groups + slabs_l2 slabs in the narrow groups
        g.lead_slabs = lvs_tune("LVS_LEAD", 1) != 0;
        s = slabs_l2 + g.lead_slabs;
    }
    if (r.min_slabs > 0 && s < r.min_slabs) {  // the caller needs at least this many per-slab candidate lists
        s = lvs_round_up(r.min_slabs, gs);
        if (s > g.ntiles) s = g.ntiles;
    }
    if (r.max_slabs > 0 && s > r.max_slabs) s = r.max_slabs;  // ... and at most this many
    if (r.min_slabs == 0 && r.max_slabs == 0 && (int64_t)g.nqt * s >= lvs_tune("LVS_TAIL_MIN_ITEMS", 256) &&
        lvs_tune("LVS_TAIL", 1) != 0)
        s = lvs_tile_tail_slabs(g, s, slabs_l2 > 0 ? g.lead_slabs + g.ntiles / lvs_tune("LVS_L2_MIN_TILES", 40) : max_slabs);
    if (lvs_tune_set("LVS_NSLAB")) {  // -DLVS_TUNING builds only
        const int64_t v = lvs_tune("LVS_NSLAB", 0);
        if (v >= 1 && v <= g.ntiles) s = v;
    }
    g.tiles_per_slab = (int)lvs_ceil_div(g.ntiles, s);
    g.nslab = (int)lvs_ceil_div(g.ntiles, g.tiles_per_slab);
    *used_l2 = slabs_l2 > 0;
    return g;
}
// With around a hundred query tiles the item count pushes the 8 x 4 plan to 45-49 slabs of 40-90 tiles, and there the wide
// groups win (same box, profiles/r05d_plan_sweep.log: 20 k x 1 M 31.1 -> 28.5 ms, 25 k x 1 M 36.7 -> 35.6, 25 k x 500 k 19.4 ->
// 18.6); with 196 / 391 query tiles the 8 x 4 groups stay ahead even on 55-109-tile slabs (100 k x 125 k 20.0 vs 20.5 ms,
// 100 k x 250 k 37.4 vs 38.6), and from 118 query tiles on the slabs are long anyway.
inline bool lvs_tile_l2_slabs_short(const LvsTileGeom& g) {
    return g.nqt <= lvs_tune("LVS_L2_SHORT_NQT", 128) && g.tiles_per_slab < lvs_tune("LVS_L2_MIN_FINAL", 120) &&
           !lvs_tune_set("LVS_GQ") && !lvs_tune_set("LVS_NSLAB");
}
inline LvsTileGeom lvs_tile_geometry(const LvsTileRequest& r) {
    bool used_l2 = false;
    LvsTileGeom g = lvs_tile_geometry_eval(r, true, &used_l2);
    if (used_l2 && lvs_tile_l2_slabs_short(g)) g = lvs_tile_geometry_eval(r, false, &used_l2);  // fall back to wide groups
#ifdef LVS_TUNING
    if (lvs_tune("LVS_PLAN_PRINT", 0) != 0)
        fprintf(stderr, "lvs plan: nq %lld nb %lld k %d -> nqt %d ntiles %d gq %d lead %d slabs %d x %d tiles, items %lld, xcd rounds %d\n",
                (long long)r.nq, (long long)r.nb, r.k, g.nqt, g.ntiles, g.gq, g.lead_slabs, g.nslab, g.tiles_per_slab,
                (long long)g.nqt * g.nslab, lvs_tile_xcd_rounds(g.nqt, g.nslab, g.gq, g.lead_slabs));
#endif
    return g;
}

// Seeded thresholds of a list launch.  A launch cuts the corpus into slabs that run concurrently, and a slab whose queries
// have no threshold yet pays a cold start of ~k (1 + ln(slab rows / k)) lock-protected insertions per query: with few query
// tiles EVERY slab starts cold (256 queries x 1 M rows: 0.36 ms of a 1.08 ms launch), with many it is the leading slab of
// every query tile (100 k x 125 k: 1.3 ms of 21.2).  So LVS_MODE_SEED first scores a sample (the first rows of the shard,
// one tile per workgroup, no lists), one wave per query takes the k-th largest of the per-tile maxima as the starting
// threshold, and the list launch only inserts rows that reach it.  Exact for the same reason as the small-batch kernel's
// seeding: every value is a real row's score, computed by the same instructions in the same order as the list mode
// computes it, and at least k rows reach the threshold.  Sample size: a sixteenth of the corpus for up to 64 query tiles
// (the sample pass is negligible there and a tight threshold saves the most); beyond, the pass costs MFMA time in
// proportion to the queries, and the smallest useful sample - max(k, 8) tiles: the threshold is the k-th largest of one
// maximum per tile - already removes the first tiles' insertions, which is most of a cold start (100 k x 1 M, same box:
// 10 / 61 tiles 138.5 / 139.5 ms against 140.0 unseeded; 100 k x 125 k 21.2 -> 20.4 ms, 25 k x 500 k 20.9 -> 20.3;
// tools/seed_big_sweep.py), so it is nb / 512 rows there; never more than a sixteenth of the corpus or 64 tiles.
// Returns the sample tiles or 0: no seeding.
#define LVS_TILE_SEED_MAXTILES 64
#define LVS_TILE_SEED_MAXQT 4096  // 2^20 queries: 256 B of seed workspace per query at most
inline int tile_seed_tiles(int64_t nq, int64_t nb, int k) {
    if (lvs_tune("LVS_TILE_SEED", 1) == 0 || k < 1 || k > LVS_KPASS) return 0;
    const int64_t nqt = lvs_ceil_div(nq, LVS2_BQ);
    long long maxqt = lvs_tune("LVS_TILE_SEED_MAXQT", LVS_TILE_SEED_MAXQT);
    if (maxqt > LVS_TILE_SEED_MAXQT) maxqt = LVS_TILE_SEED_MAXQT;  // the workspace holds seeds up to here
    if (nqt > maxqt) return 0;
    const int64_t kt = k > 8 ? k : 8;
    if (nb < 16 * (int64_t)LVS_BC * kt) return 0;
    int64_t tiles = nb / LVS_BC / (nqt <= 64 ? lvs_tune("LVS_TILE_SEED_DIV", 16) : lvs_tune("LVS_TILE_SEED_DIV_BIG", 512));
    if (tiles < kt) tiles = kt;
    if (tiles > LVS_TILE_SEED_MAXTILES) tiles = LVS_TILE_SEED_MAXTILES;
    return (int)tiles;
}

// ---- chunked calls of lvs_rq_kernel / lvs_rj_kernel ------------------------------------------------------------------
// A chunk is 4 096 queries (16 groups x 16 corpus ranges) or 8 192 x 2^i
// (32 / 64 / 128 / 256 groups x 8 / 4 / 2 / 1 ranges: a multiple of 32 groups - lvs_rq_item).  rq_chunk_size: the largest such
// size up to `want`, the call's maximum.  A call is cut greedily (rq_chunk_len): every chunk is the largest of 65 536, 32 768,
// 16 384, 8 192 that is <= the queries left and <= the maximum, then one of 4 096 while more than 4 096 are left, then the rest -
// 100 000 = 65 536 + 32 768 + 1 696, 50 000 = 32 768 + 16 384 + 848.  (Before this rule whatever was left below the maximum went out
// in 8 192s - the slowest of these geometries: 100 000 at a maximum of 65 536 ran 65 536 + 4 x 8 192 + 1 696, which is what the
// "65 536" lines of profiles/r10j_join_variants.log and r12d_knobs.log measured.)
inline int64_t rq_chunk_size(int64_t want) {
    int64_t c = LVS_RQ_MAXQ;
    while (2 * c <= want && 2 * c <= LVS_RQ_CHUNK_MAX) c *= 2;
    return c;
}
inline int64_t rq_chunk_len(int64_t left, int64_t chunk_max) {
    for (int64_t c = chunk_max; c >= 8192; c /= 2)
        if (left >= c) return c;
    return left > LVS_RQ_MAXQ ? LVS_RQ_MAXQ : left;
}
// the threshold join's cut (lvs_range_join), unchanged: chunks of LVS_RANGE_CHUNK rows, what is left in 8 192s, 4 096, the rest
inline int64_t range_chunk_len(int64_t left) {
    return left >= LVS_RANGE_CHUNK ? LVS_RANGE_CHUNK : (left >= 8192 ? 8192 : (left > LVS_RQ_MAXQ ? LVS_RQ_MAXQ : left));
}

// ---- grouped launches (lvs_rq_kernel, lvs_rj_kernel) ---------------------------------------------------------------------
// blockIdx -> (corpus range, query group) of a grouped launch.  Workgroup b lands on XCD b % 8
// (observed; used for speed only): the siblings of a range take slots of ONE XCD, so the range comes from HBM once per XCD and
// reaches the siblings - which run in step - through that XCD's L2.  Up to 32 groups: 32 / groups ranges per XCD at a time
// (ranges 8 i + x on XCD x).  More than 32 groups (a multiple of 32; r6): the launch is 256 items in range-major order, XCD x runs
// items 32 x .. 32 x + 31 - its 32 workgroups share one range, 256 / groups ranges in all: every query sees FEWER, LONGER
// ranges, i.e. fewer list cold starts and candidates per query (16 groups x 16 ranges: ~24 candidates per query and range; 64 x 4: ~37).
// lvs_rq_ranges_for: corpus ranges a launch of `groups` query groups uses at most: every range has one workgroup per group, all
// on one XCD (32 CUs), a workgroup fills a CU
LVS_HD inline int lvs_rq_ranges_for(int groups) {
    return groups <= 1 ? 256 : (groups <= 32 ? 8 * (32 / groups) : 256 / groups);
}
LVS_HD inline int lvs_rq_grid(int groups, int ranges) {
    return groups <= 1 ? ranges : (groups <= 32 ? 8 * groups * ((ranges + 7) / 8) : 256);
}
LVS_HD inline bool lvs_rq_item(int b, int groups, int nparts, int& range, int& group) {
    if (groups <= 1) {
        range = b;
        group = 0;
        return true;
    }
    if (groups <= 32) {
        const int s = b >> 3;
        range = (s / groups) * 8 + (b & 7);
        group = s % groups;
        return range < nparts;  // (the grid is rounded up to whole XCD rows)
    }
    const int item = (b & 7) * 32 + (b >> 3);
    range = item / groups;
    group = item % groups;
    return range < nparts;
}
// groups / nparts / blocks_per_wg of a launch of nq queries over nblocks 32-row blocks: lvs_rq_kernel takes the corpus in
// rounded-up blocks ((nb + 31) / 32), lvs_rj_kernel in whole ones (nb / 32; its caller adds the tail).  nparts = corpus
// ranges = candidate lists per query.  false: not a launch of these kernels (no block, or a group count lvs_rq_item cannot deal)
struct LvsGroupedGeom {
    int groups, nparts, blocks_per_wg;
};
inline bool lvs_grouped_geometry(int64_t nq, int64_t nblocks, LvsGroupedGeom& g) {
    g.groups = (int)((nq + LVS_RQ_GROUPQ - 1) / LVS_RQ_GROUPQ);
    if (g.groups < 1) g.groups = 1;
    if (g.groups > 32 && g.groups % 32 != 0) return false;  // (chunks of a larger call: 32 x 2^i groups)
    int64_t ranges = lvs_rq_ranges_for(g.groups);
    if (ranges < 1 || nblocks < 1) return false;
    if (ranges > (nblocks + 3) / 4) ranges = (nblocks + 3) / 4;
    if (ranges < 1) ranges = 1;
    g.blocks_per_wg = (int)((nblocks + ranges - 1) / ranges);
    g.nparts = (int)((nblocks + g.blocks_per_wg - 1) / g.blocks_per_wg);
    return true;
}
// Does the register-resident-queries kernel take this call?  fp16 k-slices of one K segment (d padded to 256, 384, 512 or
// 768 halfs), k <= 16, a corpus long enough to give every CU a few blocks, and 97 .. 256 queries - or up to LVS_RQ_MAXQ in
// groups of 256 when the groups' workgroups fill (nearly) every CU (>= 224 of 256): 2 .. 8, 10, 14, 15 or 16 groups.
inline bool lvs_rq_shape_ok(int dpad, int k) {  // operand shapes the register-resident kernels are built for
    const int nj = dpad / 16;
    return dpad % 16 == 0 && k >= 1 && k <= LVS_RQ_KMAX && (nj == 16 || nj == 24 || nj == 32 || nj == 48);
}
inline bool lvs_rq_fits(int64_t nq, int64_t nb, int dpad, int k) {
    const int nj = dpad / 16;
    if (!(nq > 96 && nq <= LVS_RQ_MAXQ && k >= 1 && k <= LVS_RQ_KMAX && nb >= 32768 && (nj == 16 || nj == 24 || nj == 32 || nj == 48))) return false;
    const int groups = (int)((nq + LVS_RQ_GROUPQ - 1) / LVS_RQ_GROUPQ);
    if (groups == 1) return true;
    return groups <= lvs_tune("LVS_RQ_MAXG", LVS_RQ_MAXQ / LVS_RQ_GROUPQ) && groups * lvs_rq_ranges_for(groups) >= 224 &&
           nb >= (int64_t)32768 * groups;
}
// Does the one-wave-per-SIMD form take this launch?  Everything lvs_rq_kernel's grouped launch takes (lvs_rq_fits) with row ids
// that are positions (no id table: a candidate's key is built where it is found) and at least one whole 32-row block per range.
inline bool lvs_rj_fits(int64_t nq, int64_t nb, int dpad, int k, bool has_row_ids) {
    if (has_row_ids || !(dpad == 256 || dpad == 384 || dpad == 512 || dpad == 768) || nq <= 128 || k < 1 || k > LVS_RQ_KMAX) return false;
    if (nq <= LVS_RQ_MAXQ) return lvs_rq_fits(nq, nb, dpad, k) || (nq > 2048 && nb >= LVS_RQ_JOIN_MINROWS);  // (the last chunk of a call)
    const int64_t groups = (nq + LVS_RQ_GROUPQ - 1) / LVS_RQ_GROUPQ;  // a chunk of a larger call: 32 x 2^i groups
    return nq <= LVS_RQ_CHUNK_MAX && groups % 32 == 0 && nb >= LVS_RQ_JOIN_MINROWS;
}
// corpus ranges (= lists per query) of a launch lvs_rj_fits accepts; 0: no such launch
inline int lvs_rj_parts(int64_t nq, int64_t nb) {
    LvsGroupedGeom g;
    return lvs_grouped_geometry(nq, nb / 32, g) ? g.nparts : 0;
}
// The kernel of one chunk of cn queries (search_rq_chunks).  (r6) one wave per SIMD, 64 queries per wave (lvs_rj.hip) for the
// launches it takes: whole 32-row blocks there, the corpus' last nb % 32 rows through lvs_rq_kernel as one more list per query.
// SOLO: ONE corpus range and no tail rows - the launch writes [1][cn][k] = the chunk's [cn][k] of the result itself, no merge
enum { LVS_CHUNK_RQ = 0, LVS_CHUNK_RJ = 1, LVS_CHUNK_RJ_SOLO = 2 };
inline int lvs_rq_chunk_kernel(int64_t cn, int64_t nb, int dpad, int k, bool has_row_ids) {
    if (!(lvs_tune("LVS_RJ", LVS_RJ_DEFAULT) != 0 && lvs_rj_fits(cn, nb, dpad, k, has_row_ids))) return LVS_CHUNK_RQ;
    if (nb % 32 == 0 && lvs_rj_parts(cn, nb) == 1 && lvs_tune("LVS_RJ_SOLO", LVS_RJ_SOLO_DEFAULT) != 0) return LVS_CHUNK_RJ_SOLO;
    return LVS_CHUNK_RJ;
}
// Sample rows (the first of the corpus) whose per-range best scores seed a chunk's thresholds, scanned by the kernel's own SEED
// mode (bit-identical scores; see lvs_stream_sample_rows for why a caller's pooled sample scores are not used).  0: no sample.
// (eight groups or more: a workgroup sees 30 000+ rows and fills its own lists - a quarter of the sample costs the main
// pass 1 % and saves 3 % of the call; profiles/r09b_rq_groups_sample_probe.log)
// (chunks of 16 384 queries or more see the corpus in <= 4 long ranges whose lists fill at once: half of that sample again
// costs the launches nothing and the sample pass half - 100 k x 1 M: call 126.0-127.8 -> 125.4-126.2 ms, same box,
// profiles/r12d_knobs.log)
inline int64_t lvs_rq_sample_rows(int64_t nb, int64_t cn) {
    int64_t sample = nb / 8 / 1024 * 1024;
    const int64_t sample_cap = lvs_tune("LVS_RQ_SAMPLE", cn >= 16384 ? LVS_RQ_SEED_ROWS / 8
                                                         : (cn > 7 * LVS_RQ_GROUPQ ? LVS_RQ_SEED_ROWS / 4 : LVS_RQ_SEED_ROWS));
    if (sample > sample_cap) sample = sample_cap;
    return sample >= 4096 && lvs_tune("LVS_STREAM_SEED", 1) != 0 ? sample : 0;
}

// ---- the threshold join (lvs_range_join) ----------------------------------------------------------------------------------
// (r6) fp16 rows, inner product, one rank's tiles, 2 048 queries or more: the register-resident-queries kernel in RANGE mode
// (lvs_rj.hip) serves the call in chunks of range_chunk_len queries; every other call is one launch of the list kernel
inline bool lvs_range_rj_ok(int64_t nq, int dpad, int32_t xb_pack, int32_t xq_pack, int32_t metric, int32_t qt_stride) {
    return lvs_tune("LVS_RJ", LVS_RJ_DEFAULT) != 0 && lvs_tune("LVS_RJ_RANGE", 1) != 0 && xb_pack == LVS_PACK_F16 &&
           xq_pack == LVS_PACK_F16 && metric == LVS_METRIC_IP && qt_stride == 1 && nq >= 2048 && lvs_rq_shape_ok(dpad, 1);
}
// The launches of the chunk of queries [c0, c0 + cn) over nb rows: `kernel` over rows [r0, r0 + rn) (rn = 0: none), then the
// list kernel over [t0, t0 + tn) (tn = 0: none).  The rows start where they can still pair with the chunk - everywhere, or
// (self-join, q_row0 >= 0: query i is row q_row0 + i of a corpus whose first row is id_offset, only j > i is kept) at the
// 32-row block of the chunk's first query.  lvs_rj_kernel sees whole 32-row blocks, at least LVS_RQ_JOIN_MINROWS of them,
// and leaves the corpus' last nb % 32 rows to the list kernel; chunks left with a shorter corpus go to the list kernel whole.
enum { LVS_RANGE_LIST = 0, LVS_RANGE_RJ = 1 };
struct LvsRangeChunk {
    int kernel;
    int64_t r0, rn, t0, tn;
};
inline LvsRangeChunk lvs_range_chunk_plan(int64_t c0, int64_t cn, int64_t nb, int64_t q_row0, int64_t id_offset) {
    int64_t r0 = 0;
    if (q_row0 >= 0) {
        r0 = (q_row0 + c0 - id_offset) / 32 * 32;
        if (r0 < 0) r0 = 0;
        if (r0 > nb) r0 = nb;
    }
    const int64_t r_full = nb / 32 * 32;
    const int64_t groups = (cn + LVS_RQ_GROUPQ - 1) / LVS_RQ_GROUPQ;
    if (r_full - r0 >= LVS_RQ_JOIN_MINROWS && cn > 128 && (groups <= 32 || groups % 32 == 0))
        return {LVS_RANGE_RJ, r0, r_full - r0, r_full, nb - r_full};
    return {LVS_RANGE_LIST, r0, nb - r0, nb, 0};
}

// ---- the small-batch streaming kernel (lvs_stream.hip) -------------------------------------------------------------------
// corpus ranges of a launch: one per CU when every workgroup has its own range, 256 / G with G sibling groups
inline int lvs_stream_ranges(int64_t nb, int groups) {
    const int64_t nblocks = (nb + 31) / 32;
    int64_t r = 256 / (groups > 0 ? groups : 1) / (groups > 1 ? 8 : 1) * (groups > 1 ? 8 : 1);  // siblings: multiples of 8
    if (groups <= 1 && lvs_tune("LVS_STREAM_WGS", 0) > 0) r = lvs_tune("LVS_STREAM_WGS", 0);  // -DLVS_TUNING builds only
    if (r > LVS_STREAM_MAXWG) r = LVS_STREAM_MAXWG;
    if (groups > 1) {
        // siblings are consecutive slots of one XCD: ranges come in multiples of 8 (one per XCD and slot group)
        int64_t cap = (nblocks + 3) / 4;
        cap = cap / 8 * 8;
        if (r > cap) r = cap;
        if (r < 8) r = 8;
    } else {
        if (r > (nblocks + 3) / 4) r = (nblocks + 3) / 4;
        if (r < 1) r = 1;
    }
    return (int)r;
}
// 32-row blocks per corpus range and the ranges (= candidate lists per query) of a launch over nb rows
inline void lvs_stream_geometry(int64_t nb, int groups, int* blocks_per_wg, int* nparts) {
    const int64_t nblocks = (nb + 31) / 32;
    const int ranges = lvs_stream_ranges(nb, groups);
    *blocks_per_wg = (int)((nblocks + ranges - 1) / ranges);
    *nparts = (int)((nblocks + *blocks_per_wg - 1) / *blocks_per_wg);
    if (groups > 1) *nparts = (*nparts + 7) / 8 * 8;  // empty ranges write empty lists
}
inline size_t lvs_stream_lds_bytes(int nbfrag, int nqb, int kcap) {
    return (size_t)nqb * nbfrag * 1024 + (size_t)nqb * LVS_STREAM_BLOCKQ * kcap * 8 + (size_t)nqb * LVS_STREAM_BLOCKQ * 4;
}
// How a call is laid out: *out_nqb = 32-query blocks per workgroup (1, 2 or 3), *out_groups = sibling workgroups per corpus
// range (1 .. 4), *out_kcap = list slots per query.  Fewest groups first: every group is one more pass of the corpus
// through the fabric (measured, 1 M x 768: 64 queries in one group 0.26 ms, 128 in two 0.38 ms, 256 in four 0.70 ms - the
// siblings drift apart by more than an L2's worth of stream, so the memory-side cache, not the L2, serves the re-reads);
// then the fewest blocks per workgroup (more list slots, less LDS).  Returns 0 when the call does not fit the streaming
// kernel (too many queries / k for the LDS left beside the query fragments).
inline int lvs_stream_plan(int64_t nq, int k, int nbfrag, int* out_kcap, int* out_nqb, int* out_groups) {
    if (nq < 1 || nq > LVS_STREAM_MAXQ || k < 1 || k > LVS_KPASS) return 0;
    const int blocks = (int)((nq + LVS_STREAM_BLOCKQ - 1) / LVS_STREAM_BLOCKQ);
    for (int groups = 1; groups <= 4; ++groups) {
        const int nqb = (blocks + groups - 1) / groups;
        if (nqb > 3) continue;
        // one block keeps the full 64 slots (any k <= 56 costs the same insertion step); more blocks trade slots for queries
        const int kcap = nqb == 1 ? 64 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64));
        if (lvs_stream_lds_bytes(nbfrag, nqb, kcap) > LVS_LDS_MAX) continue;  // a workgroup may use the whole 160 KiB
        if (out_kcap) *out_kcap = kcap;
        if (out_nqb) *out_nqb = nqb;
        if (out_groups) *out_groups = groups;
        return nqb;
    }
    return 0;
}
// Sample rows of a streaming call (0: none, cold thresholds).  Every workgroup scans its own contiguous range, all at the same
// time: without help each of them starts with
// empty lists and pays its own cold start (~k (1 + ln(range / k)) insertions per query and workgroup - with
// dozens of queries that, not HBM, set the time in round 2).  So with several queries the thresholds are
// SEEDED: the same kernel first scans a sample (the first nb / 8 rows, at most 32 768) in SEED mode - no lists,
// every workgroup just keeps the best score per query over its 4 row blocks - and one wave per query takes the
// k-th largest of those per-range maxima as the starting threshold (~15 + 5 us; round 3's first version scored the
// sample into a matrix with the tile kernel and radix-selected it: 130-180 us).  A workgroup of the main scan then
// only inserts rows that beat it (~k * nb / sample per query over the WHOLE launch).  Exact: every value is a
// real row's score and the k-th largest of a subset never exceeds the k-th largest of all rows; the sample
// rows themselves are scanned again with the rest.
// A caller's pooled sample scores (ext_seeds) are NOT used here: they come from the tile kernel's SEED mode, whose
// accumulation order differs from this kernel's, and "the k-th largest of a subset is a lower bound" is only exact
// when the threshold and the scan see bit-identical scores - one ulp the wrong way could reject a true top-k row on
// its own shard.  This path seeds itself, with its own arithmetic.
inline int64_t lvs_stream_sample_rows(int64_t nq, int64_t nb) {
    int64_t sample = nb / 8 / 1024 * 1024;
    if (sample > LVS_STREAM_SEED_ROWS) sample = LVS_STREAM_SEED_ROWS;
    return nq >= lvs_tune("LVS_STREAM_SEED_MINQ", 2) && sample >= 4096 && lvs_tune("LVS_STREAM_SEED", 1) != 0 ? sample : 0;
}

// ---- workspace layout of a flat search ----------------------------------------------------------------------------------
// [status words | thresholds | the path's lists ... | tile seed block].  One path serves a call, so the streaming and grouped
// kernels' lists start where the list kernel's do; their sizes are separate terms of the total.
struct LvsWorkspace {
    int kpass, npass;       // list kernel: k per pass (k <= 15 -> one pass on the 256-query geometry) and passes
    int64_t off_gtau;       // [nq] shared running thresholds
    int64_t off_partial;    // list kernel: [nslab][nq][kpass] per-slab lists
    int64_t off_pass;       // list kernel: [nq][kpass] merged keys of one pass (multi-pass only)
    int64_t off_parts;      // streaming / grouped kernels: [nparts][nq or chunk][k] lists of a launch (= off_partial)
    int64_t off_seeds;      // ... and [nparts][nq or <= 4 096] per-range best scores of the sample that seeds their thresholds
    int64_t off_tile_seeds; // [sample tiles][nq] per-tile best scores of a seeded list launch (tile_seed_tiles)
    int64_t total;
};
// bytes reserved for the small-batch kernel's candidate lists [ranges][nq][k] and sample scores [ranges][nq]
inline int64_t lvs_stream_parts_bytes(int64_t nq, int k) {
    return lvs_round_up((int64_t)((lvs_tune_set("LVS_STREAM_WGS") ? LVS_STREAM_MAXWG : 256) + 8) * (nq > 0 ? nq : 1) *
                            (k > 0 ? k : 1) * 8, 256);
}
inline int64_t lvs_stream_seed_bytes(int64_t nq) { return lvs_round_up((int64_t)(nq > 0 ? nq : 1) * (LVS_STREAM_MAXWG + 8) * 4, 256); }
// ... and for the register-resident-queries kernel beyond 256 queries: `groups` query groups x at most 256 / groups corpus
// ranges = at most 65 536 lists (+ slack), and as many sample scores
inline int64_t lvs_rq_parts_bytes(int64_t nq, int k) {
    if (nq <= LVS_STREAM_MAXQ) return lvs_stream_parts_bytes(nq, k);
    return lvs_round_up((int64_t)(65536 + 8 * nq) * (k > 0 ? k : 1) * 8, 256);
}
inline int64_t lvs_rq_seed_bytes(int64_t nq) {
    if (nq <= LVS_STREAM_MAXQ) return lvs_stream_seed_bytes(nq);
    return lvs_round_up((int64_t)(65536 + 8 * nq) * 4, 256);
}
inline LvsWorkspace lvs_workspace(int64_t nq, int64_t nb, int k, int nslab) {
    LvsWorkspace w;
    w.kpass = k < LVS_KPASS ? (k > 0 ? k : 1) : LVS_KPASS;
    w.npass = k > 0 ? (int)lvs_ceil_div(k, w.kpass) : 0;
    const int64_t list_bytes = lvs_round_up((int64_t)nslab * nq * w.kpass * 8, 256);
    const int64_t pass_bytes = w.npass > 1 ? lvs_round_up(nq * w.kpass * 8, 256) : 0;
    int64_t parts_bytes = 0, seed_bytes = 0;
    if (nq <= LVS_STREAM_MAXQ && k <= LVS_KPASS) {  // the small-batch kernel (and lvs_rq_kernel's one group of up to 256 queries)
        parts_bytes = lvs_stream_parts_bytes(nq, k);
        seed_bytes = lvs_stream_seed_bytes(nq);
    } else if (k <= LVS_RQ_KMAX) {  // lvs_rq_kernel in query groups, beyond LVS_RQ_MAXQ queries one chunk at a time
        const int64_t cmax = rq_chunk_size(lvs_tune("LVS_RQ_CHUNK", LVS_RQ_CHUNK_DEFAULT));
        const int64_t cq = nq <= cmax ? nq : cmax;
        parts_bytes = lvs_rq_parts_bytes(cq, k);
        seed_bytes = lvs_rq_seed_bytes(cq);
    }
    const int64_t tile_seed_bytes = w.npass == 1 ? lvs_round_up((int64_t)(nq > 0 ? nq : 1) * tile_seed_tiles(nq, nb, k) * 4, 256) : 0;
    int64_t off = 256;  // the first 256 bytes hold status words (the large-k overflow flag) in every layout
    w.off_gtau = off;
    off += lvs_round_up(nq * 4, 256);
    w.off_partial = w.off_parts = off;
    w.off_seeds = off + parts_bytes;
    off += list_bytes;
    w.off_pass = off;
    off += pass_bytes + parts_bytes + seed_bytes;
    w.off_tile_seeds = off;
    w.total = off + tile_seed_bytes;
    return w;
}

// ---- the plans the entry points ask for -----------------------------------------------------------------------------------
struct LvsTilePlan {  // a launch of the list kernel in a mode without lists
    LvsLayout l;
    LvsTileGeom g;
};
inline int lvs_plain_tile_plan(int64_t nq, int64_t nb, int32_t d, int32_t xb_pack, int32_t xq_pack, LvsTilePlan& p) {
    if (nq < 0 || nb < 0 || lvs_layout(d, xb_pack, xq_pack, false, p.l) != LVS_OK) return LVS_EINVAL;
    p.g = lvs_tile_geometry(lvs_tile_request_plain(nq, nb));
    return LVS_OK;
}
struct LvsFlatPlan : LvsTilePlan {  // a top-k search: the list kernel's geometry for it and the workspace of whichever path runs
    LvsWorkspace w;
};
inline int lvs_flat_plan(int64_t nq, int64_t nb, int32_t d, int32_t xb_pack, int32_t xq_pack, bool hi_only, int32_t k,
                         LvsFlatPlan& p) {
    if (nq < 0 || nb < 0 || k < 0 || lvs_layout(d, xb_pack, xq_pack, hi_only, p.l) != LVS_OK) return LVS_EINVAL;
    p.g = lvs_tile_geometry(lvs_tile_request_topk(nq, nb, k));
    p.w = lvs_workspace(nq, nb, k, p.g.nslab);
    return LVS_OK;
}

// ---- large k in two phases (k > LVS_KPASS) ----------------------------------------------------------------------
// Phase A is a 15-per-slab top-k pass with at least 3k/15 slabs that do NOT share thresholds, so every slab's list is
// its own exact top 15.  The lists hold 15 * nslab DISTINCT rows,
// so the k-th largest of all their keys is a valid lower bound T of the query's true k-th best key - and a tight one
// unless one slab holds more than 15 of the true top k.  Phase B (LVS_MODE_COLLECT) streams the corpus once more and
// drops every key >= T into the query's bucket (>= k keys by construction); phase C sorts the bucket and keeps k.
// Exact; two corpus passes whatever k is.  If a bucket overflows (heavily tied or slab-clustered data) the caller falls
// back to ceil(k / LVS_KPASS) selection passes.
struct TwoPhasePlan {
    LvsTileGeom a;      // phase A geometry: 15-slot lists (256 x 256) for moderate k, 56-slot lists (256 x 128) beyond
    LvsTileGeom b;      // phase B (collect) geometry: always 256 x 256
    int slots;          // list slots per (query, slab) in phase A
    int capacity;       // bucket slots per query
    int64_t off_gtau, off_lists;  // [nq] thresholds and [a.nslab][nq][slots] lists of phase A
    int64_t off_thr, off_cnt, off_bucket, total;
};
inline bool make_two_phase_plan(int64_t nq, int64_t nb, int32_t k, TwoPhasePlan& tp) {
    if (k <= LVS_KPASS || nq <= 0 || nb <= 0) return false;
    if (lvs_tune("LVS_TWO_PHASE", 1) == 0) return false;
    // 15-slot lists on the fast geometry beat 56-slot lists on the 128-query geometry at every k tried (100 .. 1000:
    // 329 vs 402 ms, 545 vs 607 ms at 100 k x 1 M), although they need four times the slabs
    tp.slots = LVS2_KCAP;
    if (lvs_tune("LVS_TWO_PHASE_SLOTS", LVS2_KCAP) == LVS3_KCAP) tp.slots = LVS3_KCAP;
    const int64_t cap_slabs = LVS_SELECT_MAX / tp.slots;        // the selection kernel sorts at most 4096 keys per query
    int64_t want_slabs = lvs_ceil_div(2ll * k, tp.slots);       // ~2k candidates: a tight bound at a moderate slab count
    if (want_slabs > cap_slabs) want_slabs = cap_slabs;
    tp.a = lvs_tile_geometry({nq, nb, tp.slots, tp.slots == LVS2_KCAP, want_slabs, cap_slabs});
    if ((int64_t)tp.a.nslab * tp.slots > LVS_SELECT_MAX) return false;
    if ((int64_t)tp.a.nslab * tp.slots < (int64_t)k + k / 4) return false;  // corpus too small for a useful bound
    tp.b = lvs_tile_geometry(lvs_tile_request_plain(nq, nb));
    tp.capacity = pow2_ceil(2 * k < 512 ? 512 : 2 * k);
    if (tp.capacity > LVS_SELECT_MAX) tp.capacity = LVS_SELECT_MAX;
    if (tp.capacity < k) return false;
    const LvsWorkspace wa = lvs_workspace(nq, nb, tp.slots, tp.a.nslab);  // thresholds and per-slab lists as a one-pass search lays them out
    tp.off_gtau = wa.off_gtau;
    tp.off_lists = wa.off_partial;
    int64_t off = wa.off_pass;
    tp.off_thr = off;
    off += lvs_round_up(nq * 8, 256);
    tp.off_cnt = off;
    off += lvs_round_up(nq * 4, 256);
    tp.off_bucket = off;
    off += lvs_round_up(nq * (int64_t)tp.capacity * 8, 256);
    tp.total = off;
    if (tp.total > (24ll << 30)) return false;  // lists + buckets beyond 24 GB: not worth it, use the selection passes
    return true;
}
inline int64_t lvs_flat_workspace_bytes(int64_t nq, int64_t nb, int32_t d, int32_t k, int32_t xb_pack, int32_t xq_pack) {
    LvsFlatPlan p;
    if (lvs_flat_plan(nq, nb, d, xb_pack, xq_pack, false, k, p) != LVS_OK) return LVS_EINVAL;
    TwoPhasePlan tp;
    if (make_two_phase_plan(nq, nb, k, tp) && tp.total > p.w.total) return tp.total;
    return p.w.total;
}

// ---- route: which path serves the (rest of the) call ----------------------------------------------------------------------
enum { LVS_ROUTE_RQ = 0, LVS_ROUTE_RQ_JOIN = 1, LVS_ROUTE_STREAM = 2, LVS_ROUTE_LIST = 3 };
struct LvsStreamShape {  // the small-batch kernel's shape for a call (lvs_stream_plan)
    int nbfrag;  // B fragments per query block: query K segments x dpad / 16
    int kcap, nqb, groups;
};
struct LvsRoute {
    int kind;               // LVS_ROUTE_*: register-resident chunks without / with rq_join, streaming, list passes
    LvsStreamShape stream;  // LVS_ROUTE_STREAM only
};
// npass: of the call's workspace; kc: the banded search's (0: none); two_phase_ran: the list passes would only be its fallback
inline LvsRoute lvs_flat_route(int64_t nq, int64_t nb, const LvsLayout& l, int k, int npass, int kc, bool two_phase_ran) {
    LvsRoute r = {LVS_ROUTE_LIST, {0, 0, 0, 0}};
    // 97 .. 256 queries (and up to 4 096 in groups of 256), one K segment of fp16 k-slices: the queries live in REGISTERS
    // (lvs_rq.hip), the corpus streams through LDS once - between the HBM-bound batches below and the joins the list kernel is
    // built for.  (r6) Beyond 4 096 queries the same launch repeats per CHUNK of queries (search_rq_chunks).
    const bool rq_ok = lvs_tune("LVS_RQ", 1) != 0 && l.nseg == 1 && npass == 1 && !two_phase_ran && kc == 0;
    // (a corpus SHARD qualifies from 32 768 rows on: its thresholds may come from the caller - the pooled sample scores of all
    // shards, scored by the list kernel's SEED mode in the same arithmetic - or from its own first rows)
    const bool rq_join = rq_ok && nq > LVS_RQ_MAXQ && lvs_tune("LVS_RQ_JOIN", LVS_RQ_JOIN_DEFAULT) != 0 &&
                         lvs_rq_shape_ok(l.dpad, k) && nb >= lvs_tune("LVS_RQ_JOIN_MINROWS", LVS_RQ_JOIN_MINROWS);
    if (rq_join || (rq_ok && lvs_rq_fits(nq, nb, l.dpad, k))) {
        r.kind = rq_join ? LVS_ROUTE_RQ_JOIN : LVS_ROUTE_RQ;
        return r;
    }
    // HBM-bound regime (the literal sem_search: one query per call; small batches up to 256 queries): the small-batch kernel
    LvsStreamShape sh = {l.nbfrag, 0, 0, 0};
    const bool stream_fits = lvs_stream_plan(nq, k, sh.nbfrag, &sh.kcap, &sh.nqb, &sh.groups) > 0;
    const bool stream_want = lvs_tune("LVS_STREAM", 1) != 0 && nq <= lvs_tune("LVS_STREAM_MAXQ_RT", LVS_STREAM_MAXQ);
    // several sibling workgroups per corpus range (beyond 96 fp16 queries) leave the HBM-bound regime - the siblings'
    // re-reads are bound by the fabric behind the L2 (0.45 / 0.70 ms at 128 / 256 queries x 1 M rows) - while the seeded
    // list kernel runs such batches near its MFMA rate: the stream kernel keeps the single-group batches
    const bool stream_beyond = sh.groups > lvs_tune("LVS_STREAM_MAXG", 1) && npass == 1 && tile_seed_tiles(nq, nb, k) > 0;
    if (stream_want && stream_fits && nb >= 4096 && !stream_beyond) {
        r.kind = LVS_ROUTE_STREAM;
        r.stream = sh;
    }
    // everything else, and the predicated fallback of the two-phase search: the list kernel
    return r;
}
