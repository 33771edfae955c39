// Runs the host planners (lotus_amd/csrc/lvs_plan.h: the flat search and the threshold join; lvs_ivf_plan.h: the searches
// through the lists and the bucket sort; lvs_bound.h: the one-pass error bound's coefficients - the only project headers
// included) on a CPU.
//   plan_check           walks the grids below and fails on the first violated invariant of geometry, layout, route and chunks
//   plan_check --dump    one line per grid shape with every field of layout, geometry, two-phase plan, route, chunk list and
//                        workspace offsets; then "ivf", "bucket" and "join" lines: every field of the IVF plan, the bucket
//                        sort's plan, the join's launch list (tests/test_plan_pins.py pins some; the whole dump is what a
//                        refactor diffs)
//   plan_check --query   answers questions read from stdin, one per line, for the Python models of tests/test_rq_*.py, the
//                        route tables of tests/test_widths_host.py and tests/extent_cases.py, the IVF tests' chunks and the
//                        bound coefficients of tests/test_cert_rules_host.py
// Built with a plain host compiler by tests/plan_native.py (run from tests/test_capi.py).
#include "../../lotus_amd/csrc/lvs_bound.h"
#include "../../lotus_amd/csrc/lvs_ivf_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// ---- one dump line ----
struct Row {
    long long nq, nb;
    int d, k, bp, qp, hi;
    int lay[13];        // dpad nkd ldb ldq nseg nk seg_q[3] seg_c[3] nbfrag
    int geo[9];         // v2 nqt ntiles gq lead nslab tiles_per_slab kpass npass
    int tp_ok;
    long long tp[22];   // slots capacity | a: v2 nqt ntiles gq lead nslab tps | b: the same | off_gtau lists thr cnt bucket total
    int route[5];       // kind | stream: nbfrag kcap nqb groups
    std::string chunks; // register-resident routes: "len:kernel:lists per query" of every chunk, runs as "x count"; else "-"
    long long ws[7];    // off_gtau partial pass parts seeds tile_seeds total
    long long ws_bytes; // lvs_flat_search_workspace_bytes
};
static void print_row(const Row& r) {
    printf("nq=%lld nb=%lld d=%d k=%d pack=%d/%d hi=%d | lay", r.nq, r.nb, r.d, r.k, r.bp, r.qp, r.hi);
    for (int v : r.lay) printf(" %d", v);
    printf(" | geo");
    for (int v : r.geo) printf(" %d", v);
    printf(" | tp %d", r.tp_ok);
    if (r.tp_ok)
        for (long long v : r.tp) printf(" %lld", v);
    printf(" | route");
    for (int v : r.route) printf(" %d", v);
    printf(" | chunks %s | ws", r.chunks.c_str());
    for (long long v : r.ws) printf(" %lld", v);
    printf(" | bytes %lld\n", r.ws_bytes);
}
// ---- end of the dump line ----

static void put_geom(long long* out, const LvsTileGeom& g) {
    const int v[7] = {g.v2, g.nqt, g.ntiles, g.gq, g.lead_slabs, g.nslab, g.tiles_per_slab};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
}

#define FAIL(...)                 \
    do {                          \
        printf(__VA_ARGS__);      \
        printf("\n");             \
        return false;             \
    } while (0)

static bool geom_ok(const char* what, const LvsTileGeom& g, int64_t nq, int64_t nb) {
    if (!((int64_t)(g.nslab - 1) * g.tiles_per_slab < g.ntiles && g.ntiles <= (int64_t)g.nslab * g.tiles_per_slab))
        FAIL("%s: %d slabs x %d tiles do not cut %d tiles", what, g.nslab, g.tiles_per_slab, g.ntiles);
    if (!(g.gq == 1 || g.gq == 2 || g.gq == 4 || g.gq == 8 || g.gq == 16 || g.gq == 32)) FAIL("%s: gq %d", what, g.gq);
    if (g.lead_slabs > g.nslab || g.lead_slabs < 0) FAIL("%s: %d lead slabs of %d", what, g.lead_slabs, g.nslab);
    if ((int64_t)g.nqt * (g.v2 ? LVS2_BQ : LVS3_BQ) < nq || (int64_t)g.ntiles * LVS_BC < nb) FAIL("%s: tiles do not cover the shape", what);
    return true;
}

// the planner on one shape: fills the row and checks the invariants (false + a message: violated)
static bool plan_shape(int64_t nq, int64_t nb, int d, int k, int bp, int qp, bool hi, Row& r) {
    r.nq = nq, r.nb = nb, r.d = d, r.k = k, r.bp = bp, r.qp = qp, r.hi = hi;
    LvsFlatPlan p;
    if (lvs_flat_plan(nq, nb, d, bp, qp, hi, k, p) != LVS_OK) FAIL("the planner refuses the shape");
    const LvsLayout& l = p.l;
    const LvsWorkspace& w = p.w;
    const int lay[13] = {l.dpad, l.nkd, l.ldb, l.ldq, l.nseg, l.nk, l.seg_q[0], l.seg_q[1], l.seg_q[2], l.seg_c[0], l.seg_c[1], l.seg_c[2], l.nbfrag};
    memcpy(r.lay, lay, sizeof(lay));
    const int geo[9] = {p.g.v2, p.g.nqt, p.g.ntiles, p.g.gq, p.g.lead_slabs, p.g.nslab, p.g.tiles_per_slab, w.kpass, w.npass};
    memcpy(r.geo, geo, sizeof(geo));
    const long long ws[7] = {w.off_gtau, w.off_partial, w.off_pass, w.off_parts, w.off_seeds, w.off_tile_seeds, w.total};
    memcpy(r.ws, ws, sizeof(ws));
    r.ws_bytes = lvs_flat_workspace_bytes(nq, nb, d, k, bp, qp);

    // layout of the operands
    if (l.dpad % LVS_BK || l.dpad < d || l.dpad >= d + LVS_BK || l.nkd * LVS_BK != l.dpad) FAIL("dpad %d of d %d", l.dpad, d);
    if (l.ldb != (bp == LVS_PACK_SPLIT ? 2 : 1) * l.dpad || l.ldq != (qp == LVS_PACK_SPLIT ? 2 : 1) * l.dpad) FAIL("leading dimensions");
    if (l.nseg != 1 + (!hi && bp == LVS_PACK_SPLIT) + (!hi && qp == LVS_PACK_SPLIT) || l.nk != l.nseg * l.nkd) FAIL("K segments");
    for (int i = 0; i < l.nseg; ++i)
        if (l.seg_q[i] + l.dpad > l.ldq || l.seg_c[i] + l.dpad > l.ldb) FAIL("segment %d leaves its row", i);

    // geometry
    if (!geom_ok("search", p.g, nq, nb)) return false;
    if ((int64_t)w.npass * w.kpass < k || w.kpass > (p.g.v2 ? LVS2_KCAP : LVS3_KCAP)) FAIL("%d passes of %d for k %d", w.npass, w.kpass, k);

    // workspace: 256-aligned, ascending, every region inside the total
    const int64_t offs[5] = {w.off_gtau, w.off_partial, w.off_pass, w.off_tile_seeds, w.total};
    for (int i = 0; i < 5; ++i)
        if (offs[i] % 256 || (i && offs[i] < offs[i - 1])) FAIL("offset %d (%lld) unaligned or descending", i, (long long)offs[i]);
    if (w.off_gtau < 256 || w.off_partial - w.off_gtau < nq * 4) FAIL("thresholds overlap their neighbours");
    if (w.off_parts != w.off_partial || w.off_seeds % 256 || w.off_seeds < w.off_parts || w.off_seeds > w.off_tile_seeds) FAIL("parts / seeds offsets");

    // two phases
    TwoPhasePlan tp;
    r.tp_ok = make_two_phase_plan(nq, nb, k, tp);
    int64_t largest = w.total;
    if (r.tp_ok) {
        r.tp[0] = tp.slots, r.tp[1] = tp.capacity;
        put_geom(r.tp + 2, tp.a);
        put_geom(r.tp + 9, tp.b);
        const long long o[6] = {tp.off_gtau, tp.off_lists, tp.off_thr, tp.off_cnt, tp.off_bucket, tp.total};
        memcpy(r.tp + 16, o, sizeof(o));
        if (!geom_ok("phase A", tp.a, nq, nb) || !geom_ok("phase B", tp.b, nq, nb)) return false;
        const int64_t want = lvs_ceil_div(2ll * k, tp.slots), cap = LVS_SELECT_MAX / tp.slots;
        // at most `cap` slabs, and none longer than `want` slabs (or one tile each) would make it
        const int64_t least = (want < cap ? want : cap) < tp.a.ntiles ? (want < cap ? want : cap) : tp.a.ntiles;
        if (tp.a.nslab > cap || tp.a.tiles_per_slab > lvs_ceil_div(tp.a.ntiles, least)) FAIL("phase A: %d slabs outside the request", tp.a.nslab);
        if ((int64_t)tp.a.nslab * tp.slots < k || tp.capacity < k || !tp.b.v2) FAIL("two-phase bound");
        for (int i = 0; i < 6; ++i)
            if (o[i] % 256 || (i && o[i] < o[i - 1])) FAIL("two-phase offset %d", i);
        if (tp.off_lists - tp.off_gtau < nq * 4 || tp.off_thr - tp.off_lists < (int64_t)tp.a.nslab * nq * tp.slots * 8 ||
            tp.off_cnt - tp.off_thr < nq * 8 || tp.off_bucket - tp.off_cnt < nq * 4 || tp.total - tp.off_bucket < nq * tp.capacity * 8)
            FAIL("two-phase regions too small");
        if (tp.total > largest) largest = tp.total;
    }
    if (r.ws_bytes != largest) FAIL("workspace bytes %lld, largest layout %lld", r.ws_bytes, (long long)largest);

    // route, and the region it writes against what the launch geometry says it writes
    const LvsRoute route = lvs_flat_route(nq, nb, l, k, w.npass, 0, r.tp_ok);
    const int rt[5] = {route.kind, route.stream.nbfrag, route.stream.kcap, route.stream.nqb, route.stream.groups};
    memcpy(r.route, rt, sizeof(rt));
    r.chunks = "-";
    if (nq == 0 || nb == 0 || k == 0) return true;  // the entry point returns before it routes
    const int64_t parts_room = w.off_seeds - w.off_parts, seeds_room = w.off_tile_seeds - w.off_seeds;
    if (route.kind == LVS_ROUTE_RQ || route.kind == LVS_ROUTE_RQ_JOIN) {
        r.chunks.clear();
        const int64_t chunk = rq_chunk_size(lvs_tune("LVS_RQ_CHUNK", LVS_RQ_CHUNK_DEFAULT));
        std::string last;
        int run = 0;
        auto flush = [&]() {
            if (run) r.chunks += (r.chunks.empty() ? "" : ",") + last + (run > 1 ? "x" + std::to_string(run) : "");
        };
        for (int64_t c0 = 0, cn = 0; c0 < nq; c0 += cn) {
            cn = rq_chunk_len(nq - c0, chunk);
            if (cn < 1 || cn > chunk) FAIL("chunk of %lld queries", (long long)cn);
            const int kernel = lvs_rq_chunk_kernel(cn, nb, l.dpad, k, false);
            LvsGroupedGeom g, tail = {0, 0, 0};
            if (!lvs_grouped_geometry(cn, kernel == LVS_CHUNK_RQ ? (nb + 31) / 32 : nb / 32, g)) FAIL("chunk of %lld queries: no launch", (long long)cn);
            if (kernel != LVS_CHUNK_RQ && nb % 32 && !lvs_grouped_geometry(cn, 1, tail)) FAIL("no launch for the tail rows");
            const int lists = g.nparts + tail.nparts;
            if (kernel == LVS_CHUNK_RJ_SOLO ? lists != 1 : (int64_t)lists * cn * k * 8 > parts_room)
                FAIL("chunk of %lld queries writes %d lists, room %lld bytes", (long long)cn, lists, (long long)parts_room);
            if ((int64_t)g.blocks_per_wg * g.nparts * 32 < nb / 32 * 32) FAIL("ranges do not cover the corpus");
            const int64_t sample = lvs_rq_sample_rows(nb, cn);
            for (int64_t s0 = 0; sample > 0 && s0 < cn; s0 += LVS_RQ_MAXQ) {
                const int64_t sn = cn - s0 < LVS_RQ_MAXQ ? cn - s0 : LVS_RQ_MAXQ;
                LvsGroupedGeom sg;
                if (!lvs_grouped_geometry(sn, (sample + 31) / 32, sg) || (int64_t)sg.nparts * sn * 4 > seeds_room)
                    FAIL("sample pass of %lld queries does not fit %lld bytes", (long long)sn, (long long)seeds_room);
            }
            const std::string item = std::to_string(cn) + ":" + std::to_string(kernel) + ":" + std::to_string(lists);
            if (item != last) {
                flush();
                last = item;
                run = 0;
            }
            ++run;
        }
        flush();
    } else if (route.kind == LVS_ROUTE_STREAM) {
        int bpw, nparts;
        lvs_stream_geometry(nb, route.stream.groups, &bpw, &nparts);
        if ((int64_t)nparts * nq * k * 8 > parts_room || (int64_t)bpw * nparts * 32 < nb) FAIL("streaming launch: %d lists per query", nparts);
        const int64_t sample = lvs_stream_sample_rows(nq, nb);
        if (sample > 0) {
            lvs_stream_geometry(sample, route.stream.groups, &bpw, &nparts);
            if ((int64_t)nparts * nq * 4 > seeds_room) FAIL("streaming sample pass: %d ranges", nparts);
        }
        if ((int64_t)route.stream.nqb * LVS_STREAM_BLOCKQ * route.stream.groups < nq || route.stream.kcap < k) FAIL("streaming shape");
    } else {
        if ((int64_t)p.g.nslab * nq * w.kpass * 8 > w.off_pass - w.off_partial) FAIL("per-slab lists do not fit");
        if (w.npass > 1 && nq * w.kpass * 8 > w.off_tile_seeds - w.off_pass) FAIL("pass buffer does not fit");
        if (w.npass == 1 && (int64_t)tile_seed_tiles(nq, nb, w.kpass) * nq * 4 > w.total - w.off_tile_seeds) FAIL("tile seeds do not fit");
    }
    return true;
}

// ---- the searches through the lists (lvs_ivf_plan.h) ----
static bool bucket_ok(int64_t n, int32_t k, const BucketPlan& b) {
    const int64_t maxbins = b.nbins[0] > b.nbins[1] ? b.nbins[0] : b.nbins[1];
    const int64_t o[6] = {b.off_counts, b.off_seg, b.off_rows_a, b.off_rows_b, b.off_offs, b.total};
    for (int i = 0; i < 6; ++i)
        if (o[i] % 256 || (i && o[i] < o[i - 1])) FAIL("bucket offset %d (%lld) unaligned or descending", i, (long long)o[i]);
    if (b.off_counts != 0 || b.off_seg - b.off_counts < maxbins * b.nchunks * 4 ||
        b.off_rows_a - b.off_seg < lvs_scan_scratch_bytes(maxbins * b.nchunks) || b.off_rows_b - b.off_rows_a < n * 4 ||
        b.off_offs - b.off_rows_b < (b.passes > 1 ? n * 4 : 0) || b.total - b.off_offs < (int64_t)(k + 1) * 4)
        FAIL("bucket regions too small");
    if (b.nbins[0] > BUCKET_MAX_BINS || b.nbins[1] > BUCKET_MAX_BINS || (int64_t)b.nchunks * BUCKET_CHUNK < n) FAIL("bucket bins / chunks");
    if (b.passes == 1 ? b.nbins[0] != k + 1 : (b.passes != 2 || (int64_t)b.nbins[0] * b.nbins[1] <= k)) FAIL("bucket digits do not hold k + 1 bins");
    return true;
}
static bool bucket_shape(int64_t n, int32_t k, bool dump) {
    BucketPlan b;
    const bool ok = bucket_plan(n, k, b);
    if (ok && !bucket_ok(n, k, b)) return false;
    if (ok != (lvs_bucket_workspace_bytes(n, k) >= 0) || (ok && lvs_bucket_workspace_bytes(n, k) != b.total)) FAIL("bucket bytes");
    if (!dump) return true;
    printf("bucket n=%lld k=%d | ok %d", (long long)n, k, (int)ok);
    if (ok)
        printf(" | %d %d %d %d %d %d %u %u | %lld %lld %lld %lld %lld", b.nchunks, b.passes, b.nbins[0], b.nbins[1], b.shift[0], b.shift[1],
               b.mask[0], b.mask[1], (long long)b.off_counts, (long long)b.off_seg, (long long)b.off_rows_a, (long long)b.off_rows_b,
               (long long)b.off_offs);
    printf(" | bytes %lld\n", (long long)lvs_bucket_workspace_bytes(n, k));
    return true;
}

struct IvfShape {
    int mode;
    long long nq;
    int nlist, nprobe, d, M, k, pack;
};
static const long long IVF_PRANGE_NB = 1000000;  // the corpus the dump's prange column assumes
// one search's plan: prints its dump line and checks the invariants; *chunk: the chunk planned (0: the plan refuses)
static bool ivf_shape(const IvfShape& s, bool dump, long long* chunk) {
    LvsIvfPlan L;
    const int rc = lvs_ivf_plan(s.mode, s.nq, s.nlist, s.nprobe, s.d, s.M, s.k, s.pack, s.pack, L);
    const int64_t bytes = lvs_ivf_plan_bytes(s.mode, s.nq, s.nlist, s.nprobe, s.d, s.M, s.k, s.pack);
    *chunk = rc == LVS_OK ? L.chunk : 0;
    const int64_t c = L.chunk, tail = rc == LVS_OK ? s.nq % c : 0;
    const bool pq = s.mode == LVS_IVF_PQ, tiled = !pq;
    if (dump) {
        printf("ivf mode=%d nq=%lld nlist=%d nprobe=%d d=%d M=%d k=%d pack=%d | rc %d", s.mode, s.nq, s.nlist, s.nprobe, s.d, s.M, s.k, s.pack, rc);
        if (rc == LVS_OK)
            printf(" | chunk %lld tail %lld | lay %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld | prange %d %d", (long long)c, (long long)tail,
                   (long long)L.off_coarse, (long long)L.off_extra, (long long)L.off_sort, (long long)L.off_tiles, (long long)L.off_items,
                   (long long)L.off_parts, (long long)L.flat_bytes, (long long)L.sort_bytes, (long long)L.max_items, (long long)L.total,
                   pq ? lvs_ivf_pq_prange(IVF_PRANGE_NB, s.nlist, c, s.nprobe) : 0,
                   pq && tail ? lvs_ivf_pq_prange(IVF_PRANGE_NB, s.nlist, tail, s.nprobe) : 0);
        printf(" | bytes %lld\n", (long long)bytes);
    }
    const bool args_ok = s.nq >= 0 && s.nlist >= 1 && s.nprobe >= 1 && s.nprobe <= s.nlist && s.nprobe <= LVS_MAX_K && s.d > 0 &&
                         (s.mode == LVS_IVF_RANGE || (s.k >= 1 && s.k <= LVS_KPASS && s.M >= 1 && s.d % s.M == 0));
    if (bytes != (rc == LVS_OK ? L.total : (int64_t)rc)) FAIL("declared bytes %lld, plan %d / %lld", (long long)bytes, rc, (long long)L.total);
    if (!args_ok) {
        if (rc != LVS_EINVAL) FAIL("bad arguments answered %d", rc);
        return true;
    }
    if ((rc == LVS_EUNSUPPORTED) != !lvs_ivf_fits(s.mode, s.d, s.M, s.k, s.pack)) FAIL("fit and error code disagree (%d)", rc);
    if (rc == LVS_EUNSUPPORTED) return true;
    if (rc != LVS_OK) FAIL("a valid shape that fits answered %d", rc);
    const int k = s.mode == LVS_IVF_RANGE ? 0 : s.k;
    const int64_t extra = pq ? (int64_t)s.M * LVS_PQ_KSUB * 4 : 0, npairs = c * s.nprobe;

    // the chunk: the first of min(nq, 16 384), halved rounding up, whose scratch fits the budget (or 1); the chunks cover nq
    for (int64_t h = s.nq < IVF_CHUNK_MAX ? (s.nq > 0 ? s.nq : 1) : IVF_CHUNK_MAX;; h = (h + 1) / 2) {
        LvsIvfPlan H;
        if (!lvs_ivf_layout(h, s.nq % h, s.nlist, s.nprobe, s.d, k, s.pack, s.pack, extra, tiled, H)) FAIL("no layout at chunk %lld", (long long)h);
        if (H.total <= IVF_WS_BUDGET || h == 1) {
            if (h != c || H.total != L.total) FAIL("chunk %lld, the first that fits is %lld", (long long)c, (long long)h);
            break;
        }
        if (h == c) FAIL("chunk %lld is beyond the budget", (long long)c);
    }
    if (L.total > IVF_WS_BUDGET && c != 1) FAIL("total %lld beyond the budget at chunk %lld", (long long)L.total, (long long)c);
    if (c < 1 || tail < 0 || tail >= c || (s.nq / c) * c + tail != s.nq) FAIL("chunks of %lld and %lld do not cover %lld", (long long)c, (long long)tail, s.nq);
    if (npairs >= (1ll << 32)) FAIL("%lld pairs in a chunk", (long long)npairs);

    // regions: 256-aligned, in order, each at least what its user reads or writes
    const int64_t o[8] = {0, L.off_coarse, L.off_extra, L.off_sort, L.off_tiles, L.off_items, L.off_parts, L.total};
    for (int i = 0; i < 8; ++i)
        if (o[i] % 256 || (i && o[i] < o[i - 1])) FAIL("offset %d (%lld) unaligned or descending", i, (long long)o[i]);
    const int64_t need[7] = {L.flat_bytes, npairs * 8, c * extra, L.sort_bytes, tiled ? (int64_t)(s.nlist + 1) * 4 : 0, L.max_items * 4,
                             npairs * k * 8};
    for (int i = 0; i < 7; ++i)
        if (o[i + 1] - o[i] < need[i]) FAIL("region %d holds %lld bytes, its user needs %lld", i, (long long)(o[i + 1] - o[i]), (long long)need[i]);
    // the coarse step's own scratch, for both chunk lengths run
    if (L.flat_bytes < lvs_flat_workspace_bytes(c, s.nlist, s.d, s.nprobe, s.pack, s.pack) ||
        (tail && L.flat_bytes < lvs_flat_workspace_bytes(tail, s.nlist, s.d, s.nprobe, s.pack, s.pack)))
        FAIL("coarse region below the flat search's declared size");
    if (tiled) {
        // work items: sum over lists of ceil(pairs / 32) <= (npairs + 31 x non-empty lists) / 32
        const int64_t lists = npairs < s.nlist ? npairs : s.nlist;
        if (L.max_items != lvs_ivf_max_items(npairs, s.nlist) || L.max_items < (npairs + 31 * lists) / 32) FAIL("max_items %lld", (long long)L.max_items);
        BucketPlan b;
        if (!bucket_plan(npairs, s.nlist, b) || b.total != L.sort_bytes || !bucket_ok(npairs, s.nlist, b)) FAIL("the pairs' bucket sort");
    } else if (L.sort_bytes || L.max_items || L.off_sort != L.off_parts) {
        FAIL("an untiled mode with tiling regions");
    }
    if (pq)
        for (long long nb : {0ll, 1ll, 4000ll, 60000ll, IVF_PRANGE_NB, 100000000ll})
            for (int64_t cn : {c, tail ? tail : c}) {
                const int pr = lvs_ivf_pq_prange(nb, s.nlist, cn, s.nprobe);
                if (pr < 1 || pr > s.nprobe || pr > LVS_PQ_MAXRANGE || (s.nprobe + pr - 1) / pr > s.nprobe) FAIL("prange %d", pr);
            }
    return true;
}
static bool ivf_grid(bool dump, long* shapes, long* halved) {
    const long long nqs[] = {0, 1, 255, 3001, 10001, 16384, 16385, 32767, 32769, 40000};
    const int lists[][2] = {{1, 1}, {1, 16}, {40, 4}, {40, 40}, {4097, 257}, {8200, 2048}, {24575, 16}, {24576, 16}, {30000, 2048}};  // nlist, nprobe
    const int ks[] = {1, 16, 17, 32, 33, 56};
    // mode, d, M: at and beside each scan's LDS limit (tests/test_ivf_edges_host.py)
    const int scans[][3] = {{LVS_IVF_FLAT, 64, 1},    {LVS_IVF_FLAT, 1088, 1},  {LVS_IVF_FLAT, 1152, 1},  {LVS_IVF_FLAT, 1216, 1},
                            {LVS_IVF_FLAT, 1280, 1},  {LVS_IVF_FLAT, 2240, 1},  {LVS_IVF_FLAT, 2304, 1},  {LVS_IVF_FLAT, 2432, 1},
                            {LVS_IVF_FLAT, 2496, 1},  {LVS_IVF_SQ8, 64, 1},     {LVS_IVF_SQ8, 2368, 1},   {LVS_IVF_SQ8, 2369, 1},
                            {LVS_IVF_SQ8, 2432, 1},   {LVS_IVF_SQ8, 2433, 1},   {LVS_IVF_PQ, 64, 8},      {LVS_IVF_PQ, 636, 159},
                            {LVS_IVF_PQ, 640, 160},   {LVS_IVF_PQ, 3072, 3},    {LVS_IVF_RANGE, 64, 1},   {LVS_IVF_RANGE, 1216, 1},
                            {LVS_IVF_RANGE, 1280, 1}, {LVS_IVF_RANGE, 2496, 1}, {LVS_IVF_RANGE, 2560, 1}};
    bool tail1 = false, tailc1 = false;
    for (const auto& sc : scans)
        for (int pack = 0; pack < 2; ++pack)
            for (const auto& ls : lists)
                for (int k : ks) {
                    if (sc[0] == LVS_IVF_RANGE && k != ks[0]) continue;  // (no k)
                    std::vector<long long> todo(nqs, nqs + sizeof(nqs) / sizeof(nqs[0]));
                    for (size_t i = 0; i < todo.size(); ++i) {
                        const IvfShape s = {sc[0], todo[i], ls[0], ls[1], sc[1], sc[2], sc[0] == LVS_IVF_RANGE ? 0 : k, pack};
                        long long c;
                        if (!ivf_shape(s, dump, &c)) {
                            printf("FAILED at ivf mode=%d nq=%lld nlist=%d nprobe=%d d=%d M=%d k=%d pack=%d\n", s.mode, s.nq, s.nlist, s.nprobe, s.d, s.M, s.k, s.pack);
                            return false;
                        }
                        ++*shapes;
                        if (c > 0 && c < (s.nq < IVF_CHUNK_MAX ? s.nq : IVF_CHUNK_MAX)) ++*halved;
                        if (c > 1 && s.nq % c == 1) tail1 = true;
                        if (c > 2 && s.nq % c == c - 1) tailc1 = true;
                        // the largest call of the list: two more, with last chunks of 1 and of c - 1 queries
                        if (i + 1 == sizeof(nqs) / sizeof(nqs[0]) && c > 2) todo.insert(todo.end(), {2 * c + 1, 3 * c - 1});
                    }
                }
    if (!tail1 || !tailc1) FAIL("the grid has no last chunk of 1 / of c - 1 queries");
    const long long ns[] = {0, 1, 8192, 8193, 1000000, 0xFFFFFFFEll, 0xFFFFFFFFll};
    const int bk[] = {0, 1, 24575, 24576, 100000, 1 << 26, 100659200, 100663296};
    for (long long n : ns)
        for (int k : bk) {
            if (!bucket_shape(n, k, dump)) {
                printf("FAILED at bucket n=%lld k=%d\n", n, k);
                return false;
            }
            ++*shapes;
        }
    return true;
}

// ---- the threshold join (lvs_range_chunk_plan) ----
struct JoinLaunch {
    int kernel;
    long long c0, cn, r0, rn;
};
static std::vector<JoinLaunch> join_launches(int64_t nq, int64_t nb, int64_t q_row0, int64_t id_offset, int d, int pack, int metric, int stride,
                                             bool* rj) {
    std::vector<JoinLaunch> out;
    LvsTilePlan p;
    *rj = false;
    if (lvs_plain_tile_plan(nq, nb, d, pack, pack, p) != LVS_OK || nq == 0 || nb == 0) return out;
    *rj = lvs_range_rj_ok(nq, p.l.dpad, pack, pack, metric, stride);
    if (!*rj) {
        out.push_back({LVS_RANGE_LIST, 0, nq, 0, nb});
        return out;
    }
    for (int64_t c0 = 0, cn = 0; c0 < nq; c0 += cn) {
        cn = range_chunk_len(nq - c0);
        const LvsRangeChunk c = lvs_range_chunk_plan(c0, cn, nb, q_row0, id_offset);
        if (c.rn > 0) out.push_back({c.kernel, c0, cn, c.r0, c.rn});
        if (c.rn > 0 && c.tn > 0) out.push_back({LVS_RANGE_LIST, c0, cn, c.t0, c.tn});
    }
    return out;
}
static bool join_shape(int64_t nq, int64_t nb, int64_t q_row0, int64_t id_offset, int d, int pack, int metric, int stride, bool dump) {
    bool rj;
    const std::vector<JoinLaunch> ls = join_launches(nq, nb, q_row0, id_offset, d, pack, metric, stride, &rj);
    if (dump) {
        printf("join nq=%lld nb=%lld q_row0=%lld id_offset=%lld d=%d pack=%d metric=%d stride=%d | rj %d | launches", (long long)nq, (long long)nb,
               (long long)q_row0, (long long)id_offset, d, pack, metric, stride, (int)rj);
        for (const JoinLaunch& l : ls) printf(" %d:%lld:%lld:%lld:%lld", l.kernel, l.c0, l.cn, l.r0, l.rn);
        printf("\n");
    }
    // The launches are rectangles (queries [c0, c0 + cn)) x (rows [r0, r0 + rn)).  Walk them in order: the query ranges are the
    // chunks, each once and in order; inside a chunk the row ranges follow each other without gap or overlap up to nb - so the
    // rectangles are disjoint and the tail rows are taken once - and start at or below the first row the chunk must see:
    // row 0 (a plain join), or the row after the chunk's first query (a self-join reports j > i only)
    size_t at = 0;
    for (int64_t c0 = 0, cn = 0; c0 < nq; c0 += cn) {
        cn = rj ? range_chunk_len(nq - c0) : nq;
        int64_t first = q_row0 >= 0 && rj ? q_row0 + c0 - id_offset + 1 : 0;  // (one launch of the list kernel takes every row)
        first = first < 0 ? 0 : (first > nb ? nb : first);
        int64_t covered = -1;
        for (; at < ls.size() && ls[at].c0 == c0; ++at) {
            const JoinLaunch& l = ls[at];
            if (l.cn != cn || l.rn <= 0 || l.r0 < 0 || (covered >= 0 && l.r0 != covered)) FAIL("launch %zu: queries or rows out of step", at);
            if (covered < 0 && l.r0 > first) FAIL("launch %zu starts at row %lld, the chunk pairs from row %lld", at, l.r0, (long long)first);
            covered = l.r0 + l.rn;
            if (l.kernel == LVS_RANGE_RJ) {
                LvsGroupedGeom g;
                if (l.r0 % 32 || l.rn % 32 || l.rn < LVS_RQ_JOIN_MINROWS || l.cn <= 128 || !lvs_grouped_geometry(l.cn, l.rn / 32, g))
                    FAIL("launch %zu: not a launch of lvs_rj_kernel", at);
            }
        }
        if (covered < 0 ? first < nb : covered != nb) FAIL("chunk at %lld: rows up to %lld of %lld", (long long)c0, (long long)covered, (long long)nb);
    }
    if (at != ls.size()) FAIL("%zu launches beyond the chunks", ls.size() - at);
    return true;
}
static bool join_grid(bool dump, long* shapes) {
    const long long nqs[] = {0, 129, 2047, 2048, 4296, 40000, 70001, 100000};
    const long long nbs[] = {0, 1000, 32767, 32768, 32800, 40001, 70001, 100000, 100031};
    const long long selfs[][2] = {{-1, 0}, {0, 0}, {5000, 0}, {5000, 5000}, {0, 1000}, {31, 0}, {99968, 0}, {200000, 0}};  // q_row0, id_offset
    const int variants[][4] = {{768, 0, 0, 1}, {384, 0, 0, 1}, {100, 0, 0, 1}, {768, 1, 0, 1}, {768, 0, 1, 1}, {768, 0, 0, 2}};  // d, pack, metric, stride
    for (long long nq : nqs)
        for (long long nb : nbs)
            for (const auto& sf : selfs)
                for (const auto& v : variants) {
                    if (!join_shape(nq, nb, sf[0], sf[1], v[0], v[1], v[2], v[3], dump)) {
                        printf("FAILED at join nq=%lld nb=%lld q_row0=%lld id_offset=%lld d=%d pack=%d metric=%d stride=%d\n", nq, nb, sf[0], sf[1], v[0],
                               v[1], v[2], v[3]);
                        return false;
                    }
                    ++*shapes;
                }
    return true;
}

static int query_mode() {
    char cmd[32];
    long long a[8];
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        const int n = sscanf(line, "%31s %lld %lld %lld %lld %lld %lld %lld %lld", cmd, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]);
        if (n < 1) continue;
        const std::string c = cmd;
        if (c == "rq_fits" && n == 5) {
            printf("%d\n", (int)lvs_rq_fits(a[0], a[1], (int)a[2], (int)a[3]));
        } else if (c == "grouped" && n == 3) {  // nq, 32-row blocks -> groups nparts blocks_per_wg grid
            LvsGroupedGeom g;
            if (lvs_grouped_geometry(a[0], a[1], g)) printf("%d %d %d %d\n", g.groups, g.nparts, g.blocks_per_wg, lvs_rq_grid(g.groups, g.nparts));
            else printf("none\n");
        } else if (c == "ranges_for" && n == 2) {
            printf("%d\n", lvs_rq_ranges_for((int)a[0]));
        } else if (c == "item" && n == 4) {  // block, groups, nparts -> range group
            int range, group;
            if (lvs_rq_item((int)a[0], (int)a[1], (int)a[2], range, group)) printf("%d %d\n", range, group);
            else printf("none\n");
        } else if (c == "chunk_size" && n == 2) {
            printf("%lld\n", (long long)rq_chunk_size(a[0]));
        } else if ((c == "chunks" && n == 3) || (c == "range_chunks" && n == 2)) {  // nq [maximum] -> the chunk lengths
            for (int64_t left = a[0]; left > 0;) {
                const int64_t cn = c == "chunks" ? rq_chunk_len(left, rq_chunk_size(a[1])) : range_chunk_len(left);
                printf("%lld ", (long long)cn);
                left -= cn;
            }
            printf("\n");
        } else if (c == "route" && n == 7) {  // nq nb d k xb_pack xq_pack -> kind nbfrag kcap nqb groups sample_rows jper nseg
            LvsFlatPlan p;
            TwoPhasePlan tp;
            if (lvs_flat_plan(a[0], a[1], (int)a[2], (int)a[4], (int)a[5], false, (int)a[3], p) != LVS_OK) {
                printf("none\n");
                continue;
            }
            const LvsRoute r = lvs_flat_route(a[0], a[1], p.l, (int)a[3], p.w.npass, 0, make_two_phase_plan(a[0], a[1], (int)a[3], tp));
            printf("%d %d %d %d %d %lld %d %d\n", r.kind, r.stream.nbfrag, r.stream.kcap, r.stream.nqb, r.stream.groups,
                   (long long)(r.kind == LVS_ROUTE_STREAM ? lvs_stream_sample_rows(a[0], a[1]) : 0), p.l.dpad / 16, p.l.nseg);
        } else if (c == "chunk_kernel" && n == 5) {  // cn nb dpad k -> LVS_CHUNK_* of a chunk of cn queries (no row ids)
            printf("%d\n", lvs_rq_chunk_kernel(a[0], a[1], (int)a[2], (int)a[3], false));
        } else if (c == "tile_geom" && n == 4) {  // nq nb k -> the list kernel's geometry for a top-k pass: v2 (1: 256 x 256) nslab
            const LvsTileGeom g = lvs_tile_geometry(lvs_tile_request_topk(a[0], a[1], (int)a[2]));
            printf("%d %d\n", g.v2, g.nslab);
        } else if (c == "two_phase" && n == 4) {  // nq nb k -> ran (0 / 1), selection passes, the plan's bytes (0: no plan)
            TwoPhasePlan tp;
            const bool ok = make_two_phase_plan(a[0], a[1], (int)a[2], tp);
            printf("%d %d %lld\n", (int)ok, lvs_workspace(a[0], a[1], (int)a[2], 1).npass, (long long)(ok ? tp.total : 0));
        } else if (c == "ivf_limits" && n == 1) {  // -> IVF_WS_BUDGET IVF_CHUNK_MAX
            printf("%lld %lld\n", (long long)IVF_WS_BUDGET, (long long)IVF_CHUNK_MAX);
        } else if (c == "ivf_chunk" && n == 9) {  // mode (LVS_IVF_*) nq nlist nprobe d M k pack -> chunk tail total
            LvsIvfPlan L;
            if (lvs_ivf_plan((int)a[0], a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[7], L) == LVS_OK)
                printf("%lld %lld %lld\n", (long long)L.chunk, (long long)(a[1] % L.chunk), (long long)L.total);
            else printf("none\n");
        } else if (c == "ivf_fits" && n == 6) {  // mode d M k pack
            printf("%d\n", (int)lvs_ivf_fits((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4]));
        } else if (c == "range_plan" && n == 9) {  // nq nb q_row0 id_offset d pack metric stride -> kernel c0 cn r0 rn of every launch
            bool rj;
            for (const JoinLaunch& l : join_launches(a[0], a[1], a[2], a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], &rj))
                printf("%d %lld %lld %lld %lld ", l.kernel, l.c0, l.cn, l.r0, l.rn);
            printf("\n");
        } else if (c == "bound_coef" && n == 5) {  // metric pack d exp_sum -> the five floats' bit patterns
            LvsBoundCoef k;
            if (lvs_nearest_bound_coef((int)a[0], (int)a[1], (int)a[2], (int)a[3], k) == LVS_OK) {
                uint32_t bits[5];
                memcpy(bits, k.c, sizeof(bits));
                printf("%u %u %u %u %u\n", bits[0], bits[1], bits[2], bits[3], bits[4]);
            } else printf("none\n");
        } else {
            printf("?\n");
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--query")) return query_mode();
    const bool dump = argc > 1 && !strcmp(argv[1], "--dump");
    const long long nqs[] = {0, 1, 2, 96, 97, 128, 129, 256, 257, 4096, 4097, 8192, 12500, 20000, 25000, 50000, 65236, 65536, 100000, 1000000};
    const long long nbs[] = {0, 1, 255, 4096, 32767, 32768, 65536, 125000, 250001, 500000, 1000000, 10000000};
    const int ds[] = {8, 64, 100, 256, 384, 768, 1536};
    const int ks[] = {1, 2, 10, 15, 16, 48, 56, 57, 100, 1000, 2048};
    long shapes = 0;
    for (long long nq : nqs)
        for (long long nb : nbs)
            for (int d : ds)
                for (int k : ks)
                    for (int bp = 0; bp < 2; ++bp)
                        for (int qp = 0; qp < 2; ++qp)
                            for (int hi = 0; hi < 2; ++hi) {
                                Row r;
                                if (!plan_shape(nq, nb, d, k, bp, qp, hi != 0, r)) {
                                    printf("FAILED at nq=%lld nb=%lld d=%d k=%d pack=%d/%d hi=%d\n", nq, nb, d, k, bp, qp, hi);
                                    return 1;
                                }
                                if (dump) print_row(r);
                                ++shapes;
                            }
    long ivf = 0, halved = 0, joins = 0;
    if (!ivf_grid(dump, &ivf, &halved) || !join_grid(dump, &joins)) return 1;
    if (!dump) printf("ok %ld shapes\nok %ld ivf and bucket shapes (%ld with a halved chunk), %ld joins\n", shapes, ivf, halved, joins);
    return 0;
}
