// Runs the flat search's host planner (lotus_amd/csrc/lvs_plan.h, the only project header included) on a CPU.
//   plan_check           walks the grid below and fails on the first violated invariant of geometry, layout, route and chunks
//   plan_check --dump    one line per grid shape with every field of layout, geometry, two-phase plan, route, chunk list and
//                        workspace offsets (tests/test_plan_pins.py pins some; the whole dump is what a refactor diffs)
//   plan_check --query   answers questions read from stdin, one per line, for the Python models of tests/test_rq_*.py and
//                        the route tables of tests/test_widths_host.py and tests/extent_cases.py
// Built with a plain host compiler by tests/plan_native.py (run from tests/test_capi.py).
#include "../../lotus_amd/csrc/lvs_plan.h"

#include <cstdio>
#include <cstring>
#include <string>

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

static int query_mode() {
    char cmd[32];
    long long a[6];
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        const int n = sscanf(line, "%31s %lld %lld %lld %lld %lld %lld", cmd, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
        if (n < 2) continue;
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
    if (!dump) printf("ok %ld shapes\n", shapes);
    return 0;
}
