"""The flat-search shapes of the extent tests (test_gpu_workspace_extents.py, test_gpu_output_extents.py), one per path of
lvs_flat_search_keys, each with the path it is here for as the host planner (lotus_amd/csrc/lvs_plan.h through
tests/native/plan_check.cpp) states it.  ``check_routes`` compares the table with the planner, so a planner change that moves
a shape off its path fails (test_ws_guard_host.py runs it without a GPU) instead of quietly weakening the GPU tests."""
from dataclasses import dataclass, field

import plan_native
from lotus_amd import _capi

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
RQ, RQ_JOIN, STREAM, LIST = 0, 1, 2, 3  # LVS_ROUTE_* (lvs_plan.h)
CHUNK_MAX = 65536                       # LVS_RQ_CHUNK_DEFAULT
RQ_CHUNK, RJ, RJ_SOLO = 0, 1, 2         # LVS_CHUNK_*: the kernel of one chunk of a chunked join


@dataclass
class Flat:
    name: str
    nq: int
    nb: int
    d: int
    k: int
    mode: int
    metric: int
    route: int
    # what else the planner must say of the shape: groups / nqb (streaming: sibling groups, query blocks per workgroup),
    # sample (streaming: the sample pass that writes off_seeds runs), tile_seeds (list kernel: seeded, off_tile_seeds),
    # chunks / kernels (chunked join: the chunk lengths and each chunk's LVS_CHUNK_* kernel), npass (selection passes the
    # workspace is laid out for), two_phase (a two-phase plan exists: it runs, the passes are its fallback), v2 (list kernel:
    # the 256 x 256-query geometry of up to 15 slots, not the 256 x 128 one)
    plan: dict = field(default_factory=dict)

    @property
    def id(self):
        return self.name


FLAT = [
    # streaming kernel, one workgroup per corpus range; the second query block nearly empty, one row past a 32-row block
    Flat("stream-2blocks", 33, 4097, 100, 16, F16, IP, STREAM, dict(groups=1, nqb=2, sample=False)),
    Flat("stream-1query-k56", 1, 4096, 768, 56, F16, L2, STREAM, dict(groups=1, nqb=1, sample=False)),
    # ... seeded: the shortest corpus with a sample (nb / 8 >= 4 096 rows)
    Flat("stream-seeded", 40, 32768 + 1, 64, 10, F16, IP, STREAM, dict(groups=1, sample=True)),
    # ... sibling groups (too short to seed the list kernel): empty ranges write empty lists
    Flat("stream-siblings", 256, 4100, 64, 56, F16, L2, STREAM, dict(groups=3, nqb=3, sample=False)),
    # register-resident queries, one launch: one group; two groups, the second holding one query
    Flat("rq-1group", 97, 32768 + 1, 256, 16, F16, IP, RQ),
    Flat("rq-2groups", 257, 65536, 384, 10, F16, L2, RQ),
    # chunked join: 4 096 + 1 queries and a corpus with nb % 32 = 1 tail row (one more launch's lists behind the chunk's)
    Flat("join-ragged-tail", 4097, 32768 + 33, 256, 10, F16, IP, RQ_JOIN, dict(chunks=[4096, 1], kernels=[RJ, RQ_CHUNK])),
    Flat("join-8192+5", 8192 + 5, 32768, 256, 16, F16, L2, RQ_JOIN, dict(chunks=[8192, 5], kernels=[RJ, RQ_CHUNK])),
    # ... a solo chunk (one corpus range, whole blocks): lvs_rj_kernel writes out_keys itself
    Flat("join-solo", 65536, 32768, 256, 10, F16, IP, RQ_JOIN, dict(chunks=[65536], kernels=[RJ_SOLO])),
    # list kernel, one pass: 15 slots on the 256-query geometry, 16 on the 128-query one
    Flat("list-k15", 300, 4000, 100, 15, F16, IP, LIST, dict(npass=1, tile_seeds=False, v2=True)),
    Flat("list-k16", 300, 4000, 100, 16, F16, IP, LIST, dict(npass=1, tile_seeds=False, v2=False)),
    # ... hi|lo rows on both sides: three K segments
    Flat("list-split", 130, 3000, 200, 30, SPLIT, IP, LIST, dict(npass=1)),
    # ... seeded from sample tiles (off_tile_seeds): d = 64 keeps the shape off the register-resident kernel
    Flat("list-seeded", 129, 41000, 64, 10, F16, L2, LIST, dict(npass=1, tile_seeds=True)),
    # selection passes (off_pass): 56 + 1
    # (four tiles cannot give the two-phase search its 72 candidates: 3 000 rows can, see below)
    Flat("passes-57", 200, 1000, 384, 57, F16, IP, LIST, dict(npass=2, two_phase=False)),
    Flat("passes-57-tiny", 2, 255, 64, 57, F16, IP, LIST, dict(npass=2, two_phase=False)),
    # two phases (the selection passes are their predicated fallback)
    Flat("two-phase-k57", 200, 3000, 384, 57, F16, IP, LIST, dict(npass=2, two_phase=True)),
    Flat("two-phase-k100", 300, 60000, 64, 100, F16, IP, LIST, dict(npass=2, two_phase=True)),
    Flat("two-phase-k2048", 40, 150000, 100, 2048, SPLIT, IP, LIST, dict(npass=37, two_phase=True)),
    # k > nb: padded with key 0
    Flat("k-beyond-nb", 5, 3, 8, 5, F16, IP, LIST, dict(npass=1)),
]
FLAT_BY_NAME = {c.name: c for c in FLAT}


def planner_says(c: Flat) -> dict:
    """Everything ``Flat.plan`` may name, as the planner has it."""
    kind, _, _, nqb, groups, sample, _, _ = plan_native.ask([f"route {c.nq} {c.nb} {c.d} {c.k} {c.mode} {c.mode}"])[0]
    ran, npass, tp_bytes = plan_native.ask([f"two_phase {c.nq} {c.nb} {c.k}"])[0]
    v2, _ = plan_native.ask([f"tile_geom {c.nq} {c.nb} {min(c.k, 56)}"])[0]
    lib = _capi.load()
    chunks = plan_native.ask([f"chunks {c.nq} {CHUNK_MAX}"])[0]
    dpad = -(-c.d // 64) * 64
    kernels = [a[0] for a in plan_native.ask([f"chunk_kernel {cn} {c.nb} {dpad} {c.k}" for cn in chunks])]
    return dict(route=kind, groups=groups, nqb=nqb, sample=sample > 0, chunks=chunks, kernels=kernels,
                npass=npass, two_phase=bool(ran), tp_bytes=tp_bytes, v2=bool(v2),
                tile_seeds=int(lib.lvs_flat_search_seed_tiles(c.nq, c.nb, c.k)) > 0,
                bytes=int(lib.lvs_flat_search_workspace_bytes(c.nq, c.nb, c.d, c.k, c.mode, c.mode)))


def check_routes():
    for c in FLAT:
        says = planner_says(c)
        assert says["route"] == c.route, (c.name, says)
        for key, want in c.plan.items():
            assert says[key] == want, (c.name, key, says)
        assert says["bytes"] > 0
    assert {c.route for c in FLAT} == {RQ, RQ_JOIN, STREAM, LIST}  # every route id the planner can return
