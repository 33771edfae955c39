"""Exact-arithmetic inputs for every flat search route, the threshold join, the score rows and the nearest search: the generator,
the reference, the guards, the case tables and one ``run_*`` function per kind of leg, taking a backend.  No test lives here:
tests/test_lattice_host.py runs the guards, asks the compiled planner which kernel each case reaches and runs every ``run_*`` on
the CPU oracle's backend; tests/test_gpu_lattice.py runs the same functions on ``HipBackend``.  Imports no GPU module.

The data are small integers times a power of two (``lattice``): every value fits fp16 (a hi|lo image stores it with lo == 0),
row norms are exact, and every partial sum of q.y and of |q|^2 + |y|^2 - 2 q.y is an integer multiple of one unit far below
2^24 units - float32 arithmetic on them is EXACT IN ANY SUMMATION ORDER.  So the device must return the oracle's keys bit for
bit, the last rank included, and no comparison here has a tolerance: top-k legs assert ``np.array_equal(device keys, ref_keys)``,
join legs the exact pair set and the scores' bits.  Such data are also full of ties - hundreds of rows share a query's k-th
score, thresholds sit on attained values - which is what the Gaussian rows of the other GPU tests never give.

Large batches are few distinct queries tiled (a query's result does not depend on its batch: the reference is the small one,
and every query of a 65 536-query launch is checked); long corpora are drawn with replacement from a few thousand rows (exact
duplicates at every distance, across every block and range boundary)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import oracle
import plan_native
from oracle.flat import pack_keys
from oracle_backend import OracleBackend

F16, SPLIT = 0, 1  # lotus_amd._capi.PACK_F16 / PACK_SPLIT
IP, L2 = 0, 1      # lotus_amd._capi.METRIC_IP / METRIC_L2
STEP = 2.0 ** -3   # the lattice step of every operand; a score's unit is STEP^2 = 2^-6
TILE, STREAM, RQ, RJ = "lvs_tile_kernel", "lvs_stream_kernel", "lvs_rq_kernel", "lvs_rj_kernel"
ROUTE_RQ, ROUTE_RQ_JOIN, ROUTE_STREAM, ROUTE_LIST = 0, 1, 2, 3  # lvs_plan.h: LVS_ROUTE_*
CHUNK_RQ, CHUNK_RJ, CHUNK_RJ_SOLO = 0, 1, 2                     # LVS_CHUNK_*
RANGE_LIST, RANGE_RJ = 0, 1                                     # LVS_RANGE_*
BASE_ROWS = 4096       # distinct rows of a corpus drawn with replacement
LONG_CORPUS = 8000     # from this many rows on a corpus is drawn with replacement
SCALED_DOWN = 2.0 ** -9  # the scaled legs pack lattice x 2^-9 with exp="auto"
LO_STEP = 2.0 ** -14   # the lo half planted by the real-lo leg: (1 + 2^-11) 2^-3 = 2^-3 + 2^-14


def lattice(n, d, seed, levels, keep, scale=STEP):
    """float32 [n, d]: scale x integers(-levels .. levels), each entry kept with probability ``keep``, else 0.  Not normalised."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-levels, levels + 1, (n, d))
    return (np.where(rng.random((n, d)) < keep, v, 0) * scale).astype(np.float32)


def flavour(d, dense):
    """ternary (few distinct scores, mass ties; denser at d = 64) or dense (more distinct scores)."""
    return dict(levels=2, keep=1.0) if dense else dict(levels=1, keep=0.5 if d <= 64 else 0.25)


def split_lo(x):
    """The lo half of the CPU emulation of hi|lo packing: fp16(x - fp16(x))."""
    x = np.asarray(x, np.float32)
    return (x - x.astype(np.float16).astype(np.float32)).astype(np.float16)


def scores64(xb, xq, metric):
    """float64 score matrix [nq, nb], larger is better: q.y, or -(|q|^2 + |y|^2 - 2 q.y)."""
    b, q = np.asarray(xb, np.float64), np.asarray(xq, np.float64)
    s = q @ b.T
    return s if metric == IP else -np.maximum((q * q).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * s, 0.0)


def guard_exact(xb, xq, metric, unit, lo_free=(True, True)):
    """Guard 1: float32 arithmetic on the case is exact in any summation order.  The float64 scores equal their float32 rounding;
    the sum of the MAGNITUDES of every term (which bounds every partial sum of every order, so it is stricter than max |score|)
    stays below 2^24 units; every term is a whole number of units; lo == 0 on every lo-free operand.  -> float64 scores."""
    s = scores64(xb, xq, metric)
    assert np.array_equal(s, s.astype(np.float32).astype(np.float64))
    b, q = np.abs(np.asarray(xb, np.float64)), np.abs(np.asarray(xq, np.float64))
    mag = q @ b.T if metric == IP else (q * q).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * (q @ b.T)
    assert mag.max() / unit < 2.0 ** 24, mag.max() / unit
    assert np.array_equal(s / unit, np.rint(s / unit))
    for x, free in ((xb, lo_free[0]), (xq, lo_free[1])):
        assert np.array_equal(x, np.asarray(x, np.float32).astype(np.float16).astype(np.float32)) == free
        assert not free or not split_lo(x).any()
    return s


def ref_keys(xb, xq, k, metric, id_offset=0):
    """``oracle.flat.pack_keys`` over ``oracle.flat_search``'s (D, I): better = D for inner product, -D for squared L2; empty slots
    are key 0; ids + id_offset."""
    D, I = oracle.flat_search(xb, xq, k, metric)
    return _keys_of(D, I, metric, id_offset)


def _keys_of(D, I, metric, id_offset=0):
    valid = I >= 0
    better = np.where(valid, D if metric == IP else -D, np.float32(0)).astype(np.float32)
    return np.where(valid, pack_keys(better, np.where(valid, I + id_offset, 0)), np.uint64(0))


def _u64(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def _np(t):
    return t.cpu().numpy()


def _pack(be, x, mode, **kw):
    return be.pack(x.astype(np.float16) if mode == F16 else np.ascontiguousarray(x, np.float32), mode, **kw)


class ExactOracleBackend(OracleBackend):
    """``OracleBackend`` with the one thing it leaves open settled as the device settles it: with ``row_ids`` the keys carry the
    MAPPED ids, so among equal scores the lower mapped id wins a list's last slots (the double picks by row position and only
    re-sorts what it picked - the same thing wherever no tie straddles rank k, which on these inputs is nowhere)."""

    def search_keys(self, corpus, queries, k, metric, id_offset=0, row_ids=None, **kw):
        if row_ids is None or corpus.n == 0:
            return super().search_keys(corpus, queries, k, metric, id_offset=id_offset, row_ids=row_ids, **kw)
        import torch

        rid = row_ids.numpy().view(np.uint32).astype(np.int64)
        order = np.argsort(rid, kind="stable")  # rows in the order of their ids: position order is then id order
        D, I = oracle.flat_search(corpus.rows.numpy()[order], queries.rows.numpy(), min(k, corpus.n), metric)
        keys = _keys_of(D, np.where(I >= 0, rid[order][np.where(I >= 0, I, 0)], -1), metric)
        keys = np.concatenate([keys, np.zeros((keys.shape[0], k - keys.shape[1]), np.uint64)], axis=1)
        return torch.from_numpy(keys.view(np.int64))


# ---- top-k cases -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TopK:
    name: str
    nq: int
    nb: int
    d: int
    k: int
    metric: int
    bpack: int = F16
    qpack: int = F16
    kernel: str = TILE          # what timing_read_full()["kernel"] reports after the call: the last timed launch's kernel
    plan: tuple = ()            # (field, value) pairs the compiled planner must confirm (``planned``)
    launches: int = 0           # > 0: the case is about chunking - timed launches of the one call
    dense: bool = False         # the dense flavour: the tie bar is 0.1 instead of 0.5
    one_pass: bool = False      # the certified one-pass search (hi|lo operands)
    id_offset: int = 0
    permuted_ids: bool = False  # row_ids = a permutation + 7
    scaled: bool = False        # lattice x 2^-9 packed hi|lo with exp="auto"
    real_lo: bool = False       # corpus rows carry one 12-bit coordinate: the lo halves are not zero (inner product only)
    host_nq: int = 0            # > 0: the CPU double runs only the first so many queries (its BLAS search of 65 536 is slow)
    seed: int = 0

    @property
    def m(self):
        """distinct queries: a batch of 64 or more holds every query at least twice, in different waves / workgroups"""
        return self.nq if self.nq < 64 else min(512, self.nq // 2)


def _topk_table():
    out = []

    def add(route, nq, nb, d, k, kernel, plan, metrics=(IP, L2), packs=((F16, F16),), **kw):
        for bp, qp in packs:
            for metric in metrics:
                name = f"{route}-{nq}x{nb}x{d}-k{k}-{'FS'[bp]}{'FS'[qp]}-{'IL'[metric]}"
                out.append(TopK(name, nq, nb, d, k, metric, bp, qp, kernel, tuple(sorted(plan.items())), **kw))

    FF, SS, FS = (F16, F16), (SPLIT, SPLIT), (F16, SPLIT)
    # stream, cold: the literal sem_search call; 64-slot lists full of ties
    add("stream-cold", 1, 6001, 64, 10, STREAM, dict(kind=ROUTE_STREAM, sample=0, groups=1))
    add("stream-cold", 32, 6001, 100, 56, STREAM, dict(kind=ROUTE_STREAM, sample=0, groups=1, kcap=64))
    # stream, self-seeded from a sample of 4 096 rows: the threshold is an attained score; three query blocks
    add("stream-seeded", 96, 33001, 64, 15, STREAM, dict(kind=ROUTE_STREAM, sample=4096, groups=1, nqb=3), packs=(FF, SS, FS))
    # stream, three sibling groups: hi|lo operands go here, not to lvs_rq_kernel
    add("stream-siblings", 200, 32805, 256, 10, STREAM, dict(kind=ROUTE_STREAM, sample=4096, groups=3), packs=(SS,))
    # lvs_rq_kernel: 97 .. 128 queries
    for k in (10, 16):
        add("rq", 128, 32800, 256, k, RQ, dict(kind=ROUTE_RQ, chunk_kernels=(CHUNK_RQ,)))
    # lvs_rj_kernel, one group, shared thresholds; the corpus' last 5 rows through lvs_rq_kernel; the last rank at k = 1
    for k in (1, 10, 16):
        add("rj-group", 200, 32805, 256, k, RJ, dict(kind=ROUTE_RQ, chunk_kernels=(CHUNK_RJ,)))
    for d in (384, 512, 768):
        add("rj-group", 200, 32805, d, 10, RJ, dict(kind=ROUTE_RQ, chunk_kernels=(CHUNK_RJ,)), dense=d == 768)
    # lvs_rj_kernel, two groups, 16-slot lists
    add("rj-two-groups", 300, 65541, 256, 16, RJ, dict(kind=ROUTE_RQ, chunk_kernels=(CHUNK_RJ,)), metrics=(IP,))
    # chunked calls: two launches, one call
    add("chunked", 4396, 32869, 256, 10, RQ, dict(kind=ROUTE_RQ_JOIN, chunks=(4096, 300), chunk_kernels=(CHUNK_RJ, CHUNK_RQ)),
        launches=2, host_nq=600)
    add("chunked-xcd", 8492, 32869, 256, 10, RQ, dict(kind=ROUTE_RQ_JOIN, chunks=(8192, 300), chunk_kernels=(CHUNK_RJ, CHUNK_RQ)),
        metrics=(IP,), launches=2, host_nq=600)
    # lvs_rj_kernel SOLO: one range, the lists written straight into the result
    add("rj-solo", 65536, 32768, 256, 10, RJ, dict(kind=ROUTE_RQ_JOIN, chunks=(65536,), chunk_kernels=(CHUNK_RJ_SOLO,)),
        metrics=(IP,), launches=1, host_nq=1024)
    # the list kernel, seeded by seed_kth on attained scores: 256 x 256 geometry, 15 slabs; 256 x 128 geometry, 29 slabs
    add("list-256x256", 300, 41001, 64, 10, TILE, dict(kind=ROUTE_LIST, v2=1, nslab=15, seeded=1, npass=1), packs=(FF, SS))
    add("list-256x128", 300, 65541, 64, 16, TILE, dict(kind=ROUTE_LIST, v2=0, nslab=29, seeded=1, npass=1), metrics=(IP,))
    # the largest single pass and the first k beyond it
    add("list-last-pass", 300, 5000, 100, 56, TILE, dict(kind=ROUTE_LIST, npass=1, two_phase=0), dense=True)
    add("list-first-beyond", 300, 5000, 100, 57, TILE, dict(kind=ROUTE_LIST, npass=2), dense=True)
    # two phases under mass ties: the bucket, the selection passes behind it
    add("two-phase", 64, 3000, 128, 100, TILE, dict(kind=ROUTE_LIST, npass=2, two_phase=1))
    add("two-phase", 40, 20000, 64, 300, TILE, dict(kind=ROUTE_LIST, npass=6, two_phase=1))
    # padding: key 0 behind the last row
    add("padding", 5, 3, 8, 5, TILE, dict(kind=ROUTE_LIST))
    # hi|lo one-pass certified against the same reference as the plain search of list-256x256
    add("certified", 300, 41001, 64, 10, TILE, dict(kind=ROUTE_LIST), packs=(SS,), one_pass=True)
    # ids: mapped row ids on a list case, the top of the id range on a list and a stream case
    add("ids-permuted", 300, 41001, 64, 10, TILE, dict(kind=ROUTE_LIST), metrics=(IP,), permuted_ids=True)
    add("ids-top", 300, 41001, 64, 10, TILE, dict(kind=ROUTE_LIST), metrics=(L2,), id_offset=2 ** 32 - 1 - 41001)
    add("ids-top", 200, 32805, 256, 10, RJ, dict(kind=ROUTE_RQ), metrics=(IP,), id_offset=2 ** 32 - 1 - 32805)
    # scaled operands: lattice x 2^-9, hi|lo with exp="auto" - one list case, one stream case
    add("scaled", 300, 41001, 64, 10, TILE, dict(kind=ROUTE_LIST), packs=(SS,), scaled=True)
    add("scaled", 96, 33001, 64, 15, STREAM, dict(kind=ROUTE_STREAM), packs=(SS,), scaled=True)
    # real lo halves in the corpus (inner product only: under L2 the row norm needs 30 bits and guard 1 refuses it)
    add("real-lo", 300, 41001, 64, 10, TILE, dict(kind=ROUTE_LIST), metrics=(IP,), packs=(SS,), real_lo=True)
    add("real-lo", 200, 32805, 256, 10, STREAM, dict(kind=ROUTE_STREAM, groups=3), metrics=(IP,), packs=(SS,), real_lo=True)
    return out


TOPK_CASES = _topk_table()
SHARD_CASE = next(c for c in TOPK_CASES if c.name == "list-256x256-300x41001x64-k10-FF-I")
SHARD_BOUNDS = [(0, 200), (200, 200), (200, 17003), (17003, 41001)]  # one of 200 rows, one empty, two ragged
SHARD_TILES = 12


@functools.lru_cache(maxsize=3)
def _topk_arrays(nq, nb, d, dense, seed, m, real_lo):
    """(xb [nb, d], base_q [m, d], the corpus' distinct rows) float32: the corpus (drawn with replacement from BASE_ROWS rows when
    long) and the distinct queries, every second one a copy of a corpus row."""
    rng = np.random.default_rng(1000 + seed)
    fl = flavour(d, dense)
    distinct = lattice(min(nb, BASE_ROWS) if nb >= LONG_CORPUS else nb, d, 11 + seed, **fl)
    xb = distinct[rng.integers(0, len(distinct), nb)] if nb >= LONG_CORPUS else distinct
    q = lattice(m, d, 23 + seed, **fl)
    q[::2] = xb[rng.integers(0, nb, len(q[::2]))]
    if real_lo:  # after the queries were drawn: they stay lo-free, so lo . lo is zero everywhere
        xb = xb.copy()
        xb[np.arange(nb), rng.integers(0, d, nb)] = rng.choice([-1.0, 1.0], nb).astype(np.float32) * np.float32(STEP + LO_STEP)
        distinct = xb
    return xb, q, distinct


def topk_data(c):
    """(xb, base_q, tile): the batch is base_q[tile]"""
    xb, q, _ = _topk_arrays(c.nq, c.nb, c.d, c.dense, c.seed, c.m, c.real_lo)
    return xb, q, np.arange(c.nq) % c.m


@functools.lru_cache(maxsize=8)
def _topk_ref(c):
    """(D, I) of the distinct queries at k + 1 (k where k >= nb): the first k columns are the top k, the last one says whether
    the k-th score is tied with the next.  With permuted ids the rows are searched in the order of their ids."""
    xb, q, _ = topk_data(c)
    if c.permuted_ids:
        xb = xb[np.argsort(row_ids_of(c), kind="stable")]
    return oracle.flat_search(xb, q, c.k + (c.k < c.nb), c.metric)


def row_ids_of(c):
    return (np.random.default_rng(77).permutation(c.nb) + 7).astype(np.int64)


def topk_ref_keys(c):
    """ref_keys of the distinct queries, [m, k] uint64"""
    D, I = _topk_ref(c)
    return _keys_of(D[:, :c.k], I[:, :c.k], c.metric, 7 if c.permuted_ids else c.id_offset)


def topk_guards(c):
    """Guards 1 and 2 of a top-k case.  -> the share of queries whose k-th and (k + 1)-th reference scores are equal (None:
    k >= nb, exempt)."""
    xb, q, _ = topk_data(c)
    unit = STEP * LO_STEP if c.real_lo else STEP * STEP  # real lo: every term is a multiple of 2^-3 x 2^-14
    guard_exact(_topk_arrays(c.nq, c.nb, c.d, c.dense, c.seed, c.m, c.real_lo)[2], q, c.metric, unit, lo_free=(not c.real_lo, True))
    assert not c.real_lo or c.metric == IP
    D, I = _topk_ref(c)
    # the oracle's float32 BLAS blocks give the float64 scores exactly, in the plain (score desc, id asc) order
    s = scores64(xb if not c.permuted_ids else xb[np.argsort(row_ids_of(c), kind="stable")], q[:8], c.metric)
    for i in range(min(8, len(q))):
        order = np.lexsort((np.arange(c.nb), -s[i]))[:D.shape[1]]
        assert np.array_equal(I[i, :len(order)], order) and np.array_equal((D if c.metric == IP else -D)[i, :len(order)], s[i, order])
    if c.k >= c.nb:
        return None
    tied = float((D[:, c.k - 1] == D[:, c.k]).mean())
    assert tied >= (0.1 if c.dense else 0.5), (c.name, tied)
    return tied


def planned(c):
    """What the compiled planner (tests/native/plan_check.cpp) says about the call: route kind; stream shape and sample; the
    chunks of a register-resident call and each chunk's kernel; the list kernel's geometry, passes, seed tiles, two-phase plan."""
    kind, nbfrag, kcap, nqb, groups, sample, jper, nseg = plan_native.ask([f"route {c.nq} {c.nb} {c.d} {c.k} {c.bpack} {c.qpack}"])[0]
    p = dict(kind=kind)
    dpad = jper * 16
    if kind == ROUTE_STREAM:
        p.update(kcap=kcap, nqb=nqb, groups=groups, sample=sample)
    elif kind in (ROUTE_RQ, ROUTE_RQ_JOIN):
        chunks = plan_native.ask([f"chunks {c.nq} 65536"])[0]
        p["chunks"] = tuple(chunks)
        p["chunk_kernels"] = tuple(a[0] for a in plan_native.ask([f"chunk_kernel {cn} {c.nb} {dpad} {c.k}" for cn in chunks]))
    else:
        from lotus_amd import _capi

        (v2, nslab), (ok, npass, _) = plan_native.ask([f"tile_geom {c.nq} {c.nb} {c.k}", f"two_phase {c.nq} {c.nb} {c.k}"])
        p.update(v2=v2, nslab=nslab, npass=npass, two_phase=ok,
                 seeded=int(_capi.load().lvs_flat_search_seed_tiles(c.nq, c.nb, c.k) > 0) if c.k <= 56 else 0)
    return p


def _timed(be, call):
    """-> (call's result, timing dict or None on a backend without the hook)"""
    hook = hasattr(be, "timing_read_full")
    if hook:
        be.timing_enable(True)
    out = call()
    if not hook:
        return out, None
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    return out, t


def _assert_keys(got, want, what):
    """THE assertion of a top-k leg.  (The message names the first difference: query, rank, the two keys.)"""
    if not np.array_equal(got, want):
        q, r = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).any(axis=1).sum())} of {len(got)} queries differ; first at query {q} rank {r}: "
                             f"device {int(got[q, r]):#018x} reference {int(want[q, r]):#018x}")


def run_topk(be, c, host=False):
    """One search of the case on ``be``: the keys equal ``ref_keys`` bit for bit.  -> dict(kernel, launches, stats) as the timing
    hook reports them (None values on a backend without one)."""
    xb, q, tile = topk_data(c)
    want = topk_ref_keys(c)
    if host and c.host_nq:
        tile = tile[:c.host_nq]
    xq = q[tile]
    scale = np.float32(SCALED_DOWN if c.scaled else 1.0)
    cb = _pack(be, xb * scale, c.bpack, exp="auto" if c.scaled else 0)
    cq = _pack(be, xq * scale, c.qpack, exp=cb.exp)
    kw, stats = {}, {}
    if c.permuted_ids:
        kw["row_ids"] = be.to_device(row_ids_of(c).astype(np.uint32).view(np.int32))
    keys, t = _timed(be, lambda: be.search_keys(cb, cq, c.k, c.metric, id_offset=c.id_offset, one_pass=c.one_pass, stats=stats, **kw))
    if c.scaled:
        # the image holds lattice x 2^-9 x 2^exp: the reference of THOSE rows is the lattice's with every score x 2^(2 (exp - 9))
        assert cb.exp != 0 and cq.exp == cb.exp
        D, I = _topk_ref(c)
        up = np.float32(2.0 ** (2 * (cb.exp - 9)))
        want = _keys_of(D[:, :c.k] * up, I[:, :c.k], c.metric, c.id_offset)
        Dd, Id = be.keys_to_result(keys, c.metric, score_exp=be.score_exp_of(cb, cq))
        assert np.array_equal(_np(Id), I[tile][:, :c.k])
        assert np.array_equal(_np(Dd), (D[:, :c.k] * np.float32(2.0 ** -18))[tile])  # the caller's units, exactly
    _assert_keys(_u64(keys), want[tile], c.name)
    if c.one_pass and t is not None:
        assert stats.get("queries") == c.nq, stats  # the certified route ran ("uncertified" may be large under ties: not asserted)
    return dict(kernel=t and t["kernel"], launches=t and t["launches"], calls=t and t["calls"], stats=stats)


def run_shards(be):
    """The seeded list case cut into uneven shards - one of 200 rows, one empty, two ragged -, searched with the pooled sample
    scores of all shards and merged: the keys of the whole corpus."""
    import torch

    c = SHARD_CASE
    xb, q, tile = topk_data(c)
    cq = _pack(be, q[tile], c.qpack)
    shards = [_pack(be, xb[lo:hi], c.bpack) for lo, hi in SHARD_BOUNDS]
    pooled = torch.cat([be.seed_scores(sh, cq, c.metric, SHARD_TILES) for sh in shards])
    parts = torch.stack([be.search_keys(sh, cq, c.k, c.metric, id_offset=lo, seed_scores=pooled) for sh, (lo, _) in zip(shards, SHARD_BOUNDS)])
    _assert_keys(_u64(be.merge_keys(parts)), topk_ref_keys(c)[tile], "shards")


# ---- threshold-join cases ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Join:
    name: str
    nq: int
    nb: int
    d: int
    metric: int
    pack: int = F16
    q_row0: int = -1            # >= 0: a self-join - the queries are rows [q_row0, q_row0 + nq) of the corpus
    plan: tuple = ()            # the launches ``range_plan`` must give: (kernel, c0, cn, r0, rn) each
    kernel: str = TILE          # the last timed launch's kernel
    stride: int = 1             # > 1: the phases 0 .. stride - 1 partition the result
    capacity: int = 1 << 22
    scaled: bool = False


JOIN_BIG = dict(nq=2048, nb=33917, d=256)
JOIN_SMALL = dict(nq=700, nb=3001, d=96)
JOIN_CASES = [
    Join("rj-plain-I", **JOIN_BIG, metric=IP, plan=((RANGE_RJ, 0, 2048, 0, 33888), (RANGE_LIST, 0, 2048, 33888, 29))),
    Join("rj-self-I", **JOIN_BIG, metric=IP, q_row0=1000, plan=((RANGE_RJ, 0, 2048, 992, 32896), (RANGE_LIST, 0, 2048, 33888, 29))),
    Join("list-plain-L", **JOIN_BIG, metric=L2, plan=((RANGE_LIST, 0, 2048, 0, 33917),)),
    Join("list-self-L", **JOIN_BIG, metric=L2, q_row0=1000, plan=((RANGE_LIST, 0, 2048, 0, 33917),)),
    Join("small-self-S-I", **JOIN_SMALL, metric=IP, pack=SPLIT, q_row0=0, plan=((RANGE_LIST, 0, 700, 0, 3001),)),
    Join("small-self-S-L", **JOIN_SMALL, metric=L2, pack=SPLIT, q_row0=0, plan=((RANGE_LIST, 0, 700, 0, 3001),)),
    Join("small-stride3-I", **JOIN_SMALL, metric=IP, stride=3, plan=((RANGE_LIST, 0, 700, 0, 3001),)),
    Join("rj-capacity16-I", **JOIN_BIG, metric=IP, capacity=16, plan=((RANGE_RJ, 0, 2048, 0, 33888), (RANGE_LIST, 0, 2048, 33888, 29))),
    Join("small-scaled-S-I", **JOIN_SMALL, metric=IP, pack=SPLIT, q_row0=0, scaled=True, plan=((RANGE_LIST, 0, 700, 0, 3001),)),
]


@functools.lru_cache(maxsize=4)
def _join_arrays(nq, nb, d, q_row0):
    rng = np.random.default_rng(500 + nb)
    fl = flavour(d, False)
    xb = lattice(BASE_ROWS, d, 31, **fl)[rng.integers(0, BASE_ROWS, nb)] if nb >= LONG_CORPUS else lattice(nb, d, 31, **fl)
    if q_row0 >= 0:
        return xb, xb[q_row0:q_row0 + nq]
    xq = lattice(nq, d, 37, **fl)
    xq[::2] = xb[rng.integers(0, nb, len(xq[::2]))]
    return xb, xq


@functools.lru_cache(maxsize=2)
def join_reference(nq, nb, d, metric, q_row0):
    """(S float32 [nq, nb] with -inf where a self-join keeps no pair, thr, pairs above, pairs at thr).  thr: the smallest attained
    score with at most 200 000 pairs strictly above it.  (float32 BLAS: exact on these inputs, which ``join_guards`` checks.)"""
    xb, xq = _join_arrays(nq, nb, d, q_row0)
    S = xq @ xb.T
    if metric == L2:
        S = -((xq * xq).sum(1)[:, None] + (xb * xb).sum(1)[None, :] - np.float32(2.0) * S)
    if q_row0 >= 0:
        S[np.arange(nb)[None, :] <= (q_row0 + np.arange(nq))[:, None]] = -np.inf
    units = np.rint(S[np.isfinite(S)] / np.float32(STEP * STEP)).astype(np.int64)  # scores are whole units: count them per value
    lo = int(units.min())
    counts = np.bincount(units - lo)
    above = np.concatenate([np.cumsum(counts[::-1])[::-1][1:], [0]])  # pairs strictly above each value
    i = int(np.argmax((above <= 200_000) & (counts > 0)))
    return S, float((lo + i) * STEP * STEP), int(above[i]), int(counts[i])


def join_guards(c):
    """Guards 1 and 2 of a join case -> (thr, pairs above, pairs at thr)"""
    xb, xq = _join_arrays(c.nq, c.nb, c.d, c.q_row0)
    guard_exact(np.unique(xb, axis=0), np.unique(xq, axis=0), c.metric, STEP * STEP)
    S, thr, above, at = join_reference(c.nq, c.nb, c.d, c.metric, c.q_row0)
    assert 1000 <= above <= 200_000 and at >= 0.1 * above, (c.name, thr, above, at)
    assert np.float32(thr) == thr and np.float32(thr * SCALED_DOWN ** 2) == thr * SCALED_DOWN ** 2
    return thr, above, at


def join_planned(c):
    a = plan_native.ask([f"range_plan {c.nq} {c.nb} {c.q_row0} 0 {c.d} {c.pack} {c.metric} {c.stride}"])[0]
    return tuple(tuple(a[i:i + 5]) for i in range(0, len(a), 5))


def _assert_pairs(got, S, thr, what, keep=None):
    """THE assertions of a join leg: the set of (q, j) is exactly {S > thr}, no pair twice, out_s is the reference's, bit for bit."""
    q, j, s = (_np(t) for t in got)
    want = S > np.float32(thr)
    if keep is not None:
        want = want & keep[:, None]
    wq, wj = np.nonzero(want)  # row-major: sorted by (q, j)
    order = np.lexsort((j, q))
    q, j, s = q[order], j[order], s[order]
    assert len(q) == len(wq), f"{what}: {len(q)} pairs, the reference has {len(wq)} above {thr}"
    assert np.array_equal(q, wq) and np.array_equal(j, wj), f"{what}: the pair set differs"  # (equal sorted lists: no pair twice)
    assert np.array_equal(s, S[wq, wj]), f"{what}: {int((s != S[wq, wj]).sum())} scores differ"
    return len(q)


def run_join(be, c):
    """-> dict(kernel, launches, pairs)"""
    xb, xq = _join_arrays(c.nq, c.nb, c.d, c.q_row0)
    S, thr, _, _ = join_reference(c.nq, c.nb, c.d, c.metric, c.q_row0)
    scale = np.float32(SCALED_DOWN if c.scaled else 1.0)
    cb = _pack(be, xb * scale, c.pack, exp="auto" if c.scaled else 0)
    cq = be.slice_rows(cb, c.q_row0, c.q_row0 + c.nq) if c.q_row0 >= 0 else _pack(be, xq * scale, c.pack, exp=cb.exp)
    if c.scaled:  # the threshold in the caller's units lies exactly on an attained value; out_s comes back in those units
        assert cb.exp != 0
        S, thr = S * np.float32(SCALED_DOWN ** 2), thr * SCALED_DOWN ** 2
    kw = dict(q_row0=c.q_row0, capacity=c.capacity)
    if c.stride > 1:
        n = 0
        for phase in range(c.stride):  # each phase exactly its 256-query tiles: together they partition the result
            got = be.range_join(cb, cq, thr, c.metric, stride=c.stride, phase=phase, **kw)
            n += _assert_pairs(got, S, thr, f"{c.name} phase {phase}", keep=(np.arange(c.nq) // 256) % c.stride == phase)
        assert n == int((S > np.float32(thr)).sum())
        return dict(kernel=None, launches=None, pairs=n)
    got, t = _timed(be, lambda: be.range_join(cb, cq, thr, c.metric, **kw))
    n = _assert_pairs(got, S, thr, c.name)
    return dict(kernel=t and t["kernel"], launches=t and t["launches"], pairs=n)


# ---- the other exact legs ----------------------------------------------------------------------------------------------------
SCORES_SHAPE = (150, 777, 200)  # nq, nb, d
SCORES_PACKS = ((F16, F16), (SPLIT, SPLIT), (F16, SPLIT), (SPLIT, F16))
RANK_SHAPE = (7, 10001, 64)
NEAREST_SHAPES = ((3000, 3001, 96), (3000, 40000, 96))  # nq, nb, d: lvs_nearest3 (nb <= 16 384) and lvs_nearest_hi
NEAREST_PACKS = ((F16, F16), (SPLIT, SPLIT), (F16, SPLIT))


@functools.lru_cache(maxsize=4)
def plain_arrays(nq, nb, d):
    rng = np.random.default_rng(900 + nb)
    fl = flavour(d, False)
    base = min(BASE_ROWS, nb // 3)  # every row about three times: a query ON a row still has tied winners
    xb = lattice(base, d, 41, **fl)[rng.integers(0, base, nb)]
    xq = lattice(nq, d, 43, **fl)
    xq[::2] = xb[rng.integers(0, nb, len(xq[::2]))]
    return xb, xq


def _bits(x):
    """float32 bit patterns with -0 folded onto +0, as the oracle folds it"""
    return (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)


def run_scores(be, bpack, qpack, metric):
    """be.scores: the reference matrix, bit for bit (squared L2 is -d^2)."""
    nq, nb, d = SCORES_SHAPE
    xb, xq = plain_arrays(nq, nb, d)
    got = _np(be.scores(_pack(be, xb, bpack), _pack(be, xq, qpack), metric))
    want = guard_exact(xb, xq, metric, STEP * STEP).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


def run_rank_all(be, metric):
    """be.rank_all (K = N beyond LVS_MAX_K): pack_keys of the fully sorted rows."""
    nq, nb, d = RANK_SHAPE
    xb, xq = plain_arrays(nq, nb, d)
    guard_exact(xb, xq, metric, STEP * STEP)
    keys = be.rank_all(_pack(be, xb, F16), _pack(be, xq, F16), metric, id_offset=5)
    _assert_keys(_u64(keys), ref_keys(xb, xq, nb, metric, id_offset=5), "rank_all")


@functools.lru_cache(maxsize=2)
def _nearest_ref(nq, nb, d):
    xb, xq = plain_arrays(nq, nb, d)
    return oracle.flat_search(xb, xq, 2, L2)


def nearest_guards(nq, nb, d):
    """-> the share of queries whose best two reference scores are equal (the winner is then the lower id)"""
    xb, xq = plain_arrays(nq, nb, d)
    guard_exact(np.unique(xb, axis=0), xq, L2, STEP * STEP)
    D, _ = _nearest_ref(nq, nb, d)
    tied = float((D[:, 0] == D[:, 1]).mean())
    assert tied >= 0.5, tied
    return tied


def run_nearest(be, nq, nb, d, bpack, qpack):
    """be.nearest under squared L2: the k = 1 reference - the lowest id among the tied winners - and its exact score.  -> stats"""
    xb, xq = plain_arrays(nq, nb, d)
    D, I = _nearest_ref(nq, nb, d)
    want = _keys_of(D[:, :1], I[:, :1], L2, 3)
    cb, cq = _pack(be, xb, bpack), _pack(be, xq, qpack)
    stats = {}
    _assert_keys(_u64(be.nearest(cb, cq, L2, id_offset=3, stats=stats, exact_scores=True)), want, "nearest")
    # exact_scores=False: the ids are exact either way; a certified query keeps its one-pass score, which include/lotus_hip.h
    # documents as perturbed - "The kernel carries a score's position in the low six mantissa bits of u = q.y (inner product)
    # or u = 2 q.y - |y|^2 (L2) while it runs, so the reported winner and runner-up scores are each perturbed by less than
    # 2^-17 |u|".  |u| < 2^8 units here, so the perturbation is below 2^-9 of a unit: the score ROUNDED TO THE LATTICE UNIT is
    # the reference's.  This is that rounding, not a tolerance.
    Dg, Ig = (_np(t) for t in be.keys_to_result(be.nearest(cb, cq, L2, id_offset=3, exact_scores=False), L2))
    unit = np.float32(STEP * STEP)
    assert np.array_equal(Ig, I[:, :1] + 3)
    assert np.array_equal(np.rint(Dg / unit) * unit, D[:, :1])
    return stats
