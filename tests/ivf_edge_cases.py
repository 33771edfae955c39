"""Planted inputs for the three IVF list scans (lvs_ivf_scan_kernel, lvs_ivf_sq8_scan_kernel, lvs_ivf_pq_scan_kernel) and
the one driver that runs them through a backend.  No test lives here: test_ivf_edges_host.py runs every case through
``PqOracleBackend`` (is the case what it claims to be?), test_gpu_ivf_edges.py through ``HipBackend``.

A case is plain numpy data - rows, queries, centroids, optionally explicit lists (``ivf_build(..., offsets=, rows=)``; row
numbers ascend inside a list, as the builder guarantees) and the codec inputs (SQ8 training ids; PQ codebooks are sampled
from the residuals, a quantizer whose training is not the subject).  ``run_case`` works in the image's STORED scale (values
x 2^exp) and reports scores in the caller's units, as ``keys_to_result(..., score_exp=)`` does.

Bars: 1e-5 on scores and a tie gap of 2e-5 wherever a case does not say otherwise (the scaled operands of family 7a scale
both with s^2).  Outside the exact-tie cases at most 15 % of the reference's slots may lie within the tie gap of a
neighbour (``NEAR_TIE_CAP``): compare_topk excuses id mismatches there, so a case made of near ties checks no ids."""
from __future__ import annotations

import functools
import heapq
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

import oracle
import plan_native
import synth
from ivf_oracle_backend import ivf_reference
from ivf_pq_oracle_backend import pq_decode, pq_reference
from ivf_sq8_oracle_backend import list_of_rows, sq8_decode, sq8_reference
from lotus_amd import _capi

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
FLAT, SQ8, PQ = "Flat", "SQ8", "PQ"
SCAN_KERNEL = {FLAT: "lvs_ivf_scan_kernel", SQ8: "lvs_ivf_sq8_scan_kernel", PQ: "lvs_ivf_pq_scan_kernel"}
NEAR_TIE_CAP = 0.15
FLT_MAX = float(np.float32(3.4028234663852886e38))
# scratch of one search call (beyond it the library halves its chunk of queries) and the largest chunk: lvs_ivf_plan.h's own
WS_BUDGET, CHUNK_MAX = plan_native.ivf_limits()


@dataclass
class Case:
    xb: np.ndarray          # float32 [n, d], the caller's units
    xq: np.ndarray          # float32 [nq, d]
    centroids: np.ndarray   # float32 [nlist, d]
    metric: int
    pack: int
    k: int
    nprobe: int
    offsets: Optional[np.ndarray] = None   # planted lists; None: ivf_build's own assignment
    rows: Optional[np.ndarray] = None
    train_ids: Optional[np.ndarray] = None  # SQ8: rows the ranges are taken over (None: all)
    M: int = 8                              # PQ
    ksub: int = 256
    exp: object = 0                         # pack exponent of the corpus (the queries take the corpus')
    bar: float = 1e-5
    tie_gap: float = 2e-5
    tie_cap: bool = True                    # False: an exact-tie case, checked by exact equality in `post`
    ignore_exact_ties: bool = False         # decoded duplicates: equal scores do not count towards the near-tie share
    pick: Optional[np.ndarray] = None       # the queries checked (None: all)
    host_queries: Optional[int] = None      # the host test may check only the first so many of `pick`
    pre: Optional[Callable] = None          # pre(case, mode, res): asserts about the inputs and the reference alone
    post: Optional[Callable] = None         # post(case, mode, res): the case's own assertions on the device result
    bar_fn: Optional[Callable] = None       # bar_fn(case, res) -> bar measured on the case's own pairs (family 7e)


# ---- the driver ------------------------------------------------------------------------------------------------------------
def _inp(x, pack):
    return x.astype(np.float16) if pack == F16 else np.ascontiguousarray(x, np.float32)


def _np(t):
    return t.cpu().numpy()


def codebooks(h, M, ksub, seed):
    """Codebooks of ksub sampled residuals per subspace (stored scale)."""
    rng = np.random.default_rng(seed)
    r = h["x"] - h["c"][h["where"]]
    n, d = r.shape
    dsub = d // M
    return np.stack([r[rng.choice(n, ksub, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)


def grouped_reference(xref, xq, k, metric, off, rows, probe):
    """The rule of ivf_reference / sq8_reference - the exact float64 top k over the rows of the probed lists, ties to the
    lower row number - for many queries that share few probe sets: one matrix product per set instead of one gather per
    query.  (D float64, I int64), padded like the oracle."""
    nq = xq.shape[0]
    D = np.full((nq, k), FLT_MAX if metric == L2 else -FLT_MAX, np.float64)
    I = np.full((nq, k), -1, np.int64)
    groups = {}
    for q in range(nq):
        groups.setdefault(tuple(sorted(int(l) for l in probe[q] if l >= 0)), []).append(q)
    for ls, qs in groups.items():
        ids = np.sort(np.concatenate([rows[off[l]:off[l + 1]] for l in ls] + [np.zeros(0, np.uint32)]).astype(np.int64))
        if ids.size == 0:
            continue
        X = np.asarray(xref[ids], np.float64)
        m = min(k, ids.size)
        step = max(1, (64 << 20) // (8 * ids.size))
        for c0 in range(0, len(qs), step):
            qc = np.asarray(qs[c0:c0 + step])
            Q = np.asarray(xq[qc], np.float64)
            if metric == L2:
                S = np.stack([((X - Q[j]) ** 2).sum(axis=1) for j in range(len(qc))], axis=1)
                better = -S
            else:
                S = X @ Q.T
                better = S
            for j, q in enumerate(qc):
                b = better[:, j]
                kth = np.partition(b, ids.size - m)[ids.size - m]
                cand = np.nonzero(b >= kth)[0]
                order = cand[np.lexsort((ids[cand], -b[cand]))[:m]]
                D[q, :m] = S[order, j]
                I[q, :m] = ids[order]
    return D, I


def near_tie_share(D_ref, I_ref, tie_gap, ignore_exact=False):
    """Share of the reference's slots within tie_gap of a neighbouring slot: where compare_topk excuses an id mismatch."""
    D, valid = np.asarray(D_ref, np.float64), np.asarray(I_ref) >= 0
    if not valid.any() or D.shape[1] < 2:
        return 0.0
    gap = np.abs(np.diff(D, axis=1))
    near = (gap <= tie_gap) & valid[:, 1:] & valid[:, :-1]
    if ignore_exact:
        near &= gap > 0
    slot = np.zeros(valid.shape, bool)
    slot[:, 1:] |= near
    slot[:, :-1] |= near
    return float(slot[valid].mean())


def rescoring_args(xref, xq, metric, off, rows, probe, scale=1.0):
    """(score_fn, allowed_ids_per_query) for synth.check_ids_by_rescoring: the float64 score of given rows of ``xref`` (the
    stored rows for Flat, the decoded rows for SQ8 and PQ) against query q, and the rows of the lists q probed."""
    xq = np.asarray(xq)
    rows = np.asarray(rows, np.uint32)

    def score_fn(q, ids):
        X, qv = np.asarray(xref[ids], np.float64), np.asarray(xq[q], np.float64)
        return (((X - qv) ** 2).sum(axis=1) if metric == L2 else X @ qv) * scale

    nlist = len(off) - 1
    if probe.shape[1] == nlist:  # every list probed: every row is allowed
        allowed = [rows] * xq.shape[0]
    else:
        allowed = [np.concatenate([rows[off[l]:off[l + 1]] for l in p if l >= 0] + [np.zeros(0, np.uint32)]) for p in probe]
    return score_fn, allowed


def fits(be, case, mode, d=None, k=None, M=None):
    d = case.xb.shape[1] if d is None else d
    k = case.k if k is None else k
    if mode == FLAT:
        return be.ivf_fits(d, k, case.pack)
    if mode == SQ8:
        return be.ivf_sq8_fits(d, k, case.pack)
    return be.ivf_pq_fits(d, case.M if M is None else M, k, case.pack)


def run_case(be, case, mode, pick=None, only_picked=False):
    """Build the index of ``case`` on ``be``, search it with ``mode``'s scan and compute the float64 reference over the
    lists the backend probed.  ``pick``: the queries to check (default: the case's own sample, else all);
    ``only_picked``: search no other queries either (the CPU backend computes every query it is given).  Returns a dict:
    D, I, probe (of the checked queries), D_ref, I_ref, Dp, Ip (the reference's coarse search), the host copy ``h`` of the
    index, ``xref`` (stored or decoded rows), ``kernel`` (the dominant kernel of the search, None without timing)."""
    nq = case.xq.shape[0]
    pick = (np.arange(nq) if case.pick is None else case.pick) if pick is None else np.asarray(pick)
    xq = case.xq
    if only_picked:
        xq, pick = xq[pick], np.arange(len(pick))
    packed = be.pack(_inp(case.xb, case.pack), case.pack, exp=case.exp)
    qp = be.pack(_inp(xq, case.pack), case.pack, exp=int(packed.exp))
    lists = be.ivf_build(packed, case.centroids, case.metric, offsets=case.offsets, rows=case.rows)
    be.synchronize()
    off, rows = _np(lists.offsets), _np(lists.rows).view(np.uint32)
    h = dict(off=off, rows=rows, where=list_of_rows(off, rows, packed.n), c=_np(be.unpack(lists.centroids, raw=True)),
             x=_np(be.unpack(packed, raw=True)), q=_np(be.unpack(qp, raw=True)), exp=int(packed.exp))
    lrows = rows.astype(np.int64)
    timed = hasattr(be, "timing_enable")
    k, metric, nprobe = case.k, case.metric, case.nprobe

    def search(fn, *head):
        if timed:
            be.timing_enable(True)
        try:
            keys, probe = fn(*head, qp, k, metric, nprobe, want_probe=True)
            be.synchronize()
            t = be.timing_read_full() if timed else None
        finally:
            if timed:
                be.timing_enable(False)
        return keys, probe, t

    if mode == FLAT:
        keys, probe, t = search(be.ivf_search, packed, lists)
        xref = h["x"]
    elif mode == SQ8:
        train = np.arange(packed.n) if case.train_ids is None else case.train_ids
        vmin, vdiff = be.ivf_sq8_train(packed, lists, train)
        sq = be.ivf_sq8_encode(packed, lists, vmin, vdiff)
        be.synchronize()
        codes = np.empty((packed.n, packed.d), np.uint8)
        codes[lrows] = _np(sq.codes)[:, :packed.d]
        h.update(vmin=_np(sq.vmin), vdiff=_np(sq.vdiff), codes=codes, csq=_np(sq.centroids))
        keys, probe, t = search(be.ivf_sq8_search, packed, lists, sq)
        xref = sq8_decode(h["csq"], h["where"], h["vmin"], h["vdiff"], codes)
    else:
        books = codebooks(h, case.M, case.ksub, seed=case.M + case.ksub)
        pq = be.ivf_pq_encode(packed, lists, books)
        be.synchronize()
        codes = np.empty((packed.n, pq.M), np.uint8)
        codes[lrows] = _np(pq.codes)[:, :pq.M]
        h.update(books=books, codes=codes, cpq=_np(pq.centroids))
        keys, probe, t = search(be.ivf_pq_search, packed, lists, pq)
        xref = pq_decode(h["cpq"], h["where"], books, codes)
    score_exp = be.score_exp_of(packed, qp)
    D, I = be.keys_to_result(keys, metric, score_exp=score_exp)
    be.synchronize()
    scale = 2.0 ** -score_exp

    q_s, pr = h["q"][pick], _np(probe)[pick]
    Dp, Ip = oracle.flat_search(h["c"], q_s, nprobe, metric)
    if len(pick) * packed.n > 400000:  # the per-query references gather every probed row once per query
        D_ref, I_ref = grouped_reference(xref, q_s, k, metric, off, rows, pr)
    elif mode == FLAT:
        D_ref, I_ref = ivf_reference(xref, q_s, k, metric, h["c"], off, rows, pr)
    else:
        D_ref, I_ref = (sq8_reference if mode == SQ8 else pq_reference)(xref, q_s, k, metric, off, rows, pr)
    res = dict(D=_np(D)[pick], I=_np(I)[pick], probe=pr, D_ref=np.asarray(D_ref, np.float64) * scale, I_ref=I_ref,
               Dp=np.asarray(Dp, np.float64) * scale, Ip=Ip, h=h, xref=xref, q=q_s, scale=scale, pick=pick,
               kernel=None if t is None else t["kernel"])
    res["bar"] = case.bar if case.bar_fn is None else case.bar_fn(case, res)
    return res


def preconditions(be, case, mode, res):
    """Asserts about the inputs and the reference alone: the case is what it claims to be and stays inside every cap."""
    n, d = case.xb.shape
    nlist = case.centroids.shape[0]
    assert 1 <= case.k <= 56 and 1 <= case.nprobe <= min(nlist, 2048)
    assert fits(be, case, mode), f"{mode} refuses d={d} k={case.k}"
    h = res["h"]
    assert h["off"][0] == 0 and h["off"][-1] == n and len(h["off"]) == nlist + 1
    assert np.array_equal(np.sort(h["rows"].astype(np.int64)), np.arange(n))
    assert ((res["I_ref"] >= -1) & (res["I_ref"] < n)).all()
    if case.tie_cap:
        share = near_tie_share(res["D_ref"], res["I_ref"], case.tie_gap, case.ignore_exact_ties)
        assert share <= NEAR_TIE_CAP, f"near-tie share {share:.3f}: take another seed or a smaller k"
    if case.pre is not None:
        case.pre(case, mode, res)


def check_result(case, mode, res):
    """The assertions every case holds a backend's result to (the kernel's name is asserted by the GPU test)."""
    bar = res["bar"]
    err, hard, _ = synth.compare_topk(res["D_ref"], res["I_ref"], res["D"], res["I"], atol=bar, tie_gap=case.tie_gap)
    assert err <= bar and hard == 0, (err, hard)
    assert np.array_equal(res["I"] == -1, res["I_ref"] == -1)
    probe, nlist = res["probe"], case.centroids.shape[0]
    assert ((probe >= 0) & (probe < nlist)).all() and all(len(set(p.tolist())) == len(p) for p in probe)
    assert synth.compare_topk(res["Dp"], res["Ip"], res["Dp"], probe, tie_gap=case.tie_gap)[1] == 0
    h = res["h"]
    score_fn, allowed = rescoring_args(res["xref"], res["q"], case.metric, h["off"], h["rows"], probe, res["scale"])
    synth.check_ids_by_rescoring(score_fn, res["D"], res["I"], allowed, bar)
    if case.post is not None:
        case.post(case, mode, res)


def chunk_boundary_sample(nq, seed, chunks=()):
    """The queries checked of a search that runs in chunks: 300 random ones, plus every multiple of the chunk the planner
    reports for each mode the case runs in (``chunks``: ``plan_native.ivf_chunk`` answers) with its two neighbours.  Each
    reported chunk is one of c, ceil(c / 2), ceil(c / 4), ... for c = min(nq, CHUNK_MAX) and at least 128 - any chunk of up to
    255 queries fits the budget at these shapes (test_budget_cases_halve_the_chunk) -, and the multiples of the other sizes
    of that sequence down to 128 stay in the sample: it does not shrink when a layout change moves the chunk."""
    pick = set(np.random.default_rng(seed).choice(nq, min(nq, 300), replace=False).tolist()) | {0, nq - 1}
    halvings = [min(nq, CHUNK_MAX)]
    while halvings[-1] > 1:
        halvings.append((halvings[-1] + 1) // 2)
    for chunk, tail, _ in chunks:
        assert chunk in halvings and chunk >= 128 and tail == nq % chunk, (chunk, tail, halvings)
    for c in sorted({c for c in halvings if c >= 128} | {ch[0] for ch in chunks}):
        for b in range(c, nq + 1, c):
            pick |= {b - 1, b, b + 1}
    return np.array(sorted(p for p in pick if 0 <= p < nq))


# ---- the data --------------------------------------------------------------------------------------------------------------
def deal(lengths, seed):
    """(offsets, rows): lists of the given lengths over sum(lengths) rows, dealt irrespective of the rows' position in the
    corpus; row numbers ascend inside a list."""
    n = int(sum(lengths))
    perm = np.random.default_rng(seed).permutation(n)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    rows = np.concatenate([np.sort(perm[off[l]:off[l + 1]]) for l in range(len(lengths))]).astype(np.uint32)
    return off, rows


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _gauss(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _sampled_centroids(xb, nlist, seed):
    return xb[np.random.default_rng(seed).choice(xb.shape[0], nlist, replace=False)].copy()


def _better(case, D):
    return -D if case.metric == L2 else D


# 1. planted lengths: around the scans' block sizes (Flat 32 / 128, SQ8 16 / 64, PQ 64 / 512), two empty lists, one long list
PLANTED = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 0, 20000]


def planted(metric, pack, own):
    """own: every list's centroid is a query and nprobe = 1 - query l probes list l and must get exactly that list's top
    56, with max(0, 56 - len) slots at -1.  Otherwise 40 queries over all lists (nprobe = nlist)."""
    d, nlist = 64, len(PLANTED)
    xb = synth.corpus(int(sum(PLANTED)), d, seed=101)
    c = synth.corpus(nlist, d, seed=102)
    off, rows = deal(PLANTED, 103)
    xq = c.copy() if own else synth.queries(xb, 40, seed=104)[0]

    def pre(case, mode, res):
        assert np.array_equal(np.diff(res["h"]["off"]), PLANTED)
        if own:
            assert np.array_equal(res["Ip"][:, 0], np.arange(nlist)) and np.array_equal(res["probe"][:, 0], res["Ip"][:, 0])
            assert np.array_equal((res["I_ref"] == -1).sum(axis=1), np.maximum(0, 56 - np.array(PLANTED)))

    def post(case, mode, res):
        if own:
            assert np.array_equal((res["I"] == -1).sum(axis=1), np.maximum(0, 56 - np.array(PLANTED)))
            for l in range(nlist):
                got = res["I"][l][res["I"][l] >= 0]
                assert np.isin(got, rows[off[l]:off[l + 1]]).all()

    return Case(xb, xq, c, metric, pack, 56, 1 if own else nlist, offsets=off, rows=rows, ignore_exact_ties=True, pre=pre,
                post=post)


# 2. a hot list: 5 000 queries share their best centroid, whose list holds half of the rows - hundreds of work items on one list
def hot_list(metric, pack, last, k):
    n, d, nlist, nq = 40000, 64, 8, 5000
    hot = nlist - 1 if last else 0
    xb = synth.corpus(n, d, seed=201)
    c = synth.corpus(nlist, d, seed=202)
    lengths = [2857] * nlist
    lengths[hot] = 20000
    lengths[1 if hot == 0 else 0] += n - sum(lengths)
    off, rows = deal(lengths, 203)
    xq = _unit(c[hot] + 0.35 * _unit(_gauss(nq, d, 204)))

    def pre(case, mode, res):
        assert (res["Ip"][:, 0] == hot).all() and (res["probe"][:, 0] == hot).all()
        assert res["h"]["off"][hot + 1] - res["h"]["off"][hot] == 20000

    return Case(xb, xq, c, metric, pack, k, 2, offsets=off, rows=rows, ignore_exact_ties=True, host_queries=150, pre=pre)


# 3. insertion pressure
def _ramp(metric, pack, rising):
    """Rows a_i u + noise orthogonal to u in one list, a_i rising (every row enters the sorted list while all waves of the
    workgroup contend for its lock) or falling with the row number; 32 queries near u."""
    n, d, extra = 1536, 64, 64
    rng = np.random.default_rng(301)
    u = _unit(rng.standard_normal((1, d)))[0]
    g = rng.standard_normal((n, d)).astype(np.float32)
    g -= np.outer(g @ u, u)
    a = 0.05 + 0.9 * np.arange(n, dtype=np.float32) / n
    if not rising:
        a = a[::-1]
    xb = np.concatenate([a[:, None] * u + 0.004 * _unit(g), 0.1 * synth.corpus(extra, d, seed=302)]).astype(np.float32)
    c = np.stack([0.5 * u, -0.5 * u]).astype(np.float32)
    off = np.array([0, n, n + extra], np.int64)
    rows = np.arange(n + extra, dtype=np.uint32)
    xq = np.float32(1.5) * _unit(u + 0.05 * _unit(_gauss(32, d, 303)))  # |q| = 1.5: the L2 score keeps its slope in a_i

    def pre(case, mode, res):
        if not rising:
            return
        for q in range(0, 32, 8):  # along list order at least 90 % of the rows beat the running k-th best
            s = _better(case, _scores(case, res, q, np.arange(n)))
            heap, entered = [], 0
            for v in s:
                if len(heap) < case.k:
                    heapq.heappush(heap, v)
                    entered += 1
                elif v > heap[0]:
                    heapq.heapreplace(heap, v)
                    entered += 1
            assert entered >= 0.9 * n, (q, entered)

    return Case(xb, xq, c, metric, pack, 56, 2, offsets=off, rows=rows, pre=pre)


def _scores(case, res, q, ids):
    X, qv = np.asarray(res["xref"][ids], np.float64), np.asarray(res["q"][q], np.float64)
    return ((X - qv) ** 2).sum(axis=1) if case.metric == L2 else X @ qv


def tied_in_one_list(metric, pack):
    """3 000 identical rows interleaved with distinct rows inside one list: their codes, and so their scores, are equal,
    and the 56 smallest of their ids come back with bit-identical scores."""
    n, d, extra = 6000, 64, 64
    xb = 0.5 * synth.corpus(n + extra, d, seed=311)
    z = synth.corpus(1, d, seed=312)[0]
    tied = np.arange(0, n, 2)
    xb[tied] = z
    c = np.stack([0.5 * z, -0.5 * z]).astype(np.float32)
    off = np.array([0, n, n + extra], np.int64)
    rows = np.arange(n + extra, dtype=np.uint32)
    xq = _unit(z + 0.05 * _unit(_gauss(8, d, 313)))

    def pre(case, mode, res):
        assert (res["xref"][tied] == res["xref"][tied[0]]).all()
        assert np.array_equal(res["I_ref"], np.tile(tied[:56], (8, 1))) and (res["D_ref"] == res["D_ref"][:, :1]).all()

    def post(case, mode, res):
        assert np.array_equal(res["I"], np.tile(tied[:56], (8, 1)))
        assert (res["D"] == res["D"][:, :1]).all()

    return Case(xb, xq, c, metric, pack, 56, 2, offsets=off, rows=rows, tie_cap=False, pre=pre, post=post)


def tied_across_lists():
    """Flat only: 600 rows that score exactly 0.5 against q = e0, spread over the lists by ivf_build's own assignment."""
    d, n, nlist = 64, 6000, 32
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 0] = 0.0
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= 0.75
    tied = np.sort(rng.choice(n, 600, replace=False))
    x[:, 0] = 0.25
    x[tied, 0] = 0.5
    x = x.astype(np.float16).astype(np.float32)
    q = np.zeros((1, d), np.float32)
    q[0, 0] = 1.0

    def pre(case, mode, res):
        assert len(set(res["h"]["where"][tied].tolist())) >= 8
        assert np.array_equal(res["I_ref"][0], tied[:56]) and (res["D_ref"] == 0.5).all()

    def post(case, mode, res):
        assert np.array_equal(res["I"][0], tied[:56]) and (res["D"] == np.float32(0.5)).all()

    return Case(x, q, _sampled_centroids(x, nlist, 6), IP, F16, 56, nlist, tie_cap=False, pre=pre, post=post)


# 4. wide indexes, built with ivf_build's own assignment
def wide(nlist, nprobe, k, nq, metric, pack, sample=False):
    n, d = 60000, 64
    xb = synth.corpus(n, d, seed=401)
    xq = synth.queries(xb, nq, seed=402 + nq)[0]
    c = _sampled_centroids(xb, nlist, 403 + nlist)
    pick = None
    if sample:  # the case runs in all three modes (Flat and SQ8 share one layout; PQ has its tables and no tiling)
        chunks = [plan_native.ivf_chunk(m, nq, nlist, nprobe, d, k, pack, M=Case.M if m == PQ else 1) for m in (FLAT, SQ8, PQ)]
        pick = chunk_boundary_sample(nq, 404, chunks)

    def pre(case, mode, res):
        if sample:  # the scratch of all queries at once is beyond the budget: the planner halves the chunk
            assert nq * nprobe * k * 8 > WS_BUDGET

    return Case(xb, xq, c, metric, pack, k, nprobe, pick=pick, host_queries=24 if nprobe > 256 else 60, pre=pre)


def wide_pq_tables(metric, pack):
    """PQ at M = 159 and 10 001 queries: the tables (159 KB per query) bound the chunk, halved to an odd size.  The index is
    small (4 000 rows): what is planted here is the number of queries, and the CPU encoder twin is slow at this M."""
    n, d, nq, nlist = 4000, 636, 10001, 40
    xb = synth.corpus(n, d, seed=411)
    xq = synth.queries(xb, nq, seed=412)[0]

    def pre(case, mode, res):
        assert nq * 159 * 256 * 4 > WS_BUDGET

    chunk = plan_native.ivf_chunk(PQ, nq, nlist, 4, d, 56, pack, M=159)
    return Case(xb, xq, _sampled_centroids(xb, nlist, 413), metric, pack, 56, 4, M=159,
                pick=chunk_boundary_sample(nq, 414, [chunk]), host_queries=40, pre=pre)


# 5. k sweep over one fixed index per mode (lvs_ivf_kcap switches at 16 and 32)
KS = [1, 2, 15, 16, 17, 31, 32, 33, 55, 56]


def k_sweep(k, metric, pack):
    xb = synth.corpus(5000, 64, seed=501)
    return Case(xb, synth.queries(xb, 33, seed=502)[0], _sampled_centroids(xb, 16, 503), metric, pack, k, 4)


# 6. widths
def width(d, metric, pack, M=8, ksub=256, k=10):
    n = 2000
    xb = synth.corpus(n, d, seed=601 + d)
    # one subspace, or one or two entries per subspace: many rows of a list decode alike - an exact-tie case, held to the
    # reference's ids (ties to the lower row number) and to bit-identical scores inside every tied group instead of the cap
    tied = M <= 3 or ksub <= 2
    return Case(xb, synth.queries(xb, 9, seed=602)[0], _sampled_centroids(xb, 8, 603), metric, pack, k, 3, M=M, ksub=ksub,
                train_ids=np.arange(0, n, 2), tie_cap=not tied, post=_tied_groups_post if tied else None)


def _tied_groups_post(case, mode, res):
    """Wherever neighbouring reference scores are exactly equal, the device returns the reference's ids (the lower row
    number first, and the lowest ids where the group is cut at rank k) with bit-identical scores."""
    D_ref, I_ref, D, I = res["D_ref"], res["I_ref"], res["D"], res["I"]
    same = (np.diff(D_ref, axis=1) == 0) & (I_ref[:, 1:] >= 0)
    for q, r in zip(*np.nonzero(same)):
        assert I[q, r] == I_ref[q, r] and I[q, r + 1] == I_ref[q, r + 1], (q, r, I[q].tolist(), I_ref[q].tolist())
        assert D[q, r] == D[q, r + 1], (q, r)
    if case.pre is None:  # a case that is exact ties by construction has some
        assert same.any()


def largest_flat_d(be, pack, k=56):
    """The largest d the Flat scan takes at this k and packing (its LDS image holds a tile's queries)."""
    return max(d for d in range(64, 8193, 64) if be.ivf_fits(d, k, pack))


# 7. values
def scaled(s, metric, pack):
    """Both operands x s, packed with exp="auto": bar and tie gap are the project's own, scaled with the operands."""
    xb = synth.corpus(4000, 64, seed=701)
    xq = synth.queries(xb, 33, seed=702)[0]
    c = _sampled_centroids(xb, 16, 703)
    f = np.float32(s)

    def pre(case, mode, res):
        if pack == SPLIT:
            assert res["h"]["exp"] != 0

    return Case(xb * f, xq * f, c * f, metric, pack, 10, 4, exp="auto", bar=1e-5 * s * s, tie_gap=2e-5 * s * s,
                pre=pre)


def common_mean(metric, pack):
    """Rows and queries normalize(0.9 m + 0.45 g) around one unit vector m, as real embeddings: <q, c_l> dwarfs the
    residual term."""
    n, d = 4000, 64
    m = synth.corpus(1, d, seed=711)[0]
    xb = _unit(0.9 * m + 0.45 * synth.corpus(n, d, seed=712))
    xq = _unit(0.9 * m + 0.45 * synth.corpus(33, d, seed=713))
    return Case(xb, xq, _sampled_centroids(xb, 16, 714), metric, pack, 10, 4)


def signs_and_zeros(metric, pack):
    """A zero query, a zero row, and queries -x_j (inner product: every score of the top k is negative, after the zero
    row's exact 0).  Row norms vary, so
    the zero query's L2 scores are distinct; its inner products are all exactly 0 - ties, resolved to the lowest ids."""
    n, d = 4000, 64
    rng = np.random.default_rng(721)
    m = synth.corpus(1, d, seed=720)[0]  # a common mean: every pair of rows has a positive inner product
    xb = _unit(0.9 * m + 0.45 * synth.corpus(n, d, seed=722)) * rng.uniform(0.6, 1.4, (n, 1)).astype(np.float32)
    xb[17] = 0.0
    neg = rng.choice(n, 8, replace=False)
    xq = np.concatenate([np.zeros((1, d), np.float32), -xb[neg], synth.queries(xb, 8, seed=723)[0]])
    xq[1:9] /= np.linalg.norm(xq[1:9], axis=1, keepdims=True)

    def pre(case, mode, res):
        assert not res["q"][0].any() and not res["h"]["x"][17].any()
        if metric == IP:
            # every row scores below zero against -x_j, but for the zero row, which leads every list it is in with exactly 0
            assert (res["D_ref"][1:9][res["I_ref"][1:9] != 17] < 0).all()
            if mode == FLAT:  # (decoded, the zero row is only near zero)
                assert (res["I_ref"][1:9, 0] == 17).all() and (res["D_ref"][1:9, 0] == 0).all()
            assert (res["D_ref"][0] == 0).all() if mode == FLAT else True

    return Case(xb, xq, _sampled_centroids(xb, 16, 724), metric, pack, 10, 16, pre=pre, post=_tied_groups_post)


def degenerate_dims(metric, pack):
    """Five dimensions constant over the corpus (SQ8: vdiff == 0 there) and the PQ subspace [8, 16) identically zero."""
    n, d = 4000, 64
    xb = synth.corpus(n, d, seed=731)
    xb[:, 8:16] = 0.0
    xb[:, [1, 20, 33, 47, 63]] = np.float32(0.0625)
    xq = synth.queries(xb, 33, seed=732)[0]

    def pre(case, mode, res):
        h = res["h"]
        if mode == SQ8:
            assert (h["vdiff"][[1, 20, 33, 47, 63]] == 0).all() and (h["vdiff"][8:16] == 0).all()
            assert int((h["vdiff"] == 0).sum()) == 13
        if mode == PQ:
            assert not h["books"][1].any() and (h["codes"][:, 1] == 0).all()

    return Case(xb, xq, _sampled_centroids(xb, 16, 733), metric, pack, 10, 4, pre=pre)


def sq8_float32_scores(case, res, q, ids):
    """The documented formula of the SQ8 scan, cst + sum_j w_j code_j, restated in float32 numpy for query q and the rows
    ``ids`` of its probed lists (stored scale)."""
    h = res["h"]
    f = np.float32
    b = (h["vdiff"] / f(255)).astype(f)
    a = (h["vmin"] + f(0.5) * b).astype(f)
    qv = res["q"][q].astype(f)
    out = np.empty(len(ids), f)
    for i, r in enumerate(ids):
        cl = h["csq"][h["where"][r]].astype(f)
        code = h["codes"][r].astype(f)
        if case.metric == L2:
            u = qv - cl
            rh = a + b * code
            out[i] = (u * u).sum(dtype=f) - f(2) * ((u * a).sum(dtype=f) + ((u * b) * code).sum(dtype=f)) + (rh * rh).sum(dtype=f)
        else:
            out[i] = ((qv * cl).sum(dtype=f) + (qv * a).sum(dtype=f)) + ((qv * b) * code).sum(dtype=f)
    return out


def sq8_outliers(metric, pack):
    """SQ8 with outliers: 1 % of the rows carry a residual 50 times the typical one in 8 dimensions, so the per-pair
    power-of-two scale of w is set by dimensions most rows do not use.  The bar is measured on the case's own pairs: four
    times the error of the float32 restatement of the formula against the float64 reference (the MFMA sums in another
    order), or 1e-5 max|q| max|xhat| if that is larger.  Measured on the CPU: restatement error 1.29e-6 (IP) / 2.50e-6
    (L2), so four times it is 5.2e-6 / 1.0e-5 and the bar is the second term, 4.07e-5 for both metrics."""
    n, d = 4000, 64
    rng = np.random.default_rng(741)
    xb = synth.corpus(n, d, seed=742)
    out = rng.choice(n, n // 100, replace=False)
    dims = rng.choice(d, 8, replace=False)
    xb[np.ix_(out, dims)] += 50 * 0.18 * rng.choice([-1.0, 1.0], (len(out), 8)).astype(np.float32)
    xq = synth.queries(xb, 17, seed=743)[0]
    c = _sampled_centroids(xb[np.setdiff1d(np.arange(n), out)], 16, 744)

    def bar_fn(case, res):
        worst = 0.0
        for q in range(len(res["q"])):
            ids = res["I_ref"][q][res["I_ref"][q] >= 0]
            exact = _scores(case, res, q, ids)
            worst = max(worst, float(np.abs(sq8_float32_scores(case, res, q, ids).astype(np.float64) - exact).max()))
        floor = 1e-5 * float(np.abs(res["q"]).max()) * float(np.abs(res["xref"]).max())
        res["restated_err"], res["bar_floor"] = worst, floor
        return max(4 * worst, floor)

    return Case(xb, xq, c, metric, pack, 10, 4, bar_fn=bar_fn)


# ---- the table: name -> (builder, modes).  Metrics and packings are spread over the cases, not multiplied out.
def _entry(fn, *args, modes=(FLAT, SQ8, PQ), **kw):
    return functools.partial(fn, *args, **kw), modes


CASES = {
    "planted-all-ip-f16": _entry(planted, IP, F16, False),
    "planted-all-l2-split": _entry(planted, L2, SPLIT, False),
    "planted-own-l2-f16": _entry(planted, L2, F16, True),
    "planted-own-ip-split": _entry(planted, IP, SPLIT, True),
    "hot-first-ip-f16-k10": _entry(hot_list, IP, F16, False, 10),
    "hot-last-l2-split-k56": _entry(hot_list, L2, SPLIT, True, 56),
    "ramp-up-ip-split": _entry(_ramp, IP, SPLIT, True),
    "ramp-up-l2-f16": _entry(_ramp, L2, F16, True),
    "ramp-down-l2-split": _entry(_ramp, L2, SPLIT, False),
    "ramp-down-ip-f16": _entry(_ramp, IP, F16, False),
    "tied-one-list-ip-f16": _entry(tied_in_one_list, IP, F16),
    "tied-one-list-l2-split": _entry(tied_in_one_list, L2, SPLIT),
    "tied-across-lists": _entry(tied_across_lists, modes=(FLAT,)),
    # nlist, nprobe, k, nq
    "wide-1-1": _entry(wide, 1, 1, 10, 3, IP, F16),
    "wide-2-1": _entry(wide, 2, 1, 56, 301, L2, SPLIT),
    "wide-2-2": _entry(wide, 2, 2, 1, 3, L2, F16),
    "wide-4097-16": _entry(wide, 4097, 16, 10, 301, IP, SPLIT),
    "wide-4097-17": _entry(wide, 4097, 17, 56, 3, L2, F16),
    "wide-4097-33": _entry(wide, 4097, 33, 1, 301, IP, F16),
    "wide-4097-257": _entry(wide, 4097, 257, 10, 301, L2, SPLIT),
    "wide-8200-1": _entry(wide, 8200, 1, 56, 301, IP, SPLIT),
    "wide-8200-257": _entry(wide, 8200, 257, 1, 3, L2, F16),
    "wide-8200-2048-nq3": _entry(wide, 8200, 2048, 56, 3, IP, F16),
    "wide-8200-2048-nq301": _entry(wide, 8200, 2048, 10, 301, L2, SPLIT),
    "wide-8200-2048-budget": _entry(wide, 8200, 2048, 56, 3001, IP, F16, sample=True),
    "wide-pq-m159-nq10001": _entry(wide_pq_tables, L2, SPLIT, modes=(PQ,)),
    **{f"k{k}": _entry(k_sweep, k, (IP, L2)[i % 2], (F16, SPLIT)[(i // 2) % 2]) for i, k in enumerate(KS)},
    **{f"flat-d{d}": _entry(width, d, (IP, L2)[i % 2], (SPLIT, F16)[i % 2], modes=(FLAT,)) for i, d in enumerate([8, 72, 100, 1000])},
    "flat-dmax-f16": _entry(width, 2240, L2, F16, k=56, modes=(FLAT,)),
    "flat-dmax-split": _entry(width, 1088, IP, SPLIT, k=56, modes=(FLAT,)),
    **{f"sq8-d{d}": _entry(width, d, (L2, IP)[i % 2], (SPLIT, F16)[i % 2], k=56 if d == 2368 else 10, modes=(SQ8,))
       for i, d in enumerate([8, 100, 1001, 1002, 2368])},
    **{f"pq-d{d}-m{M}": _entry(width, d, (IP, L2)[i % 2], (F16, SPLIT)[i % 2], M=M, k=56 if M == 159 else 10, modes=(PQ,))
       for i, (d, M) in enumerate([(8, 8), (100, 20), (130, 1), (3072, 3), (636, 159)])},
    **{f"pq-ksub{ks}": _entry(width, 64, (L2, IP)[i % 2], (F16, SPLIT)[i % 2], ksub=ks, modes=(PQ,))
       for i, ks in enumerate([1, 2, 255, 256])},
    "scaled-2^-7-ip-split": _entry(scaled, 2.0 ** -7, IP, SPLIT),
    "scaled-2^-7-l2-f16": _entry(scaled, 2.0 ** -7, L2, F16),
    "scaled-48-l2-split": _entry(scaled, 48.0, L2, SPLIT),
    "scaled-48-ip-f16": _entry(scaled, 48.0, IP, F16),
    "common-mean-ip-f16": _entry(common_mean, IP, F16),
    "common-mean-l2-split": _entry(common_mean, L2, SPLIT),
    "signs-zeros-ip-split": _entry(signs_and_zeros, IP, SPLIT),
    "signs-zeros-l2-f16": _entry(signs_and_zeros, L2, F16),
    "degenerate-dims-ip-f16": _entry(degenerate_dims, IP, F16, modes=(SQ8, PQ)),
    "degenerate-dims-l2-split": _entry(degenerate_dims, L2, SPLIT, modes=(SQ8, PQ)),
    "sq8-outliers-ip-split": _entry(sq8_outliers, IP, SPLIT, modes=(SQ8,)),
    "sq8-outliers-l2-f16": _entry(sq8_outliers, L2, F16, modes=(SQ8,)),
}
# the widest Flat rows each packing takes at k = 56 (asserted against ivf_fits by the host test, with d + 64 refused)
FLAT_DMAX = {F16: 2240, SPLIT: 1088}
PARAMS = [(name, mode) for name, (_, modes) in CASES.items() for mode in modes]


@functools.lru_cache(maxsize=2)
def build(name):
    return CASES[name][0]()
