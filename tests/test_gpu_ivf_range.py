"""The threshold search through the lists on the device (lvs_ivf_range_search / lvs_ivf_range_kernel) against float64 on the
CPU.  The rule: the result is every (query, row) of the query's probed lists (and of the selection) whose score passes the
threshold - ``ivf_range_reference``'s ``want``, give or take its ``near`` (pairs within 2e-5 of the threshold, where fp32 and
float64 may disagree) -, each once, with scores within 1e-5 of the float64 ones; nprobe = nlist is the brute-force join.
Every case first asserts on the reference alone that it is worth running: >= 1000 pairs, at most 1 % of them near."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import synth
from ivf_range_oracle_backend import check_pairs, codes, float64_scores, ivf_range_reference
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi, dedup, ops
from test_gpu_ivf import _centroids, _data

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _probe(be, packed, lists, qp, metric, nprobe):
    """The lists every query probes: all of them, or the device's own coarse step (the top-1 search reports it)."""
    if nprobe == lists.nlist:
        return np.tile(np.arange(nprobe), (qp.n, 1))
    return _np(be.ivf_search(packed, lists, qp, 1, metric, nprobe, want_probe=True)[1])


def _setup(be, nb, d, nq, mode, metric, nlist, seed):
    xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=seed)
    packed = be.pack(xb, mode)
    lists = be.ivf_build(packed, _centroids(xb_s, nlist, metric, seed=nb + seed), metric)
    off, rows = _np(lists.offsets), _np(lists.rows).view(np.uint32)
    assert off[-1] == nb and (np.diff(off) == 0).any()  # every row in a list, and the dead centroid's list is empty
    return xb_s, xq_s, packed, lists, be.pack(xq, mode), off, rows


def _accept(xb_s, xq_s, metric, thr, off, rows, probe, q, j, s, mask=None, queries=None, own=None):
    """``queries``: check these queries only (the reference of a long call is taken on a sample).  ``own``: the row every
    query is (``q_rows``) - the reference is taken without those pairs."""
    q, j, s = _np(q), _np(j), _np(s)
    if queries is not None:
        keep = np.isin(q, queries)
        q, j, s = np.searchsorted(queries, q[keep]), j[keep], s[keep]
        xq_s, probe = xq_s[queries], probe[queries]
        own = None if own is None else own[queries]
    want, near = ivf_range_reference(xb_s, xq_s, thr, metric, off, rows, probe, sel=mask)
    if own is not None:
        want, near = want[want[:, 1] != own[want[:, 0]]], near[near[:, 1] != own[near[:, 0]]]
    print(f"want {len(want)} near {len(near)} got {len(q)}")
    assert len(want) >= 1000 and len(near) <= 0.01 * len(want), (len(want), len(near))
    got = np.stack([q, j], axis=1)
    check_pairs(got, want, near, xb_s.shape[0])
    ref = float64_scores(xb_s, xq_s, metric, got)
    err = np.abs((s if metric == IP else -s).astype(np.float64) - ref).max()
    print(f"score err {err:.3g}")
    assert err <= 1e-5, err
    assert np.all(s > thr) if metric == IP else np.all(-s < thr)  # strict, in fp32
    return got


def _search(be, packed, lists, qp, metric, thr, nprobe, **kw):
    return be.ivf_range_search(packed, lists, qp, thr if metric == IP else -thr, metric, nprobe, **kw)


# 1. every list probed is the brute-force join: U = 4 (d = 64) and U = 8, both storages and metrics, ragged last blocks, the
# dead centroid's empty list, one query and seven, and 20 000 queries against the whole reference
FULL = [
    # nb, d, nq, mode, metric, nlist, threshold
    (3000, 64, 300, F16, IP, 16, 0.30),
    (3000, 64, 300, SPLIT, L2, 16, 1.40),
    (4000, 384, 500, SPLIT, IP, 24, 0.12),
    (2000, 1000, 200, F16, IP, 12, 0.075),
    (3000, 64, 1, SPLIT, IP, 16, 0.02),
    (4000, 384, 7, F16, L2, 24, 1.96),
    (4000, 384, 20000, F16, IP, 24, 0.12),  # two in-call chunks, ~625 tiles per list, 800 k hits on the one counter
]


@pytest.mark.parametrize("nb,d,nq,mode,metric,nlist,thr", FULL)
def test_all_lists_probed_is_brute_force(hip_backend, nb, d, nq, mode, metric, nlist, thr):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _setup(be, nb, d, nq, mode, metric, nlist, seed=d + nq)
    q, j, s = _search(be, packed, lists, qp, metric, thr, nlist)
    _accept(xb_s, xq_s, metric, thr, off, rows, _probe(be, packed, lists, qp, metric, nlist), q, j, s)


# 2. fewer lists than there are: the join over the lists the device's coarse step picked
PART = [
    (6000, 384, 300, F16, IP, 40, 4, 0.05),
    (4000, 768, 300, SPLIT, IP, 64, 8, 0.04),
    (3000, 64, 200, F16, IP, 200, 1, -0.05),  # ~15 rows per list: most blocks are ragged
]


@pytest.mark.parametrize("nb,d,nq,mode,metric,nlist,nprobe,thr", PART)
def test_partial_probe_is_the_join_over_the_probed_lists(hip_backend, nb, d, nq, mode, metric, nlist, nprobe, thr):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _setup(be, nb, d, nq, mode, metric, nlist, seed=7 * d + nq)
    q, j, s = _search(be, packed, lists, qp, metric, thr, nprobe)
    _accept(xb_s, xq_s, metric, thr, off, rows, _probe(be, packed, lists, qp, metric, nprobe), q, j, s)


# 3. 5 000 queries on 24 lists: ~150 tiles of 32 pairs per list
def test_many_tiles_per_list(hip_backend):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _setup(be, 4000, 384, 5000, SPLIT, IP, 24, seed=3)
    q, j, s = _search(be, packed, lists, qp, IP, 0.12, 24)
    _accept(xb_s, xq_s, IP, 0.12, off, rows, _probe(be, packed, lists, qp, IP, 24), q, j, s)


# 4. 40 000 queries: three chunks inside one C call (16 384 each), one counter, query numbers from the call's first query
def test_beyond_one_in_call_chunk(hip_backend):
    be = hip_backend
    nq = 40000
    xb_s, xq_s, packed, lists, qp, off, rows = _setup(be, 20000, 64, nq, F16, IP, 64, seed=11)
    q, j, s = _search(be, packed, lists, qp, IP, 0.30, 4)
    assert int(_np(q).min()) >= 0 and int(_np(q).max()) < nq
    rng = np.random.default_rng(4)
    sample = np.unique(np.concatenate([[0, 16383, 16384, 16385, 32767, 32768, 32769, nq - 1], rng.choice(nq, 200, replace=False)]))
    _accept(xb_s, xq_s, IP, 0.30, off, rows, _probe(be, packed, lists, qp, IP, 4), q, j, s, queries=sample)


# 4b. own rows across an in-call chunk boundary: test 4's index searched with its 20 000 rows as the queries (two in-call
# chunks), q_rows = their numbers - the second chunk's launch reads q_rows from its own first query on
def test_own_rows_across_an_in_call_chunk_boundary(hip_backend):
    import torch

    be = hip_backend
    nq = 20000
    xb_s, _, packed, lists, _, off, rows = _setup(be, nq, 64, 1, F16, IP, 64, seed=11)
    qp = be.pack(xb_s.astype(np.float16), F16)
    rng = np.random.default_rng(4)
    sample = np.unique(np.concatenate([[0, 16383, 16384, 16385, nq - 1], rng.choice(nq, 200, replace=False)]))
    probe = _probe(be, packed, lists, qp, IP, 4)
    q_rows = torch.arange(nq, dtype=torch.int32, device=be.device)
    q, j, s = _search(be, packed, lists, qp, IP, 0.30, 4, q_rows=q_rows)
    got = _accept(xb_s, xb_s, IP, 0.30, off, rows, probe, q, j, s, queries=sample, own=np.arange(nq))
    assert np.all(_np(q) != _np(j)) and np.all(sample[got[:, 0]] != got[:, 1])
    # teeth: without q_rows every sampled query comes back paired with itself (its own list is among its probes, score 1)
    q, j, s = _search(be, packed, lists, qp, IP, 0.30, 4)
    q, j = _np(q), _np(j)
    assert np.array_equal(np.sort(q[(q == j) & np.isin(q, sample)]), sample)


# 5. + 6. share one index
@pytest.fixture(scope="module")
def small(hip_backend):
    return _setup(hip_backend, 3000, 64, 1300, F16, IP, 16, seed=5)


def test_python_chunks_and_regrowth(hip_backend, small, monkeypatch):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = small
    q, j, s = (_np(t) for t in _search(be, packed, lists, qp, IP, 0.30, 16))
    got = _accept(xb_s, xq_s, IP, 0.30, off, rows, _probe(be, packed, lists, qp, IP, 16), q, j, s)
    monkeypatch.setattr(type(be), "IVF_RANGE_CHUNK_ROWS", 512)  # three Python-level chunks, each outgrowing 16 slots
    q2, j2, s2 = (_np(t) for t in _search(be, packed, lists, qp, IP, 0.30, 16, capacity=16))
    a, b = np.argsort(codes(got, 3000)), np.argsort(codes(np.stack([q2, j2], axis=1), 3000))
    assert np.array_equal(q[a], q2[b]) and np.array_equal(j[a], j2[b]) and np.array_equal(s[a], s2[b])


def test_capacity_is_a_wall(hip_backend, small):
    import torch

    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = small
    true = int(_search(be, packed, lists, qp, IP, 0.30, 16)[0].numel())
    cap = true // 3
    assert cap > 1000
    oq = torch.full((cap + 64,), -7, dtype=torch.int64, device=be.device)
    oj = torch.full((cap + 64,), -7, dtype=torch.int64, device=be.device)
    os_ = torch.full((cap + 64,), -7.0, dtype=torch.float32, device=be.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=be.device)
    need = int(be.lib.lvs_ivf_range_workspace_bytes(qp.n, lists.nlist, 16, 64, qp.mode))
    ws = torch.empty((need,), dtype=torch.uint8, device=be.device)
    cpk = lists.centroids
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = be.lib.lvs_ivf_range_search(p(packed.rows), packed.mode, packed.n, p(packed.norms), p(lists.offsets), p(lists.rows), None,
                                     lists.nlist, p(cpk.rows), cpk.mode, p(cpk.norms), p(qp.rows), qp.mode, qp.n, p(qp.norms), None,
                                     64, IP, 16, 0.30, 0, cap, p(oq), p(oj), p(os_), p(cnt), p(ws), need,
                                     ctypes.c_void_p(be._stream()))
    assert rc == _capi.OK
    be.synchronize()
    assert int(cnt.item()) == true  # hits past the capacity are counted ...
    q, j, s = _np(oq), _np(oj), _np(os_)
    assert np.all(q[cap:] == -7) and np.all(j[cap:] == -7) and np.all(s[cap:] == -7.0)  # ... and never stored
    got = np.stack([q[:cap], j[:cap]], axis=1)
    assert q[:cap].min() >= 0 and q[:cap].max() < qp.n and j[:cap].min() >= 0 and j[:cap].max() < 3000
    assert np.unique(codes(got, 3000)).size == cap  # every stored triple is a pair of the full result, once
    want, near = ivf_range_reference(xb_s, xq_s, 0.30, IP, off, rows, np.tile(np.arange(16), (qp.n, 1)))
    assert np.setdiff1d(codes(got, 3000), np.union1d(codes(want, 3000), codes(near, 3000))).size == 0
    assert np.abs(s[:cap].astype(np.float64) - float64_scores(xb_s, xq_s, IP, got)).max() <= 1e-5


# 7. a row selector: every third row, and one whole list deselected (its blocks are skipped)
def test_selector(hip_backend):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _setup(be, 4000, 384, 500, SPLIT, IP, 24, seed=9)
    mask = np.zeros(4000, bool)
    mask[::3] = True
    big = int(np.argmax(np.diff(off)))
    mask[rows[off[big]:off[big + 1]].astype(np.int64)] = False
    sel, count = be.row_bitmap(np.flatnonzero(mask), 4000)
    assert count == int(mask.sum())
    q, j, s = _search(be, packed, lists, qp, IP, 0.12, 24, sel=sel)
    got = _accept(xb_s, xq_s, IP, 0.12, off, rows, _probe(be, packed, lists, qp, IP, 24), q, j, s, mask=mask)
    assert mask[got[:, 1]].all()


# 8. the LDS edge: d = 2304 fp16 fits this kernel (144 fragments) and not the top-k scan at k = 56; one d past the bound the
# workspace call says so and HipVS answers exactly
def test_lds_edge(hip_backend, tmp_path):
    be = hip_backend
    assert be.ivf_range_fits(2304, F16) and not be.ivf_fits(2304, 56, F16)
    xb_s, xq_s, packed, lists, qp, off, rows = _setup(be, 1000, 2304, 64, F16, IP, 8, seed=2)
    q, j, s = _search(be, packed, lists, qp, IP, 0.02, 8)
    _accept(xb_s, xq_s, IP, 0.02, off, rows, _probe(be, packed, lists, qp, IP, 8), q, j, s)
    dmax = 2496
    assert be.ivf_range_fits(dmax, F16) and not be.ivf_range_fits(dmax + 1, F16)
    assert be.lib.lvs_ivf_range_workspace_bytes(64, 8, 8, dmax + 1, F16) == _capi.EUNSUPPORTED
    xb, _, xq, xq_s = _data(600, 16, dmax + 1, F16, seed=8)
    vs = HipVS(backend=be, factory_string="IVF4,Flat", nprobe=4)
    vs.index(None, xb, str(tmp_path / "wide"), persist=False)
    be.timing_enable(True)
    lims, D, I = vs.range_search(xq, 0.02)
    kernel = be.timing_read_full()["kernel"]
    be.timing_enable(False)
    assert kernel != "lvs_ivf_range_kernel"  # the exact join served it
    sc = xq_s.astype(np.float64) @ xb.astype(np.float64).T
    got = codes(np.stack([np.repeat(np.arange(16), np.diff(lims)), I], axis=1), 600)
    w, n = codes(np.argwhere(sc > 0.02 + 2e-5), 600), codes(np.argwhere(np.abs(sc - 0.02) <= 2e-5), 600)
    assert len(w) >= 1000 and len(n) <= 0.01 * len(w), (len(w), len(n))
    assert np.setdiff1d(w, got).size == 0 and np.setdiff1d(got, np.union1d(w, n)).size == 0


# 9. the self-join
def _planted():
    """6 000 unit fp16 rows: 5 500 base rows, 299 near-duplicates (noise 0.05) of distinct base rows, one exact duplicate,
    200 hard negatives (noise 0.5, cos ~ 0.89)."""
    rng = np.random.default_rng(77)
    n, d = 6000, 384
    x = np.empty((n, d), np.float32)
    x[:5500] = synth.corpus(5500, d, seed=77)
    src = rng.choice(5500, 500, replace=False)

    def near(rows, eps):
        u = rng.standard_normal((len(rows), d)).astype(np.float32)
        y = x[rows] + np.float32(eps) * u / np.linalg.norm(u, axis=1, keepdims=True)
        return y / np.linalg.norm(y, axis=1, keepdims=True)

    x[5500:5799] = near(src[:299], 0.05)
    x[5799] = x[src[299]]
    x[5800:] = near(src[300:], 0.5)
    return x.astype(np.float16)


@pytest.fixture(scope="module")
def dup_store(hip_backend, tmp_path_factory):
    x = _planted()
    vs = HipVS(backend=hip_backend, factory_string="IVF32,Flat")
    vs.index(None, x, str(tmp_path_factory.mktemp("dups")), persist=False)
    return vs, x


def _cpu_pairs(x, ids=None):
    xs = x.astype(np.float64) if ids is None else x[ids].astype(np.float64)
    sc = np.triu(xs @ xs.T, 1)
    return np.argwhere(sc > 0.95 + 2e-5), int(((np.abs(sc - 0.95) <= 2e-5) & (sc != 0)).sum())


def _rule(vs, x, ref, nprobe, ids=None):
    """The pairs of ``ref`` (positions into ids) whose one row's list is among the other's probes."""
    _, off, rows = vs.ivf_lists()
    lid = np.empty(len(x), np.int64)
    lid[rows.astype(np.int64)] = np.repeat(np.arange(len(off) - 1), np.diff(off))
    ids = np.arange(len(x)) if ids is None else ids
    probe = vs.ivf_probe(x[ids], nprobe)
    return [(a, b) for a, b in zip(ref[0].tolist(), ref[1].tolist())
            if lid[ids[b]] in probe[a] or lid[ids[a]] in probe[b]]


def test_self_join(hip_backend, dup_store):
    vs, x = dup_store
    above, band = _cpu_pairs(x)
    assert len(above) == 300 and band == 0
    ref = dedup.threshold_pairs(hip_backend, vs.packed_rows(), 0.95)
    assert sorted(zip(ref[0].tolist(), ref[1].tolist())) == sorted(map(tuple, above.tolist()))
    full = dedup.threshold_pairs_ivf(vs, 0.95, nprobe=32)
    assert np.array_equal(full[0], ref[0]) and np.array_equal(full[1], ref[1]) and np.abs(full[2] - ref[2]).max() <= 1e-5
    two = dedup.threshold_pairs_ivf(vs, 0.95, nprobe=2)
    rule = _rule(vs, x, ref, 2)
    assert list(zip(two[0].tolist(), two[1].tolist())) == rule and 0 < len(rule) <= 300
    assert np.all(two[0] < two[1]) and np.all(np.diff(two[0] * 6000 + two[1]) > 0)  # i < j, unique, sorted
    assert np.abs(two[2].astype(np.float64) - float64_scores(x, x, IP, np.stack([two[0], two[1]], axis=1))).max() <= 1e-5


def test_self_join_over_ids(hip_backend, dup_store):
    vs, x = dup_store
    ids = np.arange(0, 6000, 2)
    above, band = _cpu_pairs(x, ids)
    assert len(above) >= 50 and band == 0
    ref = dedup.threshold_pairs(hip_backend, vs.packed_rows(ids), 0.95)
    assert sorted(zip(ref[0].tolist(), ref[1].tolist())) == sorted(map(tuple, above.tolist()))
    full = dedup.threshold_pairs_ivf(vs, 0.95, ids=ids, nprobe=32)
    assert np.array_equal(full[0], ref[0]) and np.array_equal(full[1], ref[1])
    two = dedup.threshold_pairs_ivf(vs, 0.95, ids=ids, nprobe=2)
    assert list(zip(two[0].tolist(), two[1].tolist())) == _rule(vs, x, ref, 2, ids)
    assert np.all(two[0] < two[1]) and np.all(np.diff(two[0] * 6000 + two[1]) > 0)


# 10. through HipVS and ops
def test_range_search_through_hipvs(hip_backend, tmp_path):
    be = hip_backend
    xb, xb_s, xq, xq_s = _data(3000, 300, 64, SPLIT, seed=31)
    for metric, thr in ((METRIC_INNER_PRODUCT, 0.30), (METRIC_L2, 1.40)):
        vs = HipVS(metric=metric, backend=be, factory_string="IVF16,PQ8", nprobe=16)
        vs.index(None, xb, str(tmp_path / f"pq{metric}"), persist=False)
        be.timing_enable(True)
        lims, D, I = vs.range_search(xq, thr)
        kernel = be.timing_read_full()["kernel"]
        be.timing_enable(False)
        assert kernel == "lvs_ivf_range_kernel"
        _, off, rows = vs.ivf_lists()
        want, near = ivf_range_reference(xb_s, xq_s, thr, metric, off, rows, np.tile(np.arange(16), (300, 1)))
        assert len(want) >= 1000 and len(near) <= 0.01 * len(want)
        got = np.stack([np.repeat(np.arange(300), np.diff(lims)), I], axis=1)
        check_pairs(got, want, near, 3000)
        assert np.abs(D.astype(np.float64) - float64_scores(xb_s, xq_s, metric, got)).max() <= 1e-5  # exact, not PQ's
        for q in range(300):
            d, i = D[lims[q]:lims[q + 1]], I[lims[q]:lims[q + 1]]
            better = d if metric == METRIC_INNER_PRODUCT else -d
            assert np.all((np.diff(better) < 0) | ((np.diff(better) == 0) & (np.diff(i) > 0)))
        ex = vs.range_search(xq, thr, exact=True)
        check_pairs(np.stack([np.repeat(np.arange(300), np.diff(ex[0])), ex[2]], axis=1), want, near, 3000)


def test_sem_dedup_through_the_lists(hip_backend, tmp_path):
    rng = np.random.default_rng(6)
    x = synth.corpus(2000, 128, seed=6)
    dst = 1000 + rng.choice(1000, 150, replace=False)
    x[dst] = x[rng.choice(1000, 150, replace=False)] + 0.004 * rng.standard_normal((150, 128)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    vs = HipVS(backend=hip_backend, factory_string="IVF16,Flat")
    df = ops.sem_index(pd.DataFrame({"t": [f"t{i}" for i in range(2000)]}), "t", str(tmp_path / "i"), vs=vs, embeddings=x)
    ref = ops.sem_dedup(df, "t", 0.95, vs=vs)
    assert len(ref) == 1850
    assert ops.sem_dedup(df, "t", 0.95, vs=vs, nprobe=16).index.tolist() == ref.index.tolist()
