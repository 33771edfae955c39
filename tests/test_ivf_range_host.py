"""Host side of the threshold search through the lists, on the CPU (``IvfRangeOracleBackend``): the routes of
``HipVS.range_search``, its ``(lims, D, I)`` layout under both metrics, ``ids`` selectors, ``dedup.threshold_pairs_ivf``'s
both-direction canonicalisation, ``ops.sem_dedup(nprobe=...)`` and the C entry points' declarations and argument checks.  The
device path is covered by tests/test_gpu_ivf_range.py."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import synth
from ivf_range_oracle_backend import IvfRangeOracleBackend, check_pairs, ivf_range_reference
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi, dedup, ops
from lotus_amd.backend import HipBackend, ivf_range_fits

N, D_, NLIST = 1500, 32, 16


@pytest.fixture(scope="module")
def data():
    xb = synth.corpus(N, D_, seed=21)
    xq, _ = synth.queries(xb, 25, seed=22)
    return xb, xq


def store(xb, fs="IVF16,Flat", metric=METRIC_INNER_PRODUCT, **kw):
    vs = HipVS(metric=metric, backend=IvfRangeOracleBackend(), factory_string=fs, **kw)
    vs.index(None, xb, "range", persist=False)
    vs.backend.calls.clear()
    return vs


def names(vs):
    return [c[0] for c in vs.backend.calls if c[0] in ("ivf_range_search", "range_join", "gather", "row_bitmap")]


def brute(xb, xq, thr, metric, ids=None):
    """(lims, D, I) by the definition: float32 scores of the stored values, strict compare, best first, ascending id."""
    ids = np.arange(len(xb)) if ids is None else np.asarray(ids)
    s = (xq.astype(np.float32) @ xb[ids].astype(np.float32).T).astype(np.float32)
    if metric == METRIC_L2:
        qn = np.einsum("ij,ij->i", xq, xq, dtype=np.float32)
        bn = np.einsum("ij,ij->i", xb[ids], xb[ids], dtype=np.float32)
        s = np.maximum((qn[:, None] + bn[None, :]) - 2 * s, 0).astype(np.float32)
    lims, D, I = [0], [], []
    for q in range(len(xq)):
        hit = np.flatnonzero(s[q] > np.float32(thr) if metric == METRIC_INNER_PRODUCT else s[q] < np.float32(thr))
        key = -s[q, hit].astype(np.float64) if metric == METRIC_INNER_PRODUCT else s[q, hit].astype(np.float64)
        o = np.lexsort((ids[hit], key))
        D.append(s[q, hit][o])
        I.append(ids[hit][o])
        lims.append(lims[-1] + len(hit))
    return np.asarray(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def same(a, b, atol=2e-6):
    assert np.array_equal(a[0], b[0])
    assert a[1].dtype == np.float32 and a[2].dtype == np.int64 and a[0].dtype == np.int64
    if np.array_equal(a[2], b[2]):
        assert np.allclose(a[1], b[1], atol=atol, rtol=0)
        return
    for q in range(len(a[0]) - 1):  # the twins' sgemm shapes differ: near-equal scores may swap places
        sl = slice(a[0][q], a[0][q + 1])
        assert sorted(a[2][sl].tolist()) == sorted(b[2][sl].tolist())
        assert np.allclose(np.sort(a[1][sl]), np.sort(b[1][sl]), atol=atol, rtol=0)


# ---- routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", ["IVF16,Flat", "IVF16,SQ8", "IVF16,PQ8", "IVF16,PQ8,Refine(Flat)"])
def test_ivf_stores_go_through_the_lists_with_exact_scores(data, fs):
    xb, xq = data
    vs = store(xb, fs)
    got = vs.range_search(xq, 0.3, nprobe=NLIST)
    assert names(vs) == ["ivf_range_search"] and vs.backend.calls[-1][2] == NLIST
    same(got, brute(xb, xq, 0.3, METRIC_INNER_PRODUCT))  # all lists probed: the exact result, exact scores on a code store
    vs.backend.calls.clear()
    part = vs.range_search(xq, 0.3)  # the store's nprobe = 1
    assert vs.backend.calls[-1][2] == 1 and 0 < part[0][-1] < got[0][-1]


def test_partial_probe_is_the_reference_over_the_probed_lists(data):
    xb, xq = data
    vs = store(xb, nprobe=3)
    lims, D, I = vs.range_search(xq, 0.3)
    _, off, rows = vs.ivf_lists()
    want, near = ivf_range_reference(xb, xq, 0.3, 0, off, rows, vs.ivf_probe(xq, 3))
    got = np.stack([np.repeat(np.arange(len(xq)), np.diff(lims)), I], axis=1)
    assert len(want) > 20
    check_pairs(got, want, near, N)


def test_exact_routes(data, monkeypatch):
    xb, xq = data
    ref = brute(xb, xq, 0.3, METRIC_INNER_PRODUCT)
    vs = store(xb)
    same(vs.range_search(xq, 0.3, exact=True), ref)
    assert names(vs) == ["range_join"]
    flat = store(xb, "Flat")
    same(flat.range_search(xq, 0.3), ref)
    same(flat.range_search(xq, 0.3, nprobe=4), ref)  # nothing to probe: ignored as __call__ ignores it
    assert names(flat) == ["range_join", "range_join"]
    vs.backend.calls.clear()
    monkeypatch.setattr(vs.backend, "ivf_range_fits", lambda d, mode: False, raising=False)  # a shape too wide for the scan
    same(vs.range_search(xq, 0.3), ref)
    assert names(vs) == ["range_join"]
    with pytest.raises(ValueError, match="exact must be a bool"):
        vs.range_search(xq, 0.3, exact=1)
    with pytest.raises(ValueError, match="nprobe"):
        vs.range_search(xq, 0.3, nprobe=0)
    with pytest.raises(ValueError, match="dimension"):
        vs.range_search(xq[:, :8], 0.3)


def test_a_sharded_store_is_refused(data):
    xb, xq = data
    vs = HipVS(backend=IvfRangeOracleBackend(), shard=True)
    vs.index(None, xb, "sharded", persist=False)
    assert vs.range_search(xq, 0.3)[0][-1] > 0  # no process group: one rank holds every row, nothing is sharded
    for lay in ((0, 1, 1, 2, None, None), (1, 2, 0, 1, None, None)):  # rows, then queries, split over two ranks
        vs._lay = lay
        with pytest.raises(ValueError, match="unsharded"):
            vs.range_search(xq, 0.3)
    ivf = store(xb)
    ivf._lay = (0, 1, 1, 2, None, None)
    with pytest.raises(ValueError, match="unsharded"):
        ivf.ivf_self_pairs(0.9, nprobe=2)


# ---- layout and order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,thr", [(METRIC_INNER_PRODUCT, 0.25), (METRIC_L2, 1.5)])
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
def test_layout_and_order(data, metric, thr, storage):
    xb, xq = data
    if storage == "fp16":
        xb, xq = xb.astype(np.float16).astype(np.float32), xq.astype(np.float16).astype(np.float32)
    vs = store(xb, metric=metric, storage=storage)
    lims, D, I = vs.range_search(xq, thr, nprobe=NLIST)
    same((lims, D, I), brute(xb, xq, thr, metric))
    assert lims[0] == 0 and lims[-1] == len(D) == len(I) > 100 and np.all(np.diff(lims) >= 0)
    for q in range(len(xq)):
        d, i = D[lims[q]:lims[q + 1]], I[lims[q]:lims[q + 1]]
        better = d if metric == METRIC_INNER_PRODUCT else -d
        assert np.all(np.diff(better) <= 0)  # best first: products descending, squared distances ascending
        assert np.all((np.diff(better) < 0) | (np.diff(i) > 0))  # ascending id among equal scores
        assert np.all(d > thr) if metric == METRIC_INNER_PRODUCT else np.all(d < thr)
    # no queries, a threshold nothing passes, a query alone
    e = vs.range_search(np.zeros((0, D_), np.float32), thr)
    assert e[0].tolist() == [0] and len(e[1]) == len(e[2]) == 0
    none = vs.range_search(xq, 5.0 if metric == METRIC_INNER_PRODUCT else -1.0, nprobe=NLIST)
    assert none[0].tolist() == [0] * (len(xq) + 1) and none[1].dtype == np.float32 and none[2].dtype == np.int64
    one = vs.range_search(xq[3], thr, nprobe=NLIST)
    assert np.array_equal(one[2], I[lims[3]:lims[4]])


def test_equal_scores_come_in_ascending_id_order():
    xb = synth.corpus(400, D_, seed=5)
    xb[[390, 17, 200]] = xb[5]  # four equal rows
    vs = store(xb, "IVF8,Flat")
    lims, D, I = vs.range_search(xb[5], 0.99, nprobe=8)
    assert I.tolist() == [5, 17, 200, 390] and np.all(D == D[0])


# ---- ids -------------------------------------------------------------------------------------------------------------------
def test_ids_become_a_selector_on_the_list_route(data):
    xb, xq = data
    vs = store(xb)
    ids = np.sort(np.random.default_rng(1).choice(N, 500, replace=False))
    got = vs.range_search(xq, 0.2, ids=ids, nprobe=NLIST)
    assert names(vs) == ["row_bitmap", "ivf_range_search"] and vs.backend.calls[-1][4] == 500
    same(got, brute(xb, xq, 0.2, METRIC_INNER_PRODUCT, ids))
    assert got[0][-1] > 50 and set(got[2].tolist()) <= set(ids.tolist())
    vs.backend.calls.clear()
    same(vs.range_search(xq, 0.2, ids=ids, exact=True), brute(xb, xq, 0.2, METRIC_INNER_PRODUCT, ids))  # gathered, ids mapped back
    assert names(vs) == ["gather", "range_join"]
    vs.backend.calls.clear()
    full = vs.range_search(xq, 0.2, ids=np.arange(N), nprobe=NLIST)  # every row in order: no selector
    assert names(vs) == ["ivf_range_search"] and vs.backend.calls[-1][4] is None
    same(full, brute(xb, xq, 0.2, METRIC_INNER_PRODUCT))
    assert vs.range_search(xq, 0.2, ids=[])[0].tolist() == [0] * (len(xq) + 1)
    for route in (dict(), dict(exact=True)):
        with pytest.raises(ValueError, match="more than once"):
            vs.range_search(xq, 0.2, ids=[3, 9, 3], **route)
    with pytest.raises(IndexError):
        vs.range_search(xq, 0.2, ids=[N])


# ---- self-join -------------------------------------------------------------------------------------------------------------
def planted(n, d, ndup, seed):
    rng = np.random.default_rng(seed)
    x = synth.corpus(n, d, seed=seed)
    src = rng.choice(n // 2, ndup, replace=False)
    dst = n // 2 + rng.choice(n - n // 2, ndup, replace=False)
    x[dst] = x[src] + 0.05 * rng.standard_normal((ndup, d)).astype(np.float32) / np.sqrt(d)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


class _Pairs:
    """Stands in for a HipVS: hands ``threshold_pairs_ivf`` ready-made records."""

    def __init__(self, q, j, s):
        self.rec = (np.asarray(q, np.int64), np.asarray(j, np.int64), np.asarray(s, np.float32))

    def ivf_self_pairs(self, threshold, ids=None, nprobe=None):
        return self.rec


def test_both_directions_become_one_record():
    # (2, 7) from both sides with scores one bit apart, (9, 4) found from the larger side only, (1, 3) from the smaller side only
    vs = _Pairs([7, 2, 9, 1], [2, 7, 4, 3], [0.97000006, 0.97, 0.96, 0.99])
    i, j, s = dedup.threshold_pairs_ivf(vs, 0.95)
    assert i.tolist() == [1, 2, 4] and j.tolist() == [3, 7, 9]
    assert s.tolist() == [np.float32(0.99), np.float32(0.97), np.float32(0.96)]  # (2, 7): the record asked from row 2
    assert i.dtype == j.dtype == np.int64 and s.dtype == np.float32
    i, j, s = dedup.threshold_pairs_ivf(vs, 0.95, ids=[9, 7, 4, 3, 2, 1])  # positions into ids: 9->0 7->1 4->2 3->3 2->4 1->5
    assert list(zip(i.tolist(), j.tolist())) == [(0, 2), (1, 4), (3, 5)]
    assert s.tolist() == [np.float32(0.96), np.float32(0.97000006), np.float32(0.99)]  # (1, 4): asked from position 1, row 7
    e = dedup.threshold_pairs_ivf(_Pairs([], [], []), 0.95)
    assert all(len(a) == 0 for a in e)


def test_threshold_pairs_ivf_against_the_exact_join_and_the_rule():
    x = planted(1200, D_, 60, seed=3)
    vs = store(x, "IVF12,Flat")
    ref = dedup.threshold_pairs(vs.backend, vs.packed_rows(), 0.95)
    assert len(ref[0]) >= 60
    got = dedup.threshold_pairs_ivf(vs, 0.95, nprobe=12)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.allclose(got[2], ref[2], atol=2e-6)
    assert vs.backend.calls[-1][:4] == ("ivf_range_search", 1200, 12, True)
    # nprobe = 1: exactly the pairs of the rule - score above the threshold and list(j) in probes(i) or list(i) in probes(j)
    _, off, rows = vs.ivf_lists()
    lid = np.empty(1200, np.int64)
    lid[rows.astype(np.int64)] = np.repeat(np.arange(12), np.diff(off))
    probe = vs.ivf_probe(x, 1)
    rule = [(a, b) for a, b in zip(ref[0], ref[1]) if lid[b] in probe[a] or lid[a] in probe[b]]
    one = dedup.threshold_pairs_ivf(vs, 0.95, nprobe=1)
    assert list(zip(one[0].tolist(), one[1].tolist())) == rule and 0 < len(rule) <= len(ref[0])
    assert np.all(one[0] < one[1]) and np.all(np.diff(one[0] * 1200 + one[1]) > 0)
    # ids: positions into ids, the other rows out of the join on both sides
    ids = np.arange(0, 1200, 2)
    sub = dedup.threshold_pairs_ivf(vs, 0.95, ids=ids, nprobe=12)
    assert vs.backend.calls[-1][:5] == ("ivf_range_search", 600, 12, True, 600)  # 600 gathered queries, 600 rows selected
    ref_sub = dedup.threshold_pairs(vs.backend, vs.packed_rows(ids), 0.95)
    assert len(ref_sub[0]) > 5 and np.array_equal(sub[0], ref_sub[0]) and np.array_equal(sub[1], ref_sub[1])
    with pytest.raises(ValueError, match="more than once"):
        dedup.threshold_pairs_ivf(vs, 0.95, ids=[1, 1], nprobe=2)
    with pytest.raises(ValueError, match="no IVF lists"):
        dedup.threshold_pairs_ivf(store(x, "Flat"), 0.95, nprobe=2)


# ---- sem_dedup -------------------------------------------------------------------------------------------------------------
def test_sem_dedup_through_the_lists(tmp_path):
    x = planted(800, D_, 50, seed=9)
    vs = store(x, "IVF8,Flat")
    df = ops.sem_index(pd.DataFrame({"t": [f"t{i}" for i in range(800)]}), "t", str(tmp_path / "i"), vs=vs, embeddings=x)
    ref = ops.sem_dedup(df, "t", 0.95, vs=vs)
    assert 700 <= len(ref) < 800
    vs.backend.calls.clear()
    got = ops.sem_dedup(df, "t", 0.95, vs=vs, nprobe=8)
    assert got.index.tolist() == ref.index.tolist() and "ivf_range_search" in names(vs)
    part = df[df.index % 3 != 0]  # a filtered frame: positions are remapped through ids
    assert ops.sem_dedup(part, "t", 0.95, vs=vs, nprobe=8).index.tolist() == ops.sem_dedup(part, "t", 0.95, vs=vs).index.tolist()
    few = ops.sem_dedup(df, "t", 0.95, vs=vs, nprobe=1)
    assert len(ref) <= len(few) <= 800  # fewer pairs found: never more rows dropped


def test_sem_dedup_nprobe_refusals(tmp_path):
    x = planted(300, D_, 10, seed=4)
    frame = pd.DataFrame({"t": [f"t{i}" for i in range(300)]})
    flat = store(x, "Flat")
    df = ops.sem_index(frame.copy(), "t", str(tmp_path / "f"), vs=flat, embeddings=x)
    with pytest.raises(ValueError, match="IVF"):
        ops.sem_dedup(df, "t", 0.95, vs=flat, nprobe=2)
    ivf = store(x, "IVF4,Flat")
    df = ops.sem_index(frame.copy(), "t", str(tmp_path / "v"), vs=ivf, embeddings=x)
    with pytest.raises(ValueError, match="shard=False"):
        ops.sem_dedup(df, "t", 0.95, vs=ivf, nprobe=2, shard=True)
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="nprobe"):
            ops.sem_dedup(df, "t", 0.95, vs=ivf, nprobe=bad)
    twice = df.iloc[[0, 1, 1, 2]]  # the exact join takes a frame whose index repeats a row, a bitmap cannot
    assert len(ops.sem_dedup(twice, "t", 0.95, vs=ivf)) >= 3
    with pytest.raises(ValueError, match="more than once"):
        ops.sem_dedup(twice, "t", 0.95, vs=ivf, nprobe=2)
    l2 = store(x, "IVF4,Flat", metric=METRIC_L2)
    df = ops.sem_index(frame.copy(), "t", str(tmp_path / "l"), vs=l2, embeddings=x)
    with pytest.raises(ValueError, match="METRIC_INNER_PRODUCT"):
        ops.sem_dedup(df, "t", 0.95, vs=l2, nprobe=2)
    assert len(ops.sem_dedup(df.copy(), "t", 0.95, vs=ivf, nprobe=4)) == len(ops.sem_dedup(df.copy(), "t", 0.95, vs=ivf))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_agree_on_the_new_entries():
    assert sorted(_capi.SIGNATURES) == _capi.declared_symbols()
    for name, arity in (("lvs_ivf_range_workspace_bytes", 5), ("lvs_ivf_range_search", 29)):
        assert len(_capi.PROTOTYPES[name].names) == len(_capi.SIGNATURES[name][1]) == arity, name
    assert _capi.DEFINES["LVS_KERNEL_IVF_RANGE"] == 8 and HipBackend.KERNEL_NAMES[8] == "lvs_ivf_range_kernel"


def test_workspace_bytes_and_the_lds_bound():
    lib = _capi.load()
    ws = lib.lvs_ivf_range_workspace_bytes
    assert ws(100, 16, 4, 64, _capi.PACK_F16) > 0 and ws(0, 16, 4, 64, _capi.PACK_SPLIT) >= 0
    for bad in ((-1, 16, 4, 64, 0), (10, 0, 1, 64, 0), (10, 16, 0, 64, 0), (10, 16, 17, 64, 0), (10, 4096, 2049, 64, 0),
                (10, 16, 4, 0, 0), (10, 16, 4, 64, 2)):
        assert ws(*bad) == _capi.EINVAL, bad
    # fragments of 1 KB per 16 columns (two sets for hi|lo) + the slot table, within 160 KB: wider than the top-k scan's
    assert ivf_range_fits(2496, _capi.PACK_F16) and not ivf_range_fits(2497, _capi.PACK_F16)
    assert ivf_range_fits(1216, _capi.PACK_SPLIT) and not ivf_range_fits(1217, _capi.PACK_SPLIT)
    assert ws(10, 16, 4, 2497, _capi.PACK_F16) == _capi.EUNSUPPORTED == ws(10, 16, 4, 1217, _capi.PACK_SPLIT)
    from lotus_amd.backend import ivf_fits

    assert not ivf_fits(2304, 56, _capi.PACK_F16) and not ivf_fits(2496, 1, _capi.PACK_F16)
    # a million queries: chunked, so the scratch stays bounded
    assert 0 < ws(1 << 20, 4096, 8, 768, _capi.PACK_F16) <= 600 << 20


def test_search_argument_checks():
    lib = _capi.load()
    one = ctypes.c_uint64(0)
    p = ctypes.addressof(one)  # checks run before any pointer is followed
    f = lib.lvs_ivf_range_search

    def call(metric=0, nb=100, nq=10, d=64, nlist=16, nprobe=4, score_exp=0, capacity=8, count=p, xb_pack=0, xq_pack=0, c_pack=0,
             xb=p, out=p, ws=p, ws_bytes=1 << 30, norms=None):
        return f(xb, xb_pack, nb, norms, p, p, None, nlist, p, c_pack, norms, p, xq_pack, nq, norms, None, d, metric, nprobe, 0.5,
                 score_exp, capacity, out, out, out, count, ws, ws_bytes, None)

    for kw in (dict(metric=2), dict(nb=-1), dict(nq=-1), dict(d=0), dict(nlist=0), dict(nprobe=0), dict(nprobe=17),
               dict(nlist=4096, nprobe=2049), dict(xb_pack=3), dict(xq_pack=3), dict(c_pack=3), dict(score_exp=121),
               dict(capacity=-1), dict(count=None), dict(xb=None), dict(out=None), dict(ws=None), dict(metric=1)):
        assert call(**kw) == _capi.EINVAL, kw
        assert lib.lvs_last_error()
    assert call(nq=0) == _capi.OK  # nothing to do
    assert call(d=2497) == _capi.EUNSUPPORTED and b"lvs_ivf_range_workspace_bytes" in lib.lvs_last_error()
    assert call(ws_bytes=16) == _capi.ENOMEM and b"need" in lib.lvs_last_error()
