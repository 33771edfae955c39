"""Host side of the ``"...,Refine(Flat)"`` stores of HipVS (factory strings, ``k_factor``, the candidate count, routing, the
shared sidecars and ``lvs_refine_keys``'s argument checks), on the CPU with the oracle-backed double of
tests/ivf_refine_oracle_backend.py.  The device path is covered by tests/test_gpu_ivf_refine.py."""
import ctypes
import math
import os

import numpy as np
import pytest

import oracle
import synth
from ivf_pq_oracle_backend import PqOracleBackend
from ivf_refine_oracle_backend import RefineOracleBackend, exact_scores, refine_reference
from ivf_sq8_oracle_backend import Sq8OracleBackend
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi
from oracle_backend import _emulate_storage

BAR, TIE_GAP = 1e-5, 2e-5  # the project's bars
CODECS = {"PQ8": "ivf_pq_search", "SQ8": "ivf_sq8_search"}


def make_vs(**kw):
    return HipVS(backend=RefineOracleBackend(), **kw)


def clustered(n, d, centers=12, seed=3):
    """Unit rows around a few centres: scores of magnitude <= 1, so the project's absolute bars apply as they stand."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + 0.5 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def stored(vs, x):
    """float64 values the store holds for ``x``, in the caller's units (the index's power-of-two scale applied and undone)."""
    pk = vs._current().packed
    f = np.float32(2.0 ** pk.exp)
    return _emulate_storage(np.asarray(x, np.float32) * f, pk.mode).astype(np.float64) / np.float64(f)


def _no_kmeans(monkeypatch):
    from lotus_amd import cluster

    def boom(*a, **k):
        raise AssertionError("k-means was called")

    monkeypatch.setattr(cluster, "kmeans", boom)


@pytest.fixture(scope="module")
def rows():
    return clustered(2000, 32), clustered(25, 32, seed=5)


# ---- factory strings and k_factor ----------------------------------------------------------------------------------------
def test_factory_string_parsing():
    for fs, kind, M in (("IVF16,SQ8,Refine(Flat)", "SQ8", None), ("IVF16,PQ8,Refine(Flat)", "PQ", 8),
                        ("IVF4096,PQ64x8,Refine(Flat)", "PQ", 64), ("IVF1,PQ1,Refine(Flat)", "PQ", 1)):
        vs = make_vs(factory_string=fs, nprobe=4)
        assert vs._nlist == int(fs[3:fs.index(",")]) and vs._mode.kind == kind and vs._mode.M == M and vs._mode.refine
        assert vs.factory_string == fs and vs.k_factor == 1.0
    for fs in ("IVF16,SQ8", "IVF16,PQ8", "IVF16,PQ8x8", "IVF16,Flat"):
        assert not make_vs(factory_string=fs)._mode.refine
    for bad in ("IVF16,PQ8,RFlat", "IVF16,SQ8,RFlat", "IVF16,Flat,Refine(Flat)", "IVF16,Flat,RFlat", "IVF16,PQ8,Refine(SQ8)",
                "IVF16,PQ8,Refine(PQ8)", "IVF16,PQ8,Refine(Flat),Refine(Flat)", "IVF16,PQ8,Refine(Flat) ", "IVF16,PQ8,refine(flat)",
                "IVF16,PQ8,Refine()", "IVF16,PQ8x4,Refine(Flat)", "IVF0,PQ8,Refine(Flat)", "IVF16,PQ0,Refine(Flat)",
                "IVF16,Refine(Flat)", "Flat,Refine(Flat)", "Refine(Flat)", "IVF16,PQ8,Refine(Flat"):
        with pytest.raises(ValueError, match="PQ<M>"):
            make_vs(factory_string=bad)


def test_backends_without_the_re_ranking_are_refused():
    for fs in ("IVF16,PQ8,Refine(Flat)", "IVF16,SQ8,Refine(Flat)"):
        with pytest.raises(ValueError, match="refine_keys"):
            HipVS(backend=PqOracleBackend(), factory_string=fs)
    with pytest.raises(ValueError, match="no IVF-PQ codec"):
        HipVS(backend=Sq8OracleBackend(), factory_string="IVF16,PQ8,Refine(Flat)")
    with pytest.raises(ValueError, match="refine_keys"):
        HipVS(backend=Sq8OracleBackend(), factory_string="IVF16,SQ8,Refine(Flat)")
    HipVS(backend=PqOracleBackend(), factory_string="IVF16,PQ8")  # the plain modes ask for nothing new


@pytest.mark.parametrize("shard", [True, "rows", "queries", "auto", (1, 2)])
def test_refined_stores_refuse_every_shard_setting(shard):
    with pytest.raises(ValueError, match="shard"):
        make_vs(factory_string="IVF8,PQ4,Refine(Flat)", shard=shard)


GOOD_FACTORS = (1, 1.0, 2.5, 5, 100, np.float32(3), np.int64(2), np.float64(1.5))
BAD_FACTORS = (0.5, 0, -1, 0.999, float("nan"), float("inf"), -float("inf"), "5", None, True, False, 1j, [2.0], (3,))


def test_k_factor_values(tmp_path):
    for f in GOOD_FACTORS:
        assert make_vs(factory_string="IVF16,PQ8,Refine(Flat)", k_factor=f).k_factor == float(f)
    for f in BAD_FACTORS:
        with pytest.raises(ValueError, match="k_factor"):
            make_vs(factory_string="IVF16,PQ8,Refine(Flat)", k_factor=f)
        with pytest.raises(ValueError, match="k_factor"):
            make_vs(k_factor=f)  # checked whatever the store
    vs = make_vs(factory_string="IVF4,SQ8,Refine(Flat)", nprobe=2)
    vs.index(None, clustered(200, 8), str(tmp_path / "i"))
    q = clustered(3, 8, seed=4)
    for f in BAD_FACTORS:
        with pytest.raises(ValueError, match="k_factor"):
            vs(q, 5, k_factor=f)
        if f is not None:  # (None there: the store's own factor)
            with pytest.raises(ValueError, match="k_factor"):
                vs.refine_candidates(5, f)
    for f in GOOD_FACTORS:
        assert vs(q, 5, k_factor=f).indices.shape == (3, 5)


def test_refine_candidates(tmp_path):
    vs = make_vs(factory_string="IVF4,PQ2,Refine(Flat)", k_factor=2.5)
    with pytest.raises(ValueError, match="not loaded"):
        vs.refine_candidates(10)
    vs.index(None, clustered(300, 8), str(tmp_path / "big"))
    want = {(1, 1): 1, (1, 2.5): 3, (1, 5): 5, (1, 100): 56, (10, 1): 10, (10, 2.5): 25, (10, 5): 50, (10, 100): 56,
            (14, 1): 14, (14, 2.5): 35, (14, 5): 56, (14, 100): 56, (56, 1): 56, (56, 2.5): 56, (56, 5): 56, (56, 100): 56}
    for (K, f), kc in want.items():
        assert vs.refine_candidates(K, f) == kc == min(max(K, math.ceil(K * f)), 56, 300), (K, f)
    assert vs.refine_candidates(10) == 25 and vs.refine_candidates(3) == 8  # the store's own factor; ceil(7.5)
    assert vs.refine_candidates(60, 1) == 56  # (such a K is searched exactly: the count is the scan's bound)
    for bad in (0, -1, 2.5, "3", True, None):
        with pytest.raises(ValueError, match="K must"):
            vs.refine_candidates(bad)
    vs.index(None, clustered(40, 8), str(tmp_path / "small"))  # fewer rows than candidates
    assert vs.refine_candidates(10, 5) == 40 and vs.refine_candidates(10, 3) == 30 and vs.refine_candidates(14, 100) == 40


# ---- search and routing --------------------------------------------------------------------------------------------------
def _pair(tmp_path, codec, metric, xb, k_factor, nprobe=3):
    """A refined store and a plain store of the same codec on one directory (the plain one loads what the refined one wrote)."""
    d = str(tmp_path / f"{codec}-{metric}")
    vr = make_vs(factory_string=f"IVF16,{codec},Refine(Flat)", nprobe=nprobe, metric=metric, k_factor=k_factor)
    vr.index(None, xb, d)
    vp = make_vs(factory_string=f"IVF16,{codec}", nprobe=nprobe, metric=metric)
    vp.load_index(d)
    return vr, vp


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
@pytest.mark.parametrize("codec", list(CODECS))
def test_refined_search_is_the_exact_top_k_of_the_plain_stores_candidates(tmp_path, rows, codec, metric):
    xb, xq = rows
    K = 10
    vr, vp = _pair(tmp_path, codec, metric, xb, k_factor=5)
    kc = vr.refine_candidates(K)
    assert kc == 50
    vr.backend.calls.clear()
    out = vr(xq, K)
    first, second = [c for c in vr.backend.calls if c[0] in (CODECS[codec], "refine_keys")]
    assert first == (CODECS[codec], len(xq), kc, 3) and second == ("refine_keys", len(xq), kc, K)  # the scan at kc, then the re-rank
    cand = vp(xq, kc).indices
    xb_s, xq_s = stored(vr, xb), stored(vr, xq)
    D_ref, I_ref = refine_reference(xb_s, xq_s, cand, K, metric)
    err, hard, _ = synth.compare_topk(D_ref, I_ref, out.distances, out.indices, atol=BAR, tie_gap=TIE_GAP)
    print(f"{codec} metric={metric}: max score error {err:.3e}, hard id mismatches {hard}")
    assert err <= BAR and hard == 0
    assert out.distances.dtype == np.float32 and out.indices.dtype == np.int64
    # every returned row is one of the query's candidates, and its distance is that row's exact one
    for q in range(len(xq)):
        assert set(out.indices[q]) <= set(cand[q])
        s = exact_scores(xb_s, xq_s[q], out.indices[q], metric)
        assert np.abs((s if metric == METRIC_INNER_PRODUCT else -s) - out.distances[q]).max() <= BAR
    # a per-call factor overrides the store's
    vr.backend.calls.clear()
    vr(xq, K, k_factor=2)
    assert (CODECS[codec], len(xq), 20, 3) in vr.backend.calls and ("refine_keys", len(xq), 20, K) in vr.backend.calls
    # the codes' accessors are the plain store's
    assert np.array_equal(vr.ivf_probe(xq), vp.ivf_probe(xq))
    codes = (lambda v: v.pq_codes()) if codec == "PQ8" else (lambda v: v.sq8_codes())
    for a, b in zip(codes(vr), codes(vp)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
@pytest.mark.parametrize("codec", list(CODECS))
def test_k_factor_one_reorders_the_plain_stores_answer(tmp_path, rows, codec, metric):
    xb, xq = rows
    K = 10
    vr, vp = _pair(tmp_path, codec, metric, xb, k_factor=1)
    out, plain = vr(xq, K), vp(xq, K)
    xb_s, xq_s = stored(vr, xb), stored(vr, xq)
    D_ref, I_ref = refine_reference(xb_s, xq_s, plain.indices, K, metric)
    for q in range(len(xq)):
        assert set(out.indices[q]) == set(plain.indices[q])  # the same rows ...
    err, hard, _ = synth.compare_topk(D_ref, I_ref, out.distances, out.indices, atol=BAR, tie_gap=TIE_GAP)
    assert err <= BAR and hard == 0  # ... ordered by exact score, with exact distances
    better = out.distances if metric == METRIC_INNER_PRODUCT else -out.distances
    assert (np.diff(better, axis=1) <= 0).all()


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
@pytest.mark.parametrize("codec", list(CODECS))
def test_refinement_keeps_every_true_neighbour_among_the_candidates(tmp_path, rows, codec, metric):
    """refined & T == C & T per query (T: the exact top K over all rows, C: the candidates) outside the tie gap at the K-th
    candidate score, so recall@K never falls below the plain store's."""
    xb, xq = rows
    K = 10
    vr, vp = _pair(tmp_path, codec, metric, xb, k_factor=5)
    kc = vr.refine_candidates(K)
    out, cand, plain = vr(xq, K).indices, vp(xq, kc).indices, vp(xq, K).indices
    xb_s, xq_s = stored(vr, xb), stored(vr, xq)
    T = oracle.flat_search(xb_s.astype(np.float32), xq_s.astype(np.float32), K, metric)[1]
    kept = lost_plain = 0
    for q in range(len(xq)):
        C, R, Tq = set(cand[q][cand[q] >= 0]), set(out[q][out[q] >= 0]), set(T[q])
        assert R <= C and R & Tq <= C & Tq
        ids = np.array(sorted(C))
        s = exact_scores(xb_s, xq_s[q], ids, metric)
        kth = np.sort(s)[::-1][min(K, len(s)) - 1]
        clear = {int(i) for i, v in zip(ids, s) if v > kth + TIE_GAP}  # candidates clearly above the K-th candidate score
        assert (C & Tq) & clear <= R, (q, sorted((C & Tq) & clear - R))
        near = (C & Tq) - clear - R  # inside the tie gap and not returned: excused
        assert len(near) <= 1
        assert len(R & Tq) >= len(set(plain[q]) & Tq) - len(near)
        kept += len(R & Tq)
        lost_plain += len(set(plain[q]) & Tq)
    assert kept > lost_plain  # and on these rows the re-ranking does find more of them


def test_directories_are_interchangeable(tmp_path, rows, monkeypatch):
    xb, xq = rows
    for codec, side in (("PQ8", "ivf_pq.npz"), ("SQ8", "ivf_sq8.npz")):
        d1, d2 = str(tmp_path / f"r-{codec}"), str(tmp_path / f"p-{codec}")
        vr = make_vs(factory_string=f"IVF16,{codec},Refine(Flat)", nprobe=3, k_factor=5)
        vr.index(None, xb, d1)
        vp = make_vs(factory_string=f"IVF16,{codec}", nprobe=3)
        vp.index(None, xb, d2)
        assert sorted(os.listdir(d1)) == sorted(os.listdir(d2)) == sorted(["index", "ivf.npz", side, "rows.json", "vecs"])
        for name in ("ivf.npz", side):  # the same arrays under the same names
            with np.load(os.path.join(d1, name), allow_pickle=False) as a, np.load(os.path.join(d2, name), allow_pickle=False) as b:
                assert set(a.files) == set(b.files)
                for f in set(a.files) - {"header"}:  # (the header names the directory's own files)
                    assert np.array_equal(a[f], b[f]), (name, f)
        _no_kmeans(monkeypatch)
        a = make_vs(factory_string=f"IVF16,{codec}", nprobe=3)
        a.load_index(d1)  # a plain store on the refined store's directory
        b = make_vs(factory_string=f"IVF16,{codec},Refine(Flat)", nprobe=3, k_factor=5)
        b.load_index(d2)  # and the other way round
        for v in (a, b):
            assert not [c for c in v.backend.calls if c[0].endswith("_train")]
            assert ({"PQ8": "ivf_pq_encode", "SQ8": "ivf_sq8_encode"}[codec], True) in v.backend.calls  # uploaded, not encoded
        assert sorted(os.listdir(d1)) == sorted(os.listdir(d2)) == sorted(["index", "ivf.npz", side, "rows.json", "vecs"])
        r1, r2 = vr(xq, 10), b(xq, 10)
        assert np.array_equal(r1.indices, r2.indices) and np.array_equal(r1.distances, r2.distances)
        p1, p2 = vp(xq, 10), a(xq, 10)
        assert np.array_equal(p1.indices, p2.indices) and np.array_equal(p1.distances, p2.distances)
        monkeypatch.undo()


@pytest.mark.parametrize("codec", list(CODECS))
def test_fallbacks_take_the_exact_path(tmp_path, rows, codec):
    xb, xq = rows
    vs = make_vs(factory_string=f"IVF16,{codec},Refine(Flat)", nprobe=3, k_factor=5)
    vs.index(None, xb, str(tmp_path / "i"))
    flat = make_vs()
    flat.load_index(str(tmp_path / "i"))
    be = vs.backend
    be.calls.clear()
    ids = list(range(0, 2000, 3))
    for kw in (dict(K=5, ids=ids), dict(K=57), dict(K=2000), dict(K=2500)):
        a, b = vs(xq, **kw), flat(xq, **kw)
        assert np.array_equal(a.indices, b.indices) and np.array_equal(a.distances, b.distances), kw
    assert not [c for c in be.calls if c[0] in ("ivf_search", "ivf_sq8_search", "ivf_pq_search", "refine_keys")]
    vs(xq, 56)
    assert [c for c in be.calls if c[0] in (CODECS[codec], "refine_keys")] == [(CODECS[codec], len(xq), 56, 3),
                                                                               ("refine_keys", len(xq), 56, 56)]


def test_a_scan_that_does_not_take_kc_leaves_the_call_exact(tmp_path):
    """The SQ8 scan takes d = 2 400 up to k = 32 only: K = 10 at k_factor 5 asks it for 50 candidates - the call is exact, as
    for any shape the scan does not fit - while k_factor 3 (30 candidates) is served and re-ranked."""
    xb, xq = clustered(60, 2400, centers=3), clustered(2, 2400, centers=3, seed=6)
    vs = make_vs(factory_string="IVF3,SQ8,Refine(Flat)", nprobe=1, k_factor=5, ivf_niter=2)
    vs.index(None, xb, str(tmp_path / "i"))
    be = vs.backend
    assert be.ivf_sq8_fits(2400, 10, _capi.PACK_SPLIT) and be.ivf_sq8_fits(2400, 30, _capi.PACK_SPLIT)
    assert not be.ivf_sq8_fits(2400, 50, _capi.PACK_SPLIT)
    be.calls.clear()
    out = vs(xq, 10)
    assert not [c for c in be.calls if c[0] in ("ivf_sq8_search", "refine_keys")]
    flat = make_vs()
    flat.load_index(str(tmp_path / "i"))
    assert np.array_equal(out.indices, flat(xq, 10).indices)
    vs(xq, 10, k_factor=3)
    assert [c for c in be.calls if c[0] in ("ivf_sq8_search", "refine_keys")] == [("ivf_sq8_search", 2, 30, 1), ("refine_keys", 2, 30, 10)]


def test_l2_refuses_unequal_pack_exponents():
    be = RefineOracleBackend()
    xb, xq = clustered(50, 8), clustered(2, 8, seed=2)
    corpus, queries = be.pack(xb, _capi.PACK_SPLIT, exp=3), be.pack(xq, _capi.PACK_SPLIT, exp=0)
    cand = be.search_keys(corpus, queries, 5, 0)
    with pytest.raises(ValueError, match="scale exponent"):
        be.refine_keys(corpus, queries, cand, 3, 1)
    assert be.refine_keys(corpus, queries, cand, 3, 0).shape == (2, 3)  # inner products take any pair of exponents


# ---- C entry point -------------------------------------------------------------------------------------------------------
def test_refine_entry_point_validates_before_device_work():
    lib = _capi.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its argument checks first
    args = dict(xb=p, xb_pack=0, nb=1000, xbn=None, xq=p, xq_pack=0, nq=4, xqn=None, d=64, metric=0, cand=p, kc=50, k=10, out=p,
                st=None)

    def call(**kw):
        return lib.lvs_refine_keys(*dict(args, **kw).values())

    for kw, msg in ((dict(metric=2), b"metric"), (dict(metric=-1), b"metric"), (dict(xb_pack=2), b"xb_pack"),
                    (dict(xq_pack=5), b"xq_pack"), (dict(d=0), b"shape"), (dict(d=-3), b"shape"), (dict(nb=-1), b"shape"),
                    (dict(nq=-1), b"shape"), (dict(nb=1 << 32), b"shape"), (dict(k=0), b"k=0"), (dict(k=-1), b"k=-1"),
                    (dict(k=51), b"k=51"), (dict(kc=65, k=65), b"kc=65"), (dict(kc=65), b"kc=65"), (dict(kc=0, k=0), b"kc=0"),
                    (dict(out=None), b"NULL"), (dict(cand=None), b"NULL"), (dict(xq=None), b"NULL"), (dict(xb=None), b"NULL"),
                    (dict(metric=1), b"norms"), (dict(metric=1, xbn=p), b"norms"), (dict(metric=1, xqn=p), b"norms")):
        assert call(**kw) == _capi.EINVAL, kw
        assert msg in lib.lvs_last_error(), (kw, lib.lvs_last_error())
    # no queries: nothing to do, whatever the buffers - but the arguments are still checked
    null = dict(xb=None, xq=None, cand=None, out=None, nq=0)
    assert call(**null) == _capi.OK and call(**null, metric=1) == _capi.OK and call(**null, kc=64, k=64) == _capi.OK
    for kw in (dict(metric=3), dict(xb_pack=9), dict(xq_pack=9), dict(d=0), dict(k=0), dict(k=51), dict(kc=65)):
        assert call(**null, **kw) == _capi.EINVAL, kw
    assert lib.lvs_abi_version() == 7
