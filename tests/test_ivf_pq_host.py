"""Host side of the IVF-PQ mode of HipVS (factory strings, routing, the ``ivf_pq.npz`` sidecar, the codec rules and the C entry
points' argument checks), on the CPU with the oracle-backed double of tests/ivf_pq_oracle_backend.py.  The device path is
covered by tests/test_gpu_ivf_pq.py."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import plan_native
from ivf_pq_oracle_backend import PqOracleBackend, list_of_rows, pq_decode, pq_encode, pq_reference, pq_residuals
from ivf_sq8_oracle_backend import Sq8OracleBackend
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi, store
from oracle_backend import _emulate_storage


def make_vs(**kw):
    return HipVS(backend=PqOracleBackend(), **kw)


def clustered(n, d, centers=12, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32) * 3
    x = c[rng.integers(0, centers, n)] + rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32)


def _no_kmeans(monkeypatch):
    from lotus_amd import cluster

    def boom(*a, **k):
        raise AssertionError("k-means was called")

    monkeypatch.setattr(cluster, "kmeans", boom)


def decoded(vs):
    c, off, rows = vs.ivf_lists()
    books, codes, _ = vs.pq_codes()
    return pq_decode(c, list_of_rows(off, rows, codes.shape[0]), books, codes)


def reference(vs, xq, k, nprobe=None):
    """The float64 search over the decoded rows of the probed lists, from the store's own accessors."""
    _, off, rows = vs.ivf_lists()
    probe = vs.ivf_probe(xq, nprobe)
    return pq_reference(decoded(vs), _emulate_storage(xq, _capi.PACK_SPLIT), k, vs.metric, off, rows, probe)


# ---- factory strings ---------------------------------------------------------------------------------------------------
def test_factory_string_parsing():
    for fs, M in (("IVF16,PQ8", 8), ("IVF16,PQ8x8", 8), ("IVF4096,PQ64", 64), ("IVF1,PQ1", 1), ("IVF16,PQ96x8", 96)):
        vs = make_vs(factory_string=fs, nprobe=4)
        assert vs._nlist == int(fs[3:fs.index(",")]) and vs._mode.M == M and vs._mode.kind != "SQ8"
    assert make_vs(factory_string="IVF16,SQ8")._mode.M is None
    for bad in ("IVF16,PQ16x4", "IVF16,PQ16x4fs", "IVF16,PQ8x8fs", "IVF16,PQ0", "IVF16,PQ0x8", "IVF16,PQ", "IVF0,PQ8",
                "IVF16,PQ8x", "IVF16,PQ8x16", "IVF16,pq8", "IVF16,PQ8 ", "IVF16,PQ8,RFlat", "OPQ8,IVF16,PQ8", "PQ8"):
        with pytest.raises(ValueError, match="PQ<M>"):
            make_vs(factory_string=bad)


def test_backend_without_the_pq_codec_is_refused():
    with pytest.raises(ValueError, match="no IVF-PQ codec"):
        HipVS(backend=Sq8OracleBackend(), factory_string="IVF16,PQ8")


@pytest.mark.parametrize("shard", [True, "rows", "queries", "auto", (1, 2)])
def test_pq_refuses_every_shard_setting(shard):
    with pytest.raises(ValueError, match="shard"):
        make_vs(factory_string="IVF8,PQ4", shard=shard)


def test_d_must_be_divisible_by_m(tmp_path):
    vs = make_vs(factory_string="IVF4,PQ5")
    with pytest.raises(ValueError, match="divisible by M=5"):
        vs.index(None, clustered(100, 12), str(tmp_path / "i"))
    assert not os.path.exists(tmp_path / "i")
    make_vs().index(None, clustered(100, 12), str(tmp_path / "flat"))
    with pytest.raises(ValueError, match="divisible by M=5"):
        vs.load_index(str(tmp_path / "flat"))


# ---- the codec -----------------------------------------------------------------------------------------------------------
def test_codec_rules():
    # argmin with ties to the smaller j, beta = |rhat|^2 + 2 <c, rhat>
    books = np.zeros((2, 3, 2), np.float32)
    books[0] = [[1, 0], [-1, 0], [1, 0]]   # entries 0 and 2 identical: a tie
    books[1] = [[0, 0], [0, 2], [0, -2]]
    x = np.array([[1, 0, 0, 1], [3, 0, 0, 0.9], [-1, 0, 0, -1]], np.float32)
    c = np.array([[0, 0, 0, 0], [2, 0, 0, 0]], np.float32)
    where = np.array([0, 1, 0])
    codes, beta = pq_encode(x, c, where, books)
    assert codes.tolist() == [[0, 0], [0, 0], [1, 0]]  # row 0 sub 1: |1 - 0| = |1 - 2|: the smaller j; row 2 sub 1 likewise
    rh = pq_residuals(books, codes)
    assert np.allclose(beta, (rh ** 2).sum(1) + 2 * (c[where] * rh).sum(1))
    assert np.array_equal(pq_decode(c, where, books, codes), c[where] + rh)
    # fewer than 256 entries: codes stay below ksub
    rng = np.random.default_rng(2)
    books = rng.standard_normal((3, 5, 4)).astype(np.float32)
    xs = rng.standard_normal((200, 12)).astype(np.float32)
    codes, _ = pq_encode(xs, np.zeros((1, 12), np.float32), np.zeros(200, np.int64), books)
    assert codes.max() < 5 and len(np.unique(codes)) == 5


def test_small_training_sets_shrink_the_codebooks(tmp_path):
    xb = clustered(120, 8, centers=3)
    vs = make_vs(factory_string="IVF3,PQ2", nprobe=3)
    vs.index(None, xb, str(tmp_path / "i"))
    books, codes, beta = vs.pq_codes()
    assert books.shape == (2, 120, 4) and codes.shape == (120, 2) and beta.shape == (120,)  # ksub = training rows < 256
    assert int(codes.max()) < 120
    # with as many entries as training rows, every row is its own entry: the decoded rows are the rows
    assert np.allclose(decoded(vs), _emulate_storage(xb, _capi.PACK_SPLIT), atol=1e-5)


def test_pq_codes_decode_to_the_rows(tmp_path):
    xb = clustered(600, 16)
    vs = make_vs(factory_string="IVF4,PQ4", nprobe=2)
    vs.index(None, xb, str(tmp_path / "i"))
    c, off, rows = vs.ivf_lists()
    books, codes, beta = vs.pq_codes()
    assert books.shape == (4, 256, 4) and books.dtype == np.float32
    assert codes.shape == (600, 4) and codes.dtype == np.uint8 and beta.dtype == np.float32
    where = list_of_rows(off, rows, 600)
    xhat = decoded(vs)
    rh = xhat - c[where]
    assert np.allclose(beta, (rh ** 2).sum(1) + 2 * (c[where] * rh).sum(1), rtol=1e-4, atol=1e-4)
    # every code is the nearest entry of its sub-vector's residual
    xs = _emulate_storage(xb, _capi.PACK_SPLIT)
    r = xs - c[where]
    for m in range(4):
        dist = ((r[:, None, 4 * m:4 * m + 4] - books[m][None]) ** 2).sum(-1)
        assert (dist[np.arange(600), codes[:, m]] <= dist.min(1) * (1 + 1e-5) + 1e-6).all()
    # the quantizer is a real one: the decoded rows are much closer than the centroids alone
    assert ((xhat - xs) ** 2).sum() < 0.5 * ((c[where] - xs) ** 2).sum()


# ---- search and routing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_pq_search_is_the_decoded_search_over_the_probed_lists(tmp_path, metric):
    xb = clustered(600, 24)
    xq = clustered(9, 24, seed=5)
    vs = make_vs(factory_string="IVF10,PQ6", nprobe=3, metric=metric)
    vs.index(None, xb, str(tmp_path / "i"))
    out = vs(xq, 7)
    D, I = reference(vs, xq, 7)
    assert np.array_equal(out.indices, I) and np.allclose(out.distances, D, atol=1e-4)
    assert ("ivf_pq_search", 9, 7, 3) in vs.backend.calls
    assert not [c for c in vs.backend.calls if c[0] in ("ivf_search", "ivf_sq8_search")]


def test_pq_sq8_and_flat_stores_share_the_coarse_quantizer(tmp_path):
    xb = clustered(700, 20)
    xq = clustered(6, 20, seed=8)
    stores = []
    for i, fs in enumerate(("IVF9,PQ5", "IVF9,SQ8", "IVF9,Flat")):
        v = make_vs(factory_string=fs, nprobe=3)
        v.index(None, xb, str(tmp_path / str(i)))
        stores.append(v)
    for v in stores[1:]:
        for u, w in zip(stores[0].ivf_lists(), v.ivf_lists()):
            assert np.array_equal(u, w)
        assert np.array_equal(stores[0].ivf_probe(xq), v.ivf_probe(xq))


def test_fallbacks_take_the_exact_path(tmp_path):
    xb = clustered(500, 16)
    xq = clustered(3, 16, seed=9)
    vs = make_vs(factory_string="IVF8,PQ4", nprobe=1)
    vs.index(None, xb, str(tmp_path / "i"))
    xb_s, xq_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(xq, _capi.PACK_SPLIT)
    be = vs.backend
    be.calls.clear()
    ids = list(range(0, 500, 3))
    assert np.array_equal(vs(xq, 5, ids=ids).indices, oracle.flat_search(xb_s, xq_s, 5, ids=ids)[1])
    assert np.array_equal(vs(xq, 57).indices, oracle.flat_search(xb_s, xq_s, 57)[1])
    assert np.array_equal(vs(xq, 500).indices, oracle.flat_search(xb_s, xq_s, 500)[1])
    ivf_calls = ("ivf_search", "ivf_sq8_search", "ivf_pq_search")
    assert not [c for c in be.calls if c[0] in ivf_calls]
    vs(xq, 56)
    assert [c for c in be.calls if c[0] in ivf_calls] == [("ivf_pq_search", 3, 56, 1)]


@pytest.mark.parametrize("d,M,storage,served", [(3072, 96, "auto", True), (3072, 64, "fp16", True), (318, 159, "auto", True),
                                                (320, 160, "auto", False)])
def test_widths(tmp_path, d, M, storage, served, monkeypatch):
    mode = _capi.PACK_F16 if storage == "fp16" else _capi.PACK_SPLIT
    xb = clustered(60, d, centers=3)
    xq = clustered(2, d, centers=3, seed=6)
    vs = make_vs(factory_string=f"IVF3,PQ{M}", nprobe=1, storage=storage, ivf_niter=2)
    # the codebooks' training is not the subject here: one k-means iteration per subspace
    monkeypatch.setattr(PqOracleBackend, "ivf_pq_train", _quick_train)
    vs.index(None, xb, str(tmp_path / "i"))
    assert vs.backend.ivf_pq_fits(d, M, 10, mode) is served
    vs.backend.calls.clear()
    out = vs(xq, 10)
    assert bool([c for c in vs.backend.calls if c[0] == "ivf_pq_search"]) is served
    if not served:
        xb_s, xq_s = _emulate_storage(xb, mode), _emulate_storage(xq, mode)
        assert np.array_equal(out.indices, oracle.flat_search(xb_s, xq_s, 10)[1])
    assert vs.ivf_probe(xq, 2).shape == (2, 2)


def _quick_train(self, packed, lists, train_ids, M):
    """Codebooks of 16 training residual sub-vectors (a stand-in for the trained ones where only routing is tested)."""
    import torch

    x = packed.rows.numpy()
    where = list_of_rows(lists.offsets.numpy(), lists.rows.numpy().view(np.uint32), packed.n)
    r = x[:16] - lists.centroids.rows.numpy()[where[:16]]
    return torch.from_numpy(np.ascontiguousarray(r.reshape(16, M, -1).transpose(1, 0, 2)).astype(np.float32))


def test_more_than_2048_probes_are_searched_exactly(tmp_path, monkeypatch):
    monkeypatch.setattr(PqOracleBackend, "ivf_pq_train", _quick_train)
    xb = clustered(2200, 4, centers=50)
    xq = clustered(3, 4, centers=50, seed=4)
    vs = make_vs(factory_string="IVF2100,PQ2", nprobe=2049, ivf_niter=2)
    vs.index(None, xb, str(tmp_path / "i"))
    vs.backend.calls.clear()
    vs(xq, 5)
    assert not [c for c in vs.backend.calls if c[0] == "ivf_pq_search"]
    vs(xq, 5, nprobe=2048)
    assert [c for c in vs.backend.calls if c[0] == "ivf_pq_search"] == [("ivf_pq_search", 3, 5, 2048)]


def test_other_stores_have_no_pq_codes(tmp_path):
    for fs in ("IVF4,Flat", "IVF4,SQ8"):
        vs = make_vs(factory_string=fs)
        vs.index(None, clustered(100, 8), str(tmp_path / fs))
        with pytest.raises(ValueError, match="PQ"):
            vs.pq_codes()
        assert not os.path.exists(os.path.join(tmp_path, fs, store.IVF_PQ_SIDECAR))


# ---- persistence ---------------------------------------------------------------------------------------------------------
def test_sidecar_round_trip(tmp_path, monkeypatch):
    d = str(tmp_path / "pq")
    xb = clustered(400, 12)
    vs = make_vs(factory_string="IVF6,PQ3", nprobe=2, metric=METRIC_L2)
    vs.index(None, xb, d)
    assert sorted(os.listdir(d)) == ["index", "ivf.npz", "ivf_pq.npz", "rows.json", "vecs"]
    lists, codes = vs.ivf_lists(), vs.pq_codes()
    _no_kmeans(monkeypatch)
    vs2 = make_vs(factory_string="IVF6,PQ3x8", nprobe=2, metric=METRIC_L2)
    vs2.load_index(d)
    assert ("ivf_pq_encode", True) in vs2.backend.calls  # uploaded, not encoded
    for a, b in zip(lists + codes, vs2.ivf_lists() + vs2.pq_codes()):
        assert np.array_equal(a, b)
    q = clustered(5, 12, seed=8)
    r1, r2 = vs(q, 4), vs2(q, 4)
    assert np.array_equal(r1.indices, r2.indices) and np.array_equal(r1.distances, r2.distances)
    with np.load(os.path.join(d, store.IVF_PQ_SIDECAR), allow_pickle=False) as z:
        assert set(z.files) == {"header", "codebooks", "codes", "beta"}
    # the same directory as an IVF-Flat store of the same nlist: ivf.npz is reused; and as a flat store
    f = make_vs(factory_string="IVF6,Flat", nprobe=2, metric=METRIC_L2)
    f.load_index(d)
    for a, b in zip(lists, f.ivf_lists()):
        assert np.array_equal(a, b)
    flat = make_vs(metric=METRIC_L2)
    flat.load_index(d)
    xb_s, q_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(q, _capi.PACK_SPLIT)
    assert np.array_equal(flat(q, 4).indices, oracle.flat_search(xb_s, q_s, 4, METRIC_L2)[1])


@pytest.mark.parametrize("change", ["vecs", "pq-missing", "pq-garbage", "ivf-missing", "lists", "other-M"])
def test_stale_or_foreign_sidecar_retrains(tmp_path, change):
    d = str(tmp_path / "pq")
    xb = clustered(300, 10)
    make_vs(factory_string="IVF5,PQ2").index(None, xb, d)
    side = os.path.join(d, store.IVF_PQ_SIDECAR)
    M = 2
    if change == "vecs":  # another writer re-indexed the directory with other rows of the same shape
        make_vs().index(None, clustered(300, 10, seed=77), str(tmp_path / "other"))
        for name in ("vecs", "index"):
            with open(os.path.join(tmp_path, "other", name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
                dst.write(src.read())
        os.remove(os.path.join(d, "rows.json"))
    elif change == "pq-missing":
        os.remove(side)
    elif change == "pq-garbage":
        with open(side, "wb") as fp:
            fp.write(b"not an npz")
    elif change == "ivf-missing":
        os.remove(os.path.join(d, store.IVF_SIDECAR))
    elif change == "lists":  # an IVF-Flat store with other training settings rewrote ivf.npz: the codes belong to other lists
        make_vs(factory_string="IVF5,Flat", ivf_niter=1, ivf_max_points_per_centroid=4).index(None, xb, str(tmp_path / "o"))
        o = make_vs(factory_string="IVF5,Flat", ivf_niter=1, ivf_max_points_per_centroid=4)
        o.load_index(str(tmp_path / "o"))
        c, off, rows = o.ivf_lists()
        store.write_ivf(d, 5, 0, _capi.PACK_SPLIT, c, off, rows)
    else:  # a store of another M reads the directory
        M = 5
    vs = make_vs(factory_string=f"IVF5,PQ{M}")
    vs.load_index(d)
    assert ("ivf_pq_encode", False) in vs.backend.calls  # encoded afresh
    assert vs.pq_codes()[1].shape == (300, M)
    # ... and the rewritten sidecars are valid for the next load
    side_ivf = store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300)
    assert side_ivf is not None
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_SPLIT, vs._current().packed.exp, 10, M, 300,
                             store.ivf_digest(*side_ivf)) is not None


def test_touched_files_void_the_pq_sidecar(tmp_path):
    d = str(tmp_path / "pq")
    vs = make_vs(factory_string="IVF5,PQ2")
    vs.index(None, clustered(300, 10), d)
    exp = vs._current().packed.exp
    dig = store.ivf_digest(*store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300))
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 2, 300, dig) is not None
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_SPLIT, exp + 1, 10, 2, 300, dig) is None
    assert store.read_ivf_pq(d, 5, 1, _capi.PACK_SPLIT, exp, 10, 2, 300, dig) is None
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_F16, exp, 10, 2, 300, dig) is None
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 5, 300, dig) is None
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 2, 300, "0" * 64) is None
    st = os.stat(os.path.join(d, "vecs"))
    os.utime(os.path.join(d, "vecs"), ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))
    assert store.read_ivf_pq(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 2, 300, dig) is None


# ---- C entry points ------------------------------------------------------------------------------------------------------
def test_pq_entry_points_validate_before_device_work():
    lib = _capi.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its argument checks first
    args = dict(codes=p, beta=None, books=p, M=8, ksub=256, off=p, rows=p, nb=1000, nlist=16, c=p, c_pack=0, cn=None, c32=p,
                xq=p, xq_pack=0, nq=4, xqn=None, d=64, metric=0, nprobe=4, k=10, out=p, probe=None, ws=p, wsb=1 << 20, st=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.lvs_ivf_pq_search_keys(*a.values())

    for kw, msg in ((dict(metric=3), b"metric"), (dict(nprobe=0), b"nprobe"), (dict(nprobe=17), b"nprobe"),
                    (dict(k=0), b"k="), (dict(k=57), b"k="), (dict(xq_pack=5), b"xq_pack"), (dict(c_pack=5), b"c_pack"),
                    (dict(nlist=0), b"nlist"), (dict(out=None), b"NULL"), (dict(codes=None), b"NULL"),
                    (dict(books=None), b"NULL"), (dict(c32=None), b"NULL"), (dict(metric=1), b"norms"),
                    (dict(d=0), b"shape"), (dict(M=0), b"M="), (dict(M=7), b"M="), (dict(ksub=0), b"ksub"),
                    (dict(ksub=257), b"ksub")):
        assert call(**kw) == _capi.EINVAL, kw
        assert msg in lib.lvs_last_error(), (kw, lib.lvs_last_error())
    assert call(wsb=16) == _capi.ENOMEM and b"workspace" in lib.lvs_last_error()
    assert call(nq=0) == _capi.OK
    assert call(d=320, M=160) == _capi.EUNSUPPORTED and b"LDS" in lib.lvs_last_error()
    enc = dict(xb=p, xb_pack=0, n=100, d=64, off=p, rows=p, nlist=4, c=p, M=8, ksub=256, books=p, codes=p, beta=p, st=None)
    for kw in (dict(xb_pack=3), dict(n=-1), dict(d=0), dict(nlist=0), dict(M=0), dict(M=6), dict(ksub=0), dict(ksub=300),
               dict(codes=None), dict(books=None), dict(beta=None), dict(c=None)):
        assert lib.lvs_ivf_pq_encode(*dict(enc, **kw).values()) == _capi.EINVAL, kw
    assert lib.lvs_ivf_pq_encode(*dict(enc, n=0).values()) == _capi.OK


def test_pq_workspace_sizes_and_widths():
    lib = _capi.load()
    for d, M, k in ((3072, 96, 56), (3072, 64, 10), (768, 64, 56), (1536, 128, 1), (318, 159, 56), (128, 1, 10)):
        for pack in (0, 1):
            assert lib.lvs_ivf_pq_search_workspace_bytes(10, 64, 4, d, M, k, pack) > 0, (d, M, k, pack)
    for d, M, k in ((320, 160, 1), (3072, 192, 10), (1536, 256, 56)):
        assert lib.lvs_ivf_pq_search_workspace_bytes(10, 64, 4, d, M, k, 1) == _capi.EUNSUPPORTED
    # the per-query tables are part of the scratch: chunked within 512 MB
    big = lib.lvs_ivf_pq_search_workspace_bytes(1_000_000, 4096, 32, 3072, 96, 56, _capi.PACK_SPLIT)
    assert 0 < big <= plan_native.ivf_limits()[0]
    one = lib.lvs_ivf_pq_search_workspace_bytes(1, 16, 4, 768, 64, 10, _capi.PACK_F16)
    assert one >= 64 * 256 * 4
    for bad in ((-1, 16, 4, 64, 8, 10, 0), (10, 0, 1, 64, 8, 10, 0), (10, 16, 17, 64, 8, 10, 0), (10, 16, 4, 0, 8, 10, 0),
                (10, 16, 4, 64, 8, 57, 0), (10, 16, 4, 64, 8, 10, 7), (10, 16, 4, 64, 0, 10, 0), (10, 16, 4, 64, 7, 10, 0)):
        assert lib.lvs_ivf_pq_search_workspace_bytes(*bad) < 0, bad
