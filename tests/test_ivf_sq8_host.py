"""Host side of the IVF-SQ8 mode of HipVS (factory strings, routing, the ``ivf_sq8.npz`` sidecar, the codec rules and the C
entry points' argument checks), on the CPU with the oracle-backed double of tests/ivf_sq8_oracle_backend.py.  The device
path is covered by tests/test_gpu_ivf_sq8.py."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import plan_native
from ivf_sq8_oracle_backend import (Sq8OracleBackend, list_of_rows, sq8_decode, sq8_encode, sq8_reference, sq8_train)
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi, store
from oracle_backend import _emulate_storage


def make_vs(**kw):
    return HipVS(backend=Sq8OracleBackend(), **kw)


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


def reference(vs, xq, k, nprobe=None):
    """The float64 search over the decoded rows of the probed lists, from the store's own accessors."""
    c, off, rows = vs.ivf_lists()
    vmin, vdiff, codes, _ = vs.sq8_codes()
    xhat = sq8_decode(c, list_of_rows(off, rows, codes.shape[0]), vmin, vdiff, codes)
    probe = vs.ivf_probe(xq, nprobe)
    return sq8_reference(xhat, _emulate_storage(xq, _capi.PACK_SPLIT), k, vs.metric, off, rows, probe)


# ---- factory strings ---------------------------------------------------------------------------------------------------
def test_factory_string_parsing():
    vs = make_vs(factory_string="IVF16,SQ8", nprobe=4)
    assert vs._nlist == 16 and vs._mode.kind == "SQ8" and vs.nprobe == 4
    assert make_vs(factory_string="IVF16,Flat")._mode.kind != "SQ8"
    for bad in ("SQ8", "IVF16,SQ4", "IVF16,SQ8 ", "IVF0,SQ8", "IVF,SQ8", "IVF16,sq8", "IVF16,SQ8,Flat", "IVF16,PQ8", "HNSW32"):
        with pytest.raises(ValueError, match="'Flat' or 'IVF<nlist>,Flat' or 'IVF<nlist>,SQ8'"):
            make_vs(factory_string=bad)


@pytest.mark.parametrize("shard", [True, "rows", "queries", "auto", (1, 2)])
def test_sq8_refuses_every_shard_setting(shard):
    with pytest.raises(ValueError, match="shard"):
        make_vs(factory_string="IVF8,SQ8", shard=shard)


# ---- the codec -----------------------------------------------------------------------------------------------------------
def test_codec_rules():
    rng = np.random.default_rng(1)
    n, d = 200, 6
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 2] = 0.25  # a constant dimension: vdiff = 0
    c = np.zeros((1, d), np.float32)
    where = np.zeros(n, np.int64)
    train = np.arange(0, n, 2)
    vmin, vdiff = sq8_train(x, c, where, train)
    assert vdiff[2] == 0 and vmin[2] == np.float32(0.25)
    codes, rn = sq8_encode(x, c, where, vmin, vdiff)
    assert (codes[:, 2] == 0).all()
    xhat = sq8_decode(c, where, vmin, vdiff, codes)
    assert (xhat[:, 2] == 0.25).all()  # vdiff = 0 decodes to vmin
    # the training extremes: vmin -> code 0, vmax -> 255 (truncation), every decoded training value within half a cell
    tr = x[train]
    for j in (0, 1, 3):
        assert codes[train][np.argmin(tr[:, j]), j] == 0 and codes[train][np.argmax(tr[:, j]), j] == 255
        assert np.abs(xhat[train, j] - tr[:, j]).max() <= vdiff[j] / 255 * 0.5 * (1 + 1e-5) + 1e-6
    # rows outside the training range clamp to the end codes
    out = x[1::2]
    lo, hi = out < vmin, out > vmin + vdiff
    assert (lo[:, [0, 1, 3]].any() or hi[:, [0, 1, 3]].any())
    assert (codes[1::2][lo & (vdiff > 0)] == 0).all() and (codes[1::2][hi & (vdiff > 0)] == 255).all()
    # the stored norm is |rhat|^2 of the decoded residual
    assert np.allclose(rn, ((xhat - c[where]) ** 2).sum(axis=1), rtol=1e-6)


def test_sq8_codes_decode_to_the_rows(tmp_path):
    xb = clustered(500, 16)
    vs = make_vs(factory_string="IVF8,SQ8", nprobe=2)
    vs.index(None, xb, str(tmp_path / "i"))
    c, off, rows = vs.ivf_lists()
    vmin, vdiff, codes, rn = vs.sq8_codes()
    assert codes.shape == (500, 16) and codes.dtype == np.uint8 and rn.shape == (500,)
    where = list_of_rows(off, rows, 500)
    xhat = sq8_decode(c, where, vmin, vdiff, codes)
    xs = _emulate_storage(xb, _capi.PACK_SPLIT)
    # every row is a training row here (500 < 8 x 256): each decodes within half a cell of its stored value
    assert (np.abs(xhat - xs) <= vdiff / 255 * 0.5 * (1 + 1e-4) + 1e-6).all()
    assert np.allclose(rn, ((xhat - c[where]) ** 2).sum(axis=1), rtol=1e-5)


# ---- search and routing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_sq8_search_is_the_decoded_search_over_the_probed_lists(tmp_path, metric):
    xb = clustered(600, 24)
    xq = clustered(9, 24, seed=5)
    vs = make_vs(factory_string="IVF10,SQ8", nprobe=3, metric=metric)
    vs.index(None, xb, str(tmp_path / "i"))
    out = vs(xq, 7)
    D, I = reference(vs, xq, 7)
    assert np.array_equal(out.indices, I) and np.allclose(out.distances, D, atol=1e-4)
    assert ("ivf_sq8_search", 9, 7, 3) in vs.backend.calls
    assert not [c for c in vs.backend.calls if c[0] == "ivf_search"]


def test_sq8_and_flat_stores_share_the_coarse_quantizer(tmp_path):
    xb = clustered(700, 20)
    xq = clustered(6, 20, seed=8)
    a = make_vs(factory_string="IVF9,SQ8", nprobe=3)
    a.index(None, xb, str(tmp_path / "a"))
    b = make_vs(factory_string="IVF9,Flat", nprobe=3)
    b.index(None, xb, str(tmp_path / "b"))
    for u, v in zip(a.ivf_lists(), b.ivf_lists()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.ivf_probe(xq), b.ivf_probe(xq))


def test_fallbacks_take_the_exact_path(tmp_path):
    xb = clustered(500, 16)
    xq = clustered(3, 16, seed=9)
    vs = make_vs(factory_string="IVF8,SQ8", nprobe=1)
    vs.index(None, xb, str(tmp_path / "i"))
    xb_s, xq_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(xq, _capi.PACK_SPLIT)
    be = vs.backend
    be.calls.clear()
    ids = list(range(0, 500, 3))
    assert np.array_equal(vs(xq, 5, ids=ids).indices, oracle.flat_search(xb_s, xq_s, 5, ids=ids)[1])
    assert np.array_equal(vs(xq, 57).indices, oracle.flat_search(xb_s, xq_s, 57)[1])
    assert np.array_equal(vs(xq, 500).indices, oracle.flat_search(xb_s, xq_s, 500)[1])
    assert not [c for c in be.calls if c[0] in ("ivf_search", "ivf_sq8_search")]
    vs(xq, 56)
    assert [c for c in be.calls if c[0] in ("ivf_search", "ivf_sq8_search")] == [("ivf_sq8_search", 3, 56, 1)]


@pytest.mark.parametrize("d,storage,served", [(1536, "auto", True), (1536, "fp16", True), (2368, "auto", True),
                                              (3072, "auto", False)])
def test_widths(tmp_path, d, storage, served):
    xb = clustered(120, d, centers=4)
    xq = clustered(2, d, centers=4, seed=6)
    vs = make_vs(factory_string="IVF4,SQ8", nprobe=1, storage=storage, ivf_niter=2)
    vs.index(None, xb, str(tmp_path / "i"))
    mode = _capi.PACK_F16 if storage == "fp16" else _capi.PACK_SPLIT
    assert vs.backend.ivf_sq8_fits(d, 10, mode) is served
    vs.backend.calls.clear()
    out = vs(xq, 10)
    assert bool([c for c in vs.backend.calls if c[0] == "ivf_sq8_search"]) is served
    if not served:
        xb_s, xq_s = _emulate_storage(xb, mode), _emulate_storage(xq, mode)
        assert np.array_equal(out.indices, oracle.flat_search(xb_s, xq_s, 10)[1])
    assert vs.ivf_probe(xq, 2).shape == (2, 2)


def test_more_than_2048_probes_are_searched_exactly(tmp_path):
    xb = clustered(2200, 4, centers=50)
    xq = clustered(3, 4, centers=50, seed=4)
    vs = make_vs(factory_string="IVF2100,SQ8", nprobe=2049, ivf_niter=2)
    vs.index(None, xb, str(tmp_path / "i"))
    vs.backend.calls.clear()
    vs(xq, 5)
    assert not [c for c in vs.backend.calls if c[0] == "ivf_sq8_search"]
    vs(xq, 5, nprobe=2048)
    assert [c for c in vs.backend.calls if c[0] == "ivf_sq8_search"] == [("ivf_sq8_search", 3, 5, 2048)]


def test_flat_store_has_no_sq8_codes(tmp_path):
    vs = make_vs(factory_string="IVF4,Flat")
    vs.index(None, clustered(100, 8), str(tmp_path / "i"))
    with pytest.raises(ValueError, match="SQ8"):
        vs.sq8_codes()
    assert not os.path.exists(os.path.join(tmp_path, "i", store.IVF_SQ8_SIDECAR))


# ---- persistence ---------------------------------------------------------------------------------------------------------
def test_sidecar_round_trip(tmp_path, monkeypatch):
    d = str(tmp_path / "sq8")
    xb = clustered(400, 12)
    vs = make_vs(factory_string="IVF6,SQ8", nprobe=2, metric=METRIC_L2)
    vs.index(None, xb, d)
    assert sorted(os.listdir(d)) == ["index", "ivf.npz", "ivf_sq8.npz", "rows.json", "vecs"]
    lists, codes = vs.ivf_lists(), vs.sq8_codes()
    _no_kmeans(monkeypatch)
    vs2 = make_vs(factory_string="IVF6,SQ8", nprobe=2, metric=METRIC_L2)
    vs2.load_index(d)
    assert ("ivf_sq8_encode", True) in vs2.backend.calls  # uploaded, not encoded
    for a, b in zip(lists + codes, vs2.ivf_lists() + vs2.sq8_codes()):
        assert np.array_equal(a, b)
    q = clustered(5, 12, seed=8)
    assert np.array_equal(vs(q, 4).indices, vs2(q, 4).indices)
    with np.load(os.path.join(d, store.IVF_SQ8_SIDECAR), allow_pickle=False) as z:
        assert set(z.files) == {"header", "vmin", "vdiff", "codes", "rnorm"}
    # the same directory as an IVF-Flat store of the same nlist: ivf.npz is reused; and as a flat store
    f = make_vs(factory_string="IVF6,Flat", nprobe=2, metric=METRIC_L2)
    f.load_index(d)
    for a, b in zip(lists, f.ivf_lists()):
        assert np.array_equal(a, b)
    flat = make_vs(metric=METRIC_L2)
    flat.load_index(d)
    xb_s, q_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(q, _capi.PACK_SPLIT)
    assert np.array_equal(flat(q, 4).indices, oracle.flat_search(xb_s, q_s, 4, METRIC_L2)[1])


@pytest.mark.parametrize("change", ["vecs", "sq8-missing", "sq8-garbage", "ivf-missing", "lists"])
def test_stale_or_foreign_sidecar_retrains(tmp_path, change):
    d = str(tmp_path / "sq8")
    xb = clustered(300, 10)
    make_vs(factory_string="IVF5,SQ8").index(None, xb, d)
    side = os.path.join(d, store.IVF_SQ8_SIDECAR)
    if change == "vecs":  # another writer re-indexed the directory with other rows of the same shape
        make_vs().index(None, clustered(300, 10, seed=77), str(tmp_path / "other"))
        for name in ("vecs", "index"):
            with open(os.path.join(tmp_path, "other", name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
                dst.write(src.read())
        os.remove(os.path.join(d, "rows.json"))
    elif change == "sq8-missing":
        os.remove(side)
    elif change == "sq8-garbage":
        with open(side, "wb") as fp:
            fp.write(b"not an npz")
    elif change == "ivf-missing":
        os.remove(os.path.join(d, store.IVF_SIDECAR))
    else:  # an IVF-Flat store with other training settings rewrote ivf.npz: the codes belong to other lists
        make_vs(factory_string="IVF5,Flat", ivf_niter=1, ivf_max_points_per_centroid=4).index(None, xb, str(tmp_path / "o"))
        o = make_vs(factory_string="IVF5,Flat", ivf_niter=1, ivf_max_points_per_centroid=4)
        o.load_index(str(tmp_path / "o"))
        c, off, rows = o.ivf_lists()
        store.write_ivf(d, 5, 0, _capi.PACK_SPLIT, c, off, rows)
    vs = make_vs(factory_string="IVF5,SQ8")
    vs.load_index(d)
    assert ("ivf_sq8_encode", False) in vs.backend.calls  # encoded afresh
    assert vs.sq8_codes()[2].shape == (300, 10)
    # ... and the rewritten sidecars are valid for the next load
    side_ivf = store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300)
    assert side_ivf is not None
    assert store.read_ivf_sq8(d, 5, 0, _capi.PACK_SPLIT, vs._current().packed.exp, 10, 300,
                              store.ivf_digest(*side_ivf)) is not None


def test_touched_files_void_the_sq8_sidecar(tmp_path):
    d = str(tmp_path / "sq8")
    vs = make_vs(factory_string="IVF5,SQ8")
    vs.index(None, clustered(300, 10), d)
    exp = vs._current().packed.exp
    dig = store.ivf_digest(*store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300))
    assert store.read_ivf_sq8(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 300, dig) is not None
    assert store.read_ivf_sq8(d, 5, 0, _capi.PACK_SPLIT, exp + 1, 10, 300, dig) is None
    assert store.read_ivf_sq8(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 300, "0" * 64) is None
    st = os.stat(os.path.join(d, "vecs"))
    os.utime(os.path.join(d, "vecs"), ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))
    assert store.read_ivf_sq8(d, 5, 0, _capi.PACK_SPLIT, exp, 10, 300, dig) is None


# ---- C entry points ------------------------------------------------------------------------------------------------------
def test_sq8_entry_points_validate_before_device_work():
    lib = _capi.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its argument checks first
    args = dict(codes=p, rn=None, vmin=p, vdiff=p, off=p, rows=p, nb=1000, nlist=16, c=p, c_pack=0, cn=None, c32=p, xq=p,
                xq_pack=0, nq=4, xqn=None, d=64, metric=0, nprobe=4, k=10, out=p, probe=None, ws=p, wsb=1 << 20, st=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.lvs_ivf_sq8_search_keys(*a.values())

    for kw, msg in ((dict(metric=3), b"metric"), (dict(nprobe=0), b"nprobe"), (dict(nprobe=17), b"nprobe"),
                    (dict(k=0), b"k="), (dict(k=57), b"k="), (dict(xq_pack=5), b"xq_pack"), (dict(c_pack=5), b"c_pack"),
                    (dict(nlist=0), b"nlist"), (dict(out=None), b"NULL"), (dict(codes=None), b"NULL"),
                    (dict(c32=None), b"NULL"), (dict(metric=1), b"norms"), (dict(d=0), b"shape")):
        assert call(**kw) == _capi.EINVAL, kw
        assert msg in lib.lvs_last_error(), (kw, lib.lvs_last_error())
    assert call(wsb=16) == _capi.ENOMEM and b"workspace" in lib.lvs_last_error()
    assert call(nq=0) == _capi.OK
    assert call(d=3072) == _capi.EUNSUPPORTED and b"LDS" in lib.lvs_last_error()
    enc = dict(xb=p, xb_pack=0, n=100, d=64, off=p, rows=p, nlist=4, c=p, vmin=p, vdiff=p, codes=p, rn=p, st=None)
    for kw in (dict(xb_pack=3), dict(n=-1), dict(d=0), dict(nlist=0), dict(codes=None), dict(vdiff=None), dict(rn=None)):
        assert lib.lvs_ivf_sq8_encode(*dict(enc, **kw).values()) == _capi.EINVAL, kw
    assert lib.lvs_ivf_sq8_encode(*dict(enc, n=0).values()) == _capi.OK


def test_sq8_workspace_sizes_and_widths():
    lib = _capi.load()
    for d, k in ((2368, 56), (2432, 32), (2432, 16), (1536, 56), (1536, 10)):
        for pack in (0, 1):
            assert lib.lvs_ivf_sq8_search_workspace_bytes(10, 64, 4, d, k, pack) > 0, (d, k, pack)
    for d, k in ((2369, 56), (2433, 32), (3072, 10)):
        assert lib.lvs_ivf_sq8_search_workspace_bytes(10, 64, 4, d, k, 1) == _capi.EUNSUPPORTED
    big = lib.lvs_ivf_sq8_search_workspace_bytes(1_000_000, 4096, 32, 1536, 56, _capi.PACK_SPLIT)
    assert 0 < big <= plan_native.ivf_limits()[0]
    for bad in ((-1, 16, 4, 64, 10, 0), (10, 0, 1, 64, 10, 0), (10, 16, 17, 64, 10, 0), (10, 16, 4, 0, 10, 0),
                (10, 16, 4, 64, 57, 0), (10, 16, 4, 64, 10, 7)):
        assert lib.lvs_ivf_sq8_search_workspace_bytes(*bad) < 0, bad
