"""Host side of the IVF-Flat mode of HipVS (factory strings, fallbacks to the exact path, the ``ivf.npz`` sidecar and the
C entry points' argument checks), on the CPU with the oracle-backed double of tests/ivf_oracle_backend.py.  The device path
is covered by tests/test_gpu_ivf.py."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import plan_native
import synth
from ivf_oracle_backend import IvfOracleBackend, ivf_reference, probe_lists
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi, store
from oracle_backend import _emulate_storage


def make_vs(**kw):
    return HipVS(backend=IvfOracleBackend(), **kw)


def clustered(n, d, centers=12, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32) * 3
    x = c[rng.integers(0, centers, n)] + rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32)


# ---- factory strings ---------------------------------------------------------------------------------------------------
def test_factory_string_parsing():
    assert make_vs().factory_string == "Flat"
    vs = make_vs(factory_string="IVF16,Flat", nprobe=4)
    assert vs._nlist == 16 and vs.nprobe == 4
    for bad in ("IVF0,Flat", "IVF,Flat", "IVF16", "IVF16,PQ8", "HNSW32", "flat", "IVF16,Flat ", "", None, 16):
        with pytest.raises(ValueError, match="'Flat' or 'IVF<nlist>,Flat'"):
            make_vs(factory_string=bad)
    for bad in (0, -1, 1.5, "4", True):
        with pytest.raises(ValueError, match="nprobe"):
            make_vs(factory_string="IVF16,Flat", nprobe=bad)


@pytest.mark.parametrize("shard", [True, "rows", "queries", "auto", (1, 2)])
def test_ivf_refuses_every_shard_setting(shard):
    with pytest.raises(ValueError, match="shard"):
        make_vs(factory_string="IVF8,Flat", shard=shard)
    make_vs(factory_string="Flat", shard=shard)  # unchanged for a flat store


# ---- search --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_ivf_search_is_exact_over_the_probed_lists(tmp_path, metric):
    xb = clustered(600, 24)
    xq = clustered(9, 24, seed=5)
    vs = make_vs(factory_string="IVF10,Flat", nprobe=3, metric=metric)
    vs.index(None, xb, str(tmp_path / "i"))
    c, off, rows = vs.ivf_lists()
    assert c.shape == (10, 24) and off[0] == 0 and off[-1] == 600 and sorted(rows.tolist()) == list(range(600))
    for l in range(10):  # ascending rows inside every list
        assert np.all(np.diff(rows[off[l]:off[l + 1]].astype(np.int64)) > 0)
    out = vs(xq, 7)
    xb_s, xq_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(xq, _capi.PACK_SPLIT)
    probe = vs.ivf_probe(xq)
    assert probe.shape == (9, 3) and np.array_equal(probe, probe_lists(c, xq_s, 3, metric))
    D, I = ivf_reference(xb_s, xq_s, 7, metric, c, off, rows, probe)
    assert np.array_equal(out.indices, I) and np.allclose(out.distances, D, atol=1e-4)
    # nprobe = nlist is the exact search; the per-call override arrives through **kwargs
    full = vs(xq, 7, nprobe=10)
    De, Ie = oracle.flat_search(xb_s, xq_s, 7, metric)
    assert np.array_equal(full.indices, Ie)
    assert vs(xq, 7, nprobe=1000).indices.tolist() == full.indices.tolist()  # clamped to nlist
    assert ("ivf_search", 9, 7, 10) in vs.backend.calls


def test_probed_lists_shorter_than_k_pad_like_faiss(tmp_path):
    xb = clustered(300, 16, centers=30)
    vs = make_vs(factory_string="IVF30,Flat", nprobe=1)
    vs.index(None, xb, str(tmp_path / "i"))
    _, off, _ = vs.ivf_lists()
    out = vs(xb[:4], 50)
    probe = vs.ivf_probe(xb[:4], 1)
    for q in range(4):
        size = int(off[probe[q, 0] + 1] - off[probe[q, 0]])
        assert size < 50
        assert (out.indices[q, :size] >= 0).all() and (out.indices[q, size:] == -1).all()
        assert (out.distances[q, size:] == -np.float32(3.4028234663852886e38)).all()


def test_fallbacks_take_the_exact_path(tmp_path):
    xb = clustered(500, 16)
    xq = clustered(3, 16, seed=9)
    vs = make_vs(factory_string="IVF8,Flat", nprobe=1)
    vs.index(None, xb, str(tmp_path / "i"))
    xb_s, xq_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(xq, _capi.PACK_SPLIT)
    be = vs.backend
    be.calls.clear()
    ids = list(range(0, 500, 3))
    out = vs(xq, 5, ids=ids)  # an ids subset
    D, I = oracle.flat_search(xb_s, xq_s, 5, ids=ids)
    assert np.array_equal(out.indices, I)
    out = vs(xq, 57)  # K beyond the one-pass list scan
    D, I = oracle.flat_search(xb_s, xq_s, 57)
    assert np.array_equal(out.indices, I)
    out = vs(xq, 500)  # K = N
    assert np.array_equal(out.indices, oracle.flat_search(xb_s, xq_s, 500)[1])
    assert not [c for c in be.calls if c[0] == "ivf_search"]
    vs(xq, 56)
    assert [c for c in be.calls if c[0] == "ivf_search"] == [("ivf_search", 3, 56, 1)]


def test_flat_store_never_touches_the_sidecar(tmp_path, monkeypatch):
    d = str(tmp_path / "flat")
    vs = make_vs()
    vs.index(None, clustered(200, 8), d)
    assert not os.path.exists(os.path.join(d, store.IVF_SIDECAR))
    monkeypatch.setattr(store, "read_ivf", lambda *a, **k: pytest.fail("a flat store read the sidecar"))
    monkeypatch.setattr(store, "write_ivf", lambda *a, **k: pytest.fail("a flat store wrote the sidecar"))
    vs2 = make_vs()
    vs2.load_index(d)
    vs2(clustered(2, 8), 3)
    with pytest.raises(ValueError, match="no IVF lists"):
        vs2.ivf_lists()


# ---- persistence ---------------------------------------------------------------------------------------------------------
def _no_kmeans(monkeypatch):
    from lotus_amd import cluster

    def boom(*a, **k):
        raise AssertionError("k-means was called")

    monkeypatch.setattr(cluster, "kmeans", boom)


def test_sidecar_round_trip(tmp_path, monkeypatch):
    d = str(tmp_path / "ivf")
    xb = clustered(400, 12)
    vs = make_vs(factory_string="IVF6,Flat", nprobe=2, metric=METRIC_L2)
    vs.index(None, xb, d)
    assert os.path.exists(os.path.join(d, store.IVF_SIDECAR))
    assert sorted(os.listdir(d)) == ["index", "ivf.npz", "rows.json", "vecs"]
    lists = vs.ivf_lists()
    sig = store.signature(d)
    _no_kmeans(monkeypatch)
    vs2 = make_vs(factory_string="IVF6,Flat", nprobe=2, metric=METRIC_L2)
    vs2.load_index(d)
    for a, b in zip(lists, vs2.ivf_lists()):
        assert np.array_equal(a, b)
    assert store.signature(d) == sig  # the sidecar is not part of the signature
    q = clustered(5, 12, seed=8)
    assert np.array_equal(vs(q, 4).indices, vs2(q, 4).indices)
    with np.load(os.path.join(d, store.IVF_SIDECAR), allow_pickle=False) as z:
        assert set(z.files) == {"header", "centroids", "offsets", "rows"}


@pytest.mark.parametrize("change", ["vecs", "nlist", "metric", "missing", "garbage"])
def test_stale_or_foreign_sidecar_retrains(tmp_path, change):
    d = str(tmp_path / "ivf")
    xb = clustered(300, 10)
    make_vs(factory_string="IVF5,Flat").index(None, xb, d)
    kw = dict(factory_string="IVF5,Flat")
    side = os.path.join(d, store.IVF_SIDECAR)
    if change == "vecs":  # another writer (stock LOTUS) re-indexed the directory with other rows of the same shape
        make_vs().index(None, clustered(300, 10, seed=77), str(tmp_path / "other"))
        for name in ("vecs", "index"):
            with open(os.path.join(tmp_path, "other", name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
                dst.write(src.read())
        os.remove(os.path.join(d, "rows.json"))
    elif change == "nlist":
        kw["factory_string"] = "IVF7,Flat"
    elif change == "metric":
        kw["metric"] = METRIC_L2
    elif change == "missing":
        os.remove(side)
    else:
        with open(side, "wb") as fp:
            fp.write(b"not an npz")
    vs = make_vs(**kw)
    vs.load_index(d)
    assert [c for c in vs.backend.calls if c[0] == "ivf_build"][-1][2] is False  # built from fresh centroids
    c, off, rows = vs.ivf_lists()
    assert c.shape[0] == vs._nlist and off[-1] == 300
    # ... and the rewritten sidecar is valid for the next load
    assert store.read_ivf(d, vs._nlist, vs.metric, _capi.PACK_SPLIT, 10, 300) is not None


def test_sidecar_rewrite_failure_is_ignored_on_load(tmp_path, monkeypatch):
    d = str(tmp_path / "ivf")
    make_vs(factory_string="IVF4,Flat").index(None, clustered(100, 8), d)
    os.remove(os.path.join(d, store.IVF_SIDECAR))

    def denied(*a, **k):
        raise PermissionError("read-only directory")

    monkeypatch.setattr(store, "write_ivf", denied)
    vs = make_vs(factory_string="IVF4,Flat")
    vs.load_index(d)
    assert vs.ivf_lists()[0].shape == (4, 8)


def test_fewer_rows_than_lists(tmp_path):
    vs = make_vs(factory_string="IVF64,Flat", nprobe=64)
    xb = clustered(10, 8)
    vs.index(None, xb, str(tmp_path / "i"))
    assert vs.ivf_lists()[0].shape == (10, 8)
    assert vs.ivf_probe(xb[:2]).shape == (2, 10)
    out = vs(xb[:2], 10)
    assert sorted(out.indices[0].tolist()) == list(range(10))


# ---- C entry points ------------------------------------------------------------------------------------------------------
def test_ivf_entry_points_validate_before_device_work():
    lib = _capi.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its argument checks first
    args = dict(xb=p, xb_pack=0, nb=1000, xbn=None, off=p, rows=p, nlist=16, c=p, c_pack=0, cn=None, xq=p, xq_pack=0,
                nq=4, xqn=None, d=64, metric=0, nprobe=4, k=10, out=p, probe=None, ws=p, wsb=1 << 20, st=None)

    def call(**kw):
        a = dict(args, **kw)
        return lib.lvs_ivf_search_keys(*a.values())

    for kw, msg in ((dict(metric=3), b"metric"), (dict(nprobe=0), b"nprobe"), (dict(nprobe=17), b"nprobe"),
                    (dict(k=0), b"k="), (dict(k=57), b"k="), (dict(xb_pack=5), b"xb_pack"), (dict(c_pack=5), b"c_pack"),
                    (dict(nlist=0), b"nlist"), (dict(out=None), b"NULL"), (dict(metric=1), b"norms"),
                    (dict(d=0), b"shape")):
        assert call(**kw) == _capi.EINVAL, kw
        assert msg in lib.lvs_last_error(), (kw, lib.lvs_last_error())
    assert call(wsb=16) == _capi.ENOMEM and b"workspace" in lib.lvs_last_error()
    assert call(nq=0) == _capi.OK  # nothing to do
    assert lib.lvs_ivf_build_lists(None, 10, 0, p, p, p, 1 << 20, None) == _capi.EINVAL
    assert lib.lvs_ivf_build_lists(p, -1, 4, p, p, p, 1 << 20, None) == _capi.EINVAL
    assert lib.lvs_ivf_build_lists(p, 10, 4, None, p, p, 1 << 20, None) == _capi.EINVAL
    assert lib.lvs_ivf_build_lists(p, 1 << 20, 4, p, p, p, 16, None) == _capi.ENOMEM


def test_ivf_workspace_sizes_are_sane():
    lib = _capi.load()
    one = lib.lvs_ivf_search_workspace_bytes(1, 4096, 32, 768, 10, 0)
    assert 32 * 10 * 8 < one < 64 << 20
    w10k = lib.lvs_ivf_search_workspace_bytes(10000, 4096, 32, 768, 10, 0)
    assert 10000 * 32 * 10 * 8 <= w10k < plan_native.ivf_limits()[0]
    # many queries go through in chunks: the scratch stays bounded whatever nq is
    big = lib.lvs_ivf_search_workspace_bytes(1_000_000, 4096, 32, 768, 56, _capi.PACK_SPLIT)
    assert 0 < big <= plan_native.ivf_limits()[0]
    assert lib.lvs_ivf_search_workspace_bytes(1_000_000, 4096, 2048, 768, 56, 0) <= plan_native.ivf_limits()[0]
    for bad in ((-1, 16, 4, 64, 10, 0), (10, 0, 1, 64, 10, 0), (10, 16, 17, 64, 10, 0), (10, 16, 4, 0, 10, 0),
                (10, 16, 4, 64, 57, 0), (10, 16, 4, 64, 10, 7)):
        assert lib.lvs_ivf_search_workspace_bytes(*bad) < 0, bad
    assert 1_000_000 * 4 <= lib.lvs_ivf_build_workspace_bytes(1_000_000, 4096) < 64 << 20
    assert lib.lvs_ivf_build_workspace_bytes(10, 0) < 0


# ---- the reference's operator on an IVF store ---------------------------------------------------------------------------
def test_reference_sem_search_ends_on_an_ivf_store(tmp_path):
    import ref_harness

    if not ref_harness.available():
        pytest.skip("reference checkout not present")
    import pandas as pd

    lotus = ref_harness.import_lotus()
    from lotus.models.rm import RM

    import fake_rm
    from lotus_amd import HipVS as RefHipVS  # re-imported against the reference's ABCs

    rows = [f"course {i} on topic {i % 7}" for i in range(40)]
    # 40 rows in 20 lists and one probe: a list holds ~2 rows, fewer than K, so the unmodified K-doubling loop
    # (sem_search.py:120-138) sees -1 slots until K passes the list scan's limit and the exact path answers
    vs = RefHipVS(backend=IvfOracleBackend(), factory_string="IVF20,Flat", nprobe=1)
    lotus.settings.configure(rm=fake_rm.make_rm(RM, np.float32), vs=vs)
    df = pd.DataFrame({"T": rows}).sem_index("T", str(tmp_path / "idx"))
    out = df.sem_search("T", "topic 3", K=8)
    assert len(out) == 8 and out.index.is_unique


# ---- shapes the list scan cannot take go to the exact path ----------------------------------------------------------------
@pytest.mark.parametrize("d,storage,served", [(1536, "auto", False), (1088, "auto", True), (1536, "fp16", True),
                                              (3072, "fp16", False)])
def test_rows_too_wide_for_the_list_scan_are_searched_exactly(tmp_path, d, storage, served):
    xb = clustered(300, d, centers=6)
    xq = clustered(4, d, centers=6, seed=6)
    vs = make_vs(factory_string="IVF6,Flat", nprobe=1, storage=storage)
    vs.index(None, xb, str(tmp_path / "i"))
    mode = _capi.PACK_F16 if storage == "fp16" else _capi.PACK_SPLIT
    assert vs.backend.ivf_fits(d, 10, mode) is served
    vs.backend.calls.clear()
    out = vs(xq, 10)
    used = [c for c in vs.backend.calls if c[0] == "ivf_search"]
    assert bool(used) is served
    xb_s, xq_s = _emulate_storage(xb, mode), _emulate_storage(xq, mode)
    if not served:
        assert np.array_equal(out.indices, oracle.flat_search(xb_s, xq_s, 10)[1])
    c, _, _ = vs.ivf_lists()
    assert np.array_equal(vs.ivf_probe(xq, 3), probe_lists(c, xq_s, 3, METRIC_INNER_PRODUCT))


def test_more_than_2048_probes_are_searched_exactly(tmp_path):
    xb = clustered(2200, 4, centers=50)
    xq = clustered(3, 4, centers=50, seed=4)
    vs = make_vs(factory_string="IVF2100,Flat", nprobe=2049, ivf_niter=2)
    vs.index(None, xb, str(tmp_path / "i"))
    vs.backend.calls.clear()
    out = vs(xq, 5)
    assert not [c for c in vs.backend.calls if c[0] == "ivf_search"]
    xb_s, xq_s = _emulate_storage(xb, _capi.PACK_SPLIT), _emulate_storage(xq, _capi.PACK_SPLIT)
    assert np.array_equal(out.indices, oracle.flat_search(xb_s, xq_s, 5)[1])
    vs(xq, 5, nprobe=2048)
    assert [c for c in vs.backend.calls if c[0] == "ivf_search"] == [("ivf_search", 3, 5, 2048)]
    with pytest.raises(ValueError, match="2048"):
        vs.ivf_probe(xq, 2049)


def test_ivf_workspace_reports_unsupported_shapes():
    lib = _capi.load()
    for d, k, pack in ((1088, 56, 1), (1216, 16, 1), (2240, 56, 0), (2432, 16, 0)):
        assert lib.lvs_ivf_search_workspace_bytes(10, 64, 4, d, k, pack) > 0
        assert lib.lvs_ivf_search_workspace_bytes(10, 64, 4, d + 1, k, pack) == _capi.EUNSUPPORTED
    p = ctypes.c_void_p(16)
    st = lib.lvs_ivf_search_keys(p, 1, 100, None, p, p, 4, p, 1, None, p, 1, 4, None, 1536, 0, 2, 10, p, None, p, 1 << 30,
                                 None)
    assert st == _capi.EUNSUPPORTED and b"LDS" in lib.lvs_last_error()


def test_touched_files_void_the_sidecar(tmp_path):
    d = str(tmp_path / "ivf")
    make_vs(factory_string="IVF5,Flat").index(None, clustered(300, 10), d)
    assert store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300) is not None
    st = os.stat(os.path.join(d, "vecs"))
    os.utime(os.path.join(d, "vecs"), ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))  # same bytes, new mtime (a copy)
    assert store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300) is None
    vs = make_vs(factory_string="IVF5,Flat")
    vs.load_index(d)  # retrains once and records the new stamps
    assert [c for c in vs.backend.calls if c[0] == "ivf_build"][-1][2] is False
    assert store.read_ivf(d, 5, 0, _capi.PACK_SPLIT, 10, 300) is not None
