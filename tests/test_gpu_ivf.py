"""IVF-Flat on the device (lvs_ivf_search_keys / lvs_ivf_scan_kernel) against the CPU oracle.  The rule: a search is the exact
top k over the rows of the lists it probed (oracle.flat_search with ids = their union), so nprobe = nlist is the exact
search; slots past those rows are -1 exactly where the oracle pads."""
import numpy as np
import pytest

import oracle
import synth
from ivf_edge_cases import rescoring_args
from ivf_oracle_backend import ivf_reference
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2


def _data(nb, nq, d, mode, seed):
    """Unit rows with a positive first coordinate (so that centroid +e0 beats the dead centroid under either metric) and
    queries; returned as (device input, stored values the oracle consumes)."""
    xb = synth.corpus(nb, d, seed=seed)
    xb[:, 0] = np.abs(xb[:, 0])
    xq, _ = synth.queries(xb, nq, seed=seed + 1)
    if mode == F16:
        xb, xq = xb.astype(np.float16), xq.astype(np.float16)
    return xb, xb.astype(np.float32), xq, xq.astype(np.float32)


def _centroids(xb_s, nlist, metric, seed):
    """nlist - 2 sampled rows, +e0, and a centroid no row picks (-e0 for inner products, far away for L2): one empty list."""
    d = xb_s.shape[1]
    rng = np.random.default_rng(seed)
    c = np.zeros((nlist, d), np.float32)
    c[:nlist - 2] = xb_s[rng.choice(xb_s.shape[0], nlist - 2, replace=False)]
    c[nlist - 2, 0] = 1.0
    c[nlist - 1, 0] = -1.0 if metric == IP else 100.0
    return c


def _search(be, xb, xq, c, k, mode, metric, nprobe):
    packed = be.pack(xb, mode)
    lists = be.ivf_build(packed, c, metric)
    qp = be.pack(xq, mode)
    keys, probe = be.ivf_search(packed, lists, qp, k, metric, nprobe, want_probe=True)
    D, I = be.keys_to_result(keys, metric)
    be.synchronize()
    off = lists.offsets.cpu().numpy()
    rows = lists.rows.cpu().numpy().view(np.uint32)
    cdev = be.unpack(lists.centroids).cpu().numpy()
    return D.cpu().numpy(), I.cpu().numpy(), probe.cpu().numpy(), off, rows, cdev


def _check(D_ref, I_ref, D, I, rescore=None):
    """rescore = (rows scored: stored or decoded, queries, metric, offsets, rows, probe): every returned id is one of the
    query's probed rows, unrepeated, and its float64 score is the returned one (synth.check_ids_by_rescoring)."""
    err, hard, _ = synth.compare_topk(D_ref, I_ref, D, I)
    assert err <= 1e-5 and hard == 0, (err, hard)
    assert np.array_equal(I == -1, I_ref == -1)
    if rescore is not None:
        score_fn, allowed = rescoring_args(*rescore)
        synth.check_ids_by_rescoring(score_fn, D, I, allowed, 1e-5)


def _check_lists(xb_s, cdev, off, rows, metric):
    nlist = cdev.shape[0]
    assert off[0] == 0 and off[-1] == xb_s.shape[0] and sorted(rows.tolist()) == list(range(xb_s.shape[0]))
    D, best = oracle.flat_search(cdev, xb_s, 2, metric)
    assign = np.repeat(np.arange(nlist), np.diff(off))
    got = np.empty_like(assign)
    got[rows.astype(np.int64)] = assign
    clear = np.abs(D[:, 0] - D[:, 1]) > 2e-5  # rows whose two best centroids are not a near tie
    assert np.array_equal(got[clear], best[clear, 0])
    for l in range(nlist):
        assert np.all(np.diff(rows[off[l]:off[l + 1]].astype(np.int64)) > 0)
    assert (np.diff(off) == 0).any()  # the dead centroid's list


# 1. nprobe == nlist is the exact search: every metric, storage, d, k and query count appears
FULL = [
    # nb, d, nq, k, mode, metric, nlist
    (3000, 64, 1, 1, F16, IP, 16),
    (3000, 64, 300, 56, SPLIT, L2, 16),
    (4000, 384, 7, 10, F16, L2, 24),
    (4000, 384, 5000, 10, SPLIT, IP, 24),
    (5000, 768, 300, 1, F16, IP, 32),
    (5000, 768, 1, 56, SPLIT, IP, 32),
    (2000, 1000, 7, 56, F16, L2, 12),
    (2000, 1000, 300, 10, SPLIT, L2, 12),
    (2500, 768, 5000, 56, F16, IP, 20),
]


@pytest.mark.parametrize("nb,d,nq,k,mode,metric,nlist", FULL)
def test_all_lists_probed_is_exact_search(hip_backend, nb, d, nq, k, mode, metric, nlist):
    xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=d + nq)
    c = _centroids(xb_s, nlist, metric, seed=nb)
    D, I, probe, off, rows, cdev = _search(hip_backend, xb, xq, c, k, mode, metric, nlist)
    _check_lists(xb_s, cdev, off, rows, metric)
    D_ref, I_ref = oracle.flat_search(xb_s, xq_s, k, metric)
    _check(D_ref, I_ref, D, I, rescore=(xb_s, xq_s, metric, off, rows, probe))


# 2. + 3. nprobe < nlist: exact over the probed lists, and the probes are the nprobe best centroids
PART = [
    (6000, 384, 300, 10, F16, IP, 40, 4),
    (6000, 384, 7, 56, SPLIT, L2, 40, 3),
    (4000, 768, 300, 1, SPLIT, IP, 64, 8),
    (4000, 1000, 50, 10, F16, L2, 30, 2),
    (3000, 64, 200, 56, F16, IP, 200, 1),  # ~15 rows per list: the probed lists hold fewer than k rows
]


@pytest.mark.parametrize("nb,d,nq,k,mode,metric,nlist,nprobe", PART)
def test_partial_probe_is_exact_over_probed_lists(hip_backend, nb, d, nq, k, mode, metric, nlist, nprobe):
    xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=7 * d + nq)
    c = _centroids(xb_s, nlist, metric, seed=nb + 1)
    D, I, probe, off, rows, cdev = _search(hip_backend, xb, xq, c, k, mode, metric, nprobe)
    _check_lists(xb_s, cdev, off, rows, metric)
    Dp, Ip = oracle.flat_search(cdev, xq_s, nprobe, metric)
    err, hard, _ = synth.compare_topk(Dp, Ip, Dp, probe)
    assert hard == 0
    D_ref, I_ref = ivf_reference(xb_s, xq_s, k, metric, cdev, off, rows, probe)
    _check(D_ref, I_ref, D, I, rescore=(xb_s, xq_s, metric, off, rows, probe))
    if k == 56 and nlist == 200:
        assert (I == -1).any()


# ---- through HipVS ---------------------------------------------------------------------------------------------------------
def _clustered(n, d, centers, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + 0.5 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype)


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_kth_score_never_gets_worse_with_nprobe(hip_backend, tmp_path, metric):
    xb = _clustered(20000, 128, 50, seed=1)
    xq = _clustered(200, 128, 50, seed=2)
    vs = HipVS(factory_string="IVF64,Flat", metric=metric, device="cuda:0")
    vs.index(None, xb, str(tmp_path / "i"), persist=False)
    prev = None
    for nprobe in (1, 2, 4, 8, 16, 64):
        kth = vs(xq, 10, nprobe=nprobe).distances[:, 9].astype(np.float64)
        better = kth if metric == METRIC_INNER_PRODUCT else -kth
        if prev is not None:
            assert (better >= prev).all()
        prev = better
    D, I = oracle.flat_search(xb, xq, 10, metric)
    out = vs(xq, 10, nprobe=64)
    _check(D, I, out.distances, out.indices)


def test_ties_across_lists_come_back_in_ascending_id_order(hip_backend, tmp_path):
    d, n = 64, 4000
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 0] = 0.0
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= 0.75
    tied = rng.choice(n, 40, replace=False)
    x[tied, 0] = 0.5  # q = e0 scores exactly 0.5 on every tied row, whatever list it is in
    x[np.setdiff1d(np.arange(n), tied), 0] = 0.25
    x = x.astype(np.float16)
    vs = HipVS(factory_string="IVF32,Flat", nprobe=32, storage="fp16", device="cuda:0")
    vs.index(None, x, str(tmp_path / "i"), persist=False)
    _, off, rows = vs.ivf_lists()
    where = np.empty(n, np.int64)
    where[rows.astype(np.int64)] = np.repeat(np.arange(32), np.diff(off))
    assert len(set(where[tied].tolist())) > 1
    q = np.zeros((1, d), np.float16)
    q[0, 0] = 1.0
    out = vs(q, 40)
    assert np.array_equal(out.indices[0], np.sort(tied)) and (out.distances[0] == np.float32(0.5)).all()


def test_build_is_deterministic_and_persists(hip_backend, tmp_path, monkeypatch):
    import torch

    from lotus_amd import cluster

    xb = _clustered(30000, 96, 40, seed=3)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    a = HipVS(factory_string="IVF48,Flat", nprobe=6, device="cuda:0")
    a.index(None, xb, d1)
    b = HipVS(factory_string="IVF48,Flat", nprobe=6, device="cuda:0")
    b.index(None, xb, d2)
    la, lb = a.ivf_lists(), b.ivf_lists()
    for u, v in zip(la, lb):
        assert np.array_equal(u, v)
    q = _clustered(100, 96, 40, seed=4)
    ref = a(q, 10)

    calls = []
    real = cluster.kmeans

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    def boom(*args, **kw):
        raise AssertionError("k-means was called")

    monkeypatch.setattr(cluster, "kmeans", boom)
    c = HipVS(factory_string="IVF48,Flat", nprobe=6, device="cuda:0")
    c.load_index(d1)  # the sidecar: no training
    for u, v in zip(la, c.ivf_lists()):
        assert np.array_equal(u, v)
    assert np.array_equal(c(q, 10).indices, ref.indices)

    monkeypatch.setattr(cluster, "kmeans", counted)
    xb2 = _clustered(30000, 96, 40, seed=9)
    HipVS(device="cuda:0").index(None, xb2, d1)  # a flat writer rewrites vecs / index and leaves the old sidecar behind
    e = HipVS(factory_string="IVF48,Flat", nprobe=6, device="cuda:0")
    e.load_index(d1)
    assert calls == [1]
    D, I = oracle.flat_search(xb2, q, 10)
    out = e(q, 10, nprobe=48)
    _check(D, I, out.distances, out.indices)

    t = HipVS(factory_string="IVF48,Flat", nprobe=6, device="cuda:0")  # a CUDA tensor straight from an encoder
    t.index(None, torch.from_numpy(xb).to("cuda:0"), str(tmp_path / "t"))
    for u, v in zip(la, t.ivf_lists()):
        assert np.array_equal(u, v)
    assert np.array_equal(t(q, 10).indices, ref.indices)


def test_the_ivf_kernel_serves_the_search(hip_backend, tmp_path):
    xb = _clustered(20000, 384, 30, seed=6, dtype=np.float16)
    vs = HipVS(factory_string="IVF32,Flat", nprobe=4, device="cuda:0")
    vs.index(None, xb, str(tmp_path / "i"), persist=False)
    q = _clustered(5, 384, 30, seed=7, dtype=np.float16)
    vs.backend.timing_enable(True)
    vs(q, 10)
    t = vs.backend.timing_read_full()
    vs.backend.timing_enable(False)
    assert t["kernel"] == "lvs_ivf_scan_kernel" and t["calls"] == 1 and t["launches"] >= 1


def test_full_size_1m_x_768(hip_backend):
    n, d, nq = 1_000_000, 768, 10_000
    rng = np.random.default_rng(11)
    xb = np.empty((n, d), np.float16)
    for r0 in range(0, n, 100_000):
        blk = rng.standard_normal((100_000, d), dtype=np.float32)
        blk /= np.linalg.norm(blk, axis=1, keepdims=True)
        xb[r0:r0 + 100_000] = blk
    xq, _ = synth.queries(xb[:200_000].astype(np.float32), nq, seed=12)
    xq = xq.astype(np.float16)
    vs = HipVS(factory_string="IVF4096,Flat", nprobe=32, storage="fp16", device="cuda:0")
    vs.index(None, xb, "unused", persist=False)
    out = vs(xq, 10)
    c, off, rows = vs.ivf_lists()
    assert c.shape == (4096, d) and off[-1] == n
    pick = np.random.default_rng(13).choice(nq, 64, replace=False)
    probe = vs.ivf_probe(xq[pick], 32)
    xq_s = xq[pick].astype(np.float32)
    D_ref, I_ref = ivf_reference(xb, xq_s, 10, IP, c, off, rows, probe)
    _check(D_ref, I_ref, out.distances[pick], out.indices[pick], rescore=(xb, xq_s, IP, off, rows, probe))


def test_queries_beyond_one_chunk(hip_backend):
    """40 000 queries run as three chunks of at most 16 384 inside lvs_ivf_search_keys: queries, norms, keys and probes of
    the later chunks are offset, the scratch is reused."""
    nb, d, nq, k, nlist, nprobe = 20000, 64, 40000, 10, 64, 4
    for mode, metric in ((F16, IP), (SPLIT, L2)):
        xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=31 + mode)
        c = _centroids(xb_s, nlist, metric, seed=32)
        D, I, probe, off, rows, cdev = _search(hip_backend, xb, xq, c, k, mode, metric, nprobe)
        pick = np.unique(np.concatenate([np.random.default_rng(33).choice(nq, 200, replace=False),
                                         [0, 16383, 16384, 16385, 32767, 32768, 32769, nq - 1]]))
        Dp, Ip = oracle.flat_search(cdev, xq_s[pick], nprobe, metric)
        assert synth.compare_topk(Dp, Ip, Dp, probe[pick])[1] == 0
        D_ref, I_ref = ivf_reference(xb_s, xq_s[pick], k, metric, cdev, off, rows, probe[pick])
        _check(D_ref, I_ref, D[pick], I[pick], rescore=(xb_s, xq_s[pick], metric, off, rows, probe[pick]))


def test_fp32_rows_of_1536_dims(hip_backend, tmp_path):
    """text-embedding-3-small's width: hi|lo rows of 1 536 dims do not fit the list scan's LDS image and are searched exactly;
    the same rows stored as fp16 go through the list scan."""
    xb = _clustered(8000, 1536, 20, seed=21)
    xq = _clustered(50, 1536, 20, seed=22)
    vs = HipVS(factory_string="IVF16,Flat", nprobe=2, device="cuda:0")
    vs.index(None, xb, str(tmp_path / "a"))
    assert not vs.backend.ivf_fits(1536, 10, _capi.PACK_SPLIT)
    out = vs(xq, 10)
    D, I = oracle.flat_search(xb, xq, 10)
    _check(D, I, out.distances, out.indices)
    c, off, rows = vs.ivf_lists()
    assert vs.ivf_probe(xq, 2).shape == (50, 2)

    h = HipVS(factory_string="IVF16,Flat", nprobe=2, storage="fp16", device="cuda:0")
    h.index(None, xb, str(tmp_path / "b"), persist=False)
    h.backend.timing_enable(True)
    out = h(xq, 10)
    t = h.backend.timing_read_full()
    h.backend.timing_enable(False)
    assert t["kernel"] == "lvs_ivf_scan_kernel"
    x16, q16 = xb.astype(np.float16).astype(np.float32), xq.astype(np.float16).astype(np.float32)
    c, off, rows = h.ivf_lists()
    probe = h.ivf_probe(xq, 2)
    D_ref, I_ref = ivf_reference(x16, q16, 10, IP, c, off, rows, probe)
    _check(D_ref, I_ref, out.distances, out.indices, rescore=(x16, q16, IP, off, rows, probe))
