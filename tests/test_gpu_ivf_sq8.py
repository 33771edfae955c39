"""IVF-SQ8 on the device (lvs_ivf_sq8_encode / lvs_ivf_sq8_search_keys / lvs_ivf_sq8_scan_kernel) against the numpy codec and
the float64 reference.  The rule: a search is the exact top k, in float64, over the DECODED rows (c_l + vmin + (code + 0.5)
vdiff / 255) of the lists it probed; slots past those rows are -1 exactly where the reference pads."""
import numpy as np
import pytest

import oracle
import synth
from ivf_edge_cases import rescoring_args
from ivf_sq8_oracle_backend import list_of_rows, sq8_boundary_distance, sq8_decode, sq8_encode, sq8_reference, sq8_train
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2


def _data(nb, nq, d, mode, seed):
    """Unit rows with a positive first coordinate (so that centroid +e0 beats the dead centroid under either metric) and
    queries; returned as (device input, stored values)."""
    xb = synth.corpus(nb, d, seed=seed)
    xb[:, 0] = np.abs(xb[:, 0])
    xq, _ = synth.queries(xb, nq, seed=seed + 1)
    if mode == F16:
        xb, xq = xb.astype(np.float16), xq.astype(np.float16)
    return xb, xb.astype(np.float32), xq, xq.astype(np.float32)


def _centroids(xb_s, nlist, metric, seed):
    """nlist - 2 sampled rows, +e0, and a centroid no row picks: one empty list."""
    d = xb_s.shape[1]
    rng = np.random.default_rng(seed)
    c = np.zeros((nlist, d), np.float32)
    c[:nlist - 2] = xb_s[rng.choice(xb_s.shape[0], nlist - 2, replace=False)]
    c[nlist - 2, 0] = 1.0
    c[nlist - 1, 0] = -1.0 if metric == IP else 100.0
    return c


def _build(be, xb, c, mode, metric, train_ids):
    packed = be.pack(xb, mode)
    lists = be.ivf_build(packed, c, metric)
    vmin, vdiff = be.ivf_sq8_train(packed, lists, train_ids)
    sq = be.ivf_sq8_encode(packed, lists, vmin, vdiff)
    be.synchronize()
    off = lists.offsets.cpu().numpy()
    rows = lists.rows.cpu().numpy().view(np.uint32)
    n, d = packed.n, packed.d
    codes = np.empty((n, d), np.uint8)
    codes[rows.astype(np.int64)] = sq.codes[:, :d].cpu().numpy()
    rn = np.empty(n, np.float32)
    rn[rows.astype(np.int64)] = sq.rnorm.cpu().numpy()
    host = dict(off=off, rows=rows, where=list_of_rows(off, rows, n), c=be.unpack(lists.centroids).cpu().numpy(),
                x=be.unpack(packed).cpu().numpy(), vmin=sq.vmin.cpu().numpy(), vdiff=sq.vdiff.cpu().numpy(), codes=codes,
                rn=rn)
    return packed, lists, sq, host


def _check_codec(h, train_ids):
    vmin, vdiff = sq8_train(h["x"], h["c"], h["where"], train_ids)
    assert np.array_equal(vmin, h["vmin"]) and np.array_equal(vdiff, h["vdiff"])
    codes, rn = sq8_encode(h["x"], h["c"], h["where"], h["vmin"], h["vdiff"])
    diff = codes != h["codes"]
    near = sq8_boundary_distance(h["x"], h["c"], h["where"], h["vmin"], h["vdiff"]) < 1e-4
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    assert (np.abs(codes.astype(np.int32) - h["codes"]) <= 1).all()
    if not diff.any():
        np.testing.assert_allclose(h["rn"], rn, rtol=1e-5, atol=1e-7)


def _search(be, packed, lists, sq, xq, mode, k, metric, nprobe):
    qp = be.pack(xq, mode)
    keys, probe = be.ivf_sq8_search(packed, lists, sq, qp, k, metric, nprobe, want_probe=True)
    D, I = be.keys_to_result(keys, metric)
    be.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), probe.cpu().numpy()


def _check(D_ref, I_ref, D, I, rescore=None):
    """rescore = (rows scored: stored or decoded, queries, metric, offsets, rows, probe): every returned id is one of the
    query's probed rows, unrepeated, and its float64 score is the returned one (synth.check_ids_by_rescoring)."""
    err, hard, _ = synth.compare_topk(D_ref, I_ref, D, I)
    assert err <= 1e-5 and hard == 0, (err, hard)
    assert np.array_equal(I == -1, I_ref == -1)
    if rescore is not None:
        score_fn, allowed = rescoring_args(*rescore)
        synth.check_ids_by_rescoring(score_fn, D, I, allowed, 1e-5)


CASES = [
    # nb, d, nq, k, mode, metric, nlist, nprobe
    (3000, 64, 1, 1, F16, IP, 16, 16),
    (3000, 64, 300, 56, SPLIT, L2, 16, 8),
    (4000, 384, 7, 10, F16, L2, 24, 1),
    (4000, 384, 300, 10, SPLIT, IP, 24, 24),
    (5000, 768, 300, 56, SPLIT, L2, 32, 8),
    (5000, 768, 7, 1, F16, IP, 32, 32),
    (4000, 1536, 300, 10, SPLIT, IP, 20, 8),
    (4000, 1536, 7, 56, F16, L2, 20, 20),
    (3000, 1536, 1, 10, SPLIT, L2, 12, 1),
    (3000, 64, 200, 56, F16, IP, 200, 1),  # ~15 rows per list: the probed lists hold fewer than k rows
]


@pytest.mark.parametrize("nb,d,nq,k,mode,metric,nlist,nprobe", CASES)
def test_codes_and_search_match_the_reference(hip_backend, nb, d, nq, k, mode, metric, nlist, nprobe):
    be = hip_backend
    xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=d + nq + k)
    c = _centroids(xb_s, nlist, metric, seed=nb + nprobe)
    train = np.random.default_rng(d).choice(nb, nb // 2, replace=False)  # rows outside the training range are clamped
    packed, lists, sq, h = _build(be, xb, c, mode, metric, train)
    assert (np.diff(h["off"]) == 0).any()  # the dead centroid's empty list
    _check_codec(h, train)
    D, I, probe = _search(be, packed, lists, sq, xq, mode, k, metric, nprobe)
    Dp, Ip = oracle.flat_search(h["c"], xq_s, nprobe, metric)
    assert synth.compare_topk(Dp, Ip, Dp, probe)[1] == 0
    xhat = sq8_decode(h["c"], h["where"], h["vmin"], h["vdiff"], h["codes"])
    D_ref, I_ref = sq8_reference(xhat, xq_s, k, metric, h["off"], h["rows"], probe)
    _check(D_ref, I_ref, D, I, rescore=(xhat, xq_s, metric, h["off"], h["rows"], probe))
    if nlist == 200:
        assert (I == -1).any()


def test_queries_beyond_one_chunk(hip_backend):
    """40 000 queries run as three chunks of at most 16 384 inside lvs_ivf_sq8_search_keys."""
    be = hip_backend
    nb, d, nq, k, nlist, nprobe = 20000, 64, 40000, 10, 64, 4
    for mode, metric in ((F16, IP), (SPLIT, L2)):
        xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=41 + mode)
        c = _centroids(xb_s, nlist, metric, seed=42)
        packed, lists, sq, h = _build(be, xb, c, mode, metric, np.arange(nb))
        D, I, probe = _search(be, packed, lists, sq, xq, mode, k, metric, nprobe)
        pick = np.unique(np.concatenate([np.random.default_rng(43).choice(nq, 200, replace=False),
                                         [0, 16383, 16384, 16385, 32767, 32768, 32769, nq - 1]]))
        Dp, Ip = oracle.flat_search(h["c"], xq_s[pick], nprobe, metric)
        assert synth.compare_topk(Dp, Ip, Dp, probe[pick])[1] == 0
        xhat = sq8_decode(h["c"], h["where"], h["vmin"], h["vdiff"], h["codes"])
        D_ref, I_ref = sq8_reference(xhat, xq_s[pick], k, metric, h["off"], h["rows"], probe[pick])
        _check(D_ref, I_ref, D[pick], I[pick], rescore=(xhat, xq_s[pick], metric, h["off"], h["rows"], probe[pick]))


@pytest.mark.parametrize("metric", [IP, L2])
def test_duplicated_rows_score_alike_in_row_order(hip_backend, metric):
    be = hip_backend
    nb, d = 4000, 384
    xb, xb_s, _, _ = _data(nb, 1, d, SPLIT, seed=51)
    dup = np.sort(np.random.default_rng(52).choice(nb, 30, replace=False))
    xb[dup] = xb[dup[0]]
    xb_s = xb.astype(np.float32)
    c = _centroids(xb_s, 16, metric, seed=53)
    packed, lists, sq, h = _build(be, xb, c, SPLIT, metric, np.arange(nb))
    assert len(set(h["where"][dup].tolist())) == 1
    q = xb[dup[0]:dup[0] + 1] + np.float32(1e-3)
    D, I, _ = _search(be, packed, lists, sq, q, SPLIT, 56, metric, 16)
    at = np.isin(I[0], dup)
    assert at.sum() == 30
    assert np.array_equal(I[0][at], dup)  # ascending row order
    assert (D[0][at] == D[0][at][0]).all()  # bit-identical scores


def _clustered(n, d, centers, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + 0.5 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype)


def _reference_of(vs, xq, k, nprobe):
    c, off, rows = vs.ivf_lists()
    vmin, vdiff, codes, _ = vs.sq8_codes()
    xhat = sq8_decode(c, list_of_rows(off, rows, codes.shape[0]), vmin, vdiff, codes)
    probe = vs.ivf_probe(xq, nprobe)
    D, I = sq8_reference(xhat, np.asarray(xq, np.float32), k, vs.metric, off, rows, probe)
    return D, I, (xhat, np.asarray(xq, np.float32), vs.metric, off, rows, probe)


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_hipvs_1536_dims_from_float64(hip_backend, tmp_path, monkeypatch, metric):
    """text-embedding-3-small's width from float64 input (hi|lo storage): served by the SQ8 scan, persisted and reloaded
    without training; ids subsets and K > 56 are the flat store's answers exactly."""
    from lotus_amd import cluster

    xb = _clustered(8000, 1536, 20, seed=21).astype(np.float64)
    xq = _clustered(50, 1536, 20, seed=22).astype(np.float64)
    d1 = str(tmp_path / "sq8")
    vs = HipVS(factory_string="IVF16,SQ8", nprobe=2, metric=metric, device="cuda:0")
    vs.index(None, xb, d1)
    vs.backend.timing_enable(True)
    out = vs(xq, 10)
    t = vs.backend.timing_read_full()
    vs.backend.timing_enable(False)
    assert t["kernel"] == "lvs_ivf_sq8_scan_kernel" and t["calls"] == 1
    D_ref, I_ref, rescore = _reference_of(vs, xq, 10, 2)
    _check(D_ref, I_ref, out.distances, out.indices, rescore=rescore)

    monkeypatch.setattr(cluster, "kmeans", lambda *a, **k: pytest.fail("k-means was called"))
    r2 = HipVS(factory_string="IVF16,SQ8", nprobe=2, metric=metric, device="cuda:0")
    r2.load_index(d1)
    for u, v in zip(vs.ivf_lists() + vs.sq8_codes(), r2.ivf_lists() + r2.sq8_codes()):
        assert np.array_equal(u, v)
    again = r2(xq, 10)
    assert np.array_equal(again.indices, out.indices) and np.array_equal(again.distances, out.distances)

    flat = HipVS(metric=metric, device="cuda:0")
    flat.index(None, xb, str(tmp_path / "flat"), persist=False)
    ids = list(range(0, 8000, 7))
    a, b = r2(xq, 10, ids=ids), flat(xq, 10, ids=ids)
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.distances, b.distances)
    a, b = r2(xq, 60), flat(xq, 60)
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.distances, b.distances)


def test_sq8_and_flat_stores_probe_the_same_lists(hip_backend, tmp_path):
    xb = _clustered(20000, 384, 30, seed=61, dtype=np.float16)
    xq = _clustered(300, 384, 30, seed=62, dtype=np.float16)
    a = HipVS(factory_string="IVF32,SQ8", nprobe=4, device="cuda:0")
    a.index(None, xb, str(tmp_path / "a"), persist=False)
    b = HipVS(factory_string="IVF32,Flat", nprobe=4, device="cuda:0")
    b.index(None, xb, str(tmp_path / "b"), persist=False)
    for u, v in zip(a.ivf_lists(), b.ivf_lists()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.ivf_probe(xq, 4), b.ivf_probe(xq, 4))
    # the decoded search finds most of the full-precision one's neighbours
    ra, rb = a(xq, 10).indices, b(xq, 10).indices
    assert np.mean([len(set(x) & set(y)) / 10 for x, y in zip(ra, rb)]) > 0.9
