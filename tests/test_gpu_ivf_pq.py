"""IVF-PQ on the device (lvs_ivf_pq_encode / lvs_ivf_pq_search_keys / lvs_ivf_pq_lut_kernel + lvs_ivf_pq_scan_kernel) against
the numpy codec and the float64 reference.  The rule: a search is the exact top k, in float64, over the DECODED rows
(c_l + concat_m codebooks[m][code_m]) of the lists it probed; slots past those rows are -1 exactly where the reference pads."""
import numpy as np
import pytest

import oracle
import plan_native
import synth
from ivf_edge_cases import rescoring_args
from ivf_oracle_backend import ivf_reference
from ivf_pq_oracle_backend import list_of_rows, pq_decode, pq_encode, pq_margin, pq_reference
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2


def _data(nb, nq, d, mode, seed, dtype=np.float32):
    """Unit rows with a positive first coordinate (so that centroid +e0 beats the dead centroid under either metric) and
    queries; returned as (device input, stored values)."""
    xb = synth.corpus(nb, d, seed=seed)
    xb[:, 0] = np.abs(xb[:, 0])
    xq, _ = synth.queries(xb, nq, seed=seed + 1)
    if mode == F16:
        xb, xq = xb.astype(np.float16), xq.astype(np.float16)
    else:
        xb, xq = xb.astype(dtype), xq.astype(dtype)
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


def _codebooks(h, M, ksub, seed):
    """Codebooks of ksub sampled residuals per subspace (a quantizer whose training is not the subject)."""
    rng = np.random.default_rng(seed)
    r = h["x"] - h["c"][h["where"]]
    n, d = r.shape
    return np.stack([r[rng.choice(n, ksub, replace=False), m * (d // M):(m + 1) * (d // M)] for m in range(M)]).astype(np.float32)


def _host(be, packed, lists):
    be.synchronize()
    off = lists.offsets.cpu().numpy()
    rows = lists.rows.cpu().numpy().view(np.uint32)
    n = packed.n
    return dict(off=off, rows=rows, where=list_of_rows(off, rows, n), c=be.unpack(lists.centroids).cpu().numpy(),
                x=be.unpack(packed).cpu().numpy())


def _encode(be, packed, lists, h, books):
    pq = be.ivf_pq_encode(packed, lists, books)
    be.synchronize()
    rows = h["rows"].astype(np.int64)
    codes = np.empty((packed.n, pq.M), np.uint8)
    codes[rows] = pq.codes[:, :pq.M].cpu().numpy()
    beta = np.empty(packed.n, np.float32)
    beta[rows] = pq.beta.cpu().numpy()
    assert (pq.codes[:, pq.M:].cpu().numpy() == 0).all()
    return pq, codes, beta


def _check_codes(h, books, codes, beta):
    """Codes equal the twin's wherever its best and second-best sub-distances are further apart than an fp32 tolerance;
    elsewhere the two codes' distances lie within it."""
    tw, tb = pq_encode(h["x"], h["c"], h["where"], books)
    margin = pq_margin(h["x"], h["c"], h["where"], books)
    r = (h["x"] - h["c"][h["where"]]).astype(np.float64)
    M, _, dsub = books.shape
    scale = np.stack([(r[:, m * dsub:(m + 1) * dsub] ** 2).sum(1) for m in range(M)], 1) + (books.astype(np.float64) ** 2).sum(2).max()
    tol = 1e-5 * (1.0 + scale)
    diff = tw != codes
    assert not (diff & (margin > tol)).any(), int((diff & (margin > tol)).sum())
    same = ~diff.any(axis=1)
    np.testing.assert_allclose(beta[same], tb[same], rtol=1e-4, atol=1e-5)


def _search(be, packed, lists, pq, xq, mode, k, metric, nprobe):
    qp = be.pack(xq, mode)
    keys, probe = be.ivf_pq_search(packed, lists, pq, qp, k, metric, nprobe, want_probe=True)
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
    # nb, d, M, ksub, nq, k, mode, metric, nlist, nprobe
    (3000, 128, 16, 256, 1, 1, F16, IP, 16, 16),
    (3000, 128, 8, 256, 17, 56, SPLIT, L2, 16, 8),
    (3000, 128, 32, 100, 17, 10, SPLIT, IP, 16, 1),  # ksub < 256
    (4000, 768, 64, 256, 17, 10, F16, L2, 24, 8),
    (4000, 768, 96, 256, 300, 56, SPLIT, IP, 24, 24),
    (4000, 768, 24, 256, 1, 10, SPLIT, L2, 24, 1),
    (4000, 1536, 64, 256, 300, 10, SPLIT, IP, 20, 8),
    (4000, 1536, 128, 256, 17, 1, F16, L2, 20, 20),
    (3000, 3072, 96, 256, 17, 56, SPLIT, L2, 12, 8),
    (3000, 3072, 64, 256, 1, 10, F16, IP, 12, 12),
    (3000, 3072, 48, 256, 300, 10, SPLIT, IP, 12, 1),
    (3000, 128, 8, 256, 200, 56, F16, IP, 200, 1),  # ~15 rows per list: the probed lists hold fewer than k rows
]


@pytest.mark.parametrize("nb,d,M,ksub,nq,k,mode,metric,nlist,nprobe", CASES)
def test_codes_and_search_match_the_reference(hip_backend, nb, d, M, ksub, nq, k, mode, metric, nlist, nprobe):
    be = hip_backend
    xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=d + nq + k)
    c = _centroids(xb_s, nlist, metric, seed=nb + nprobe)
    packed = be.pack(xb, mode)
    lists = be.ivf_build(packed, c, metric)
    h = _host(be, packed, lists)
    assert (np.diff(h["off"]) == 0).any()  # the dead centroid's empty list
    books = _codebooks(h, M, ksub, seed=M)
    pq, codes, beta = _encode(be, packed, lists, h, books)
    _check_codes(h, books, codes, beta)
    assert int(codes.max()) < ksub
    D, I, probe = _search(be, packed, lists, pq, xq, mode, k, metric, nprobe)
    Dp, Ip = oracle.flat_search(h["c"], xq_s, nprobe, metric)
    assert synth.compare_topk(Dp, Ip, Dp, probe)[1] == 0
    xhat = pq_decode(h["c"], h["where"], books, codes)
    D_ref, I_ref = pq_reference(xhat, xq_s, k, metric, h["off"], h["rows"], probe)
    _check(D_ref, I_ref, D, I, rescore=(xhat, xq_s, metric, h["off"], h["rows"], probe))
    if nlist == 200:
        assert (I == -1).any()


def test_queries_beyond_one_chunk(hip_backend):
    """40 000 queries at M = 64 run as several chunks inside lvs_ivf_pq_search_keys (the tables bound a chunk)."""
    be = hip_backend
    nb, d, M, nq, k, nlist, nprobe = 20000, 128, 64, 40000, 10, 64, 4
    assert be.lib.lvs_ivf_pq_search_workspace_bytes(nq, nlist, nprobe, d, M, k, SPLIT) <= plan_native.ivf_limits()[0]
    for mode, metric in ((F16, IP), (SPLIT, L2)):
        xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=41 + mode)
        c = _centroids(xb_s, nlist, metric, seed=42)
        packed = be.pack(xb, mode)
        lists = be.ivf_build(packed, c, metric)
        h = _host(be, packed, lists)
        books = _codebooks(h, M, 256, seed=43)
        pq, codes, _ = _encode(be, packed, lists, h, books)
        D, I, probe = _search(be, packed, lists, pq, xq, mode, k, metric, nprobe)
        pick = np.unique(np.concatenate([np.random.default_rng(43).choice(nq, 200, replace=False),
                                         [0, 4095, 4096, 8191, 8192, 16383, 16384, 16385, 32767, 32768, nq - 1]]))
        Dp, Ip = oracle.flat_search(h["c"], xq_s[pick], nprobe, metric)
        assert synth.compare_topk(Dp, Ip, Dp, probe[pick])[1] == 0
        xhat = pq_decode(h["c"], h["where"], books, codes)
        D_ref, I_ref = pq_reference(xhat, xq_s[pick], k, metric, h["off"], h["rows"], probe[pick])
        _check(D_ref, I_ref, D[pick], I[pick], rescore=(xhat, xq_s[pick], metric, h["off"], h["rows"], probe[pick]))


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d,M", [(128, 16), (768, 96)])
def test_planted_lossless_rows(hip_backend, metric, d, M):
    """Rows c_l + concat_m cb[m][j_m], on a grid every storage holds exactly, encoded against that codebook: the decoded rows
    ARE the rows, so the IVF-PQ search equals the exact search over the probed lists."""
    be = hip_backend
    rng = np.random.default_rng(d + metric)
    nlist, nb, nq, k, dsub = 8, 4000, 17, 10, d // M
    books = (rng.integers(-16, 17, (M, 256, dsub)) / 64.0).astype(np.float32)
    c = np.zeros((nlist, d), np.float32)
    c[np.arange(nlist), np.arange(nlist)] = 4.0
    lid = rng.integers(0, nlist - 1, nb)  # list nlist - 1 stays empty
    j = rng.integers(0, 256, (nb, M))
    xb = (c[lid] + np.concatenate([books[m][j[:, m]] for m in range(M)], axis=1)).astype(np.float32)
    xq = (rng.integers(-16, 17, (nq, d)) / 64.0).astype(np.float32)
    xq[:, :nlist] += 2.0
    packed = be.pack(xb, SPLIT)
    lists = be.ivf_build(packed, c, metric)
    h = _host(be, packed, lists)
    assert np.array_equal(h["where"], lid) and np.array_equal(h["x"], xb)
    pq, codes, _ = _encode(be, packed, lists, h, books)
    assert np.array_equal(codes, j)
    for nprobe in (1, 3, nlist):
        D, I, probe = _search(be, packed, lists, pq, xq, SPLIT, k, metric, nprobe)
        D_ref, I_ref = ivf_reference(xb, xq, k, metric, c, h["off"], h["rows"], probe)
        _check(D_ref, I_ref, D, I, rescore=(xb, xq, metric, h["off"], h["rows"], probe))


@pytest.mark.parametrize("metric", [IP, L2])
def test_duplicated_rows_score_alike_in_row_order(hip_backend, metric):
    be = hip_backend
    nb, d, M = 4000, 384, 48
    xb, xb_s, _, _ = _data(nb, 1, d, SPLIT, seed=51)
    dup = np.sort(np.random.default_rng(52).choice(nb, 30, replace=False))
    xb[dup] = xb[dup[0]]
    packed = be.pack(xb, SPLIT)
    lists = be.ivf_build(packed, _centroids(xb.astype(np.float32), 16, metric, seed=53), metric)
    h = _host(be, packed, lists)
    assert len(set(h["where"][dup].tolist())) == 1
    pq, _, _ = _encode(be, packed, lists, h, _codebooks(h, M, 256, seed=54))
    q = xb[dup[0]:dup[0] + 1] + np.float32(1e-3)
    D, I, _ = _search(be, packed, lists, pq, q, SPLIT, 56, metric, 16)
    at = np.isin(I[0], dup)
    assert at.sum() == 30
    assert np.array_equal(I[0][at], dup)  # ascending row order
    assert (D[0][at] == D[0][at][0]).all()  # bit-identical scores


def test_device_training_matches_the_twin_rules(hip_backend):
    """ivf_pq_train on the device: ksub = min(256, training rows), codes of the trained codebooks as the twin's."""
    be = hip_backend
    xb, xb_s, _, _ = _data(3000, 1, 64, SPLIT, seed=61)
    packed = be.pack(xb, SPLIT)
    lists = be.ivf_build(packed, _centroids(xb_s, 8, IP, seed=62), IP)
    h = _host(be, packed, lists)
    for train, ksub in ((np.arange(0, 3000, 2), 256), (np.arange(100), 100)):
        books = be.ivf_pq_train(packed, lists, train, 8).cpu().numpy()
        assert books.shape == (8, ksub, 8) and np.isfinite(books).all()
        pq, codes, beta = _encode(be, packed, lists, h, books)
        _check_codes(h, books, codes, beta)


def _clustered(n, d, centers, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + 0.5 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype)


def _reference_of(vs, xq, k, nprobe):
    c, off, rows = vs.ivf_lists()
    books, codes, _ = vs.pq_codes()
    xhat = pq_decode(c, list_of_rows(off, rows, codes.shape[0]), books, codes)
    probe = vs.ivf_probe(xq, nprobe)
    D, I = pq_reference(xhat, np.asarray(xq, np.float32), k, vs.metric, off, rows, probe)
    return D, I, (xhat, np.asarray(xq, np.float32), vs.metric, off, rows, probe)


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_hipvs_3072_dims_from_float64(hip_backend, tmp_path, monkeypatch, metric):
    """text-embedding-3-large's width from float64 input (hi|lo storage): served by the PQ scan (no other IVF scan takes it),
    persisted and reloaded without training; ids subsets and K > 56 are the flat store's answers exactly."""
    from lotus_amd import cluster

    xb = _clustered(6000, 3072, 20, seed=21).astype(np.float64)
    xq = _clustered(40, 3072, 20, seed=22).astype(np.float64)
    d1 = str(tmp_path / "pq")
    vs = HipVS(factory_string="IVF16,PQ32", nprobe=4, metric=metric, device="cuda:0")
    vs.index(None, xb, d1)
    assert not vs.backend.ivf_fits(3072, 10, SPLIT) and not vs.backend.ivf_sq8_fits(3072, 10, SPLIT)
    vs.backend.timing_enable(True)
    out = vs(xq, 10)
    t = vs.backend.timing_read_full()
    vs.backend.timing_enable(False)
    assert t["kernel"] == "lvs_ivf_pq_scan_kernel" and t["calls"] == 1
    D_ref, I_ref, rescore = _reference_of(vs, xq, 10, 4)
    _check(D_ref, I_ref, out.distances, out.indices, rescore=rescore)

    monkeypatch.setattr(cluster, "kmeans", lambda *a, **k: pytest.fail("k-means was called"))
    r2 = HipVS(factory_string="IVF16,PQ32x8", nprobe=4, metric=metric, device="cuda:0")
    r2.load_index(d1)
    for u, v in zip(vs.ivf_lists() + vs.pq_codes(), r2.ivf_lists() + r2.pq_codes()):
        assert np.array_equal(u, v)
    again = r2(xq, 10)
    assert np.array_equal(again.indices, out.indices) and np.array_equal(again.distances, out.distances)

    flat = HipVS(metric=metric, device="cuda:0")
    flat.index(None, xb, str(tmp_path / "flat"), persist=False)
    ids = list(range(0, 6000, 7))
    a, b = r2(xq, 10, ids=ids), flat(xq, 10, ids=ids)
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.distances, b.distances)
    a, b = r2(xq, 60), flat(xq, 60)
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.distances, b.distances)


def test_pq_sq8_and_flat_stores_probe_the_same_lists(hip_backend, tmp_path):
    xb = _clustered(20000, 384, 30, seed=61, dtype=np.float16)
    xq = _clustered(300, 384, 30, seed=62, dtype=np.float16)
    stores = []
    for name in ("IVF32,PQ48", "IVF32,SQ8", "IVF32,Flat"):
        v = HipVS(factory_string=name, nprobe=4, device="cuda:0")
        v.index(None, xb, str(tmp_path / name.replace(",", "_")), persist=False)
        stores.append(v)
    for v in stores[1:]:
        for u, w in zip(stores[0].ivf_lists(), v.ivf_lists()):
            assert np.array_equal(u, w)
        assert np.array_equal(stores[0].ivf_probe(xq, 4), v.ivf_probe(xq, 4))
    # the decoded search finds a good share of the full-precision one's neighbours (0.34 measured: inside a cluster the
    # neighbours differ by noise that 8-dimensional subspaces resolve only in part; chance is ~0.004)
    ra, rb = stores[0](xq, 10).indices, stores[2](xq, 10).indices
    assert np.mean([len(set(x) & set(y)) / 10 for x, y in zip(ra, rb)]) > 0.25
