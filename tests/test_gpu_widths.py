"""The flat path at the widths users index - d = 192 .. 4 096 - on the device: every case of tests/width_cases.py asserts the
kernel that served it and is checked by ``check_topk_exact`` against the float64 scores of the stored values (bar 1e-5, gap
2e-5, nothing excused); tests/test_widths_host.py shows on the CPU which branch each stream case reaches and that the checker
rejects a kernel that drops a fragment or a segment.  Then the same widths through the score matrix, the threshold join, the
k-means assignment and sums, and the store.

Every test prints what it measured (run with -s): the class reached, the largest score error against the bar, and the certified
searches' open queries."""
import numpy as np
import pytest

import synth
import width_cases as wc
from lotus_amd import _capi
from width_cases import BAR, F16, GAP, IP, L2, SPLIT

pytestmark = pytest.mark.gpu

assert (F16, SPLIT, IP, L2) == (_capi.PACK_F16, _capi.PACK_SPLIT, _capi.METRIC_IP, _capi.METRIC_L2)
NDUP = 1000  # rows appended again for the tie-order check


def _pack(be, x, mode, **kw):
    return be.pack(x.astype(np.float16) if mode == F16 else x, mode, **kw)


def _search(be, cb, cq, k, metric, **kw):
    """-> (D in the score sense - larger is better -, I, name of the last timed kernel)"""
    be.timing_enable(True)
    keys = be.search_keys(cb, cq, k, metric, **kw)
    D, I = be.keys_to_result(keys, metric)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    assert t["calls"] >= 1, t
    D = D.cpu().numpy().astype(np.float64)
    return (D if metric == IP else -D), I.cpu().numpy(), t["kernel"]


def _with_duplicates(be, c, xb, cq, S, **kw):
    """The duplicate check of test_small_batch_streaming_kernel: the first NDUP rows appended again.  A row and its copy score
    exactly alike, so the copy never comes without the row, and only behind it; and the ids are the float64 reference's in
    every slot.  (Two DISTINCT rows can come closer at these widths than float32 resolves - the float32 CPU oracle differs from
    the float64 ids in 2 slots of stream-d1024-FF-q33 -, so a change of a kernel's summation order may move an id here without
    being wrong: check_topk_exact on the same result says whether it is.)"""
    kd = min(c.k, 8)
    xd, Sd = np.concatenate([xb, xb[:NDUP]]), np.concatenate([S, S[:, :NDUP]], axis=1)
    D, I, _ = _search(be, _pack(be, xd, c.bmode), cq, kd, c.metric, **kw)
    wc.check_topk_exact(Sd, D, I, kd)
    for q in range(c.nq):
        copies = np.flatnonzero(I[q] >= c.nb)
        firsts = [np.flatnonzero(I[q] == I[q, s] - c.nb) for s in copies]
        assert all(f.size == 1 and f[0] < s for f, s in zip(firsts, copies)), f"query {q}: a copy without its row first: {I[q].tolist()}"
    _, Ir = wc.topk64(Sd, kd)
    assert np.array_equal(I, Ir), f"{int((I != Ir).sum())} of {I.size} ids differ from the float64 reference's"


@pytest.mark.parametrize("c", wc.STREAM_CASES + wc.TILE_CASES, ids=lambda c: c.name)
def test_widths_topk(hip_backend, c):
    be = hip_backend
    xb, xq = wc.case_data(c)
    S = wc.case_scores(c, xb, xq)
    cb, cq = _pack(be, xb, c.bmode), _pack(be, xq, c.qmode)
    D, I, kernel = _search(be, cb, cq, c.k, c.metric, one_pass=False)
    assert kernel == c.kernel, (c.name, kernel)
    err = wc.check_topk_exact(S, D, I, c.k)
    print(f"\n{c.name}: {kernel} {tuple(c.cls) if c.cls else ''} max score error {err:.3e} (bar {BAR:.0e})")
    _with_duplicates(be, c, xb, cq, S, one_pass=False)


@pytest.mark.parametrize("c", wc.CERT_CASES, ids=lambda c: c.name)
def test_widths_one_pass_certified(hip_backend, c):
    """One MFMA pass over the hi parts, exact rescoring and the certificate (k = 1: winner and runner-up) at 24 and 48 K-steps per
    segment.  No bar on how many queries stay open - nothing in the project gives one at these widths -; the result obeys the
    same checker whatever the share."""
    be = hip_backend
    xb, xq = wc.case_data(c)
    S = wc.case_scores(c, xb, xq)
    cb, cq = _pack(be, xb, c.bmode), _pack(be, xq, c.qmode)
    stats = {}
    D, I, _ = _search(be, cb, cq, c.k, c.metric, one_pass=True, stats=stats)
    assert stats.get("queries") == c.nq, stats  # the certified route ran
    print(f"\n{c.name}: uncertified {stats.get('uncertified', 0)} plain {stats.get('plain', 0)} of {c.nq} queries", end="")
    err = wc.check_topk_exact(S, D, I, c.k)
    print(f", max score error {err:.3e} (bar {BAR:.0e})")
    _with_duplicates(be, c, xb, cq, S, one_pass=True)


@pytest.mark.parametrize("d", [192, 1100, 3072])
@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_widths_scores_matrix(hip_backend, mode, d):
    """lvs_tile_kernel in SCORES mode (lvs_scores has no other kernel and no timing hook to ask); data and bars of
    test_gpu_parity.py::test_scores_matrix."""
    be = hip_backend
    tol = 2e-6 if mode == F16 else 1e-5
    xb = synth.corpus(777, d, seed=3) * np.float32(2.0)
    xq, _ = synth.queries(xb, 150, seed=6)
    cb, cq = _pack(be, xb, mode), _pack(be, xq, mode)
    a, b = wc.stored64(xq, mode), wc.stored64(xb, mode)
    for metric, rel in ((IP, tol), (L2, 2e-5)):
        Sd = be.scores(cb, cq, metric).cpu().numpy()
        ref = wc.scores64(b, a, metric)
        err, bar = np.abs(Sd - ref).max(), rel * max(1.0, np.abs(ref).max())
        print(f"\nscores d={d} mode={mode} metric={metric}: max error {err:.3e} (bar {bar:.3e})", end="")
        assert err <= bar, (d, mode, metric, err, bar)


JOIN_N, JOIN_PLANTED, JOIN_THRESHOLD = 3000, 200, 0.9


def _join_rows(d):
    """Unit rows; the last JOIN_PLANTED are near-duplicates of the first, at cosines spread over 0.8 .. 0.9995."""
    x = synth.corpus(JOIN_N, d, seed=41)
    u = synth.corpus(JOIN_PLANTED, d, seed=42)
    cos = np.linspace(0.8, 0.9995, JOIN_PLANTED).astype(np.float32)[:, None]
    y = cos * x[:JOIN_PLANTED] + np.sqrt(1 - cos * cos) * u
    x[-JOIN_PLANTED:] = y / np.linalg.norm(y, axis=1, keepdims=True)
    return x


@pytest.mark.parametrize("d", [312, 1536])
@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_widths_threshold_self_join(hip_backend, mode, d):
    """lvs_tile_kernel in RANGE mode: the pair set of the float64 brute force.  The threshold sits where no float64 score lies
    within the gap of it (asserted), so no pair's membership hangs on the device's rounding."""
    be = hip_backend
    x = _join_rows(d)
    S = wc.scores64(wc.stored64(x, mode), wc.stored64(x, mode), IP)
    S[np.tril_indices(JOIN_N)] = -np.inf  # a self-join reports j > i only
    assert not (np.abs(S - JOIN_THRESHOLD) <= GAP).any()
    want = S > JOIN_THRESHOLD
    assert 60 <= want.sum() <= JOIN_PLANTED and want[:JOIN_PLANTED, -JOIN_PLANTED:].sum() == want.sum()
    p = _pack(be, x, mode)
    be.timing_enable(True)
    q, j, sc = be.range_join(p, p, JOIN_THRESHOLD, IP, q_row0=0)
    t = be.timing_read_full()
    be.timing_enable(False)
    assert t["kernel"] == "lvs_tile_kernel" and t["calls"] >= 1, t
    q, j, sc = q.cpu().numpy(), j.cpu().numpy(), sc.cpu().numpy().astype(np.float64)
    got = np.zeros_like(want)
    got[q, j] = True
    assert got.sum() == len(q), "a pair twice"
    assert np.array_equal(got, want), (int((got & ~want).sum()), int((want & ~got).sum()))
    err = np.abs(sc - S[q, j]).max()
    print(f"\njoin d={d} mode={mode}: {len(q)} pairs, max score error {err:.3e} (bar {BAR:.0e})", end="")
    assert err <= BAR


@pytest.mark.parametrize("d", [128, 192, 1536, 3072])  # nkd 2, 3 (lvs_assign_kernel's first skewed launch), 24, 48
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_widths_nearest_centroid(hip_backend, mode, metric, d):
    """be.nearest, 3 000 points x 257 centroids: the centroid returned is within the gap of the best in float64, its score within
    the bar of that centroid's float64 score."""
    be = hip_backend
    nq, nc = 3000, 257
    c = synth.corpus(nc, d, seed=51)
    x, _ = synth.queries(c, nq, seed=52)
    if metric == L2:
        c = c * wc.L2_CORPUS_SCALE
    S = wc.scores64(wc.stored64(c, mode), wc.stored64(x, mode), metric)
    stats = {}
    keys = be.nearest(_pack(be, c, mode), _pack(be, x, mode), metric, stats=stats)
    D, I = be.keys_to_result(keys, metric)
    D, I = D.cpu().numpy().astype(np.float64)[:, 0], I.cpu().numpy()[:, 0]
    D = D if metric == IP else -D
    assert ((I >= 0) & (I < nc)).all()
    mine = S[np.arange(nq), I]
    short, err = (S.max(axis=1) - mine).max(), np.abs(D - mine).max()
    print(f"\nnearest d={d} mode={mode} metric={metric}: worst choice {short:.3e} below the best (gap {GAP:.0e}), max score "
          f"error {err:.3e} (bar {BAR:.0e}), uncertified {stats.get('uncertified', 0)} of {stats.get('queries', 0)}", end="")
    assert short <= GAP and err <= BAR, (short, err)


@pytest.mark.parametrize("d,mode", [(1100, F16), (3072, SPLIT)])
def test_widths_accumulate_is_exact_and_in_row_order(hip_backend, d, mode):
    """The method of test_gpu_kmeans.py::test_accumulate_is_exact_and_in_row_order: same values, same order, the same bits."""
    be = hip_backend
    rng = np.random.default_rng(d)
    n, k = 3000, 37
    x = (rng.standard_normal((n, d)) * 2).astype(np.float32)
    assign = rng.integers(0, k, n).astype(np.int64)
    assign[rng.integers(0, n, 50)] = -1  # skipped rows
    assign[assign == 5] = 6              # an empty cluster
    sums, counts = be.kmeans_accumulate(_pack(be, x, mode), be.to_device(assign), k)
    vals = wc.stored64(x, mode).astype(np.float32)  # hi + lo is exact in float32
    assert np.array_equal(vals.astype(np.float64), wc.stored64(x, mode))
    ref, ok = np.zeros((k, d), np.float32), assign >= 0
    np.add.at(ref, assign[ok], vals[ok])
    assert np.array_equal(counts.cpu().numpy(), np.bincount(assign[ok], minlength=k).astype(np.float32))
    assert np.array_equal(sums.cpu().numpy(), ref)
    assert counts[5].item() == 0 and not sums[5].any().item()


@pytest.mark.parametrize("nq", [1, 200])
def test_widths_through_the_store(hip_backend, tmp_path, nq):
    """HipVS() flat over float32 rows of d = 1 536 - text-embedding-3-small through the default store - in the caller's units."""
    from lotus_amd import HipVS

    nb, d, k = 3000, 1536, 10
    xb = synth.corpus(nb, d, seed=61)
    xq, _ = synth.queries(xb, nq, seed=62)
    vs = HipVS(backend=hip_backend)
    vs.index(None, xb, str(tmp_path / "i"))
    ent = vs._current()
    assert ent.packed.mode == SPLIT
    # the store keeps hi|lo rows scaled by a power of two (exact), and the queries share the index's exponent
    scale = np.float32(2.0 ** ent.packed.exp)
    xb_s, xq_s = wc.stored64(xb * scale, SPLIT) / float(scale), wc.stored64(xq * scale, SPLIT) / float(scale)
    assert np.abs(xb_s - xb).max() <= 2.0 ** -21 * np.abs(xb).max()
    hip_backend.timing_enable(True)
    out = vs(xq, k)
    t = hip_backend.timing_read_full()
    hip_backend.timing_enable(False)
    assert t["kernel"] == "lvs_tile_kernel" and t["calls"] >= 1, t  # 192 hi|lo query fragments: no stream launch
    err = wc.check_topk_exact(wc.scores64(xb_s, xq_s, IP), out.distances, out.indices, k)
    print(f"\nHipVS d={d} nq={nq}: max score error {err:.3e} (bar {BAR:.0e})", end="")
