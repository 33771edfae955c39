"""Host side of the recall measurement of an IVF store, on the CPU (``IvfRecallOracleBackend``): ``HipVS.recall``,
``probe_recall_curve`` and ``tune_nprobe`` against a brute-force recall computed here, their routes and refusals, and the three
C entry points' declarations and argument checks.  The kernels are covered by tests/test_gpu_recall.py."""
import numpy as np
import pytest

from ivf_recall_oracle_backend import (IvfRecallOracleBackend, overlap_reference, probe_ranks_reference, row_lists_reference)
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, RecallReport, _capi

N, D_, NLIST, NQ, K = 600, 24, 10, 40, 10
MODES = ["IVF10,Flat", "IVF10,SQ8", "IVF10,PQ8", "IVF10,PQ8,Refine(Flat)"]
SCANS = ("ivf_search", "ivf_sq8_search", "ivf_pq_search")


def clustered(n, d, centers=12, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32) * 3
    x = c[rng.integers(0, centers, n)] + rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float16).astype(np.float32)  # fp16-exact values: every store holds what the test holds


@pytest.fixture(scope="module")
def data():
    return clustered(N, D_, seed=3), clustered(NQ, D_, seed=4)


def store(xb, fs="IVF10,Flat", metric=METRIC_INNER_PRODUCT, **kw):
    vs = HipVS(metric=metric, backend=IvfRecallOracleBackend(), factory_string=fs, **kw)
    vs.index(None, xb, "recall", persist=False)
    vs.backend.calls.clear()
    return vs


def names(vs, which=SCANS + ("keys_overlap", "ivf_probe_ranks", "search", "refine_keys")):
    return [c[0] for c in vs.backend.calls if c[0] in which]


def true_rows(xb, xq, k, metric):
    """The exact top k by the definition, float64 scores, ties to the lower row."""
    s = xq.astype(np.float64) @ xb.astype(np.float64).T
    if metric == METRIC_L2:
        s = -((xq.astype(np.float64) ** 2).sum(1)[:, None] + (xb.astype(np.float64) ** 2).sum(1)[None, :] - 2 * s)
    return np.stack([np.lexsort((np.arange(len(xb)), -s[q]))[:k] for q in range(len(xq))])


def brute_recall(vs, xq, truth, k, **kw):
    """(intersection, first, hits) of what ``vs(xq, k, **kw)`` returns against ``truth``."""
    got = vs(xq, k, **kw).indices
    hits = np.array([len(set(t.tolist()) & set(g[g >= 0].tolist())) for t, g in zip(truth, got)])
    first = np.array([t[0] in set(g.tolist()) for t, g in zip(truth, got)])
    return hits.sum() / truth.size, first.mean(), hits


def curve_by_definition(vs, xq, truth):
    """Entry p: share of the true rows whose list is among the query's best p lists."""
    _, off, rows = vs.ivf_lists()
    where = row_lists_reference(off, rows, N)
    probe = vs.ivf_probe(xq, NLIST)
    rank = np.array([[np.flatnonzero(probe[q] == where[r])[0] for r in truth[q]] for q in range(len(xq))])
    return np.array([(rank < p).mean() for p in range(NLIST + 1)])


# ---- recall ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
@pytest.mark.parametrize("fs", MODES)
def test_recall_is_the_brute_force_recall(data, fs, metric):
    xb, xq = data
    vs = store(xb, fs, metric, nprobe=2)
    truth = true_rows(xb, xq, K, metric)
    rep = vs.recall(xq, K, nprobe=[1, 3, NLIST, 4 * NLIST])
    assert isinstance(rep, RecallReport) and rep.nprobes == (1, 3, NLIST, NLIST) and rep.served == (True,) * 4
    assert (rep.nq, rep.K, rep.kc) == (NQ, K, K) and rep.hits.shape == (4, NQ) and rep.hits.dtype == np.int32
    assert rep.intersection.dtype == np.float64 and rep.first.dtype == np.float64
    assert names(vs).count("search") == 1  # the exact search: once for the four entries
    for i, p in enumerate((1, 3, NLIST, NLIST)):
        inter, first, hits = brute_recall(vs, xq, truth, K, nprobe=p)
        assert np.array_equal(rep.hits[i], hits), (fs, p)
        assert rep.intersection[i] == pytest.approx(inter, abs=1e-12) and rep.first[i] == pytest.approx(first, abs=1e-12)
    assert rep.intersection[0] < rep.intersection[2]
    if fs == "IVF10,Flat":
        assert rep.intersection[2] == 1.0 and rep.first[2] == 1.0
    one = vs.recall(xq, K)  # the store's own nprobe
    assert one.nprobes == (2,) and one.intersection[0] == pytest.approx(brute_recall(vs, xq, truth, K)[0], abs=1e-12)
    assert vs.nprobe == 2


def test_recall_measures_the_reranking_of_a_refined_store(data):
    xb, xq = data
    truth = true_rows(xb, xq, K, METRIC_INNER_PRODUCT)
    vs = store(xb, "IVF10,PQ8,Refine(Flat)", nprobe=4, k_factor=2)
    rep = vs.recall(xq, K)
    assert rep.kc == 2 * K and names(vs, SCANS + ("refine_keys",)) == ["ivf_pq_search", "refine_keys"]
    assert [c for c in vs.backend.calls if c[0] == "ivf_pq_search"][0][2] == 2 * K
    wide = vs.recall(xq, K, k_factor=5)
    assert wide.kc == 50 and vs.k_factor == 2
    for r, kw in ((rep, {}), (wide, {"k_factor": 5})):
        assert np.array_equal(r.hits[0], brute_recall(vs, xq, truth, K, **kw)[2])
    assert wide.intersection[0] >= rep.intersection[0]
    dev = vs.recall(vs.backend.to_device(xq), K)  # queries as a tensor
    assert np.array_equal(dev.hits, rep.hits)


def test_an_exact_route_is_reported_not_measured(data):
    xb, xq = data
    vs = store(xb, nprobe=3)
    rep = vs.recall(xq, 57, nprobe=[1, 5])  # K beyond the one-pass list scan: __call__ searches exactly
    assert rep.served == (False, False) and np.all(rep.intersection == 1.0) and np.all(rep.first == 1.0)
    assert np.all(rep.hits == 57) and rep.nprobes == (1, 5)
    p, one = vs.tune_nprobe(xq, 57, target=0.9)
    assert p == 3 and vs.nprobe == 3 and one.served == (False,) and one.nprobes == (3,)
    assert names(vs) == []  # no list scan, no comparison, not even the exact search


def test_refusals(data):
    xb, xq = data
    flat = store(xb, "Flat")
    for call in (lambda v: v.recall(xq, K), lambda v: v.probe_recall_curve(xq, K), lambda v: v.tune_nprobe(xq, K)):
        with pytest.raises(ValueError, match="no IVF lists"):
            call(flat)
        ivf = store(xb)
        for lay in ((0, 1, 1, 2, None, None), (1, 2, 0, 1, None, None)):  # rows, then queries, split over two ranks
            ivf._lay = lay
            with pytest.raises(ValueError, match="unsharded"):
                call(ivf)
    vs = store(xb)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="K must be"):
            vs.recall(xq, bad)
        with pytest.raises(ValueError, match="K must be"):
            vs.tune_nprobe(xq, bad)
    for bad in (0, [1, 0], [], 1.5, "3"):
        with pytest.raises(ValueError, match="nprobe"):
            vs.recall(xq, K, nprobe=bad)
    for bad in (0, 0.0, 1.5, -0.1, "0.9", None, True, float("nan")):
        with pytest.raises(ValueError, match="target"):
            vs.tune_nprobe(xq, K, target=bad)
    with pytest.raises(ValueError, match="measure"):
        vs.tune_nprobe(xq, K, measure="recall@1")
    with pytest.raises(ValueError, match="k_factor"):
        vs.tune_nprobe(xq, K, k_factor=0.5)
    with pytest.raises(ValueError, match="max_nprobe|nprobe"):
        vs.probe_recall_curve(xq, K, max_nprobe=0)
    with pytest.raises(ValueError, match="dimension"):
        vs.recall(xq[:, :8], K)
    with pytest.raises(ValueError, match="no query"):
        vs.recall(xq[:0], K)
    assert names(vs) == [] and vs.nprobe == 1


# ---- the probe-limited curve -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
def test_curve_is_the_recall_of_a_flat_store(data, metric):
    xb, xq = data
    vs = store(xb, "IVF10,Flat", metric)
    curve = vs.probe_recall_curve(xq, K)
    assert curve.dtype == np.float64 and curve.shape == (NLIST + 1,) and curve[0] == 0.0 and curve[-1] == 1.0
    assert np.all(np.diff(curve) >= 0)
    assert names(vs, SCANS) == []  # one exact search, one coarse step, the ranks: no list scan
    assert np.allclose(curve, curve_by_definition(vs, xq, true_rows(xb, xq, K, metric)), atol=1e-12, rtol=0)
    rep = vs.recall(xq, K, nprobe=range(1, NLIST + 1))
    assert np.array_equal(curve[1:], rep.intersection)  # the identity, to the bit
    short = vs.probe_recall_curve(xq, K, max_nprobe=4)
    assert np.array_equal(short, curve[:5])
    assert np.array_equal(vs.probe_recall_curve(xq, K, max_nprobe=1000), curve)


@pytest.mark.parametrize("fs", MODES[1:])
def test_curve_bounds_the_code_modes(data, fs):
    xb, xq = data
    vs = store(xb, fs, k_factor=3)
    curve = vs.probe_recall_curve(xq, K)
    rep = vs.recall(xq, K, nprobe=range(1, NLIST + 1))
    assert np.all(rep.intersection <= curve[1:] + 1e-12)
    if "Refine" not in fs:
        assert np.any(rep.intersection < curve[1:])  # ... and the codes alone do cost something at this size


def test_row_lists_are_made_once(data):
    xb, xq = data
    vs = store(xb)
    vs.probe_recall_curve(xq, K)
    vs.probe_recall_curve(xq, 3)
    assert [c[0] for c in vs.backend.calls].count("ivf_row_lists") == 1
    ent = vs._current()
    _, off, rows = vs.ivf_lists()
    assert np.array_equal(ent.ivf.row_list.numpy(), row_lists_reference(off, rows, N))
    plain = store(xb)
    plain(xq, K)
    assert plain._current().ivf.row_list is None  # stores that never ask pay nothing


# ---- tune_nprobe -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["intersection", "first"])
@pytest.mark.parametrize("target", [0.5, 0.9, 1.0])
def test_tune_a_flat_store(data, measure, target):
    xb, xq = data
    vs = store(xb, nprobe=1)
    p, rep = vs.tune_nprobe(xq, K, target=target, measure=measure)
    assert names(vs, SCANS + ("keys_overlap",)) == []  # the ceiling is the answer: nothing approximate ran
    assert vs.nprobe == p and rep.nprobes == (p,) and rep.served == (True,) and rep.hits.shape == (1, NQ)
    again = vs.recall(xq, K, nprobe=[p] if p == 1 else [p, p - 1])
    assert getattr(again, measure)[0] >= target
    assert again.intersection[0] == rep.intersection[0] and again.first[0] == rep.first[0]
    assert np.array_equal(again.hits[0], rep.hits[0])
    if p > 1:
        assert getattr(again, measure)[1] < target  # the value one below does not reach it


@pytest.mark.parametrize("fs", MODES[1:])
def test_tune_a_code_store(data, fs):
    xb, xq = data
    vs = store(xb, fs, nprobe=1, k_factor=4)
    full = vs.recall(xq, K, nprobe=range(1, NLIST + 1)).intersection
    target = float(np.sort(full)[len(full) // 2])  # a value the store does reach
    vs.backend.calls.clear()
    p, rep = vs.tune_nprobe(xq, K, target=target, apply=False)
    assert vs.nprobe == 1  # apply=False leaves the store alone
    assert rep.nprobes == (p,) and rep.intersection[0] == full[p - 1] >= target
    curve = vs.probe_recall_curve(xq, K)
    assert curve[p] >= target and (p == 1 or curve[p - 1] < target or np.any(full[:p - 1] < target))
    assert len(names(vs, SCANS)) <= 2 + 2 * int(np.ceil(np.log2(NLIST)))  # doubling and bisection, not a sweep
    p2, _ = vs.tune_nprobe(xq, K, target=target)
    assert p2 == p and vs.nprobe == p and vs.k_factor == 4


def test_an_unreachable_target_names_both_figures(data):
    xb, xq = data
    vs = store(xb, "IVF10,PQ8", nprobe=2)
    full = vs.recall(xq, K, nprobe=NLIST)
    assert full.intersection[0] < 1.0  # 8 bytes per row do not rank 600 rows exactly
    with pytest.raises(ValueError) as e:
        vs.tune_nprobe(xq, K, target=1.0)
    msg = str(e.value)
    assert f"best measured is {full.intersection[0]:.4f}" in msg and "ceiling at nprobe=10 is 1.0000" in msg
    assert vs.nprobe == 2


def test_the_coarse_ranking_widens_only_on_demand(data, monkeypatch):
    xb, xq = data
    monkeypatch.setattr(_capi, "IVF_MAX_K", 4)  # the one-pass bound of the searches: 10 lists stand in for thousands
    vs = store(xb)
    widths = lambda: [c[3] for c in vs.backend.calls if c[0] == "ivf_probe_ranks"]  # noqa: E731
    full = vs.recall(xq, 3, nprobe=range(1, NLIST + 1)).intersection
    low, high = float(full[1]), 1.0
    assert full[3] < high
    vs.backend.calls.clear()
    p, rep = vs.tune_nprobe(xq, 3, target=low)
    assert widths() == [4] and p == 1 + int(np.flatnonzero(full >= low)[0]) <= 2  # the one-pass ranking settles it
    vs.backend.calls.clear()
    p, rep = vs.tune_nprobe(xq, 3, target=high)
    assert widths() == [4, NLIST] and p == 1 + int(np.flatnonzero(full >= high)[0]) > 4 and rep.intersection[0] == 1.0
    assert names(vs, SCANS + ("keys_overlap",)) == []


@pytest.mark.parametrize("fs", ["IVF10,Flat", "IVF10,SQ8"])
def test_probes_that_fall_short_are_named(data, fs, monkeypatch):
    xb, xq = data
    monkeypatch.setattr(_capi, "MAX_K", 3)  # as if nlist were beyond the 2 048 lists a search may probe
    vs = store(xb, fs)
    curve = vs.probe_recall_curve(xq, 3)
    assert curve.shape == (4,) and curve[3] < 1.0
    with pytest.raises(ValueError) as e:
        vs.tune_nprobe(xq, 3, target=1.0)
    measured = vs.recall(xq, 3, nprobe=3).intersection[0]
    assert f"best measured is {measured:.4f} at nprobe=3" in str(e.value)
    assert f"ceiling at nprobe=3 is {curve[3]:.4f}" in str(e.value)


# ---- the doubles' own rules ------------------------------------------------------------------------------------------------
def test_reference_rules():
    k = lambda score, row: (np.uint64(score) << np.uint64(32)) | np.uint64(0xFFFFFFFF - row)  # noqa: E731
    truth = np.array([[k(9, 5), k(8, 0), k(7, 2 ** 31), 0], [0, k(3, 1), 0, 0]], np.uint64)
    got = np.array([[k(1, 2 ** 31), k(2, 5), k(2, 5)], [k(3, 1), 0, 0]], np.uint64)
    hits, first = overlap_reference(truth, got)
    assert hits.tolist() == [2, 1] and first.tolist() == [1, 0]
    off, rows = np.array([0, 0, 2, 2, 3, 3]), np.array([2, 0, 1], np.uint32)
    assert row_lists_reference(off, rows, 3).tolist() == [1, 3, 1]
    rank, hist = probe_ranks_reference(np.array([[k(1, 0), k(1, 1), 0, k(1, 7)]], np.uint64), np.array([1, 3, 1], np.int32),
                                       np.array([[3, -1]], np.int32))
    assert rank.tolist() == [[2, 0, -1, -1]] and hist.tolist() == [1, 0, 1]


# ---- the C entry points ----------------------------------------------------------------------------------------------------
def test_declared_symbols():
    assert {"lvs_keys_overlap", "lvs_ivf_row_lists", "lvs_ivf_probe_ranks"} <= set(_capi.declared_symbols())
    assert {"lvs_keys_overlap", "lvs_ivf_row_lists", "lvs_ivf_probe_ranks"} <= set(_capi.SIGNATURES)


def test_recall_argument_checks_without_a_gpu():
    # every answer below is decided before a device is touched; 256 stands for a buffer that is never read
    lib = _capi.load()
    B = 256
    overlap = lambda kt=10, kg=10, nq=5, t=B, g=B, h=B, f=B: lib.lvs_keys_overlap(t, kt, g, kg, nq, h, f, None)  # noqa: E731
    for kw, word in (({"kt": 0}, b"kt=0"), ({"kt": 2049}, b"kt=2049"), ({"kg": 0}, b"kg=0"), ({"kg": 2049}, b"kg=2049"),
                     ({"nq": -1}, b"nq=-1"), ({"t": None}, b"NULL"), ({"g": None}, b"NULL"), ({"h": None}, b"NULL"),
                     ({"f": None}, b"NULL")):
        assert overlap(**kw) == _capi.EINVAL, kw
        assert word in lib.lvs_last_error() and b"lvs_keys_overlap" in lib.lvs_last_error(), kw
    assert overlap(nq=0, t=None, g=None, h=None, f=None) == _capi.OK  # no queries: nothing to do
    assert overlap(nq=0, kt=0) == _capi.EINVAL  # ... but the arguments are still checked

    row_lists = lambda n=10, nlist=4, o=B, r=B, out=B: lib.lvs_ivf_row_lists(o, r, n, nlist, out, None)  # noqa: E731
    for kw, word in (({"nlist": 0}, b"nlist=0"), ({"nlist": -3}, b"nlist=-3"), ({"n": -1}, b"n=-1"), ({"n": 2 ** 32}, b"n="),
                     ({"o": None}, b"NULL"), ({"r": None}, b"NULL"), ({"out": None}, b"NULL")):
        assert row_lists(**kw) == _capi.EINVAL, kw
        assert word in lib.lvs_last_error() and b"lvs_ivf_row_lists" in lib.lvs_last_error(), kw
    assert row_lists(n=0, o=None, r=None, out=None) == _capi.OK
    assert row_lists(n=0, nlist=0) == _capi.EINVAL

    def ranks(kt=10, n=100, P=8, nq=5, t=B, rl=B, pr=B, rank=B, hist=B):
        return lib.lvs_ivf_probe_ranks(t, kt, rl, n, pr, P, nq, rank, hist, None)

    for kw, word in (({"kt": 0}, b"kt=0"), ({"kt": 2049}, b"kt=2049"), ({"P": 0}, b"P=0"), ({"P": 2049}, b"P=2049"),
                     ({"nq": -1}, b"nq=-1"), ({"n": -1}, b"n=-1"), ({"t": None}, b"NULL"), ({"rl": None}, b"NULL"),
                     ({"pr": None}, b"NULL"), ({"rank": None}, b"NULL"), ({"hist": None}, b"NULL")):
        assert ranks(**kw) == _capi.EINVAL, kw
        assert word in lib.lvs_last_error() and b"lvs_ivf_probe_ranks" in lib.lvs_last_error(), kw
    assert ranks(nq=0, t=None, rl=None, pr=None, rank=None, hist=None) == _capi.OK
    assert ranks(nq=0, P=0) == _capi.EINVAL
