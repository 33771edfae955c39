"""The recall kernels on the device - ``lvs_keys_overlap``, ``lvs_ivf_row_lists``, ``lvs_ivf_probe_ranks`` through their
``HipBackend`` methods, against numpy set arithmetic - and ``HipVS.recall`` / ``probe_recall_curve`` / ``tune_nprobe`` end to end
on stores of every IVF mode.  The host side is covered by tests/test_recall_host.py."""
import numpy as np
import pytest

from ivf_recall_oracle_backend import probe_ranks_reference, row_lists_reference
from lotus_amd import HipVS
from lotus_amd.backend import IvfLists, _ptr

pytestmark = pytest.mark.gpu

SPECIAL_ROWS = np.array([0, 2 ** 31, 2 ** 32 - 2], np.uint64)  # both ends of the 0xFFFFFFFF - row fold, and the sign bit
TIE_GAP, NEAR_TIE_CAP = 2e-5, 0.15


def make_keys(rng, rows):
    """rows (uint64, any shape) -> keys with a random non-zero score half each."""
    hi = rng.integers(1, 2 ** 32, rows.shape, dtype=np.uint64)
    return (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rows.astype(np.uint64))


def dev(be, a):
    return be.to_device(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a))


def host(t):
    return t.cpu().numpy()


# ---- lvs_keys_overlap ------------------------------------------------------------------------------------------------------
def overlap_case(nq, kt, kg, seed):
    """Per query: distinct truth rows and got rows drawn (with repeats) from a universe that shares about half of them, the
    special rows among both; empty tails of random length in either list; then, by query number, whole rows emptied, got
    made identical to truth (where the widths allow) and got made disjoint from truth."""
    rng = np.random.default_rng([seed, nq, kt, kg])
    universe = np.concatenate([SPECIAL_ROWS, rng.choice(np.arange(1, 10 ** 6, dtype=np.uint64), 2 * (kt + kg), replace=False)])
    truth, got = np.zeros((nq, kt), np.uint64), np.zeros((nq, kg), np.uint64)
    for q in range(nq):
        t_rows = rng.permutation(universe)[:kt]
        g_rows = rng.choice(universe, kg, replace=True)  # a row may repeat in got
        if q % 7 == 3 and kt == kg:
            g_rows = t_rows.copy()  # identical lists (other score halves)
        if q % 7 == 4:
            g_rows = np.setdiff1d(universe, t_rows)[rng.integers(0, len(universe) - kt, kg)]  # disjoint lists
        truth[q], got[q] = make_keys(rng, t_rows), make_keys(rng, g_rows)
        truth[q, kt - int(rng.integers(0, kt)):] = 0  # empty tails: 0 .. k - 1 slots (slot 0 of truth stays)
        got[q, kg - int(rng.integers(0, kg)):] = 0
        if q % 7 == 5:
            truth[q] = 0
        if q % 7 == 6:
            got[q] = 0
    return truth, got


def overlap_by_sets(truth, got):
    low = np.uint64(0xFFFFFFFF)
    hits, first = np.zeros(len(truth), np.int32), np.zeros(len(truth), np.int32)
    for q in range(len(truth)):
        g_rows = (got[q] & low)[got[q] != 0]
        found = np.isin(truth[q] & low, g_rows) & (truth[q] != 0)
        hits[q], first[q] = found.sum(), found[0]
    return hits, first


@pytest.mark.parametrize("kt,kg", [(1, 1), (10, 10), (56, 56), (10, 56), (64, 2048), (2048, 2048)])
@pytest.mark.parametrize("nq", [1, 3, 64, 257])
def test_keys_overlap(hip_backend, nq, kt, kg):
    be = hip_backend
    truth, got = overlap_case(nq, kt, kg, seed=11)
    hits, first = be.keys_overlap(dev(be, truth), dev(be, got))
    assert hits.dtype == first.dtype == be.torch.int32 and tuple(hits.shape) == tuple(first.shape) == (nq,)
    want_hits, want_first = overlap_by_sets(truth, got)
    assert np.array_equal(host(hits), want_hits) and np.array_equal(host(first), want_first)
    if nq >= 64 and kt > 1:
        assert 0 < want_hits.sum() < (truth != 0).sum() and 0 < want_first.sum() < nq  # the case does tell hits from misses


def test_keys_overlap_planted(hip_backend):
    be, rng = hip_backend, np.random.default_rng(5)
    t_rows = np.array([[0, 2 ** 31, 2 ** 32 - 2, 7, 9], [2 ** 31 - 1, 2 ** 31 + 1, 1, 2 ** 32 - 3, 5]], np.uint64)
    g_rows = np.array([[9, 9, 9, 2 ** 32 - 2, 0, 2 ** 31, 8], [2 ** 31, 2 ** 32 - 2, 0, 2, 4, 6, 5]], np.uint64)
    truth, got = make_keys(rng, t_rows), make_keys(rng, g_rows)
    hits, first = be.keys_overlap(dev(be, truth), dev(be, got))
    assert host(hits).tolist() == [4, 1] and host(first).tolist() == [1, 0]  # 9 repeated in got counts once
    truth[0, 0] = 0  # an empty first slot is no hit, whatever got holds
    hits, first = be.keys_overlap(dev(be, truth), dev(be, got))
    assert host(hits).tolist() == [3, 1] and host(first).tolist() == [0, 0]
    e = be.torch.empty((0, 5), dtype=be.torch.int64, device=be.device)
    hits, first = be.keys_overlap(e, e)  # no queries: no launch
    assert tuple(hits.shape) == (0,)


# ---- lvs_ivf_row_lists -----------------------------------------------------------------------------------------------------
def lists_case(n, nlist, shape, seed):
    """(offsets, rows): ``shape`` picks which lists hold rows - "middle": a stretch inside, empty runs at both ends and holes
    in between; "one": a single list holds every row; "all": any list may."""
    rng = np.random.default_rng([seed, n, nlist])
    if shape == "one":
        allowed = np.array([int(rng.integers(0, nlist))])
    elif shape == "all" or nlist < 3:
        allowed = np.arange(nlist)
    else:
        a, b = nlist // 3, max(nlist // 3 + 1, nlist - nlist // 4)
        allowed = np.arange(a, b)[rng.random(b - a) < 0.6]
        allowed = allowed if allowed.size else np.array([a])
    assign = allowed[rng.integers(0, allowed.size, n)]
    rows = np.argsort(assign, kind="stable")
    perm = rng.permutation(n)  # row numbers in no particular order inside a list
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(assign, minlength=nlist), out=off[1:])
    return off, perm[rows].astype(np.uint32)


@pytest.mark.parametrize("shape", ["middle", "one", "all"])
@pytest.mark.parametrize("nlist", [1, 2, 4097, 8200])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 20001])
def test_row_lists(hip_backend, n, nlist, shape):
    be = hip_backend
    off, rows = lists_case(n, nlist, shape, seed=3)
    lists = IvfLists(centroids=None, offsets=be.to_device(off), rows=be.to_device(rows.view(np.int32)), nlist=nlist, metric=0)
    out = be.ivf_row_lists(lists)
    assert out.dtype == be.torch.int32 and tuple(out.shape) == (n,) and be.ivf_row_lists(lists) is out
    got = host(out)
    assert np.array_equal(got, row_lists_reference(off, rows, n))
    pos = np.arange(n)
    assert np.all(off[got[rows]] <= pos) and np.all(pos < off[got[rows] + 1])  # position p lies inside the list of rows[p]


# ---- lvs_ivf_probe_ranks ---------------------------------------------------------------------------------------------------
def ranks_case(P, nq, kt, seed):
    rng = np.random.default_rng([seed, P, nq, kt])
    n, nlist = 5000, P + 9
    row_list = rng.integers(0, nlist, n).astype(np.int32)
    row_list[rng.random(n) < 0.02] = -1  # rows in no list
    probe = np.stack([rng.permutation(nlist)[:P] for _ in range(nq)]).astype(np.int32)
    if P > 2:
        probe[rng.random(probe.shape) < 0.1] = -1  # padding inside the ranking, not only at its end
        probe[:, 0] = np.where(probe[:, 0] < 0, 0, probe[:, 0])
    rows = rng.integers(0, n, (nq, kt)).astype(np.uint64)
    by_list = [np.flatnonzero(row_list == l) for l in range(nlist)]
    for q in range(nq):  # planted: a row of the first probed list, of the last one, and of a list that is not probed
        valid = np.flatnonzero(probe[q] >= 0)
        out = np.setdiff1d(np.arange(nlist), probe[q])
        for slot, l in ((0, probe[q, valid[0]]), (kt // 2, probe[q, valid[-1]]), (kt - 1, out[q % out.size])):
            if by_list[l].size:
                rows[q, slot] = by_list[l][q % by_list[l].size]
    truth = make_keys(rng, rows)
    truth[rng.random(truth.shape) < 0.1] = 0  # empty slots anywhere
    past = rng.random(truth.shape) < 0.03  # row numbers past the image: skipped, never read
    truth[past] = make_keys(rng, rng.integers(n, 2 ** 32 - 1, int(past.sum()), dtype=np.uint64))
    if nq > 2:
        truth[2] = 0
    return truth, row_list, probe, n


@pytest.mark.parametrize("kt", [1, 10, 130])
@pytest.mark.parametrize("P", [1, 3, 64, 65, 2048])
def test_probe_ranks(hip_backend, P, kt):
    be, nq = hip_backend, 37
    truth, row_list, probe, n = ranks_case(P, nq, kt, seed=9)
    rl = be.to_device(row_list)
    rank, hist = be.ivf_probe_ranks(dev(be, truth), rl, be.to_device(probe))
    assert rank.dtype == be.torch.int32 and hist.dtype == be.torch.int64 and tuple(hist.shape) == (P + 1,)
    want_rank, want_hist = probe_ranks_reference(truth, row_list, probe)
    low = np.uint64(0xFFFFFFFF)
    live = (truth != 0) & ((low - (truth & low)) < n)
    assert np.array_equal(host(rank), want_rank) and np.array_equal(host(hist), want_hist)
    assert want_hist.sum() == live.sum() and np.array_equal(want_rank >= 0, live)
    if kt >= 10:
        assert want_hist[P] > 0 and want_hist[0] > 0 and (want_rank == np.max(np.where(probe >= 0, np.arange(P), -1), 1)[:, None]).any()
    # accumulation into counts that are already there
    t = be.torch
    acc = t.arange(1, P + 2, dtype=t.int64, device=be.device)
    rank2 = t.empty((nq, kt), dtype=t.int32, device=be.device)
    tk, pr = dev(be, truth), be.to_device(probe)
    be._c("lvs_ivf_probe_ranks", _ptr(tk), kt, _ptr(rl), n, _ptr(pr), P, nq, _ptr(rank2), _ptr(acc), be._stream())
    assert np.array_equal(host(acc), want_hist + np.arange(1, P + 2)) and np.array_equal(host(rank2), want_rank)


# ---- end to end ------------------------------------------------------------------------------------------------------------
NB, D_, NLIST, NQ, K = 4000, 64, 16, 64, 10
# near-tie share of the queries below (exact top-(K + 1) float32 scores of the CPU oracle, neighbours closer than 2e-5):
# 5 of 64 = 7.8 % at these seeds, under the 15 % cap
SEED_B, SEED_Q = 41, 42
STORES = [("IVF16,Flat", {}, "lvs_ivf_scan_kernel"), ("IVF16,SQ8", {}, "lvs_ivf_sq8_scan_kernel"),
          ("IVF16,PQ8", {}, "lvs_ivf_pq_scan_kernel"), ("IVF16,PQ8,Refine(Flat)", {"k_factor": 1}, "lvs_refine_kernel"),
          ("IVF16,PQ8,Refine(Flat)", {"k_factor": 4}, "lvs_refine_kernel")]


def clustered(n, d, centers, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + 0.5 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16)


def near_tie_queries(D):
    """Queries whose best K + 1 scores (``D`` [nq, K + 1], best first) hold a neighbouring pair closer than the tie gap."""
    return np.any(np.abs(np.diff(np.asarray(D, np.float64), axis=1)) < TIE_GAP, axis=1)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    xb, xq = clustered(NB, D_, 20, SEED_B), clustered(NQ, D_, 20, SEED_Q)
    path = str(tmp_path_factory.mktemp("recall") / "idx")
    return xb, xq, path, {}


def open_store(corpus, fs, kw):
    """The store of this mode over the shared directory: the first one trains the lists, the others reuse the sidecar."""
    xb, _, path, made = corpus
    vs = HipVS(factory_string=fs, device="cuda:0", **kw)
    if not made:
        vs.index(None, xb, path)
        made["lists"] = True
    else:
        vs.load_index(path)
    return vs


def host_hits(exact_I, got_I):
    hits = np.array([len(set(t.tolist()) & set(g[g >= 0].tolist())) for t, g in zip(exact_I, got_I)], np.int32)
    first = np.array([t[0] in set(g.tolist()) for t, g in zip(exact_I, got_I)])
    return hits, first


@pytest.mark.parametrize("fs,kw,kernel", STORES, ids=[s[0] + "".join(f"-{v}" for v in s[1].values()) for s in STORES])
def test_hipvs_recall_end_to_end(hip_backend, corpus, fs, kw, kernel):
    xb, xq, path, _ = corpus
    vs = open_store(corpus, fs, kw)
    flat = HipVS(device="cuda:0")
    flat.load_index(path)
    exact = flat(xq, K + 1)
    exact_I = exact.indices[:, :K]
    be = vs.backend
    nprobes = [1, 2, 5, NLIST]
    be.timing_enable(True)
    try:
        rep = vs.recall(xq, K, nprobe=nprobes)
        be.synchronize()
        t = be.timing_read_full()
    finally:
        be.timing_enable(False)
    assert t["kernel"] == kernel, t  # the list scan (and the re-ranking) ran last: no exact fall-back
    assert rep.served == (True,) * 4 and rep.kc == (vs.refine_candidates(K) if "Refine" in fs else K)
    for i, p in enumerate(nprobes):
        hits, first = host_hits(exact_I, vs(xq, K, nprobe=p).indices)
        print(f"{fs} {kw} nprobe={p}: intersection {rep.intersection[i]:.4f} first {rep.first[i]:.4f}")
        assert np.array_equal(rep.hits[i], hits), (fs, p)
        assert rep.intersection[i] == pytest.approx(hits.sum() / (NQ * K), abs=1e-12)
        assert rep.first[i] == pytest.approx(first.mean(), abs=1e-12)
    curve = vs.probe_recall_curve(xq, K)
    assert curve.shape == (NLIST + 1,) and curve[0] == 0.0 and curve[NLIST] == 1.0
    assert np.all(rep.intersection <= curve[nprobes] + 1e-12)  # the ceiling holds in every mode
    # tune, then measure again: to 0.9 where all the lists together reach it; where the codec does not, that is an error
    # which names both figures, and the store is tuned to what two probes gave
    target = 0.9
    if rep.intersection[-1] < target:
        with pytest.raises(ValueError, match=f"best measured is {rep.intersection[-1]:.4f}.*ceiling at nprobe={NLIST} is 1.0000"):
            vs.tune_nprobe(xq, K, target=target)
        target = float(rep.intersection[1])
    p, one = vs.tune_nprobe(xq, K, target=target)
    assert vs.nprobe == p and 1 <= p <= NLIST and one.nprobes == (p,)
    hits, _ = host_hits(exact_I, vs(xq, K).indices)
    again = vs.recall(xq, K)
    print(f"{fs} {kw} target {target:.4f} -> nprobe={p}: reported {one.intersection[0]:.4f}, measured again {again.intersection[0]:.4f}")
    if "Flat" == fs.split(",")[1]:
        keep = ~near_tie_queries(exact.distances)
        assert 1.0 - keep.mean() <= NEAR_TIE_CAP
        # the identity: probe-limited recall IS the measured recall, at every nprobe, on the queries without a near-tie
        c_keep = vs.probe_recall_curve(xq[keep], K)
        r_keep = vs.recall(xq[keep], K, nprobe=range(1, NLIST + 1))
        assert np.array_equal(c_keep[1:], r_keep.intersection)
        p_keep, one_keep = vs.tune_nprobe(xq[keep], K, target=target, apply=False)
        assert one_keep.intersection[0] == r_keep.intersection[p_keep - 1] >= target
        assert p_keep == 1 or r_keep.intersection[p_keep - 2] < target
    else:
        assert again.intersection[0] >= target and hits.sum() / (NQ * K) >= target
        assert np.array_equal(again.hits, one.hits)
