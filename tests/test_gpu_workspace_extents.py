"""Every workspace-taking entry point at EXACTLY its declared workspace size.

The C ABI allocates nothing: a call touches its ``lvs_*_workspace_bytes`` of scratch and its outputs, nothing else.  The backend's
ordinary scratch is a reused buffer of at least 1 MiB whose whole size is passed as ``workspace_bytes``, so no other test runs a
kernel without slack behind its layout.  Here every case runs three times - on the ordinary scratch, and with every
``be._workspace(n)`` replaced by a fresh buffer of exactly ``n`` bytes between two guards (tests/ws_guard.py), once filled
with 0xFF (keys that beat every real key, NaN scores, saturated counters) and once with zeros - and must

  * leave the guards and the rounding slack untouched,
  * give bit-identical results in all three runs (a result that depends on what the scratch held is a bug),
  * agree, in the baseline, with the reference and the tolerance of the entry's home test file.

Each case prints its requested sizes (``EXTENT <case>: [bytes, ...]``; profiles/ws_extents_check.md lists them)."""
import numpy as np
import pytest
import torch

import oracle
import plan_native
import synth
from extent_cases import F16, FLAT, FLAT_BY_NAME, IP, L2, SPLIT, planner_says
from ivf_oracle_backend import ivf_reference
from ivf_pq_oracle_backend import pq_decode, pq_reference
from ivf_range_oracle_backend import check_pairs, float64_scores, ivf_range_reference
from ivf_sq8_oracle_backend import list_of_rows, sq8_decode, sq8_reference
from lotus_amd import _capi
from test_gpu_parity import _stored
from test_gpu_rj_solo import _sample_rows
from ws_guard import GUARD, GuardedPool, exact_workspace

pytestmark = pytest.mark.gpu


def _host(be, out):
    be.synchronize()
    return tuple(np.ascontiguousarray(t.cpu().numpy()) for t in out)


def _assert_same_bits(name, what, a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (name, what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        diff = a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)
        first = int(np.flatnonzero(diff)[0]) // a.dtype.itemsize
        raise AssertionError(f"{name}: output {what} differs from the baseline in {int(diff.sum())} bytes, first at element "
                             f"{first} of {a.size}: {a.reshape(-1)[first]!r} (baseline) vs {b.reshape(-1)[first]!r}")


def three_runs(be, name, run, canon=None, ran=()):
    """``run()`` -> tuple of device tensors.  Baseline, then exactly-sized scratch holding 0xFF, then zeros.  ``canon``: brings
    the host arrays of an entry whose output ORDER is unspecified into a canonical order first.  ``ran``: C entry points that
    must have been called in each exact run (the ones the case is here for).  -> the baseline's arrays, the requested sizes."""
    canon = canon or (lambda arrays: arrays)
    base = canon(_host(be, run()))
    for fill in (0xFF, 0x00):
        with exact_workspace(be, fill) as pool:
            out = run()
            pool.assert_clean()  # (synchronises)
            got = canon(_host(be, out))
            sizes, entries = pool.sizes(), set(pool.entries)
        assert sizes, f"{name}: the case never asked for a workspace"
        assert set(ran) <= entries, (name, sorted(set(ran) - entries), sorted(entries))
        for i, (a, b) in enumerate(zip(base, got)):
            _assert_same_bits(f"{name} (scratch filled with {fill:#04x})", i, a, b)
    print(f"\nEXTENT {name}: {sizes}", end="")
    return base, sizes


def _u64(keys):
    return keys.view(np.uint64)


# ---- the detector itself, on the device (test_ws_guard_host.py's cases; the writes are torch's, no library call) ---------------
@pytest.mark.parametrize("offset,side", [(-1, "before"), (-GUARD, "before"), (1000, "slack"), (1024, "after"),
                                         (1024 + GUARD - 1, "after"), (999, None)])
def test_the_detector_detects_on_the_device(hip_backend, offset, side):
    pool = GuardedPool(hip_backend.device)
    v = pool.alloc(1000, 0xFF)
    assert v.is_cuda and v.numel() == 1000 and v.data_ptr() % 256 == 0 and bool((v == 0xFF).all())
    pool.assert_clean()
    whole, lead, _ = pool._bufs[0]
    whole[lead + offset] = 0x5A
    got = [(x.ordinal, x.nbytes, x.side, x.first, x.last, x.count) for x in pool.violations()]
    assert got == ([] if side is None else [(0, 1000, side, offset, offset, 1)])
    if side is not None:
        with pytest.raises(AssertionError, match=f"{side} the payload, offsets {offset} .. {offset}"):
            pool.assert_clean()


def test_exact_workspace_hands_the_backend_exact_guarded_buffers(hip_backend):
    be = hip_backend
    ordinary = be._workspace(100)
    assert ordinary.numel() >= 1 << 20
    with exact_workspace(be, 0xFF) as pool:
        a, b = be._workspace(100), be._workspace(100)
        assert a.numel() == b.numel() == 100 and a.data_ptr() != b.data_ptr() and a.data_ptr() % 256 == 0 and bool((a == 0xFF).all())
        torch.cat([a, b])[:] = 0  # (a copy: nothing written)
        a[99] = 1
        pool.assert_clean()
    assert be._workspace(100).data_ptr() == ordinary.data_ptr() and "_workspace" not in be.__dict__


# ---- the flat search: one shape per path -------------------------------------------------------------------------------------
def _flat_data(c):
    xb = synth.corpus(c.nb, c.d, seed=c.nb % 97)
    xq, _ = synth.queries(xb, c.nq, seed=3)
    if c.metric == L2:
        xb = xb * 1.5  # break the unit norm so the norm terms matter (as test_gpu_parity)
    return xb, xq


def _pack2(be, xb, xq, mode):
    return (be.pack(xb.astype(np.float16) if mode == F16 else xb, mode), be.pack(xq.astype(np.float16) if mode == F16 else xq, mode))


def _check_flat(be, c, xb, xq, keys, id_offset=0, atol=1e-5):
    """test_gpu_parity's bars: scores within 1e-5, ids identical outside 2e-5 near-ties; beyond 4 096 queries on test_gpu_rj_solo's
    stratified sample of query rows."""
    rows = _sample_rows(c.nq) if c.nq > 4096 else np.arange(c.nq)
    D, I = be.keys_to_result(torch.from_numpy(keys[rows]).to(be.device), c.metric)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    I = np.where(I >= 0, I - id_offset, I)
    Dr, Ir = oracle.flat_search(_stored(xb, c.mode), _stored(xq[rows], c.mode), c.k, c.metric)
    err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=atol)
    assert (I >= 0).sum() == (Ir >= 0).sum()
    assert err <= atol and hard == 0 and recall >= 0.9999, (err, hard, recall)


@pytest.mark.parametrize("c", FLAT, ids=lambda c: c.name)
def test_flat_search_paths(hip_backend, c):
    be = hip_backend
    says = planner_says(c)
    assert says["route"] == c.route and all(says[key] == want for key, want in c.plan.items()), says
    xb, xq = _flat_data(c)
    cb, cq = _pack2(be, xb, xq, c.mode)
    (keys,), sizes = three_runs(be, c.name, lambda: (be.search_keys(cb, cq, c.k, c.metric, one_pass=False),),
                                ran=["lvs_flat_search_keys"])
    assert sizes == [says["bytes"]] == [int(be.lib.lvs_flat_search_workspace_bytes(c.nq, c.nb, c.d, c.k, c.mode, c.mode))]
    assert _u64(keys).shape == (c.nq, c.k)
    _check_flat(be, c, xb, xq, keys)


@pytest.mark.parametrize("name", ["stream-2blocks", "list-k15"])
def test_flat_search_with_row_ids_and_id_offset(hip_backend, name):
    be, c = hip_backend, FLAT_BY_NAME[name]
    xb, xq = _flat_data(c)
    cb, cq = _pack2(be, xb, xq, c.mode)
    (keys,), _ = three_runs(be, name + "+id_offset", lambda: (be.search_keys(cb, cq, c.k, c.metric, id_offset=123456, one_pass=False),))
    _check_flat(be, c, xb, xq, keys, id_offset=123456)
    perm = np.random.default_rng(0).permutation(c.nb).astype(np.uint32)
    ids = be.to_device(perm.view(np.int32))
    (keys,), _ = three_runs(be, name + "+row_ids", lambda: (be.search_keys(cb, cq, c.k, c.metric, row_ids=ids, one_pass=False),))
    inv = np.argsort(perm)  # the corpus in id order: row_ids only rename the rows (ties then break by the NEW ids, as the oracle's)
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys).to(be.device), c.metric))
    Dr, Ir = oracle.flat_search(_stored(xb[inv], c.mode), _stored(xq, c.mode), c.k, c.metric)
    err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=1e-5)
    assert err <= 1e-5 and hard == 0 and recall >= 0.9999, (err, hard, recall)


def test_externally_seeded_flat_search(hip_backend):
    """``seed_scores`` -> ``search_keys(..., seed_scores=)`` at the smallest shape with sample tiles (k = 10: 16 x 256 x 10 rows);
    the seeds cover the whole searched set, so the result is the plain search's."""
    be, c = hip_backend, FLAT_BY_NAME["list-seeded"]
    tiles = int(be.lib.lvs_flat_search_seed_tiles(c.nq, c.nb, c.k))
    assert tiles > 0 and int(be.lib.lvs_flat_search_seed_tiles(c.nq, 16 * 256 * c.k - 1, c.k)) == 0
    xb, xq = _flat_data(c)
    cb, cq = _pack2(be, xb, xq, c.mode)
    plain = _host(be, (be.search_keys(cb, cq, c.k, c.metric, one_pass=False),))[0]

    def run():
        seeds = be.seed_scores(cb, cq, c.metric, tiles)
        return be.search_keys(cb, cq, c.k, c.metric, seed_scores=seeds), seeds

    (keys, seeds), sizes = three_runs(be, "list-seeded+external", run, ran=["lvs_flat_search_keys_seeded"])
    assert sizes == [int(be.lib.lvs_flat_search_workspace_bytes(c.nq, c.nb, c.d, c.k, c.mode, c.mode))]
    assert seeds.shape == (tiles, c.nq) and np.isfinite(seeds).all()
    assert np.array_equal(_u64(keys), _u64(plain))
    _check_flat(be, c, xb, xq, keys)


@pytest.mark.parametrize("nq,nb,d,entry", [(300, 5000, 128, "lvs_flat_search_keys_hi_banded"),
                                           (4097, 65536, 256, "lvs_flat_search_keys_hi")])
def test_certified_one_pass_search(hip_backend, nq, nb, d, entry):
    """``_search_keys_certified`` (the one-pass search, rescore, certify, the second round and the plain search of what stays
    open): a test_gpu_parity CERT shape cut down, near-duplicate rows keeping some queries open.  The one pass has banded
    lists (lvs_flat_search_keys_hi_banded), except from 4 097 hi|lo queries x 65 536 rows at a register-resident width on,
    where it is lvs_flat_search_keys_hi on the chunked join - the smallest such shape (the reference on a sample of its queries)."""
    be = hip_backend
    k = 10
    assert (entry == "lvs_flat_search_keys_hi") == (nq >= be.CERT_RJ_MIN_QUERIES and nb >= 65536 and d in (256, 384, 512, 768))
    xb = synth.corpus(nb, d, seed=21) * 1.3
    xq, _ = synth.queries(xb, nq, seed=6)
    xq[:40] = xb[0]
    rows = np.union1d(np.arange(40), _sample_rows(nq)) if nq > 4096 else np.arange(nq)
    declared = {int(be.lib.lvs_flat_search_workspace_bytes(m, nb, d, k1, SPLIT, SPLIT)) for m in range(1, nq + 1)
                for k1 in (k, min(15, k + be.CERT_SPARE_SMALL_K), 56)}  # the first round, the second, the plain search of the rest
    cq = be.pack(xq, SPLIT)
    u = np.zeros(d, np.float32)
    u[:2] = xb[0, 1], -xb[0, 0]
    u /= np.linalg.norm(u)  # a unit vector orthogonal to row 0
    for metric in (IP, L2):
        # thirty near-copies of row 0, which forty queries equal.  Their scores lie far inside the one pass's hi-only bound
        # (2^-11 |q| |row| = 8e-4), so those queries stay open, and step by 6e-6 or more - above the hi|lo rows' own error
        # (2^-21 relative, 8e-7), so their exact order is decided: inner products 2^-18 |row|^2 apart; squared distances i^2 x 6.25e-6
        step = np.arange(30, dtype=np.float32)[:, None]
        xb[1000:1030] = xb[0] * (1 + step * 2.0 ** -18) if metric == IP else xb[0] + step * np.float32(2.5e-3) * u
        cb = be.pack(xb, SPLIT)
        stats = {}
        (keys,), sizes = three_runs(be, f"certified-{nq}x{nb}-{metric}",
                                    lambda: (be.search_keys(cb, cq, k, metric, one_pass=True, stats=stats),),
                                    ran=[entry, "lvs_rescore_keys", "lvs_certify_topk_banded"])
        assert stats.get("queries", 0) >= nq, stats  # the certified route ran
        assert set(sizes) <= declared, sizes
        print(f" stats {stats}", end="")
        D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys[rows]).to(be.device), metric))
        Dr, Ir = oracle.flat_search(xb, xq[rows], k, metric)
        err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=1e-5)
        assert err <= 1e-5 and hard == 0 and recall >= 0.9999, (err, hard, recall)


# ---- nearest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,branch", [(16385, "lvs_nearest_hi"), (3 * 256 - 1, "lvs_nearest3"), (16384, "lvs_nearest3")])
@pytest.mark.parametrize("metric", [IP, L2])
def test_nearest(hip_backend, nb, branch, metric):
    """fp16 queries against hi|lo rows (the k-means assignment): one slab past ``LVS_NEAREST3_MAX_ROWS`` takes lvs_nearest_hi, up to
    it lvs_nearest3 - a ragged last 256-row tile, and the largest corpus."""
    be = hip_backend
    assert (nb > _capi.NEAREST3_MAX_ROWS) == (branch == "lvs_nearest_hi")
    nq, d = 777, 100
    xb = synth.corpus(nb, d, seed=5) * 1.2
    xq, _ = synth.queries(xb, nq, seed=8)
    xq = xq.astype(np.float16)
    xb[nb - 1] = xq[3].astype(np.float32)  # the last row wins a query
    cb, cq = be.pack(xb, SPLIT), be.pack(xq, F16)
    stats = {}
    (keys,), sizes = three_runs(be, f"{branch}-{nb}-{metric}", lambda: (be.nearest(cb, cq, metric, id_offset=7, stats=stats),),
                                ran=[branch])
    want = {"lvs_nearest_hi": be.lib.lvs_nearest_hi_workspace_bytes, "lvs_nearest3": be.lib.lvs_nearest3_workspace_bytes}[branch]
    assert sizes[0] == int(want(nq, nb, d))
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys).to(be.device), metric))
    Dr, Ir = oracle.flat_search(xb, xq.astype(np.float32), 2, metric)
    assert np.abs(Dr[:, 0] - D[:, 0]).max() <= 1e-5
    other = I[:, 0] - 7 != Ir[:, 0]
    assert np.all(np.abs(Dr[other, 0] - Dr[other, 1]) <= 2e-5), int(other.sum())  # another winner only out of a near-tie
    assert I[3, 0] - 7 == nb - 1


# ---- k-means pieces -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 24575, 24576])  # few buckets; the last one-digit and the first two-digit bucket count
def test_kmeans_accumulate(hip_backend, k):
    be = hip_backend
    rng = np.random.default_rng(k)
    n, d = 8192 * 2 + 1, 8
    x = rng.standard_normal((n, d)).astype(np.float16)
    assign = rng.integers(0, k, n).astype(np.int64)
    assign[rng.integers(0, n, 40)] = -1     # skipped
    assign[rng.integers(0, n, 40)] = k + 5  # out of range: ignored
    assign[n - 1] = k - 1
    p = be.pack(x, F16)
    a_dev = be.to_device(assign)
    ok = (assign >= 0) & (assign < k)
    ref = np.zeros((k, d), np.float32)
    np.add.at(ref, assign[ok], x.astype(np.float32)[ok])
    cnt = np.bincount(assign[ok], minlength=k).astype(np.float32)
    need = int(be.lib.lvs_kmeans_accumulate_workspace_bytes(n, k))
    (sums, counts), sizes = three_runs(be, f"kmeans_accumulate-k{k}", lambda: be.kmeans_accumulate(p, a_dev, k),
                                       ran=["lvs_kmeans_accumulate"])
    assert sizes == [need]
    assert np.array_equal(sums, ref) and np.array_equal(counts, cnt)  # same values, same order: bit-identical float32 sums
    # ... from result keys (id = id_offset + cluster; rows of another shard's id range are ignored)
    id_offset = 1000
    score = rng.standard_normal(n).astype(np.float32)
    keys = oracle.pack_keys(score, np.where(ok, assign, k + 5) + id_offset)
    k_dev = be.to_device(np.ascontiguousarray(keys).view(np.int64))
    (sums, counts), sizes = three_runs(be, f"kmeans_accumulate_keys-k{k}", lambda: be.kmeans_accumulate_keys(p, k_dev, k, id_offset),
                                       ran=["lvs_kmeans_accumulate_keys"])
    assert sizes == [need]
    assert np.array_equal(sums, ref) and np.array_equal(counts, cnt)


@pytest.mark.parametrize("k", [3, 24576])
def test_kmeans_accumulate_keys_into_a_callers_exact_workspace(hip_backend, k):
    """The side-stream form (lotus_amd/cluster.py): the caller's own scratch of exactly ``lvs_kmeans_accumulate_workspace_bytes``,
    the rows handed over in two ranges that continue each other's sums."""
    from ws_guard import GuardedPool

    be = hip_backend
    rng = np.random.default_rng(k + 1)
    n, d = 8192 * 2 + 1, 8
    x = rng.standard_normal((n, d)).astype(np.float16)
    assign = rng.integers(0, k, n).astype(np.int64)
    p = be.pack(x, F16)
    keys = be.to_device(np.ascontiguousarray(oracle.pack_keys(np.zeros(n, np.float32), assign)).view(np.int64))
    ref = np.zeros((k, d), np.float32)
    np.add.at(ref, assign, x.astype(np.float32))
    h = 8192 + 5
    for fill in (0xFF, 0x00):
        pool = GuardedPool(be.device)
        ws = pool.alloc(int(be.lib.lvs_kmeans_accumulate_workspace_bytes(n, k)), fill)
        sums = torch.zeros((k, d), dtype=torch.float32, device=be.device)
        counts = torch.zeros((k,), dtype=torch.float32, device=be.device)
        be.kmeans_accumulate_keys_into(be.slice_rows(p, 0, h), keys[:h].contiguous(), k, sums, counts, workspace=ws)
        be.kmeans_accumulate_keys_into(be.slice_rows(p, h, n), keys[h:].contiguous(), k, sums, counts, workspace=ws)
        pool.assert_clean()
        assert np.array_equal(sums.cpu().numpy(), ref)
        assert np.array_equal(counts.cpu().numpy(), np.bincount(assign, minlength=k).astype(np.float32))


@pytest.mark.parametrize("k", [50, 64])  # 64: the partial sums fill the declared 512 bytes to the last one
def test_kmeans_objective(hip_backend, k):
    """test_gpu_kmeans' objective case; inside ``exact_workspace`` the entry runs raw on a guarded buffer of exactly its size."""
    be = hip_backend
    rng = np.random.default_rng(6)
    n, d = 30_000, 96
    x = rng.standard_normal((n, d)).astype(np.float16)
    cent = rng.standard_normal((k, d)).astype(np.float32)
    p = be.pack(x, F16)
    D, I = oracle.flat_search(cent, x.astype(np.float32), 1, 1)
    keys = be.search_keys(be.pack(cent, SPLIT), p, 1, L2)
    sums, counts = be.kmeans_accumulate_keys(p, keys, k)
    c_dev, x2 = be.to_device(cent), p.norms.double().sum().reshape(1)

    def run():
        out = torch.zeros(1, dtype=torch.float64, device=be.device)
        be.kmeans_objective(c_dev, sums, counts, x2, out)
        return (out,)

    (obj,), sizes = three_runs(be, "kmeans_objective", run, ran=["lvs_kmeans_objective"])
    assert sizes == [int(be.lib.lvs_kmeans_objective_workspace_bytes(k))]
    want = float(D[:, 0].astype(np.float64).sum())
    assert abs(float(obj[0]) - want) <= 1e-5 * want


@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_kmeans_iteration(hip_backend, mode):
    """test_gpu_kmeans' shape, two iterations: ``lvs_kmeans_iteration`` on exact scratch equals, bit for bit, the launch-by-launch
    loop on the ordinary one (which is that file's reference)."""
    import benchdata
    from lotus_amd import cluster as cl

    be = hip_backend
    K, n, d = 48, 70_001, 96
    x16, _ = benchdata.blobs(benchdata.CFG_KMEANS, n, d, K)
    x = x16.copy() if mode == F16 else (x16.astype(np.float32) * np.float32(1.0 + 2.0 ** -13))
    x[100:140] = x[7]
    kw = dict(niter=2, backend=be, max_points_per_centroid=None, bounds=False, parts=1, final_assign=False)
    cl.USE_ITERATION_OP = False
    try:
        ref = cl.kmeans(x, K, **kw)
    finally:
        cl.USE_ITERATION_OP = True

    def run():
        r = cl.kmeans(x, K, **kw)
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (r.centroids, r.obj, r.nsplit))

    (cent, obj, nsplit), sizes = three_runs(be, f"kmeans_iteration-{mode}", run, ran=["lvs_kmeans_iteration"])
    assert int(be.lib.lvs_kmeans_iteration_workspace_bytes(n, d, K, mode, SPLIT)) in sizes
    assert np.array_equal(cent, ref.centroids) and np.array_equal(obj, ref.obj) and np.array_equal(nsplit, ref.nsplit)


# ---- the row sort ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nb", [(3, 4097), (300, 2049)])
def test_rank_scores(hip_backend, nq, nb):
    be = hip_backend
    rng = np.random.default_rng(nb)
    sc = rng.standard_normal((nq, nb)).astype(np.float32)
    sc[:, 5] = sc[:, nb - 1]  # a tie with the last column: ids decide
    s_dev = be.to_device(sc)
    (keys,), sizes = three_runs(be, f"sort_rows-{nq}x{nb}", lambda: (be.rank_scores(s_dev, id_offset=9),), ran=["lvs_sort_rows_desc"])
    assert sizes == [int(be.lib.lvs_sort_rows_workspace_bytes(nq, nb))]
    ids = np.broadcast_to(np.arange(nb, dtype=np.int64) + 9, (nq, nb))
    assert np.array_equal(_u64(keys), np.sort(oracle.pack_keys(sc, ids), axis=1)[:, ::-1])  # keys are a total order


# ---- IVF ---------------------------------------------------------------------------------------------------------------------
def _ivf_data(nb, nq, d, mode, seed):
    from test_gpu_ivf import _centroids, _data

    xb, xb_s, xq, xq_s = _data(nb, nq, d, mode, seed=seed)
    return xb, xb_s, xq, xq_s, _centroids


def test_ivf_build(hip_backend):
    """``lvs_ivf_build_lists`` through ``ivf_build``: n not a multiple of 8 192; the counting sort ignores assignments out of
    range (raw call: ``ivf_build``'s own assignment never produces one)."""
    from ivf_oracle_backend import group_rows

    be = hip_backend
    n, nlist, d = 8192 * 2 + 77, 37, 64
    xb, xb_s, _, _, cents = _ivf_data(n, 1, d, F16, seed=4)
    c = cents(xb_s, nlist, IP, seed=1)
    packed = be.pack(xb, F16)
    (off, rows), sizes = three_runs(be, "ivf_build", lambda: (lambda L: (L.offsets, L.rows))(be.ivf_build(packed, c, IP)),
                                     ran=["lvs_ivf_build_lists"])
    assert int(be.lib.lvs_ivf_build_workspace_bytes(n, nlist)) in sizes
    _, best = oracle.flat_search(c.astype(np.float16).astype(np.float32), xb_s, 2, IP)
    got = np.empty(n, np.int64)
    got[rows.view(np.uint32).astype(np.int64)] = np.repeat(np.arange(nlist), np.diff(off))
    D, _ = oracle.flat_search(c.astype(np.float16).astype(np.float32), xb_s, 2, IP)
    clear = np.abs(D[:, 0] - D[:, 1]) > 2e-5
    assert off[0] == 0 and off[-1] == n and np.array_equal(got[clear], best[clear, 0])
    # some ids out of range
    rng = np.random.default_rng(3)
    assign = rng.integers(0, nlist, n).astype(np.int64)
    bad = rng.choice(n, 100, replace=False)
    assign[bad[:50]], assign[bad[50:]] = nlist + 3, -1
    a_dev = be.to_device(assign)

    def raw():
        o = torch.empty((nlist + 1,), dtype=torch.int64, device=be.device)
        r = torch.full((n,), -1, dtype=torch.int32, device=be.device)
        ws = be._workspace(int(be.lib.lvs_ivf_build_workspace_bytes(n, nlist)))
        be._c("lvs_ivf_build_lists", a_dev.data_ptr(), n, nlist, o.data_ptr(), r.data_ptr(), ws.data_ptr(), int(ws.numel()),
              be._stream())
        return o, r

    (off, rows), _ = three_runs(be, "ivf_build-out-of-range", raw, ran=["lvs_ivf_build_lists"])
    ok = (assign >= 0) & (assign < nlist)
    woff, wrows = group_rows(assign[ok], nlist)
    assert np.array_equal(off, woff)
    assert np.array_equal(rows.view(np.uint32)[:int(off[-1])], np.flatnonzero(ok).astype(np.uint32)[wrows.astype(np.int64)])


IVF = [
    # nb, d, nq, k, corpus mode, query mode, metric, nlist, nprobe, selector
    (3000, 64, 300, 10, F16, F16, IP, 16, 1, False),
    (3000, 64, 300, 56, F16, F16, L2, 16, 16, True),
    (4000, 384, 7, 10, SPLIT, SPLIT, L2, 24, 24, False),
    (4000, 200, 130, 10, SPLIT, F16, IP, 24, 5, True),  # fp16 queries against hi|lo centroids: c_pack != xq_pack
]


def _ivf_index(be, nb, d, nq, cmode, qmode, metric, nlist, seed):
    xb, xb_s, xq, xq_s, cents = _ivf_data(nb, nq, d, cmode, seed=seed)
    if qmode != cmode:
        xq = xq.astype(np.float16)
        xq_s = xq.astype(np.float32)
    packed = be.pack(xb, cmode)
    lists = be.ivf_build(packed, cents(xb_s, nlist, metric, seed=nb), metric)
    qp = be.pack(xq, qmode)
    be.synchronize()
    off, rows = lists.offsets.cpu().numpy(), lists.rows.cpu().numpy().view(np.uint32)
    return xb_s, xq_s, packed, lists, qp, off, rows


def _selector(be, nb, use):
    if not use:
        return None, None
    mask = np.zeros(nb, bool)
    mask[::3] = True
    return be.row_bitmap(np.flatnonzero(mask), nb)[0], mask


def _sel_reference(ref_fn, rows_scored, xq_s, k, metric, off, rows, probe, mask):
    """The mode's reference over the selected rows only: lists with the deselected rows taken out."""
    if mask is None:
        return ref_fn(rows_scored, xq_s, k, metric, off, rows, probe)
    keep = mask[rows.astype(np.int64)]
    off2 = np.concatenate([[0], np.cumsum(keep)])[off]
    return ref_fn(rows_scored, xq_s, k, metric, off2, rows[keep], probe)


def _check_ivf(D_ref, I_ref, D, I):
    err, hard, _ = synth.compare_topk(D_ref, I_ref, D, I)
    assert err <= 1e-5 and hard == 0, (err, hard)
    assert np.array_equal(I == -1, I_ref == -1)


@pytest.mark.parametrize("nb,d,nq,k,cmode,qmode,metric,nlist,nprobe,use_sel", IVF)
def test_ivf_search(hip_backend, nb, d, nq, k, cmode, qmode, metric, nlist, nprobe, use_sel):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, cmode, qmode, metric, nlist, seed=d + nq)
    sel, mask = _selector(be, nb, use_sel)
    (keys, probe), sizes = three_runs(be, f"ivf_search-{nb}-{d}-{nprobe}-{int(use_sel)}",
                                      lambda: be.ivf_search(packed, lists, qp, k, metric, nprobe, want_probe=True, sel=sel),
                                      ran=["lvs_ivf_search_keys_sel" if use_sel else "lvs_ivf_search_keys"])
    assert sizes == [int(be.lib.lvs_ivf_search_workspace_bytes(nq, nlist, nprobe, d, k, qp.mode))]
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys).to(be.device), metric))
    ref = lambda x, q, k_, m, o, r, p: ivf_reference(x, q, k_, m, None, o, r, p)  # noqa: E731
    _check_ivf(*_sel_reference(ref, xb_s, xq_s, k, metric, off, rows, probe, mask), D, I)


@pytest.mark.parametrize("nb,d,nq,k,cmode,qmode,metric,nlist,nprobe,use_sel", IVF)
def test_ivf_sq8_search(hip_backend, nb, d, nq, k, cmode, qmode, metric, nlist, nprobe, use_sel):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, cmode, qmode, metric, nlist, seed=d + nq + 1)
    vmin, vdiff = be.ivf_sq8_train(packed, lists, np.arange(0, nb, 2))
    sq = be.ivf_sq8_encode(packed, lists, vmin, vdiff)
    sel, mask = _selector(be, nb, use_sel)
    (keys, probe), sizes = three_runs(be, f"ivf_sq8_search-{nb}-{d}-{nprobe}-{int(use_sel)}",
                                      lambda: be.ivf_sq8_search(packed, lists, sq, qp, k, metric, nprobe, want_probe=True, sel=sel),
                                      ran=["lvs_ivf_sq8_search_keys_sel" if use_sel else "lvs_ivf_sq8_search_keys"])
    assert sizes == [int(be.lib.lvs_ivf_sq8_search_workspace_bytes(nq, nlist, nprobe, d, k, qp.mode))]
    codes = np.empty((nb, d), np.uint8)
    codes[rows.astype(np.int64)] = sq.codes[:, :d].cpu().numpy()
    xhat = sq8_decode(be.unpack(lists.centroids).cpu().numpy(), list_of_rows(off, rows, nb), sq.vmin.cpu().numpy(),
                      sq.vdiff.cpu().numpy(), codes)
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys).to(be.device), metric))
    _check_ivf(*_sel_reference(sq8_reference, xhat, xq_s, k, metric, off, rows, probe, mask), D, I)


@pytest.mark.parametrize("nb,d,nq,k,cmode,qmode,metric,nlist,nprobe,use_sel", IVF)
def test_ivf_pq_search(hip_backend, nb, d, nq, k, cmode, qmode, metric, nlist, nprobe, use_sel):
    be = hip_backend
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, cmode, qmode, metric, nlist, seed=d + nq + 2)
    M, ksub = 8, 256
    c = be.unpack(lists.centroids).cpu().numpy()
    where = list_of_rows(off, rows, nb)
    r = be.unpack(packed).cpu().numpy() - c[where]
    rng = np.random.default_rng(M)
    books = np.stack([r[rng.choice(nb, ksub, replace=False), m * (d // M):(m + 1) * (d // M)] for m in range(M)]).astype(np.float32)
    pq = be.ivf_pq_encode(packed, lists, books)
    sel, mask = _selector(be, nb, use_sel)
    (keys, probe), sizes = three_runs(be, f"ivf_pq_search-{nb}-{d}-{nprobe}-{int(use_sel)}",
                                      lambda: be.ivf_pq_search(packed, lists, pq, qp, k, metric, nprobe, want_probe=True, sel=sel),
                                      ran=["lvs_ivf_pq_search_keys_sel" if use_sel else "lvs_ivf_pq_search_keys"])
    assert sizes == [int(be.lib.lvs_ivf_pq_search_workspace_bytes(nq, nlist, nprobe, d, M, k, qp.mode))]
    codes = np.empty((nb, M), np.uint8)
    codes[rows.astype(np.int64)] = pq.codes[:, :M].cpu().numpy()
    xhat = pq_decode(c, where, books, codes)
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys).to(be.device), metric))
    _check_ivf(*_sel_reference(pq_reference, xhat, xq_s, k, metric, off, rows, probe, mask), D, I)


IVF_BUDGET, IVF_CHUNK = plan_native.ivf_limits()  # IVF_WS_BUDGET, IVF_CHUNK_MAX (lvs_ivf_plan.h): a call with more queries runs in
# chunks of that many, halved until the scratch of one chunk fits the budget


def _r256(n):
    return -(-n // 256) * 256


@pytest.mark.parametrize("nlist,nprobe,k,tail", [(64, 32, 10, 61), (4096, 100, 4, 2445)])
def test_ivf_search_with_a_short_last_chunk(hip_backend, nlist, nprobe, k, tail):
    """16 384 + ``tail`` queries: a full chunk and a short one.  The coarse step of the short chunk is a flat search of ``tail``
    queries, whose declared size EXCEEDS that of 16 384 queries - 61 queries take the streaming kernel with its 264 lists per
    query (nprobe <= 56); 2 445 queries at nprobe = 100 have a two-phase plan where 16 384 have none - so the call's declared
    size must hold the larger of the two.  (Before it did, the second chunk of such a call was refused with LVS_ENOMEM.)
    The reference on a sample of queries around the chunk edge."""
    be = hip_backend
    nb, d, nq = 6000, 64, IVF_CHUNK + tail
    flat = lambda n: int(be.lib.lvs_flat_search_workspace_bytes(n, nlist, d, nprobe, F16, F16))  # noqa: E731
    assert flat(tail) > flat(IVF_CHUNK)  # the shape is here for this
    declared = lambda n: int(be.lib.lvs_ivf_search_workspace_bytes(n, nlist, nprobe, d, k, F16))  # noqa: E731
    # every other region is the full chunk's: the declared size grows by exactly the coarse step's difference
    assert declared(nq) - declared(IVF_CHUNK) == _r256(flat(tail)) - _r256(flat(IVF_CHUNK))
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, F16, F16, IP, nlist, seed=nlist)
    (keys, probe), sizes = three_runs(be, f"ivf_search-short-last-chunk-{nlist}-{nprobe}",
                                      lambda: be.ivf_search(packed, lists, qp, k, IP, nprobe, want_probe=True),
                                      ran=["lvs_ivf_search_keys"])
    assert sizes == [declared(nq)]
    rng = np.random.default_rng(tail)
    sample = np.unique(np.concatenate([[0, IVF_CHUNK - 1, IVF_CHUNK, IVF_CHUNK + 1, nq - 1], rng.choice(nq, 60, replace=False),
                                       IVF_CHUNK + rng.choice(tail, 30, replace=False)]))
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys[sample]).to(be.device), IP))
    _check_ivf(*ivf_reference(xb_s, xq_s[sample], k, IP, None, off, rows, probe[sample]), D, I)


def test_ivf_pq_search_in_query_chunks_bounded_by_the_tables(hip_backend):
    """M = 64: the lookup tables cost 64 KiB per query, so the 512 MiB budget halves the chunk of 16 384 twice and 16 384 + 100
    queries run as four chunks of 4 096 and one of 100.  The chunk length follows from the declared size: chunks are
    16 384 / 2^i queries, the tables of one chunk are chunk x 64 KiB, and the rest of the layout is far below the 256 MiB that
    separate one candidate from the next.  The reference on a sample of queries around every chunk edge."""
    be = hip_backend
    nb, d, nq, k, nlist, nprobe, M, ksub = 6000, 128, IVF_CHUNK + 100, 10, 24, 3, 64, 64
    chunk, table = IVF_CHUNK // 4, M * 256 * 4
    declared = int(be.lib.lvs_ivf_pq_search_workspace_bytes(nq, nlist, nprobe, d, M, k, F16))
    assert chunk * table <= declared < chunk * table + (64 << 20)
    # halved twice, not once: the tables of 8 192 queries alone fill the budget, and a layout holds more than its tables
    assert 2 * chunk * table >= IVF_BUDGET >= declared > chunk * table
    assert plan_native.ivf_chunk("PQ", nq, nlist, nprobe, d, k, F16, M=M) == (chunk, 100, declared)
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, F16, F16, IP, nlist, seed=9)
    c = be.unpack(lists.centroids).cpu().numpy()
    where = list_of_rows(off, rows, nb)
    r = be.unpack(packed).cpu().numpy() - c[where]
    rng = np.random.default_rng(M)
    books = np.stack([r[rng.choice(nb, ksub, replace=False), m * (d // M):(m + 1) * (d // M)] for m in range(M)]).astype(np.float32)
    pq = be.ivf_pq_encode(packed, lists, books)
    (keys, probe), sizes = three_runs(be, "ivf_pq_search-five-chunks",
                                      lambda: be.ivf_pq_search(packed, lists, pq, qp, k, IP, nprobe, want_probe=True),
                                      ran=["lvs_ivf_pq_search_keys"])
    assert sizes == [declared]
    codes = np.empty((nb, M), np.uint8)
    codes[rows.astype(np.int64)] = pq.codes[:, :M].cpu().numpy()
    xhat = pq_decode(c, where, books, codes)
    edges = np.arange(chunk, nq, chunk)
    sample = np.unique(np.concatenate([[0, nq - 1], edges - 1, edges, edges + 1, rng.choice(nq, 80, replace=False)]))
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys[sample]).to(be.device), IP))
    _check_ivf(*pq_reference(xhat, xq_s[sample], k, IP, off, rows, probe[sample]), D, I)


def test_ivf_range_search(hip_backend):
    """The pair outputs come in no particular order: sorted by (q, j) before they are compared."""
    be = hip_backend
    nb, d, nq, nlist, nprobe, thr = 3000, 64, 1300, 16, 5, 0.30
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, F16, F16, IP, nlist, seed=5)

    def canon(arrays):
        q, j, s = arrays
        order = np.lexsort((j, q))
        return q[order], j[order], s[order]

    (q, j, s), sizes = three_runs(be, "ivf_range_search", lambda: be.ivf_range_search(packed, lists, qp, thr, IP, nprobe), canon,
                                   ran=["lvs_ivf_range_search"])
    assert sizes == [int(be.lib.lvs_ivf_range_workspace_bytes(nq, nlist, nprobe, d, qp.mode))]
    probe = be.ivf_search(packed, lists, qp, 1, IP, nprobe, want_probe=True)[1].cpu().numpy()
    want, near = ivf_range_reference(xb_s, xq_s, thr, IP, off, rows, probe)
    assert len(want) >= 1000
    got = np.stack([q, j], axis=1)
    check_pairs(got, want, near, nb)
    assert np.abs(s.astype(np.float64) - float64_scores(xb_s, xq_s, IP, got)).max() <= 1e-5 and np.all(s > thr)


# ---- the sharded search, one rank -----------------------------------------------------------------------------------------
def test_search_sharded_with_one_rank(hip_backend):
    be = hip_backend
    n, nq, d, k = 50_000, 4096, 128, 10
    xb = synth.corpus(n, d, seed=31).astype(np.float16)
    xq = synth.corpus(nq, d, seed=32).astype(np.float16)
    corpus, queries = be.pack(xb, F16), be.pack(xq, F16)
    want = _host(be, (be.search_keys(corpus, queries, k, IP),))[0]
    tiles = be.seed_tiles(nq, n, k, F16, F16)
    calls = []

    def all_gather(t):
        calls.append(int(t.numel()))
        return t.reshape(1, -1)

    (keys,), sizes = three_runs(be, "search_sharded-world1", lambda: (be.search_sharded(corpus, queries, k, IP, 3, 1, tiles, all_gather),),
                                ran=["lvs_search_sharded"])
    assert sizes == [int(be.lib.lvs_search_sharded_workspace_bytes(1, nq, n, d, k, F16, F16, tiles))]
    D, I = (t.cpu().numpy() for t in be.keys_to_result(torch.from_numpy(keys[:256]).to(be.device), IP))
    assert np.array_equal(I - 3, be.keys_to_result(torch.from_numpy(want[:256]).to(be.device), IP)[1].cpu().numpy())
    Dr, Ir = oracle.flat_search(xb.astype(np.float32), xq[:256].astype(np.float32), k, IP)
    err, hard, recall = synth.compare_topk(Dr, Ir, D, I - 3, atol=1e-5)
    assert err <= 1e-5 and hard == 0 and recall >= 0.9999


# ---- every size function and every workspace-taking entry has a case ------------------------------------------------------------
# entry point -> (its size function, the test here that runs it on exact scratch).  The test must name the size function
# (it asserts the requested sizes against it) and the entry (``ran=``: it asserts that the entry was called on exact scratch).
EXACT_SIZE_CASES = {
    "lvs_flat_search_keys": ("lvs_flat_search_workspace_bytes", "test_flat_search_paths"),
    "lvs_flat_search_keys_seeded": ("lvs_flat_search_workspace_bytes", "test_externally_seeded_flat_search"),
    "lvs_flat_search_keys_hi": ("lvs_flat_search_workspace_bytes", "test_certified_one_pass_search"),
    "lvs_flat_search_keys_hi_banded": ("lvs_flat_search_workspace_bytes", "test_certified_one_pass_search"),
    "lvs_search_sharded": ("lvs_search_sharded_workspace_bytes", "test_search_sharded_with_one_rank"),
    "lvs_sort_rows_desc": ("lvs_sort_rows_workspace_bytes", "test_rank_scores"),
    "lvs_nearest_hi": ("lvs_nearest_hi_workspace_bytes", "test_nearest"),
    "lvs_nearest3": ("lvs_nearest3_workspace_bytes", "test_nearest"),
    "lvs_kmeans_accumulate": ("lvs_kmeans_accumulate_workspace_bytes", "test_kmeans_accumulate"),
    "lvs_kmeans_accumulate_keys": ("lvs_kmeans_accumulate_workspace_bytes", "test_kmeans_accumulate"),
    "lvs_kmeans_objective": ("lvs_kmeans_objective_workspace_bytes", "test_kmeans_objective"),
    "lvs_kmeans_iteration": ("lvs_kmeans_iteration_workspace_bytes", "test_kmeans_iteration"),
    "lvs_ivf_build_lists": ("lvs_ivf_build_workspace_bytes", "test_ivf_build"),
    "lvs_ivf_search_keys": ("lvs_ivf_search_workspace_bytes", "test_ivf_search"),
    "lvs_ivf_search_keys_sel": ("lvs_ivf_search_workspace_bytes", "test_ivf_search"),
    "lvs_ivf_sq8_search_keys": ("lvs_ivf_sq8_search_workspace_bytes", "test_ivf_sq8_search"),
    "lvs_ivf_sq8_search_keys_sel": ("lvs_ivf_sq8_search_workspace_bytes", "test_ivf_sq8_search"),
    "lvs_ivf_pq_search_keys": ("lvs_ivf_pq_search_workspace_bytes", "test_ivf_pq_search"),
    "lvs_ivf_pq_search_keys_sel": ("lvs_ivf_pq_search_workspace_bytes", "test_ivf_pq_search"),
    "lvs_ivf_range_search": ("lvs_ivf_range_workspace_bytes", "test_ivf_range_search"),
}
# the same two entries behind an RCCL communicator: they need a process group (tests/test_gpu_dist.py runs them)
NEEDS_A_COMMUNICATOR = {"lvs_search_sharded_rccl", "lvs_kmeans_iteration_rccl"}


def workspace_entries():
    """Every entry point of include/lotus_hip.h that takes ``workspace_bytes``."""
    found = {name for name, p in _capi.PROTOTYPES.items() if "workspace_bytes" in p.names}
    assert len(found) >= 20 and found <= set(_capi.SIGNATURES)
    return found


def test_every_size_function_and_entry_has_an_exact_size_case():
    """A new ``lvs_*_workspace_bytes`` in the binding, or a new entry point with a ``workspace_bytes`` argument in the header,
    without a case here fails; and the test a table row names must itself name the size function and the entry."""
    import inspect
    import re

    sizes = {name for name in _capi.SIGNATURES if name.endswith("_workspace_bytes")}
    assert sizes == {size for size, _ in EXACT_SIZE_CASES.values()}, sizes ^ {size for size, _ in EXACT_SIZE_CASES.values()}
    assert workspace_entries() - NEEDS_A_COMMUNICATOR == set(EXACT_SIZE_CASES), workspace_entries() ^ set(EXACT_SIZE_CASES)
    for entry, (size, test) in EXACT_SIZE_CASES.items():
        src = inspect.getsource(globals()[test])
        assert re.search(rf"\b{size}\b", src) and re.search(rf"\b{entry}\b", src), (test, size, entry)
