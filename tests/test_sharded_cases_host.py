"""Host half of the sharded exact tests (tests/sharded_cases.py; the device runs in tests/test_gpu_sharded_abi.py).  Conditions on
the inputs and the references alone, checked before the device sees them:

* every search case is exact in float32 in any summation order (``guard_exact``), its branch is the one it declares (the
  library's own seed tile count for the nominal shard, ``sharded_plan``'s decision restated, the compiled planner's route), and
  the reference taken SHARD BY SHARD with id offsets and merged per query equals the reference of the whole corpus - which
  validates the reference, the id offsets (the 2^32 one included) and the short-list padding independently of the device;
* the k-means cases: exact distances in iteration 1, partial sums far below 2^24 units, duplicate initial centroids that really
  leave clusters empty in a float64 Lloyd step, the tripled centroid really nearest to every row, distinct chunk centroids."""
import numpy as np
import pytest

import sharded_cases as sc
from lattice_cases import F16, IP, L2, LO_STEP, SPLIT, STEP
from oracle.flat import unpack_keys


def _lib():
    from lotus_amd import _capi

    return _capi.load()


def test_the_table_covers_what_it_is_there_for():
    cs = sc.SEARCH_CASES
    assert len({c.name for c in cs}) == len(cs)
    assert {c.exchanges for c in cs} == {1, 2} and all(c.W > 1 for c in cs)
    assert any(c.metric == L2 and c.exchanges == 2 and 0 in c.sizes and min(s for s in c.sizes if s) < 256 for c in cs)
    assert any(c.opt_out and c.lib_tiles for c in cs)
    assert {(c.bpack, c.qpack) for c in cs} == {(F16, F16), (SPLIT, SPLIT), (F16, SPLIT)} and any(c.real_lo for c in cs)
    assert any(c.lib_tiles and c.bpack == SPLIT for c in cs) and any(c.lib_tiles and c.qpack == SPLIT and c.bpack == F16 for c in cs)
    assert {57, 100, 1000, 2048, 1} <= {c.k for c in cs}
    assert any(c.k > min(s for s in c.sizes if s) and c.k >= 1000 for c in cs) and any(c.nb < c.k for c in cs)
    assert {1, 96, 97, 128, 129} <= {c.nq for c in cs}
    assert {(c.route, c.chunk_kernel) for c in cs} == {(sc.ROUTE_LIST, None), (sc.ROUTE_STREAM, None), (sc.ROUTE_RQ, sc.CHUNK_RQ),
                                                       (sc.ROUTE_RQ, sc.CHUNK_RJ)}
    top = [c for c in cs if c.id_base]
    assert top and all(c.id_base + c.nb < 2 ** 32 - 1 and c.id_base > 2 ** 32 - 10 ** 6 for c in top)
    assert all(c.W > 1 for c in sc.FAILING_TRANSPORT_CASES) and {c.exchanges for c in sc.FAILING_TRANSPORT_CASES} == {1, 2}


@pytest.mark.parametrize("c", sc.SEARCH_CASES, ids=lambda c: c.name)
def test_search_case_guard_branch_and_merged_reference(c):
    xb, q, tile, distinct = sc.search_data(c)
    assert xb.shape == (c.nb, c.d) and q.shape == (c.m, c.d) and len(tile) == c.nq and set(tile) == set(range(c.m))
    # (a) exact in any order
    unit = STEP * LO_STEP if c.real_lo else STEP * STEP
    sc.guard_exact(distinct, q, c.metric, unit, lo_free=(not c.real_lo, True))
    assert not c.real_lo or c.metric == IP
    # the planted duplicate sits in two different shards
    full = [(lo, hi) for lo, hi in c.bounds if hi > lo]
    a, b = full[0][0] + min(5, full[0][1] - full[0][0] - 1), full[-1][0] + min(7, full[-1][1] - full[-1][0] - 1)
    assert len(full) >= 2 and np.array_equal(xb[a], xb[b]) and a < full[0][1] <= full[-1][0] <= b
    # the branch
    tiles = int(_lib().lvs_flat_search_seed_tiles(c.nq, c.nominal, c.k))
    assert (tiles > 0) == c.lib_tiles, tiles
    assert c.exchanges == (2 if sc.pooled(c, 0 if c.opt_out else tiles) else 1)
    assert sc.planned_route(c) == (c.route, c.chunk_kernel), sc.planned_route(c)
    assert c.id_base >= 0 and all(c.id_base + hi < 0xFFFFFFFF for _, hi in c.bounds)
    # (b) the reference shard by shard, merged = the reference of the whole corpus
    want = sc.search_ref(c)
    assert want.dtype == np.uint64 and want.shape == (c.m, c.k)
    assert np.array_equal(sc.merged_shard_ref(c), want)
    real = min(c.k, c.nb)
    assert (want[:, :real] != 0).all() and (want[:, real:] == 0).all()
    ids = unpack_keys(want[:, :real])[1].astype(np.int64)
    assert ids.min() >= c.id_base and ids.max() < c.id_base + c.nb
    if c.nb > c.k and c.k < 1000:  # ties at rank k: the order among equal scores is part of what is compared
        D = (sc.ref_keys(xb, q, c.k + 1, c.metric) >> np.uint64(32))
        print(f"\n{c.name}: tiles {tiles}, k-th and (k+1)-th score equal for {float((D[:, c.k - 1] == D[:, c.k]).mean()):.2f} of the queries", end="")


def test_a_wrong_id_offset_fails_the_merged_reference():
    """Teeth of (b): shard lists whose ids are off by one do not merge into the whole-corpus reference."""
    c = next(c for c in sc.SEARCH_CASES if c.name.startswith("top1"))
    xb, q, _, _ = sc.search_data(c)
    (lo0, hi0), (lo1, hi1) = c.bounds[:2]
    parts = [sc.ref_keys(xb[lo0:hi0], q, c.k, c.metric, id_offset=lo0), sc.ref_keys(xb[lo1:hi1], q, c.k, c.metric, id_offset=lo1 + 1),
             sc.ref_keys(xb[hi1:], q, c.k, c.metric, id_offset=hi1)]
    merged = np.sort(np.concatenate(parts, axis=1), axis=1)[:, ::-1][:, :c.k]
    assert not np.array_equal(merged, sc.search_ref(c))


# ---- (c) the k-means cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.KM_RANKS, ids=lambda c: c.name)
def test_kmeans_rank_case_preconditions(c):
    x, cent = sc.km_ranks_data(c)
    assert x.shape == (c.n, c.d) and cent.shape == (c.K, c.d)
    assert all(sum(cut) == c.n for cut in c.cuts) and any(0 in cut and 1 in cut for cut in c.cuts) and c.cuts[0] == (c.n,)
    units = sc.km_guard(x, cent)
    dup = list(sc.KM_DUP_SLOTS)
    assert np.array_equal(cent[dup[0]], cent[dup[1]]) and np.array_equal(cent[dup[0]], cent[dup[2]])
    assert len(np.unique(cent, axis=0)) == c.K - 2
    assign, sums, counts = sc.lloyd64(x, cent)
    # the duplicates really leave two clusters empty (and no other): ties went to the lowest id
    assert np.flatnonzero(counts == 0).tolist() == dup[1:] and counts[dup[0]] > 0
    assert np.array_equal(sums, sums.astype(np.float32).astype(np.float64))
    new, h, nsplit = sc.faiss_update(sums, counts, cent, c.n)
    assert nsplit == 2 and (h > 0).all() and len(np.unique(new, axis=0)) == c.K
    print(f"\n{c.name}: largest partial sum {units:.0f} units, counts {counts.tolist()}", end="")


def test_kmeans_open_rows_case_preconditions():
    c = sc.KM_OPEN
    x, cent = sc.km_open_data()
    sc.km_guard(x, cent)
    assert np.array_equal(cent[0], cent[1]) and np.array_equal(cent[0], cent[2]) and len(np.unique(cent, axis=0)) == c.K - 2
    x64, c64 = x.astype(np.float64), cent.astype(np.float64)
    d2 = ((x64[:, None, :] - c64[None, [0] + list(range(3, c.K)), :]) ** 2).sum(2)
    assert (d2[:, 0:1] < d2[:, 1:]).all()  # the tripled row is STRICTLY nearer than every other centroid, for every row
    assign, _, counts = sc.lloyd64(x, cent)
    assert not assign.any() and counts[0] == c.n
    # more open rows than one batch on the large shard, and on one rank
    assert all(cut[0] > sc.CAP_OPEN and cut[0] // 8 <= sc.CAP_OPEN for cut in c.cuts)


def test_kmeans_chunk_case_preconditions():
    cent = sc.km_chunk_centroids()
    assert cent.shape == (sc.KM_CHUNK_K, sc.KM_CHUNK_D) and len(np.unique(cent, axis=0)) == sc.KM_CHUNK_K  # pairwise distinct
    assert np.array_equal(cent, cent.astype(np.float16).astype(np.float32))
    lib = _lib()
    assert sc.KM_CHUNK_K == 16384  # LVS_NEAREST3_MAX_ROWS: the smallest chunk
    step = sc.km_chunk_step(lib.lvs_nearest3_workspace_bytes)
    n = step + sc.KM_CHUNK_TAIL
    assert step % 65536 == 0 and n <= sc.KM_CHUNK_MAX_N, (step, n)
    cmap = sc.km_chunk_map(n)
    counts = np.bincount(cmap, minlength=sc.KM_CHUNK_K)
    # sums == counts x centroid, exact: the largest is far below 2^24 units
    assert counts.min() > 0 and (counts.max() * np.abs(cent).max() / STEP) < 2.0 ** 20
    # nearest centroid of a copy of centroid j is j, strictly: pairwise distinct lattice points are at least one unit apart
    sub = cent[:512].astype(np.float64)
    d2 = ((sub[:, None, :] - sub[None, :, :]) ** 2).sum(2) + np.eye(512) * 10
    assert d2.min() >= STEP * STEP
    # the tied variant: three centroids one row, two others one row; each chunk holds copies of both groups
    tied, canon = sc.km_chunk_case(True)
    assert len(np.unique(tied, axis=0)) == sc.KM_CHUNK_K - 3 and np.array_equal(tied[canon], tied)
    assert np.flatnonzero(canon != np.arange(sc.KM_CHUNK_K)).tolist() == [6, 7, 10] and canon[[6, 7, 10]].tolist() == [5, 5, 9]
    for lo, hi in ((0, step), (step, n)):
        assert np.isin(cmap[lo:hi], sc.KM_CHUNK_DOUBLE).any() and np.isin(cmap[lo:hi], sc.KM_CHUNK_TRIPLE).any()
    print(f"\nchunk case: step {step}, n {n}, counts {counts.min()} .. {counts.max()}", end="")
