"""``lvs_search_sharded`` and ``lvs_kmeans_iteration`` with an all-reduce - the two calls that run a whole multi-GPU step inside
the library - on several ranks, bit for bit.  The ranks are threads of this process with one stream each (tests/thread_ranks.py);
the cases, their exact-arithmetic data and their references are tests/sharded_cases.py, checked on the CPU by
tests/test_sharded_cases_host.py.

Search: every rank's ``out_keys`` equal the oracle's whole-corpus ``ref_keys`` (``np.array_equal`` on the uint64 bits, every
query), the ranks made the expected number of exchanges, and every rank ran in a guarded workspace of exactly
``lvs_search_sharded_workspace_bytes(W, ...)`` for its own shard - with the scratch pre-filled with 0xFF and with 0x00.

k-means: centroids, packed image, norms, statistics and split count of every rank after every iteration are the one-rank run's,
bit for bit, whatever the shard cut; the first iteration also equals a float64 Lloyd step and the oracle's restatement of
faiss's division and split.  Run with -s for the figures each case prints (tiles, route, host counts, times)."""
import ctypes
import time

import numpy as np
import pytest

import sharded_cases as sc
import thread_ranks
import ws_guard
from lattice_cases import F16, SPLIT, _assert_keys, _pack, _u64
from lotus_amd import _capi

pytestmark = pytest.mark.gpu

SENTINEL = 0x5C  # the byte every out_keys buffer holds before the call


def _ptr(t):
    return int(t.data_ptr()) if t is not None and t.numel() else None


# ---- lvs_search_sharded ------------------------------------------------------------------------------------------------------
def _search_setup(be, c, fill, pool):
    """Everything a rank hands to the library, allocated here on the main thread: (queries, per rank (shard, lo, ws, keys), tiles)"""
    xb, q, tile, _ = sc.search_data(c)
    queries = _pack(be, q[tile], c.qpack)
    corpus = _pack(be, xb, c.bpack)
    lib_tiles = int(be.lib.lvs_flat_search_seed_tiles(c.nq, c.nominal, c.k))
    assert (lib_tiles > 0) == c.lib_tiles, lib_tiles  # the branch the case is here for
    tiles = 0 if c.opt_out else lib_tiles
    ranks = []
    for lo, hi in c.bounds:
        shard = be.slice_rows(corpus, lo, hi)
        need = int(be.lib.lvs_search_sharded_workspace_bytes(c.W, c.nq, shard.n, c.d, c.k, shard.mode, queries.mode, tiles))
        assert need > 0
        ranks.append((shard, lo, pool.alloc(need, fill), ws_guard.guarded(pool, (c.nq, c.k), be.torch.int64, SENTINEL)))
    be.synchronize()
    return queries, ranks, tiles


def _search_call(be, c, rk, queries, shard, lo, ws, keys, tiles, all_gather):
    with rk.on_stream():
        return be.lib.lvs_search_sharded(all_gather, None, c.W, _ptr(shard.rows), shard.mode, shard.n, _ptr(queries.rows), queries.mode,
                                         c.nq, c.d, c.metric, c.k, _ptr(shard.norms), _ptr(queries.norms), c.id_base + lo, tiles,
                                         _ptr(keys), _ptr(ws), int(ws.numel()), int(rk.stream.cuda_stream))


@pytest.mark.parametrize("fill", [0xFF, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("c", sc.SEARCH_CASES, ids=lambda c: c.name)
def test_sharded_search_equals_the_whole_corpus_reference_on_every_rank(hip_backend, c, fill):
    be = hip_backend
    pool = ws_guard.GuardedPool(be.device)
    queries, ranks, tiles = _search_setup(be, c, fill, pool)
    want = sc.search_ref(c)[np.arange(c.nq) % c.m]

    def rank(rk):
        shard, lo, ws, keys = ranks[rk.r]
        st = _search_call(be, c, rk, queries, shard, lo, ws, keys, tiles, rk.all_gather.ptr)
        rk.stream.synchronize()
        assert st == 0, be.lib.lvs_last_error()
        return rk.all_gather.calls

    calls = thread_ranks.run_ranks(c.W, rank, be.device, pool_bytes=max(tiles * c.nq * 4, c.nq * c.k * 8))
    assert calls == [c.exchanges] * c.W, calls
    got = [_u64(keys) for _, _, _, keys in ranks]
    for r in range(c.W):
        _assert_keys(got[r], want, f"{c.name} rank {r}")
    assert all(np.array_equal(got[0], g) for g in got[1:])
    pool.assert_clean()
    print(f"\n{c.name} fill {fill:#04x}: seed tiles {tiles} (library {'> 0' if c.lib_tiles else '== 0'}), {c.exchanges} exchange(s), nominal "
          f"shard route {c.route} chunk kernel {c.chunk_kernel}, workspace {[int(ws.numel()) for _, _, ws, _ in ranks]}", end="")


@pytest.mark.parametrize("c", sc.FAILING_TRANSPORT_CASES, ids=lambda c: c.name)
def test_a_failing_all_gather_is_reported_on_every_rank_and_out_keys_stay_untouched(hip_backend, c):
    """The transport returns LVS_EDEVICE at once on every rank (it touches neither the GPU nor the barrier): the call returns
    that status on every rank and ``out_keys`` keeps its sentinel fill - with pooled thresholds the first exchange fails, without
    them the shard has been searched into the workspace by then."""
    be = hip_backend
    pool = ws_guard.GuardedPool(be.device)
    queries, ranks, tiles = _search_setup(be, c, 0xFF, pool)
    failing = _capi.CALLBACKS["lvs_all_gather_fn"](lambda ctx, send, recv, nbytes, stream: _capi.EDEVICE)

    def rank(rk):
        shard, lo, ws, keys = ranks[rk.r]
        st = _search_call(be, c, rk, queries, shard, lo, ws, keys, tiles, ctypes.cast(failing, ctypes.c_void_p))
        rk.stream.synchronize()
        return st

    assert thread_ranks.run_ranks(c.W, rank, be.device) == [_capi.EDEVICE] * c.W
    for _, _, _, keys in ranks:
        assert bool((keys.view(be.torch.uint8) == SENTINEL).all())
    pool.assert_clean()


# ---- lvs_kmeans_iteration ----------------------------------------------------------------------------------------------------
class _KmRank:
    """One rank's buffers of a k-means run: its rows, its own copy of the centroid state, outputs and exact-size workspace."""

    def __init__(self, be, pool, packed, lo, hi, cent, K, n_total, niter, fill):
        torch = be.torch
        self.be, self.K, self.n_total = be, K, n_total
        self.x = be.slice_rows(packed, lo, hi)
        self.x2 = self.x.norms.double().sum().reshape(1)  # float64 sum of THIS shard's norms (0 for an empty one)
        self.cent = be.to_device(cent).clone()
        self.cpk, self.cstats = be.kmeans_pack_centroids(self.cent, SPLIT)
        self.keys = ws_guard.guarded(pool, (self.x.n,), torch.int64, SENTINEL)
        self.obj = ws_guard.guarded(pool, (niter,), torch.float64, 0)
        self.nsplit = ws_guard.guarded(pool, (niter,), torch.int32, SENTINEL)
        need = int(be.lib.lvs_kmeans_iteration_workspace_bytes(self.x.n, self.x.d, K, self.x.mode, SPLIT))
        assert need > 0
        self.ws = pool.alloc(need, fill)
        self.host_counts = (ctypes.c_int64 * 2)()
        self.counts = []

    def iterate(self, it, all_reduce, stream):
        x = self.x
        rc = self.be.lib.lvs_kmeans_iteration(all_reduce, None, _ptr(x.rows), x.mode, x.n, x.d, _ptr(x.norms), _ptr(self.x2), 0, self.K,
                                              self.n_total, _ptr(self.cent), SPLIT, _ptr(self.cpk.rows), _ptr(self.cpk.norms),
                                              _ptr(self.cstats), _ptr(self.keys), int(self.obj[it:].data_ptr()),
                                              int(self.nsplit[it:].data_ptr()), ctypes.addressof(self.host_counts), _ptr(self.ws),
                                              int(self.ws.numel()), stream)
        assert rc == 0, self.be.lib.lvs_last_error()
        self.counts.append((int(self.host_counts[0]), int(self.host_counts[1])))

    def state(self):
        """host copies of everything the iteration updates"""
        return dict(centroids=self.cent.cpu().numpy(), packed=self.cpk.rows.cpu().numpy().view(np.uint16), c_norms=self.cpk.norms.cpu().numpy(),
                    c_stats=self.cstats.cpu().numpy(), keys=self.keys.cpu().numpy().view(np.uint64), obj=self.obj.cpu().numpy(),
                    nsplit=self.nsplit.cpu().numpy())


def _km_run(be, x, cent, mode, cut, niter, fill=0xFF, transport=True):
    """``niter`` iterations on ``len(cut)`` thread ranks (``transport=False``: one rank, a NULL all-reduce, no thread) ->
    per iteration a list of the ranks' ``state()``, the ranks themselves"""
    pool = ws_guard.GuardedPool(be.device)
    packed = _pack(be, x, mode)
    offs = np.concatenate([[0], np.cumsum(cut)]).astype(np.int64)
    ranks = [_KmRank(be, pool, packed, int(offs[r]), int(offs[r + 1]), cent, len(cent), len(x), niter, fill) for r in range(len(cut))]
    be.synchronize()
    if not transport:
        assert len(cut) == 1
        states = []
        for it in range(niter):
            t0 = time.perf_counter()
            ranks[0].iterate(it, None, be._stream())
            be.synchronize()
            ranks[0].seconds = time.perf_counter() - t0
            states.append([ranks[0].state()])
    else:
        def rank(rk):
            mine, out = ranks[rk.r], []
            for it in range(niter):
                with rk.on_stream():
                    mine.iterate(it, rk.all_reduce.ptr, int(rk.stream.cuda_stream))
                    rk.stream.synchronize()
                    out.append(mine.state())
            assert rk.all_reduce.calls == 2 * niter  # sums | counts as one float32 block, then the float64 objective
            return out

        K, d = cent.shape
        per_rank = thread_ranks.run_ranks(len(cut), rank, be.device, pool_bytes=(K * d + K) * 4)
        states = [[per_rank[r][it] for r in range(len(cut))] for it in range(niter)]
    pool.assert_clean()
    return states, ranks


def _ids_of(keys):
    from oracle.flat import unpack_keys

    return unpack_keys(keys.reshape(-1, 1))[1].reshape(-1)


def _assert_first_iteration_is_the_float64_lloyd_step(be, x, cent, mode, state, n_total):
    """Iteration 1, where the centroids are still lattice points and the arithmetic is exact: assignment, sums, counts and the
    updated centroids against float64 numpy and the oracle's restatement of faiss's division and split."""
    assign, sums, counts = sc.lloyd64(x, cent)
    keys = np.concatenate([s["keys"] for s in state])
    assert np.array_equal(_ids_of(keys), assign)
    dsums, dcounts = be.kmeans_accumulate_keys(_pack(be, x, mode), be.to_device(keys.view(np.int64)), len(cent))
    assert np.array_equal(dsums.cpu().numpy(), sums.astype(np.float32)) and np.array_equal(dcounts.cpu().numpy(), counts.astype(np.float32))
    new, _, nsplit = sc.faiss_update(sums, counts, cent, n_total)
    for s in state:
        assert np.array_equal(s["centroids"], new) and int(s["nsplit"][0]) == nsplit
    return assign, counts, nsplit


@pytest.fixture(scope="module")
def km_one_rank(hip_backend):
    """The W = 1 run of each rank case (NULL all-reduce), computed once"""
    cache = {}

    def get(c):
        if c.name not in cache:
            x, cent = sc.km_ranks_data(c)
            cache[c.name] = _km_run(hip_backend, x, cent, c.mode, (c.n,), c.niter, transport=False)[0]
        return cache[c.name]

    return get


@pytest.mark.parametrize("cut", sc.KM_RANKS[0].cuts, ids=lambda cut: "x".join(map(str, cut)))
@pytest.mark.parametrize("c", sc.KM_RANKS, ids=lambda c: c.name)
def test_kmeans_iteration_on_several_ranks_equals_one_rank(hip_backend, km_one_rank, c, cut):
    be = hip_backend
    x, cent = sc.km_ranks_data(c)
    one = km_one_rank(c)
    states, ranks = _km_run(be, x, cent, c.mode, cut, c.niter)
    offs = np.concatenate([[0], np.cumsum(cut)])
    # |obj_W - obj_1| <= n 2^-53 sum |x|^2: the float64 reordering bound of a sum of n terms bounded by sum |x|^2.
    # n = 9 001: 9 001 x 2^-53 = 9.993e-13, times sum |x|^2
    sum_x2 = float((x.astype(np.float64) ** 2).sum())
    assert abs(c.n * 2.0 ** -53 - 9.993e-13) < 1e-15
    obj_bound = c.n * 2.0 ** -53 * sum_x2
    for it in range(c.niter):
        ref = one[it][0]
        for r, s in enumerate(states[it]):
            for name in ("centroids", "packed", "c_norms", "c_stats"):
                assert np.array_equal(s[name].view(np.uint8), ref[name].view(np.uint8)), (it, r, name)
            assert int(s["nsplit"][it]) == int(ref["nsplit"][it]), (it, r)
            assert np.array_equal(s["keys"], ref["keys"][offs[r]:offs[r + 1]]), (it, r)
            assert s["obj"][it].tobytes() == states[it][0]["obj"][it].tobytes(), (it, r)  # the same bits on all ranks
            assert abs(float(s["obj"][it]) - float(ref["obj"][it])) <= obj_bound, (it, r, s["obj"][it], ref["obj"][it], obj_bound)
    assert int(one[0][0]["nsplit"][0]) > 0  # the split ran, on every rank, from all-reduced counts
    _, counts, nsplit = _assert_first_iteration_is_the_float64_lloyd_step(be, x, cent, c.mode, states[0], c.n)
    assert nsplit == 2
    print(f"\n{c.name} cut {cut}: out_host_counts (pairs, open) per rank and iteration {[rk.counts for rk in ranks]}, nsplit "
          f"{one[-1][0]['nsplit'].tolist()}, objective bound {obj_bound:.3e}, |difference| "
          f"{max(abs(float(states[it][0]['obj'][it]) - float(one[it][0]['obj'][it])) for it in range(c.niter)):.3e}", end="")


def test_the_one_rank_baseline_is_the_float64_lloyd_step_in_iteration_one(hip_backend, km_one_rank):
    """The W = 1 baseline itself against the float64 step (so the comparison above is not one wrong run against another)."""
    for c in sc.KM_RANKS:
        x, cent = sc.km_ranks_data(c)
        _assert_first_iteration_is_the_float64_lloyd_step(hip_backend, x, cent, c.mode, km_one_rank(c)[0], c.n)


def test_kmeans_iteration_with_more_open_rows_than_one_batch(hip_backend):
    """Three equal centroids nearest to every row: every row is open (three centroids inside the bound), 66 001 / 70 001 of them
    on one rank - more than ``cap_open`` = 65 536, so the exact search of the open rows runs in two batches."""
    be, c = hip_backend, sc.KM_OPEN
    x, cent = sc.km_open_data()
    runs = {}
    for cut in c.cuts:
        states, ranks = _km_run(be, x, cent, c.mode, cut, 1)
        assert ranks[0].counts[0][1] > sc.CAP_OPEN, ranks[0].counts  # the precondition of a second batch
        assert [rk.counts[0] for rk in ranks] == [(0, n) for n in cut]  # every row open, none a pair
        for s in states[0]:
            assert not _ids_of(s["keys"]).any()  # every row's key carries id 0
        assign, counts, nsplit = _assert_first_iteration_is_the_float64_lloyd_step(be, x, cent, c.mode, states[0], c.n)
        assert counts[0] == c.n and nsplit == c.K - 1
        runs[cut] = states[0]
        print(f"\n{c.name} cut {cut}: out_host_counts {[rk.counts[0] for rk in ranks]}, nsplit {nsplit}", end="")
    one = runs[c.cuts[0]][0]
    for s in runs[c.cuts[1]]:
        for name in ("centroids", "packed", "c_norms", "c_stats", "nsplit"):
            assert np.array_equal(s[name].view(np.uint8), one[name].view(np.uint8)), name
    assert np.array_equal(np.concatenate([s["keys"] for s in runs[c.cuts[1]]]), one["keys"])


# (last in the file: about 2 GiB of scratch)
@pytest.mark.parametrize("dups", [False, True], ids=["distinct", "tied"])
def test_kmeans_iteration_with_more_rows_than_one_assignment_chunk(hip_backend, dups):
    """K = 16 384 centroids (LVS_NEAREST3_MAX_ROWS: the smallest chunk the 2 GiB assignment budget gives) and step + 70 001 rows:
    the row-chunk loop runs twice, the second time on a ragged tail.  Row i is an exact copy of centroid c[i]: its key carries
    c[i], counts == bincount(c), sums == counts x centroid (exact on the lattice) - which the division turns back into the
    centroids themselves.  ``out_host_counts`` are the totals over both chunks: the sum of what a call on each chunk alone
    reports.  On pairwise distinct centroids every row is certified and those totals are (0, 0); the ``tied`` variant makes
    three centroids one row and two others one row, so each chunk has open rows and pairs of its own - both at row offsets
    beyond the first chunk - whose numbers follow from c, and every such row must end at the lowest of its tied centroids."""
    be, K = hip_backend, sc.KM_CHUNK_K
    step = sc.km_chunk_step(be.lib.lvs_nearest3_workspace_bytes)
    n = step + sc.KM_CHUNK_TAIL
    assert n <= sc.KM_CHUNK_MAX_N, (step, n)  # a changed budget fails here instead of uncovering the loop
    cent, canon = sc.km_chunk_case(dups)
    cmap = sc.km_chunk_map(n)
    x = cent[cmap]
    want = canon[cmap]
    states, ranks = _km_run(be, x, cent, F16, (n,), 1, transport=False)
    s = states[0][0]
    assert np.array_equal(_ids_of(s["keys"]), want)
    counts = np.bincount(want, minlength=K)
    keys_dev = be.to_device(s["keys"].view(np.int64))
    dsums, dcounts = be.kmeans_accumulate_keys(_pack(be, x, F16), keys_dev, K)
    assert np.array_equal(dcounts.cpu().numpy(), counts.astype(np.float32))
    assert np.array_equal(dsums.cpu().numpy(), counts[:, None].astype(np.float32) * cent)
    new, _, nsplit = sc.faiss_update(counts[:, None].astype(np.float64) * cent, counts, cent, n)
    assert nsplit == (3 if dups else 0) and np.array_equal(s["centroids"], new) and int(s["nsplit"][0]) == nsplit
    del keys_dev, dsums, dcounts
    # the chunks on their own: a call on the first `step` rows and one on the tail - the same keys, and the host counts add up
    bounds = ((0, step), (step, n))
    parts = [_km_run(be, x[lo:hi], cent, F16, (hi - lo,), 1, transport=False) for lo, hi in bounds]
    assert np.array_equal(np.concatenate([p[0][0][0]["keys"] for p in parts]), s["keys"])
    per_chunk = [p[1][0].counts[0] for p in parts]
    assert ranks[0].counts[0] == tuple(sum(c[i] for c in per_chunk) for i in range(2)), (ranks[0].counts, per_chunk)
    if dups:  # (pairs, open) of a chunk: its copies of the doubled and of the tripled centroid
        assert per_chunk == [(int(np.isin(cmap[lo:hi], sc.KM_CHUNK_DOUBLE).sum()), int(np.isin(cmap[lo:hi], sc.KM_CHUNK_TRIPLE).sum()))
                             for lo, hi in bounds], per_chunk
        assert all(pairs > 0 and opened > 0 for pairs, opened in per_chunk)
    print(f"\nchunk case ({'tied' if dups else 'distinct'} centroids): step {step}, n {n}, out_host_counts {ranks[0].counts[0]} = "
          f"{per_chunk}, workspace {int(ranks[0].ws.numel())} bytes, {ranks[0].seconds:.3f} s for the two-chunk call", end="")
    del states, ranks, parts
    be.torch.cuda.empty_cache()
