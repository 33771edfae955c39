"""Exact-arithmetic cases for the two entry points that run a whole multi-GPU step inside one C call - ``lvs_search_sharded``
and ``lvs_kmeans_iteration`` with an all-reduce -: the case tables, their data and their references.  No test lives here:
tests/test_sharded_cases_host.py checks the cases and the references on the CPU, tests/test_gpu_sharded_abi.py runs them on
thread ranks (tests/thread_ranks.py).  Imports no GPU module.

The data are ``lattice_cases``' (small integers times 2^-3: float32 sums are exact in any order), so nothing here has a
tolerance: a sharded search returns the whole-corpus ``ref_keys`` bit for bit on every rank, and a sharded Lloyd iteration
the one-rank centroids bit for bit, whatever the shard cut."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from lattice_cases import (CHUNK_RJ, CHUNK_RQ, F16, IP, L2, ROUTE_LIST, ROUTE_RQ, ROUTE_RQ_JOIN, ROUTE_STREAM, SPLIT, STEP, _topk_arrays,
                           flavour, guard_exact, lattice, ref_keys)

ID_TOP = 4_294_000_000  # an id base in the top of the 32-bit range


# ---- lvs_search_sharded ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Sharded:
    name: str
    nq: int
    m: int                     # distinct queries: the batch is base_q[arange(nq) % m]
    sizes: tuple               # rows per rank
    k: int
    metric: int
    d: int = 64
    bpack: int = F16
    qpack: int = F16
    lib_tiles: bool = False    # lvs_flat_search_seed_tiles(nq, nominal shard, k) > 0 ?
    opt_out: bool = False      # the caller passes seed_tiles = 0 whatever the library proposes
    exchanges: int = 1         # all-gather calls per rank: 2 with pooled thresholds, 1 without, 0 on one rank
    real_lo: bool = False
    dense: bool = False
    id_base: int = 0
    seed: int = 0
    route: int = ROUTE_LIST    # the nominal shard's search, as the compiled planner routes it
    chunk_kernel: int = None   # of a register-resident route: CHUNK_RQ / CHUNK_RJ

    @property
    def W(self):
        return len(self.sizes)

    @property
    def nb(self):
        return sum(self.sizes)

    @property
    def nominal(self):
        """the shard size every rank derives the exchange's shape from"""
        return max(self.sizes)

    @property
    def bounds(self):
        offs = np.concatenate([[0], np.cumsum(self.sizes)])
        return [(int(a), int(b)) for a, b in zip(offs, offs[1:])]


def pooled(c, tiles):
    """``sharded_plan``'s decision, restated: sample scores are exchanged iff there are several ranks, fp16 rows on both sides,
    single-pass lists and at least k sample tiles over all ranks."""
    return c.W > 1 and (c.bpack, c.qpack) == (F16, F16) and c.k <= 56 and tiles * c.W >= c.k


def _search_table():
    out = []

    def add(name, nq, m, sizes, k, metrics=(IP, L2), packs=((F16, F16),), **kw):
        for bp, qp in packs:
            for metric in metrics:
                d = kw.get("d", 64)
                out.append(Sharded(f"{name}-{nq}q-d{d}-k{k}-W{len(sizes)}-{'FS'[bp]}{'FS'[qp]}-{'IL'[metric]}", nq, m, tuple(sizes), k,
                                   metric, bpack=bp, qpack=qp, **kw))

    SS, FS = (SPLIT, SPLIT), (F16, SPLIT)
    # pooled thresholds on NEGATIVE scores; one shard shorter than a sample tile, one empty (-inf blocks, NULL row pointers)
    add("pooled", 2100, 25, (41001, 200, 0, 45003), 10, metrics=(L2,), lib_tiles=True, exchanges=2)
    # the same data, inner product, the caller opts out of the pooled thresholds: one exchange, the same keys
    add("opt-out", 2100, 25, (41001, 200, 0, 45003), 10, metrics=(IP,), lib_tiles=True, opt_out=True)
    # hi|lo operands, three uneven shards of a 12 000-row corpus: the certified-precision search per shard, then the merge
    add("split", 300, 150, (5000, 2999, 4001), 10, packs=(SS, FS))
    add("split-real-lo", 300, 150, (5000, 2999, 4001), 10, metrics=(IP,), packs=(SS,), real_lo=True)
    # ... and with shards long enough that the library proposes sample tiles: sharded_plan switches them off BY PACK MODE
    add("split-tiles-off", 300, 150, (41001, 200, 20000), 10, metrics=(IP,), packs=(SS,), lib_tiles=True)
    add("split-tiles-off", 300, 150, (41001, 200, 20000), 10, metrics=(L2,), packs=(FS,), lib_tiles=True)
    # multi-pass lists: no pooling
    for k in (57, 100):
        add("multi-pass", 200, 100, (3000, 3000), k)
    # the long-list merge on gathered lists; the 1 500-row shard is shorter than k: its zero keys sort last
    add("long-lists", 12, 12, (3000, 1500), 1000)
    add("long-lists", 12, 12, (3000, 1500, 2600), 2048)
    # fewer than k rows overall: the output tail is key 0 on every rank
    add("six-rows", 5, 5, (3, 0, 1, 2), 10)
    # the top-1 merge
    add("top1", 700, 350, (2000, 1203, 1797), 1)
    # the small-batch routes inside the seeded entry.  At d = 64 every one of them is the stream kernel; at d = 256 the 97 and 128
    # queries go to lvs_rq_kernel (32 queries per wave) and the 129 to lvs_rj_kernel (the join kernel)
    for nq in (1, 96, 97, 128, 129):
        add("small-batch", nq, nq if nq < 64 else nq // 2, (33001, 33001), 15, route=ROUTE_STREAM)
        add("small-batch", nq, nq if nq < 64 else nq // 2, (33001, 33001), 15, d=256,
            route=ROUTE_STREAM if nq <= 96 else ROUTE_RQ, chunk_kernel=None if nq <= 96 else (CHUNK_RQ if nq <= 128 else CHUNK_RJ))
    # ids in the top of the 32-bit range through search, gather and merge (ties are decided by id)
    add("ids-top", 300, 150, (5000, 2999, 4001), 10, id_base=ID_TOP)
    return out


SEARCH_CASES = _search_table()
# the transport that fails at once: any small case
FAILING_TRANSPORT_CASES = [next(c for c in SEARCH_CASES if c.name.startswith("pooled")), next(c for c in SEARCH_CASES if c.name.startswith("top1"))]


def planned_route(c):
    """(route kind, chunk kernel or None) of the search of the NOMINAL shard, as the compiled planner reports it."""
    import plan_native

    kind, *_, jper, _ = plan_native.ask([f"route {c.nq} {c.nominal} {c.d} {c.k} {c.bpack} {c.qpack}"])[0]
    if kind not in (ROUTE_RQ, ROUTE_RQ_JOIN):
        return kind, None
    chunks = plan_native.ask([f"chunks {c.nq} 65536"])[0]
    assert len(chunks) == 1
    return kind, plan_native.ask([f"chunk_kernel {chunks[0]} {c.nominal} {jper * 16} {c.k}"])[0][0]


def search_data(c):
    """(xb [nb, d], base_q [m, d], tile [nq], the corpus' distinct rows).  One exact duplicate is planted across two shards:
    a row of the last non-empty shard is a copy of a row of the first one - equal scores, the ids decide."""
    xb, q, distinct = _topk_arrays(c.nq, c.nb, c.d, c.dense, c.seed, c.m, c.real_lo)
    xb = xb.copy()
    full = [(lo, hi) for lo, hi in c.bounds if hi > lo]
    (a0, a1), (b0, b1) = full[0], full[-1]
    xb[b0 + min(7, b1 - b0 - 1)] = xb[a0 + min(5, a1 - a0 - 1)]
    return xb, q, np.arange(c.nq) % c.m, distinct


@functools.lru_cache(maxsize=4)
def search_ref(c):
    """ref_keys of the distinct queries over the WHOLE corpus, [m, k] uint64"""
    xb, q, _, _ = search_data(c)
    return ref_keys(xb, q, c.k, c.metric, id_offset=c.id_base)


def merged_shard_ref(c):
    """The reference taken shard by shard and merged per query: ``ref_keys`` of every shard with its id offset (an empty shard
    gives key 0 everywhere), all lists of a query sorted descending as uint64, the first k kept - key 0 sorts last."""
    xb, q, _, _ = search_data(c)
    parts = []
    for lo, hi in c.bounds:
        parts.append(ref_keys(xb[lo:hi], q, c.k, c.metric, id_offset=c.id_base + lo) if hi > lo else np.zeros((len(q), c.k), np.uint64))
    allk = np.concatenate(parts, axis=1)
    return np.sort(allk, axis=1)[:, ::-1][:, :c.k]


# ---- lvs_kmeans_iteration ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class KMeans:
    name: str
    n: int
    K: int
    d: int
    mode: int
    cuts: tuple
    niter: int = 1


KM_RANKS = [KMeans("ranks-F", 9001, 12, 16, F16, ((9001,), (4000, 5001), (5000, 0, 1, 4000)), niter=3),
            KMeans("ranks-S", 9001, 12, 32, SPLIT, ((9001,), (4000, 5001), (5000, 0, 1, 4000)), niter=3)]
KM_OPEN = KMeans("open-rows", 70_001, 8, 16, F16, ((70_001,), (66_001, 4000)))
KM_CHUNK_K, KM_CHUNK_D, KM_CHUNK_TAIL, KM_CHUNK_MAX_N = 16384, 16, 70_001, 4_000_000
CAP_OPEN = 65536  # iter_plan: open rows searched exactly per batch, below 524 288 rows
KM_DUP_SLOTS = (2, 4, 8)  # the three initial centroids that are one row


@functools.lru_cache(maxsize=2)
def km_ranks_data(c):
    """(rows float32 [n, d], initial centroids float32 [K, d]).  The centroids are rows of the data: K - 2 pairwise different
    rows, one of them three times (``KM_DUP_SLOTS``) - ties go to the lowest id, so the two later copies' clusters stay empty."""
    x = lattice(c.n, c.d, 61 + c.d, **flavour(c.d, False))
    _, first = np.unique(x, axis=0, return_index=True)
    first = np.sort(first)
    pick = first[np.linspace(0, len(first) - 1, c.K - 2).astype(np.int64)]
    ids = list(pick)
    for slot in KM_DUP_SLOTS[1:]:
        ids.insert(slot, pick[KM_DUP_SLOTS[0]])
    assert len(ids) == c.K
    return x, x[np.asarray(ids)].copy()


@functools.lru_cache(maxsize=1)
def km_open_data():
    """(rows, centroids): centroids 0, 1 and 2 are ONE row - every coordinate one lattice step -, the other five have four steps
    in every coordinate.  A data coordinate is -1, 0 or 1 step: it is at most 2 steps from the first and at least 3 from any of
    the others, so the tripled row is the strictly nearest centroid of every data row - and three centroids tie for it."""
    c = KM_OPEN
    x = lattice(c.n, c.d, 67, levels=1, keep=0.5)
    cent = np.empty((c.K, c.d), np.float32)
    cent[:3] = np.float32(STEP)
    signs = np.random.default_rng(68).integers(0, 2, (c.K - 3, c.d)) * 2 - 1
    cent[3:] = (signs * 4 * STEP).astype(np.float32)
    return x, cent


@functools.lru_cache(maxsize=1)
def km_chunk_centroids():
    """16 384 pairwise distinct lattice centroids"""
    rows = np.unique(lattice(40_000, KM_CHUNK_D, 71, levels=2, keep=1.0), axis=0)
    assert len(rows) >= KM_CHUNK_K
    return np.ascontiguousarray(rows[np.random.default_rng(72).permutation(len(rows))[:KM_CHUNK_K]])


KM_CHUNK_TRIPLE, KM_CHUNK_DOUBLE = (5, 6, 7), (9, 10)


def km_chunk_case(dups):
    """(centroids, canon): the distinct centroids, or - ``dups`` - the same with centroids 5, 6, 7 one row and 9, 10 one row, so
    that both chunks hold open rows (three tied centroids) and pairs (two); ``canon[j]``: the lowest index among the centroids
    equal to centroid j - the id a copy of centroid j must be assigned."""
    cent, canon = km_chunk_centroids().copy(), np.arange(KM_CHUNK_K)
    if dups:
        for group in (KM_CHUNK_TRIPLE, KM_CHUNK_DOUBLE):
            cent[list(group)] = cent[group[0]]
            canon[list(group)] = group[0]
    return cent, canon


def km_chunk_map(n):
    """the fixed pseudo-random map row -> centroid"""
    return np.random.default_rng(73).integers(0, KM_CHUNK_K, n)


def km_chunk_step(nearest3_workspace_bytes):
    """``iter_plan``'s rows per assignment chunk, from the library's own size function (2 GiB KM_NEAREST3_BUDGET)."""
    per_q = int(nearest3_workspace_bytes(1 << 20, KM_CHUNK_K, KM_CHUNK_D)) >> 20
    assert per_q > 0
    return max(((2 << 30) // per_q) >> 16 << 16, 1 << 16)


def lloyd64(x, cent):
    """One float64 Lloyd assignment, the lowest centroid index on ties -> (assign int64 [n], sums float64 [K, d], counts [K])"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(cent, np.float64)
    assign = np.empty(len(x64), np.int64)
    for r0 in range(0, len(x64), 1 << 16):
        xs = x64[r0:r0 + (1 << 16)]
        d2 = (xs * xs).sum(1)[:, None] + (c64 * c64).sum(1)[None, :] - 2.0 * (xs @ c64.T)
        assign[r0:r0 + len(xs)] = np.argmin(d2, axis=1)  # the first of equal minima: the lowest index
    sums = np.zeros(c64.shape, np.float64)
    np.add.at(sums, assign, x64)
    return assign, sums, np.bincount(assign, minlength=len(c64))


def faiss_update(sums, counts, cent, n_total):
    """The oracle's restatement of faiss's division and split_clusters on float32 sums / counts -> (centroids, hassign, nsplit)"""
    from oracle.kmeans import _split_clusters

    c, h = np.array(cent, np.float32), np.array(counts, np.float32)
    s = np.asarray(sums, np.float32)
    nz = h > 0
    c[nz] = s[nz] * (np.float32(1.0) / h[nz])[:, None]
    nsplit = _split_clusters(int(n_total), h, c, False)
    return c, h, nsplit


def km_guard(x, cent):
    """The k-means counterpart of guard 1: the distances of the first iteration are exact, and every partial sum of the
    accumulation - bounded by the sum of the magnitudes per coordinate over ALL rows - stays far below 2^24 units."""
    guard_exact(np.unique(cent, axis=0), np.unique(x, axis=0)[:4096], L2, STEP * STEP)
    units = np.abs(np.asarray(x, np.float64)).sum(0).max() / STEP
    assert units < 2.0 ** 22, units
    return units
