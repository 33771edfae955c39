"""``HipVS`` - MI355X-native drop-in for the reference's default vector store.

Mirrors ``lotus.vector_store.faiss_vs.FaissVS`` (``lotus/vector_store/faiss_vs.py:13-77``): same four plugin
methods (``lotus/vector_store/vs.py:17,24,31,54``), same on-disk ``{index_dir}/vecs`` pickle (+ a faiss-format
``{index_dir}/index``), same result conventions - ``RMOutput(distances float32 [Q,K], indices int64 [Q,K])`` best
first, missing slots ``-1`` / ``-FLT_MAX`` (inner product) or ``+FLT_MAX`` (L2).  The arithmetic runs in
``liblotus_hip.so`` (tiled MFMA distance + fused top-k); there is no CPU path.

Differences that are deliberate supersets (SURVEY.md section 8(a) edge-case table):
  * ``K == 0`` returns empty ``[Q,0]`` arrays instead of faiss's ``AssertionError``;
  * a dimension mismatch raises ``ValueError``;
  * ``ids`` covering every row in order skips the gather; a strict subset is gathered on the GPU instead of
    rebuilding an index from a re-read pickle (``faiss_vs.py:57-64``);
  * several indexes stay resident (keyed by ``index_dir``) so ``sem_sim_join`` flipping left/right
    (``sem_sim_join.py:111-128``) does not reload from disk;
  * with ``torch.distributed`` initialised and ``shard=True`` the corpus is row-sharded over the ranks and the
    per-shard top-k lists are merged after one all-gather (RCCL over xGMI on GPUs);
  * ``factory_string="IVF<nlist>,Flat"`` builds the inverted-file index ``FaissVS`` advertises but cannot train
    (``faiss_vs.py:23-24`` calls ``add()`` without ``train()``): plain searches probe ``nprobe`` lists, everything else
    stays exact (see ``HipVS``); ``"IVF<nlist>,SQ8"`` adds faiss's 8-bit residual scalar quantizer on top of the same lists,
    ``"IVF<nlist>,PQ<M>"`` faiss's residual product quantizer (8-bit codes, M bytes per row); either followed by
    ``",Refine(Flat)"`` re-ranks the codes' best candidates exactly against the full-precision rows (``IndexRefineFlat``).
"""
from __future__ import annotations

import os
import pickle
import re
from collections import OrderedDict
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _capi, store
from .compat import VS, RMOutput

METRIC_INNER_PRODUCT = _capi.METRIC_IP  # == faiss.METRIC_INNER_PRODUCT (0)
METRIC_L2 = _capi.METRIC_L2  # == faiss.METRIC_L2 (1)

FLT_MAX = np.float32(3.4028234663852886e38)
_RANK_BLOCK_SCORES = 1 << 28  # K = N ranking: scores (float32) materialised at a time
_IVF_SEED = 1234  # k-means seed of the IVF centroids (faiss's ClusteringParameters default)


@dataclass
class _Resident:
    """One loaded index: its device image + where ``get_vectors_from_index`` gets the stored rows from."""

    vecs: Any  # [n,d] rows in their stored dtype: the caller's ndarray, a read-only memmap, or None (opened on demand)
    packed: Any  # backend PackedRows of this rank's shard
    n: int  # rows in the whole index
    d: int
    lo: int  # first global row of this rank's shard
    hi: int
    sig: Any = None  # store.signature() of the directory when it was loaded (None: never persisted)
    ivf: Any = None  # backend IvfLists over `packed` (IVF stores only): centroids, offsets, row numbers
    codes: Any = None  # beside `ivf`, the codec and codes in list order: backend IvfSq8Lists / IvfPqLists (None: IVF-Flat)


@dataclass(frozen=True)
class _IvfMode:
    """The mode of an IVF store, parsed once from its factory string: all that differs between IVF-Flat, IVF-SQ8 and IVF-PQ.
    ``ent``: the store's ``_Resident``, whose ``codes`` this mode's ``train`` or ``upload`` made."""

    kind: str  # "Flat" | "SQ8" | "PQ"
    M: int | None = None  # subspaces of a PQ store
    refine: bool = False  # "...,Refine(Flat)": the codes' candidates are re-ranked by their exact scores (SQ8 and PQ only)

    @property
    def requires(self):  # the methods an injected backend must have to build such a store: asked of the newest modes only
        return (("ivf_pq_search",) if self.kind == "PQ" else ()) + (("refine_keys",) if self.refine else ())

    def check_width(self, d: int, factory_string: str) -> None:
        """faiss asserts d % M == 0 for a product quantizer: rows of another width cannot back an IVF-PQ store."""
        if self.kind == "PQ" and d % self.M != 0:
            raise ValueError(f"factory_string={factory_string!r} needs a dimension divisible by M={self.M}, got d={d}")

    def fits(self, be, ent, k: int) -> bool:
        if self.kind == "SQ8":
            return be.ivf_sq8_fits(ent.d, k, ent.packed.mode)
        if self.kind == "PQ":
            return be.ivf_pq_fits(ent.d, self.M, k, ent.packed.mode)
        return be.ivf_fits(ent.d, k, ent.packed.mode)

    def search(self, be, ent, queries, k: int, metric: int, nprobe: int, want_probe: bool = False, sel=None):
        kw = {} if sel is None else {"sel": sel}  # a backend without selectors never sees the keyword
        if self.kind == "SQ8":
            return be.ivf_sq8_search(ent.packed, ent.ivf, ent.codes, queries, k, metric, nprobe, want_probe, **kw)
        if self.kind == "PQ":
            return be.ivf_pq_search(ent.packed, ent.ivf, ent.codes, queries, k, metric, nprobe, want_probe, **kw)
        return be.ivf_search(ent.packed, ent.ivf, queries, k, metric, nprobe, want_probe, **kw)

    def train(self, be, packed, lists, train_ids):
        """-> the codec trained on the residuals of the k-means training rows, with every row's codes (IVF-Flat: None)."""
        if self.kind == "SQ8":
            return be.ivf_sq8_encode(packed, lists, *be.ivf_sq8_train(packed, lists, train_ids))
        if self.kind == "PQ":
            return be.ivf_pq_encode(packed, lists, be.ivf_pq_train(packed, lists, train_ids, self.M))
        return None

    def read(self, index_dir: str, nlist: int, metric: int, ent, lists_host):
        """-> the arrays of the codes' sidecar, as ``upload`` takes them (IVF-Flat has none: ()), or None when it is not valid
        for the lists ``lists_host`` (what ``store.read_ivf`` gave)."""
        head = (index_dir, nlist, metric, ent.packed.mode, ent.packed.exp, ent.d)
        if self.kind == "SQ8":
            return store.read_ivf_sq8(*head, ent.n, store.ivf_digest(*lists_host))
        if self.kind == "PQ":
            return store.read_ivf_pq(*head, self.M, ent.n, store.ivf_digest(*lists_host))
        return ()

    def upload(self, be, packed, lists, side):
        """``side`` follows the encode call's arguments: the codec, then ``codes=`` and the per-row term - only uploaded."""
        if self.kind == "SQ8":
            return be.ivf_sq8_encode(packed, lists, *side)
        return be.ivf_pq_encode(packed, lists, *side) if self.kind == "PQ" else None

    def write(self, index_dir: str, nlist: int, metric: int, ent, lists_host) -> None:
        cd, head = ent.codes, (index_dir, nlist, metric, ent.packed.mode)
        if self.kind == "SQ8":
            store.write_ivf_sq8(*head, cd.exp, _host(cd.vmin), _host(cd.vdiff), _host(cd.codes[:, :ent.d]), _host(cd.rnorm),
                                store.ivf_digest(*lists_host))
        if self.kind == "PQ":
            store.write_ivf_pq(*head, cd.exp, _host(cd.codebooks), _host(cd.codes[:, :cd.M]), _host(cd.beta),
                               store.ivf_digest(*lists_host))

    def export(self, ent):
        """The codec and the codes in ROW order, in the caller's units (``HipVS.sq8_codes`` / ``pq_codes``)."""
        cd = ent.codes
        scale = np.float32(2.0) ** -cd.exp  # exact: the stored scale is a power of two
        rows = _host(ent.ivf.rows).view(np.uint32).astype(np.int64)

        def by_row(t):  # list order (position p holds row rows[p]) -> row order
            a = _host(t)
            out = np.empty(a.shape, a.dtype)
            out[rows] = a
            return out

        if self.kind == "SQ8":
            return _host(cd.vmin) * scale, _host(cd.vdiff) * scale, by_row(cd.codes[:, :ent.d]), by_row(cd.rnorm) * (scale * scale)
        return _host(cd.codebooks) * scale, by_row(cd.codes[:, :cd.M]), by_row(cd.beta) * (scale * scale)


@dataclass(frozen=True)
class _CallPlan:
    """What one ``HipVS.__call__`` does, decided by ``_plan_call`` before the queries are packed."""

    K: int
    k_eff: int  # min(K, rows to search): what the kernels are asked for, the rest of K is padding
    sub: Any  # ``ids`` as an int64 vector; None: every row
    route: str  # "pipelined" | "rank_all" | "ivf" | "sharded_abi" | "flat" | "subset": ``HipVS._route_<route>`` searches
    nprobe: int  # lists probed per query (0: no lists)
    kc: int  # candidates per query of the list scan: K, more on a Refine(Flat) store
    refine: bool
    sel: Any  # backend row bitmap of ``sub`` for the list scan (None: no selection)
    qexp: Any  # scale exponent the queries are packed with: the index's, the caller's ``_query_exp``, or "auto"
    return_device: bool
    layout: tuple  # ``_layout()``


@dataclass
class RecallReport:
    """What ``HipVS.recall`` measured: entry i belongs to ``nprobes[i]``."""

    nprobes: tuple  # lists probed per query, as ``__call__`` would probe them (never more than nlist)
    intersection: np.ndarray  # float64 [len(nprobes)]: mean over the queries of hits / true neighbours (faiss's
    #                           IntersectionCriterion, normalised to [0, 1])
    first: np.ndarray  # float64 [len(nprobes)]: share of the queries whose true best row is among the K returned (faiss's
    #                    OneRecallAtRCriterion at R = K)
    served: tuple  # bool per entry: True - the list scan serves this call; False - it is served exactly (recall 1.0, nothing
    #                was launched for the entry)
    nq: int
    K: int
    kc: int  # candidates per query of the list scan: K, more on a Refine(Flat) store (``refine_candidates``)
    hits: np.ndarray  # int32 [len(nprobes), nq]: true neighbours returned, per query


@dataclass
class _RecallRun:
    """One ``recall`` / ``probe_recall_curve`` / ``tune_nprobe`` call: its checked arguments, the queries packed once and, from
    the first use on, the exact keys every measurement is compared with."""

    ent: Any
    q: Any  # the query matrix as ``_plan_call`` takes it
    K: int
    kw: dict  # the per-call keywords a measured ``__call__`` would carry besides ``nprobe``
    queries: Any  # backend PackedRows
    k_eff: int
    truth: Any = None  # int64 key tensor [nq, k_eff]
    denom: Any = None  # host int64 [nq]: non-empty slots of ``truth``


def _mean_ratio(hits: np.ndarray, denom: np.ndarray) -> float:
    """Mean over the queries of hits / denom.  With one denominator for all - every exact list full, the usual case - it is
    sum / sum: ONE rounding, so that equal counts give the same float however they were gathered."""
    denom = np.maximum(np.asarray(denom, np.int64), 1)
    if np.all(denom == denom[0]):
        return float(int(np.sum(hits, dtype=np.int64)) / int(denom.sum()))
    return float(np.mean(np.asarray(hits, np.float64) / denom))


def _curve_of(hist: np.ndarray) -> np.ndarray:
    """Histogram of probe ranks [P + 1] (last bin: not probed) -> float64 [P + 1]: entry p = share of ranks below p."""
    total = int(hist.sum())
    below = np.concatenate([[0], np.cumsum(hist[:-1], dtype=np.int64)])
    return below / float(max(total, 1))


def _host(t) -> np.ndarray:
    return t.cpu().numpy()


def _ids_subset(ids, n: int) -> np.ndarray | None:
    """``ids`` as an int64 vector, checked against the ``n`` rows of the index; None for no ``ids`` and for every row in order,
    which is the same as an unfiltered search (``sem_sim_join.py:132-134``)."""
    if ids is None:
        return None
    sub = np.asarray(ids, dtype=np.int64).reshape(-1)
    if sub.size and (sub.min() < 0 or sub.max() >= n):
        raise IndexError("ids out of range for the loaded index")
    # size, first and last element first: a long ``ids`` builds an arange only when it can match
    if sub.size == n and (n == 0 or (sub[0] == 0 and sub[-1] == n - 1 and np.array_equal(sub, np.arange(n)))):
        return None
    return sub


def _serialised(fn):
    import functools

    @functools.wraps(fn)
    def run(self, *a, **k):
        with self._lock:
            shared = getattr(self._backend, "_call_lock", None)  # stores sharing one backend share its workspace too
            if shared is None:
                return fn(self, *a, **k)
            with shared:
                return fn(self, *a, **k)

    return run


class HipVS(VS):
    """Exact (brute-force) vector store on MI355X.

    Args:
        metric: ``METRIC_INNER_PRODUCT`` (default, as ``FaissVS``) or ``METRIC_L2`` (squared L2, ascending).
        storage: ``"auto"`` - fp16 embeddings are stored as fp16, fp32/fp64 embeddings as an fp16 hi|lo pair
            (fp32-accurate scores); ``"fp16"`` - round everything to fp16 (half the HBM, 3x the speed,
            ~1e-4 score error on fp32 inputs); ``"fp32"`` - always the hi|lo pair.
        device: torch device string; default current CUDA device.
        shard: how a join is split over the ``torch.distributed`` ranks.  ``True`` / ``"rows"`` - row-shard the corpus,
            queries replicated, one all-gather of the per-shard candidate keys + merge (BASELINE's configuration; scales the
            corpus beyond one GPU's HBM).  ``"queries"`` - every rank keeps the WHOLE corpus and searches its slice of the
            queries; the finished lists are all-gathered, nothing is merged.  ``(gq, gc)`` - the 2-D split: ``gq`` query
            groups x ``gc`` corpus shards (``gq * gc`` = ranks; rank r is in query group r // gc and holds corpus shard
            r % gc): every GPU searches Q / gq queries against N / gc rows, the lists are merged inside a corpus group and
            concatenated across the query groups.  ``"auto"`` - ``lotus_amd.plan.pick_split`` ranks the splits by the
            per-GPU shapes' measured rates (at configs[2] on 8 GPUs all four splits run within a point of 37 % of the
            MFMA roof, so the tie goes to the row split: least HBM per GPU).
        normalize: L2-normalise every row and every query on the device while packing (``lvs_pack_rows(normalize=1)``):
            with the inner-product metric this IS cosine similarity whatever the embedder returns.  ``FaissVS`` has no
            such switch - it relies on the RM normalising (``sentence_transformers_rm.py:30,71``) - so the default is off.
        max_resident: how many indexes stay on the GPU.
        backend: injected device backend (tests); default ``HipBackend``.
        factory_string: ``"Flat"`` (default) - exact search; ``"IVF<nlist>,Flat"`` - an inverted-file index as faiss's
            ``index_factory`` builds it: ``index()`` / ``load_index()`` train ``min(nlist, n)`` centroids with this package's
            k-means (squared L2, fixed seed, ``ivf_niter`` iterations, ``ivf_max_points_per_centroid`` subsampling) on the
            device image, put every row into the list of its best centroid under ``metric`` and keep the lists as row numbers
            into the same image.  A plain search (no ``ids``, ``K <= 56``, ``K < n``) then scans the rows of each query's ``nprobe`` best
            lists (``__call__(..., nprobe=...)`` overrides it per call); ``ids`` subsets and larger ``K`` stay exact.  The
            directory is written as for ``"Flat"`` plus an ``ivf.npz`` sidecar that a reload uses instead of retraining.
            Single GPU only: any ``shard`` but ``False`` is refused.  Rows too wide for the list scan's LDS image (hi|lo storage:
            d > 1088, fp16: d > 2240; ``HipBackend.ivf_fits``) and ``nprobe`` > 2 048 are searched exactly.
            ``"IVF<nlist>,SQ8"`` - the same centroids and lists, with every row also kept as 8-bit codes of its residual
            (faiss's ``ScalarQuantizer`` ``QT_8bit`` with ``by_residual``: per-dimension ranges trained on the residuals of
            the k-means training rows, one byte per dimension): a plain search scores each probed row as its decoded value
            ``c_l + rhat`` (``HipBackend.ivf_sq8_search``), up to d = 2368 whatever the storage; the exact fallbacks are
            IVF-Flat's, against the full-precision rows, which stay resident.  The directory is written as for
            ``"IVF<nlist>,Flat"`` (so such a store of the same nlist reuses its ``ivf.npz``) plus ``ivf_sq8.npz`` with the
            codec and the codes; ``sq8_codes()`` returns them.
            ``"IVF<nlist>,PQ<M>"`` (or ``"PQ<M>x8"``) - the same centroids and lists, with every row also kept as M one-byte
            codes of its residual (faiss's ``ProductQuantizer`` with 8-bit codes and ``by_residual``: d / M-dimensional
            subspaces, one k-means codebook of ``min(256, training rows)`` entries per subspace, trained on the residuals of
            the k-means training rows).  A plain search builds each query's lookup table once and scores each probed row as
            its decoded value ``c_l + rhat`` from M table lookups (``HipBackend.ivf_pq_search``); the scan's cost follows M,
            not d, so 3 072-dimensional rows are served.  ``index()`` / ``load_index()`` refuse rows whose d M does not
            divide; M > 159 (the table outgrows LDS) is searched exactly, as are IVF-Flat's exact fallbacks, against the
            full-precision rows, which stay resident.  The directory is written as for ``"IVF<nlist>,Flat"`` plus
            ``ivf_pq.npz`` with the codebooks and the codes; ``pq_codes()`` returns them.  Other code sizes (``PQ<M>x4``,
            ``x4fs``) are refused.
            ``"IVF<nlist>,SQ8,Refine(Flat)"`` / ``"IVF<nlist>,PQ<M>[x8],Refine(Flat)"`` - faiss's ``IndexRefineFlat`` around
            the same store: a plain search runs the codes' scan at ``refine_candidates(K)`` candidates per query and then
            re-scores those rows exactly against the full-precision image, which is resident anyway
            (``HipBackend.refine_keys``); the best ``K`` by the exact score are returned, with exact distances.  Everything
            else - the lists, the codec, the sidecars (a refined and a plain store of the same nlist and M read and write the
            same files), the exact fallbacks, ``ivf_probe`` / ``sq8_codes`` / ``pq_codes`` - is the plain store's.  No other
            refiner is taken (``RFlat``, ``Refine(SQ8)``), and ``"IVF<nlist>,Flat"`` has nothing to refine.
        nprobe: lists probed per query (faiss's default 1).
        k_factor: candidates per returned row of a ``Refine(Flat)`` store (faiss's ``IndexRefine.k_factor``, default 1: the
            codes' own top K, re-ordered by exact score); ``__call__(..., k_factor=...)`` overrides it per call.  A finite
            number >= 1.  The candidate count is ``min(max(K, ceil(K * k_factor)), 56, n)``: unlike faiss it stops at 56, the
            list scans' one-pass bound.  Stores without ``Refine(Flat)`` ignore it.
        ids_probe: ``False`` (default) - every ``ids`` subset is searched exactly, as above.  ``True`` - an IVF store answers
            a strict-subset call through its lists (faiss's ``SearchParametersIVF(sel=IDSelectorBitmap)``): ``ids`` becomes a
            bitmap over the rows (``HipBackend.row_bitmap``) and the store's list scan skips the rows - and whole blocks of
            rows - that are not selected, so the result is the top K over (rows of the probed lists) and (``ids``), re-ranked
            exactly on a ``Refine(Flat)`` store.  ``__call__(..., ids_probe=...)`` overrides it per call; anything but a
            ``bool`` is a ``ValueError``.  The call takes the lists only when the plain search's conditions hold (single GPU,
            ``K <= 56``, ``nprobe <= 2048``, a shape the scan fits) and, in addition: ``ids`` holds no duplicate (``FaissVS``
            returns a duplicated row twice, a bitmap cannot); ``K < len(ids)``; and ``len(ids) * nlist > n * nprobe`` - the
            scan scores about ``n * nprobe / nlist`` rows per query whatever the selection, so below that the gathered exact
            search scores fewer rows and keeps the call.  Every other call stays exact.  Indices are the given ids (global
            row numbers); slots are ``-1`` / ``-+FLT_MAX`` when the probed lists hold fewer than ``K`` selected rows.  Besides
            recall, one thing differs from the exact ``ids`` path: equal scores come out in ascending ROW order here, in the
            order of their position in ``ids`` there - the same thing for ascending ``ids``, which a frame's index gives.
            Flat stores ignore it.  An injected backend without ``row_bitmap`` is refused.
    """

    def __init__(self, metric: int = METRIC_INNER_PRODUCT, storage: str = "auto", device: str | None = None,
                 shard: bool | str = False, max_resident: int = 4, backend=None, process_group=None,
                 normalize: bool = False, abi_exchange: bool = False, factory_string: str = "Flat", nprobe: int = 1,
                 ivf_niter: int = 20, ivf_max_points_per_centroid: int = 256, k_factor: float = 1.0,
                 ids_probe: bool = False) -> None:
        super().__init__()
        m = (re.fullmatch(r"IVF([0-9]+),(Flat|(?:SQ8|PQ([0-9]+)(?:x8)?)(,Refine\(Flat\))?)", factory_string)
             if isinstance(factory_string, str) else None)
        if factory_string != "Flat" and (m is None or int(m.group(1)) < 1 or (m.group(3) is not None and int(m.group(3)) < 1)):
            raise ValueError("factory_string must be 'Flat' or 'IVF<nlist>,Flat' or 'IVF<nlist>,SQ8' or 'IVF<nlist>,PQ<M>[x8]' "
                             "(nlist >= 1, M >= 1, 8-bit codes; SQ8 and PQ<M> may be followed by ',Refine(Flat)', the only "
                             f"refiner), got {factory_string!r}")
        self._nlist = int(m.group(1)) if m is not None else None
        # None for "Flat"; an IVF store's mode makes every call that differs between IVF-Flat, IVF-SQ8 and IVF-PQ
        refine = m is not None and m.group(4) is not None
        self._mode = (None if m is None else _IvfMode("PQ", int(m.group(3)), refine) if m.group(3) is not None
                      else _IvfMode("SQ8" if refine else m.group(2), None, refine))
        # an injected backend without the IVF-PQ codec or the re-ranking (a test double of an earlier mode) cannot build such a store
        needs = self._mode.requires if self._mode is not None and backend is not None else ()
        missing = [a for a in needs if not hasattr(backend, a)]
        if missing and missing[0] == "ivf_pq_search":
            raise ValueError("factory_string must be 'Flat' or 'IVF<nlist>,Flat' or 'IVF<nlist>,SQ8' with a backend that has "
                             f"no IVF-PQ codec ({type(backend).__name__}), got {factory_string!r}")
        if missing:
            raise ValueError("factory_string must be 'Flat' or 'IVF<nlist>,Flat' or 'IVF<nlist>,SQ8' or 'IVF<nlist>,PQ<M>[x8]' "
                             f"with a backend that has no exact re-ranking ({type(backend).__name__} lacks refine_keys), got "
                             f"{factory_string!r}")
        self.ids_probe = self._check_ids_probe(ids_probe)
        if self.ids_probe and backend is not None and not hasattr(backend, "row_bitmap"):
            raise ValueError(f"ids_probe=True needs a backend with row selectors ({type(backend).__name__} lacks row_bitmap)")
        self.factory_string = factory_string
        self.k_factor = self._check_k_factor(k_factor)
        if self._nlist is not None and shard is not False:
            raise ValueError(f"an IVF index is single-GPU: shard must be False with factory_string={factory_string!r}")
        self.nprobe = self._check_nprobe(nprobe)
        self.ivf_niter = int(ivf_niter)
        self.ivf_max_points_per_centroid = ivf_max_points_per_centroid
        # True: a row-sharded search runs its two exchanges from inside the C ABI (lvs_search_sharded, the process group's
        # all-gather handed over as a callback) instead of from this file - same kernels, same order, same result
        self.abi_exchange = bool(abi_exchange)
        if metric not in (METRIC_INNER_PRODUCT, METRIC_L2):
            raise ValueError("metric must be METRIC_INNER_PRODUCT or METRIC_L2")
        if storage not in ("auto", "fp16", "fp32"):
            raise ValueError("storage must be 'auto', 'fp16' or 'fp32'")
        self.metric = metric
        self.normalize = bool(normalize)
        self.storage = storage
        self.index_dir: str | None = None
        self._device = device
        self._backend = backend
        self._resident: "OrderedDict[str, _Resident]" = OrderedDict()
        self._max_resident = max(1, int(max_resident))
        is_pair = (isinstance(shard, (tuple, list)) and len(shard) == 2 and all(isinstance(v, int) and v >= 1 for v in shard))
        if not is_pair and shard not in (False, True, "rows", "queries", "auto"):
            raise ValueError("shard must be False, True, 'rows', 'queries', 'auto' or a (query groups, corpus shards) pair")
        self._split = tuple(shard) if is_pair else shard
        self._shard = shard in (True, "rows")      # corpus rows split across the ranks
        self._shard_queries = shard == "queries"   # corpus replicated, queries split
        self._pg = process_group
        self._lay = None                           # resolved layout, see _layout()
        import threading

        # one call at a time per store: the reference's VS is a process-global with mutable state too, and its only concurrent
        # caller (sem_topk's group-by thread pool, sem_topk.py:770-773 -> sem_index / sem_search) must not interleave the
        # launches of two searches that share one device workspace
        self._lock = threading.RLock()

    # ------------------------------------------------------------------------------------------------ helpers
    @property
    def backend(self):
        if self._backend is None:
            from .backend import HipBackend

            self._backend = HipBackend(self._device)
        return self._backend

    def _layout(self, sizes=None):
        """-> (qg, gq, cs, gc, pg_query, pg_corpus): this rank's query group / corpus shard under the configured split and
        the process groups its two exchange steps run in (None: nothing to exchange in that direction).  Resolved once,
        at first use: a 2-D split creates its sub-groups here (a collective call - every rank reaches it together, like
        every other step of a sharded operator).  ``sizes`` = (rows, d, bytes per stored value) of the index being
        installed: what ``shard="auto"`` plans with (the split is fixed by the FIRST index this store installs; without
        sizes - a search before any index - "auto" falls back to the row split, the only one that fits any corpus)."""
        if self._lay is not None:
            return self._lay
        if self._split is False:
            return (0, 1, 0, 1, None, None)
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            return (0, 1, 0, 1, None, None)
        rank, world = dist.get_rank(self._pg), dist.get_world_size(self._pg)
        split = self._split
        if split == "auto":
            from .plan import pick_split

            if sizes is None:
                split = (1, world)
            else:
                split = pick_split(world, nb=int(sizes[0]), d=int(sizes[1]), bytes_per_value=int(sizes[2]))
        if split in (True, "rows"):
            lay = (0, 1, rank, world, None, self._pg)
        elif split == "queries":
            lay = (rank, world, 0, 1, self._pg, None)
        else:
            gq, gc = int(split[0]), int(split[1])
            if gq * gc != world:
                raise ValueError(f"shard={split}: {gq} query groups x {gc} corpus shards need {gq * gc} ranks, the group has {world}")
            if gq == 1:
                lay = (0, 1, rank, world, None, self._pg)
            elif gc == 1:
                lay = (rank, world, 0, 1, self._pg, None)
            else:
                members = dist.get_process_group_ranks(self._pg) if self._pg is not None else list(range(world))
                qg, cs = rank // gc, rank % gc
                pg_corpus = pg_query = None
                for g in range(gq):  # every rank creates every group, in the same order
                    grp = dist.new_group([members[g * gc + c] for c in range(gc)])
                    if g == qg:
                        pg_corpus = grp
                for c in range(gc):
                    grp = dist.new_group([members[g * gc + c] for g in range(gq)])
                    if c == cs:
                        pg_query = grp
                lay = (qg, gq, cs, gc, pg_query, pg_corpus)
        self._lay = lay
        return lay

    def _dist(self):
        """(rank, world) of the corpus sharding - which contiguous block of rows this rank holds; (0, 1) when every rank
        holds all rows."""
        lay = self._layout()
        return lay[2], lay[3]

    def _pg_corpus(self):
        return self._layout()[5]

    def _group(self):
        """(rank, world) of the process group this store works in under EITHER split (rows or queries) - what decides who
        writes an index directory and which collectives every rank must enter; (0, 1) when not distributed."""
        if self._split is False:
            return 0, 1
        from . import _dist

        _, rank, world = _dist.context(True, self._pg)
        return rank, world

    def _pack_mode(self, dtype) -> int:
        if self.storage == "fp16":
            return _capi.PACK_F16
        if self.storage == "fp32":
            return _capi.PACK_SPLIT
        return _capi.PACK_F16 if np.dtype(dtype) == np.float16 else _capi.PACK_SPLIT

    @staticmethod
    def _is_device_tensor(x) -> bool:
        return hasattr(x, "is_cuda") and hasattr(x, "data_ptr") and bool(x.is_cuda)

    @staticmethod
    def _as_matrix(x, what: str):
        if HipVS._is_device_tensor(x):  # embeddings that never left the GPU
            if x.dim() == 1:
                x = x[None, :]
            if x.dim() != 2:
                raise ValueError(f"{what} must be a 2-D tensor, got shape {tuple(x.shape)}")
            return x
        x = np.asarray(x)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2:
            raise ValueError(f"{what} must be a 2-D array, got shape {x.shape}")
        if x.dtype not in (np.float16, np.float32, np.float64):
            x = x.astype(np.float32)
        return x

    def _query_matrix(self, query_vectors, ent: _Resident):
        q = self._as_matrix(query_vectors, "query_vectors")
        if q.shape[1] != ent.d:
            raise ValueError(f"query dimension {q.shape[1]} does not match index dimension {ent.d}")
        return q

    def _install(self, index_dir: str, vecs, stored=None, sig=None) -> _Resident:
        """Build the device image of this rank's shard from ``vecs`` ([n,d] ndarray / memmap / CUDA tensor; only rows
        [lo, hi) are touched).  ``stored``: what ``get_vectors_from_index`` serves (None = open on demand)."""
        n, d = int(vecs.shape[0]), int(vecs.shape[1])
        is_dev = self._is_device_tensor(vecs)
        dtype = np.float16 if (is_dev and str(vecs.dtype) == "torch.float16") else (np.float32 if is_dev else vecs.dtype)
        mode = self._pack_mode(dtype)
        self._layout(sizes=(n, d, 2 if mode == _capi.PACK_F16 else 4))  # "auto" plans with THIS index's real size
        rank, world = self._dist()
        per = -(-n // world) if n else 0
        lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
        if world > 1 and mode == _capi.PACK_SPLIT and not self.normalize:
            packed = self._pack_shard_agreed(vecs, lo, hi, mode, is_dev)
        else:  # fp32-accurate rows are stored as x * 2^e with e chosen from the data (backend.pack); fp16 rows as given
            packed = self.backend.pack(vecs[lo:hi], mode, normalize=self.normalize, exp="auto", check=True)
        ent = _Resident(vecs=stored, packed=packed, n=n, d=d, lo=lo, hi=hi, sig=sig)
        self._resident[index_dir] = ent
        self._resident.move_to_end(index_dir)
        while len(self._resident) > self._max_resident:
            self._resident.popitem(last=False)
        return ent

    _EXP_HEAD_ROWS = 65536  # rows per shard the agreed exponent is sampled from

    def _pack_shard_agreed(self, vecs, lo: int, hi: int, mode: int, is_dev: bool):
        """Pack rows [lo, hi) of a row-sharded fp32-accurate index with ONE power-of-two scale for every shard (per-shard
        lists are merged by score).  The exponent is agreed from each rank's first rows (one tiny all-gather) and has 500x
        headroom; should some later row of some shard still leave fp16's range under it, every rank packs with the
        exponent of its own true maximum and the smallest of them is adopted.  Every rank of the corpus group enters every
        exchange, also one whose shard is empty - the decisions are taken from gathered values only."""
        import torch
        from . import _dist

        be, pg = self.backend, self._pg_corpus()

        def gathered(values):
            t = torch.tensor([float(v) for v in values], dtype=torch.float64)
            return _dist.all_gather_rows(t, pg).numpy()

        head = vecs[lo:min(hi, lo + self._EXP_HEAD_ROWS)]
        head = head.float().cpu().numpy() if is_dev else np.asarray(head, dtype=np.float32)
        amax = float(max(head.max(initial=0.0), -head.min(initial=0.0)))
        exp = be.exp_for(float(gathered([amax if np.isfinite(amax) else 0.0]).max()))
        packed = be.pack(vecs[lo:hi], mode, exp=exp, check="lazy")
        flags = gathered([int(packed.flags.item())]).astype(np.int64).reshape(-1)
        f = int(np.bitwise_or.reduce(flags))
        if f & _capi.PACK_FLAG_RANGE and not f & _capi.PACK_FLAG_NONFINITE:
            packed = be.pack(vecs[lo:hi], mode, exp="auto", check="lazy")
            mine = gathered([packed.exp, hi - lo, int(packed.flags.item())]).reshape(-1, 3)
            f = int(np.bitwise_or.reduce(mine[:, 2].astype(np.int64)))
            held = mine[mine[:, 1] > 0]
            exp = int(held[:, 0].min()) if len(held) else 0
            if not f and len(held) and (held[:, 0] != exp).any():  # decided from gathered values: same on every rank
                if packed.exp != exp:
                    packed = be.pack(vecs[lo:hi], mode, exp=exp, check="lazy")
                f = int(np.bitwise_or.reduce(gathered([int(packed.flags.item())]).astype(np.int64).reshape(-1)))
        be.raise_for_flags(f)
        packed.flags = None
        if hi == lo:
            packed.exp = int(exp)  # a rank without rows packs its queries with, and decodes merged keys by, the agreed exponent
        return packed

    def _current(self) -> _Resident:
        if self.index_dir is None or self.index_dir not in self._resident:
            raise ValueError("Index not loaded")  # faiss_vs.py:54-55
        return self._resident[self.index_dir]

    # ---------------------------------------------------------------------------------------- plugin methods
    @_serialised
    def index(self, docs, embeddings, index_dir: str, **kwargs: dict[str, Any]) -> None:
        """Build the index from ``embeddings`` and persist it (``faiss_vs.py:22-30``).  ``docs`` is unused, as in
        ``FaissVS``.  ``embeddings`` may also be a CUDA tensor straight from an encoder (no host round trip for the
        device image).  Rank 0 writes the reference's two files plus the mappable row store (``lotus_amd/store.py``);
        ``persist=False`` skips the disk entirely, ``raw=False`` writes the reference's files only."""
        emb = self._as_matrix(embeddings, "embeddings")
        self._check_width(int(emb.shape[1]))
        rank, world = self._group()  # under the query split every rank holds the whole corpus, but only ONE may write it
        persist = bool(kwargs.get("persist", True))
        is_dev = self._is_device_tensor(emb)
        if persist:
            if rank == 0:
                host = emb.cpu().numpy() if is_dev else emb
                store.write_dir(index_dir, embeddings, host, self.metric, raw=bool(kwargs.get("raw", True)))
            if world > 1:  # the other ranks may open the directory right after this call
                from . import _dist

                _dist.barrier(self._pg)
        # the signature is taken after the barrier: every rank records the finished directory
        ent = self._install(index_dir, emb, stored=None if is_dev else emb,
                            sig=store.signature(index_dir) if persist else None)
        if self._nlist is not None:
            ent.ivf, ent.codes = self._ivf_train(ent)
            if persist:
                self._ivf_write(index_dir, ent, best_effort=False)
        self.index_dir = index_dir

    @_serialised
    def load_index(self, index_dir: str) -> None:
        """Make ``index_dir`` the current index (``faiss_vs.py:32-36``).  Served from HBM when the directory is already
        resident AND unchanged on disk since it was loaded; otherwise this rank's rows are read through a memory map
        (nothing is unpickled, ``lotus_amd/store.py``) and packed."""
        ent = self._resident.get(index_dir)
        if ent is not None and (ent.sig is None or ent.sig == store.signature(index_dir)):
            self._resident.move_to_end(index_dir)
            self.index_dir = index_dir
            return
        sig = store.signature(index_dir)
        rows, _ = store.open_device_rows(index_dir)
        rows = self._as_matrix(rows, "stored vectors")
        self._check_width(int(rows.shape[1]))
        ent = self._install(index_dir, rows, stored=None, sig=sig)
        if self._nlist is not None and ent.n:
            side = store.read_ivf(index_dir, self._nlist, self.metric, ent.packed.mode, ent.d, ent.n)
            side_codes = self._mode.read(index_dir, self._nlist, self.metric, ent, side) if side is not None else None
            if side_codes is not None:
                c, off, rr = side
                ent.ivf = self.backend.ivf_build(ent.packed, c, self.metric, offsets=off, rows=rr)
                ent.codes = self._mode.upload(self.backend, ent.packed, ent.ivf, side_codes)
            else:  # missing, stale or built for another nlist / metric: train again and try to leave valid sidecars behind
                ent.ivf, ent.codes = self._ivf_train(ent)
                self._ivf_write(index_dir, ent, best_effort=True)
        self.index_dir = index_dir

    @_serialised
    def get_vectors_from_index(self, index_dir: str, ids) -> np.ndarray:
        """``vecs[ids]`` in the stored dtype (``faiss_vs.py:38-41``); ``ids`` may be a list or a pandas Index.  Rows
        come from the caller's array (same process), from the row store's memory map (only the touched pages are read)
        or - for an index that was never persisted - from the device image."""
        ent = self._resident.get(index_dir)
        sel = ids if isinstance(ids, slice) else np.asarray(ids, dtype=np.int64)
        if ent is not None and ent.vecs is None and ent.sig is None:  # persist=False / device tensors: HBM is the store
            if ent.lo != 0 or ent.hi != ent.n:
                raise NotImplementedError("vectors of a sharded index that was never persisted")  # sem_sim_join.py:114-117
            be = self.backend
            if isinstance(sel, slice):
                sel = np.arange(ent.n, dtype=np.int64)[sel]
            out = be.unpack(ent.packed, be.to_device(sel)).cpu().numpy()
            return out.astype(np.float16) if ent.packed.mode == _capi.PACK_F16 else out
        if ent is not None and ent.vecs is not None and (ent.sig is None or ent.sig == store.signature(index_dir)):
            vecs = ent.vecs  # the caller's array / an open map - unless the directory was rewritten since (load_index's rule)
        else:
            vecs, _ = store.open_stored_rows(index_dir)
            if ent is not None and ent.sig == store.signature(index_dir):
                ent.vecs = vecs
        return np.asarray(vecs[sel])

    @_serialised
    def __call__(self, query_vectors, K: int, ids: list[int] | None = None, **kwargs: dict[str, Any]) -> RMOutput:
        """Top-``K`` rows for every query vector (``faiss_vs.py:43-77``)."""
        ent = self._current()
        q = self._query_matrix(query_vectors, ent)
        K = int(K)
        if K < 0:
            raise ValueError("K must be >= 0")
        nq = int(q.shape[0])
        if K == 0 or nq == 0:
            return self._padded(nq, K)
        plan = self._plan_call(ent, q, K, ids, kwargs)
        if plan is None:  # no ids: nothing to search
            return self._padded(nq, K)
        again = (query_vectors, K, ids, kwargs)  # what _check_queries searches again with when the packed queries' flags say so
        if plan.route == "pipelined":
            return self._route_pipelined(plan, ent, q, again)
        queries, score_exp, flags = self._pack_queries(plan, ent, q)
        keys, id_map, score_exp, world_left = getattr(self, "_route_" + plan.route)(plan, ent, queries, score_exp)
        return self._finish(plan, keys, id_map, score_exp, world_left, flags, nq, again)

    def _padded(self, nq: int, K: int) -> RMOutput:
        """The result without a row in it: faiss pads with -1 / -+FLT_MAX (Appendix A.2)."""
        pad_d = -FLT_MAX if self.metric == METRIC_INNER_PRODUCT else FLT_MAX
        return RMOutput(distances=np.full((nq, K), pad_d, np.float32), indices=np.full((nq, K), -1, np.int64))

    def _plan_call(self, ent: _Resident, q, K: int, ids, kwargs) -> _CallPlan | None:
        """Which route this call takes and with what, from its arguments alone - nothing is packed or searched yet; None when
        ``ids`` is empty.  Every condition is one that all ranks of a sharded store evaluate alike."""
        be = self.backend
        sub = _ids_subset(ids, ent.n)
        k_eff = min(K, ent.n if sub is None else int(sub.size))
        if k_eff == 0:
            return None
        rank_all = k_eff > _capi.MAX_K  # K = N callers (sem_dedup.py:45, sem_filter.py:491-497): full score rows + sort
        layout = self._layout()
        _, qworld, _, world = layout[:4]
        # IVF stores probe lists for the plain query only; ids subsets, K = N callers, K beyond the one-pass list scan, rows too
        # wide for its LDS image and more than 2 048 probes take the exact path below - which also ends the reference
        # sem_search's K-doubling loop (sem_search.py:120-138) once the probed lists hold fewer than K rows
        nprobe = min(self._check_nprobe(kwargs.get("nprobe", self.nprobe)), ent.ivf.nlist) if ent.ivf is not None else 0
        # a Refine(Flat) store runs its codes' scan at kc >= K candidates per query and re-ranks them exactly; a scan that
        # does not take kc leaves the call exact, like any shape the scan does not fit
        k_factor = self._check_k_factor(kwargs.get("k_factor", self.k_factor))
        refine = self._mode is not None and self._mode.refine
        kc = self._refine_kc(K, k_factor, ent.n) if refine else K
        ids_probe = self._check_ids_probe(kwargs.get("ids_probe", self.ids_probe))
        use_ivf = (ent.ivf is not None and (sub is None or ids_probe) and K <= _capi.IVF_MAX_K and K < ent.n and world == 1
                   and qworld == 1 and nprobe <= _capi.MAX_K and self._mode.fits(be, ent, kc))
        # a strict subset goes through the lists only on request (ids_probe), without duplicates (a bitmap holds a row
        # once), with more ids than K, and when the scan scores fewer rows than the gathered exact search would: about
        # n nprobe / nlist per query against len(ids)
        sel = None
        if use_ivf and sub is not None:
            use_ivf = hasattr(be, "row_bitmap") and K < sub.size and sub.size * ent.ivf.nlist > ent.n * nprobe
            if use_ivf:
                sel, distinct = be.row_bitmap(sub, ent.n)
                use_ivf = distinct == sub.size
                sel = sel if use_ivf else None
        # queries share the index's power-of-two scale (required for L2; for inner products it keeps one exponent per
        # index); they are validated while they are packed, the flag word comes back together with the results
        qexp = kwargs.get("_query_exp", ent.packed.exp)
        return_device = bool(kwargs.get("return_device", False))
        if rank_all:
            route = "rank_all"
        elif use_ivf:
            route = "ivf"
        elif sub is not None:
            route = "subset"
        elif (world == 1 and qworld == 1 and not return_device and k_eff == K and not self._is_device_tensor(q)
              and qexp != "auto" and hasattr(be, "search_host_pipelined") and int(q.shape[0]) >= be.CALL_PIPELINE_MIN_QUERIES
              and not self._fp32_path(ent, q)):
            route = "pipelined"  # the plain big call (sem_sim_join.py:132-134 -> faiss_vs.py:75)
        elif world > 1 and self.abi_exchange and hasattr(be, "search_sharded") and k_eff <= 56:
            route = "sharded_abi"
        else:
            route = "flat"
        return _CallPlan(K=K, k_eff=k_eff, sub=sub, route=route, nprobe=nprobe, kc=kc, refine=refine, sel=sel, qexp=qexp,
                         return_device=return_device, layout=layout)

    def _route_pipelined(self, plan: _CallPlan, ent: _Resident, q, again) -> RMOutput:
        """Host queries in, host results out, transfers overlapped with the search: packs, searches and decodes in one
        backend call, so it returns the finished result."""
        Dh, Ih, f = self.backend.search_host_pipelined(ent.packed, q, plan.k_eff, self.metric, id_offset=ent.lo,
                                                       normalize=self.normalize, exp=int(plan.qexp))
        redo = self._check_queries(f, *again)
        return redo if redo is not None else RMOutput(distances=Dh, indices=Ih)

    def _pack_queries(self, plan: _CallPlan, ent: _Resident, q):
        """-> (packed queries, score exponent of their products with the index, validation flags or None): this rank's
        slice of the queries under a query split, packed with the index's exponent or the one the call names."""
        be, qexp = self.backend, plan.qexp
        qrank, qworld, _, _, pg_query, _ = plan.layout
        nq = int(q.shape[0])
        if qworld > 1:  # this rank's contiguous slice of the queries (possibly empty)
            per = -(-nq // qworld)
            q = q[min(nq, qrank * per):min(nq, (qrank + 1) * per)]
            nq = int(q.shape[0])
        if qexp == "auto" and qworld > 1:
            # the finished lists of all query groups are decoded with ONE score exponent: agree it from the largest magnitude
            import torch
            from . import _dist

            amax = be.absmax(q) if (nq and self._is_device_tensor(q)) else float(np.abs(q).max(initial=0.0)) if nq else 0.0
            t = torch.tensor([amax if np.isfinite(amax) else 0.0], dtype=torch.float64)
            qexp = be.exp_for(float(_dist.all_gather_rows(t, pg_query).max())) if ent.packed.mode == _capi.PACK_SPLIT else 0
        queries = be.pack(q, ent.packed.mode, normalize=self.normalize, exp=qexp, check="lazy")
        score_exp = be.score_exp_of(ent.packed, queries)
        flags = getattr(queries, "flags", None)
        if qworld > 1 and flags is not None:
            # every query group validates its own slice; the verdict (raise / search again with another exponent - both
            # collective decisions) must be the same everywhere: OR of the flag words, one tiny all-gather
            from . import _dist

            g = _dist.all_gather_rows(flags, pg_query)
            flags = ((g & 1).amax(0) | (g & 2).amax(0)).to(flags.dtype)
        return queries, score_exp, flags

    # every search route: (plan, ent, packed queries, score exponent) -> (keys [nq, k_eff], id_map or None, score exponent of
    # the keys, corpus shards whose lists are still to be merged)
    def _route_rank_all(self, plan: _CallPlan, ent: _Resident, queries, score_exp):
        """K = N: score rows of this rank's shard, exchanged so that every rank ranks the complete rows (column-sharded score
        matrix, one all-gather); the device sort goes through the queries in chunks of < 2^32 scores, and this loop in blocks
        of at most 2^28 scores (1 GB of float32), so that a K = N call never holds the whole Q x N matrix next to its Q x N
        keys (sem_dedup's reference path asks for N x N)."""
        be, sub, nq = self.backend, plan.sub, queries.n
        n_cols = ent.n if sub is None else int(sub.size)
        qstep = max(1, min(nq, _RANK_BLOCK_SCORES // max(1, n_cols)))
        parts, order = [], None
        for q0 in range(0, nq, qstep):
            sc, order = self._score_rows(ent, be.slice_rows(queries, q0, min(nq, q0 + qstep)), sub, plan.layout[3])
            parts.append(be.rank_scores(sc)[:, :plan.k_eff].contiguous())
            del sc
        if len(parts) == 1:
            keys = parts[0]
        else:
            import torch

            keys = torch.cat(parts)
        # score rows come back in the caller's units already, and complete on every rank: nothing left to merge
        return keys, (be.to_device(order) if order is not None else None), 0, 1

    def _route_ivf(self, plan: _CallPlan, ent: _Resident, queries, score_exp):
        """The scan of each query's ``nprobe`` best lists (over the rows ``sel`` selects), re-ranked on a Refine(Flat) store."""
        be = self.backend
        keys = self._mode.search(be, ent, queries, plan.kc, self.metric, plan.nprobe, sel=plan.sel)
        if plan.refine:  # the kc best by code score -> the k_eff best of them by exact score, exact scores in the keys
            keys = be.refine_keys(ent.packed, queries, keys, plan.k_eff, self.metric)
        return keys, None, score_exp, 1

    def _route_sharded_abi(self, plan: _CallPlan, ent: _Resident, queries, score_exp):
        """The same row-sharded search with its two exchanges issued from INSIDE the C ABI (lvs_search_sharded): the transport
        is this process group's all-gather, handed over as a callback."""
        from . import _dist

        be, k, world = self.backend, plan.k_eff, plan.layout[3]
        per = -(-ent.n // world) if ent.n else 0
        tiles = be.seed_tiles(queries.n, per, k, ent.packed.mode, queries.mode) if hasattr(be, "seed_tiles") else 0
        keys = be.search_sharded(ent.packed, queries, k, self.metric, ent.lo, world, max(0, tiles),
                                 lambda t: _dist.all_gather_rows(t, self._pg_corpus()))
        return keys, None, score_exp, 1  # merged already

    def _route_flat(self, plan: _CallPlan, ent: _Resident, queries, score_exp):
        """The plain exact search of this rank's shard; the shards of a row-sharded store pool their seed scores first."""
        world = plan.layout[3]
        keys = self.backend.search_keys(ent.packed, queries, plan.k_eff, self.metric, id_offset=ent.lo,
                                        seed_scores=self._pooled_seed_scores(ent, queries, plan.k_eff, world))
        return keys, None, score_exp, world

    def _route_subset(self, plan: _CallPlan, ent: _Resident, queries, score_exp):
        """The rows ``ids`` gathered on the GPU and searched exactly; keys carry positions in ``ids``."""
        be, sub = self.backend, plan.sub
        # positions (in `ids`) of the subset rows that live in this rank's shard
        pos = np.flatnonzero((sub >= ent.lo) & (sub < ent.hi))
        local = be.to_device(sub[pos] - ent.lo)
        gathered = be.gather(ent.packed, local)
        row_ids = be.to_device(pos.astype(np.uint32).view(np.int32))
        keys = be.search_keys(gathered, queries, plan.k_eff, self.metric, id_offset=0, row_ids=row_ids)
        return keys, be.to_device(sub), score_exp, plan.layout[3]

    def _finish(self, plan: _CallPlan, keys, id_map, score_exp: int, world_left: int, flags, nq: int, again) -> RMOutput:
        """Keys of this rank's queries against its shard -> the call's result: merged across the corpus shards, gathered across
        the query groups, decoded, the queries' flags acted on, copied to the host and padded to ``K``."""
        be, K, k_eff = self.backend, plan.K, plan.k_eff
        _, qworld, _, _, pg_query, _ = plan.layout
        if world_left > 1:
            keys = self._allgather_merge(keys, world_left)
        if qworld > 1:  # finished lists of every query group's slice, side by side: one all-gather, no merge
            import torch
            from . import _dist

            per = -(-nq // qworld)
            pad = torch.zeros((per, k_eff), dtype=keys.dtype, device=keys.device)
            pad[:keys.shape[0]] = keys
            keys = _dist.all_gather_rows(pad, pg_query).reshape(qworld * per, k_eff)[:nq].contiguous()
        D, I = be.keys_to_result(keys, self.metric, id_map, score_exp=score_exp)
        if plan.return_device and k_eff == K:  # results stay in HBM (torch tensors) for a GPU-side consumer
            f = int(flags.item()) if flags is not None else 0
        else:
            if hasattr(be, "to_host"):  # all copies in flight together, one synchronisation, pinned-backed result arrays
                D, I, *fh = be.to_host(D, I, *([flags] if flags is not None else []))
            else:
                D, I, *fh = [t.cpu().numpy() for t in ((D, I) + ((flags,) if flags is not None else ()))]
            f = int(fh[0][0]) if fh else 0
        redo = self._check_queries(f, *again)
        if redo is not None:
            return redo
        if k_eff == K:
            return RMOutput(distances=D, indices=I)
        out = self._padded(nq, K)  # fewer than K rows exist
        out.distances[:, :k_eff] = D
        out.indices[:, :k_eff] = I
        return out

    # ------------------------------------------------------------------------------------------------ IVF
    @staticmethod
    def _check_nprobe(nprobe) -> int:
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or int(nprobe) < 1:
            raise ValueError(f"nprobe must be an int >= 1, got {nprobe!r}")
        return int(nprobe)

    @staticmethod
    def _check_ids_probe(ids_probe) -> bool:
        if not isinstance(ids_probe, (bool, np.bool_)):
            raise ValueError(f"ids_probe must be a bool, got {ids_probe!r}")
        return bool(ids_probe)

    @staticmethod
    def _check_k_factor(k_factor) -> float:
        ok = (not isinstance(k_factor, bool) and isinstance(k_factor, (int, float, np.integer, np.floating))
              and np.isfinite(k_factor) and k_factor >= 1)
        if not ok:
            raise ValueError(f"k_factor must be a finite number >= 1, got {k_factor!r}")
        return float(k_factor)

    @staticmethod
    def _refine_kc(K: int, k_factor: float, n: int) -> int:
        """Candidates per query of a re-ranked search: faiss's ``ceil(K * k_factor)``, at least K, at most the list scans'
        one-pass bound (56 - where faiss has no bound) and the number of rows."""
        return int(min(max(K, int(np.ceil(K * k_factor))), _capi.IVF_MAX_K, n))

    def refine_candidates(self, K: int, k_factor: float | None = None) -> int:
        """How many candidates per query the codes' scan of a ``Refine(Flat)`` store hands to the exact re-ranking for a plain
        search of ``K`` rows: ``min(max(K, ceil(K * k_factor)), 56, n)`` with the loaded index's ``n`` rows (``k_factor``
        None: the store's).  The clamp at 56 is a deviation from faiss, whose ``IndexRefine`` takes any ``K * k_factor``."""
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or int(K) < 1:
            raise ValueError(f"K must be an int >= 1, got {K!r}")
        f = self.k_factor if k_factor is None else self._check_k_factor(k_factor)
        return self._refine_kc(int(K), f, self._current().n)

    def _ivf_train(self, ent: _Resident):
        """Centroids (device k-means on the packed image, squared L2, fixed seed) and lists of an IVF store, and for an SQ8 or
        PQ store the codec trained on the residuals of the k-means training rows and the codes -> (lists, codes or None);
        (None, None) without rows."""
        if ent.n == 0:
            return None, None
        from . import cluster

        be = self.backend
        nlist = max(1, min(self._nlist, ent.n))
        res = cluster.kmeans(None, nlist, niter=self.ivf_niter, seed=_IVF_SEED,
                             max_points_per_centroid=self.ivf_max_points_per_centroid, backend=be, packed=ent.packed,
                             final_assign=False)
        # rows go to their best centroid under the index's metric, against the final centroids (faiss's IVF quantizer)
        lists = be.ivf_build(ent.packed, np.asarray(res.centroids, dtype=np.float32), self.metric)
        return lists, self._mode.train(be, ent.packed, lists, res.train_ids)

    def _ivf_write(self, index_dir: str, ent: _Resident, best_effort: bool) -> None:
        if ent.ivf is None:
            return
        lists_host = self._ivf_host(ent.ivf)
        try:
            store.write_ivf(index_dir, self._nlist, self.metric, ent.packed.mode, *lists_host)
            self._mode.write(index_dir, self._nlist, self.metric, ent, lists_host)
        except OSError:
            if not best_effort:
                raise

    def _ivf_host(self, lists):
        c = self.backend.unpack(lists.centroids).cpu().numpy().astype(np.float32)
        off = lists.offsets.cpu().numpy().astype(np.int64)
        rows = lists.rows.cpu().numpy().view(np.uint32).copy()
        return c, off, rows

    def _ivf_current(self) -> _Resident:
        ent = self._current()
        if ent.ivf is None:
            raise ValueError("the loaded index has no IVF lists (factory_string='Flat', or no rows)")
        return ent

    @_serialised
    def ivf_lists(self):
        """-> (centroids float32 [nlist, d] as the device holds them, offsets int64 [nlist + 1], rows uint32 [n]): list l holds
        rows[offsets[l]:offsets[l + 1]], ascending."""
        return self._ivf_host(self._ivf_current().ivf)

    @_serialised
    def ivf_probe(self, query_vectors, nprobe: int | None = None) -> np.ndarray:
        """-> int32 [nq, nprobe] ids of the lists a search probes for every query, best first (the device's coarse step).  For
        rows too wide for the list scan (searched exactly, see ``__call__``) the same coarse ranking of the centroids."""
        ent = self._ivf_current()
        q = self._query_matrix(query_vectors, ent)
        nprobe = min(self._check_nprobe(self.nprobe if nprobe is None else nprobe), ent.ivf.nlist)
        if nprobe > _capi.MAX_K:
            raise ValueError(f"ivf_probe ranks at most {_capi.MAX_K} lists per query")
        be = self.backend
        queries = be.pack(q, ent.packed.mode, normalize=self.normalize, exp=ent.packed.exp, check=True)
        if queries.n == 0:
            return np.zeros((0, nprobe), np.int32)
        if self._mode.fits(be, ent, 1):
            _, probe = self._mode.search(be, ent, queries, 1, self.metric, nprobe, want_probe=True)
            return probe.cpu().numpy()
        return self._coarse_probe(ent, queries, nprobe).cpu().numpy()

    def _coarse_probe(self, ent: _Resident, queries, nprobe: int):
        """-> int32 device tensor [nq, nprobe], list ids best first, -1 past them: the coarse step on its own -
        lvs_flat_search_keys over the centroids, as inside lvs_ivf_search_keys - without a scan behind it."""
        import torch

        keys = self.backend.search_keys(ent.ivf.centroids, queries, nprobe, self.metric, one_pass=False)
        return torch.where(keys == 0, -1, 0xFFFFFFFF - (keys & 0xFFFFFFFF)).to(torch.int32)

    # ------------------------------------------------------------------------------------------------ recall
    def _recall_begin(self, query_vectors, K, k_factor, what: str) -> "_RecallRun":
        """What ``recall``, ``probe_recall_curve`` and ``tune_nprobe`` check alike; the queries are packed once, here."""
        ent = self._ivf_current()
        lay = self._layout()
        if lay[1] > 1 or lay[3] > 1:
            raise ValueError(f"{what} needs an unsharded store: this one is split over {lay[1]} x {lay[3]} ranks")
        q = self._query_matrix(query_vectors, ent)
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or int(K) < 1:
            raise ValueError(f"K must be an int >= 1, got {K!r}")
        if int(q.shape[0]) == 0:
            raise ValueError("query_vectors holds no query: recall over nothing is undefined")
        be = self.backend
        missing = [a for a in ("keys_overlap", "ivf_row_lists", "ivf_probe_ranks") if not hasattr(be, a)]
        if missing:
            raise ValueError(f"{what} needs a backend that compares keys ({type(be).__name__} lacks {missing[0]})")
        kw = {} if k_factor is None else {"k_factor": self._check_k_factor(k_factor)}
        queries = be.pack(q, ent.packed.mode, normalize=self.normalize, exp=ent.packed.exp, check=True)
        return _RecallRun(ent=ent, q=q, K=int(K), kw=kw, queries=queries, k_eff=min(int(K), ent.n))

    def _recall_truth(self, run: "_RecallRun"):
        """The exact keys of the run's queries over the full image at ``k_eff``, searched once, and how many slots of each
        query's list hold a row (host int64 [nq]; all of them unless the image holds non-finite scores)."""
        if run.truth is None:
            run.truth = self.backend.search_keys(run.ent.packed, run.queries, run.k_eff, self.metric, id_offset=run.ent.lo)
            run.denom = _host((run.truth != 0).sum(dim=1)).astype(np.int64)
        return run.truth

    def _recall_plan(self, run: "_RecallRun", nprobe) -> _CallPlan:
        """The plan ``__call__(query_vectors, K, nprobe=nprobe[, k_factor=...])`` would follow."""
        return self._plan_call(run.ent, run.q, run.K, None, dict(run.kw, nprobe=nprobe))

    def _recall_measure(self, run: "_RecallRun", nprobes) -> "RecallReport":
        """One ``RecallReport`` entry per value of ``nprobes``: the route is decided as ``__call__`` decides it; a list-scan
        call is searched through ``_route_ivf`` and compared with the exact keys on the device, any other call is exact."""
        be = self.backend
        plans = [self._recall_plan(run, p) for p in nprobes]
        served = [pl.route == "ivf" for pl in plans]
        nq = run.queries.n
        hits = np.full((len(plans), nq), run.k_eff, np.int32)
        first = np.ones((len(plans), nq), np.int32)
        inter = np.ones(len(plans), np.float64)
        if any(served):
            truth = self._recall_truth(run)  # ahead of the first scan
            score_exp = be.score_exp_of(run.ent.packed, run.queries)
            counts = {i: be.keys_overlap(truth, self._route_ivf(pl, run.ent, run.queries, score_exp)[0])
                      for i, pl in enumerate(plans) if served[i]}
            for i, (h, f) in counts.items():  # every launch is queued; only the counts come back
                hits[i], first[i] = _host(h), _host(f)
                inter[i] = _mean_ratio(hits[i], run.denom)
        return RecallReport(nprobes=tuple(pl.nprobe for pl in plans), intersection=inter,
                            first=first.mean(axis=1, dtype=np.float64), served=tuple(served), nq=nq, K=run.K, kc=plans[0].kc,
                            hits=hits)

    def _recall_ceiling(self, run: "_RecallRun", P: int):
        """-> (rank int32 device tensor [nq, k_eff], histogram of the ranks as host int64 [P + 1]): where the list of every
        true neighbour stands among the query's ``P`` best lists.  One exact search, one coarse step, ``lvs_ivf_probe_ranks``."""
        be, ent = self.backend, run.ent
        probe = self._coarse_probe(ent, run.queries, P)
        rank, hist = be.ivf_probe_ranks(self._recall_truth(run), be.ivf_row_lists(ent.ivf), probe)
        return rank, _host(hist).astype(np.int64)

    @_serialised
    def recall(self, query_vectors, K: int, nprobe=None, k_factor: float | None = None) -> "RecallReport":
        """What a plain ``__call__(query_vectors, K)`` of this IVF store finds of the exact answer, measured on the device.

        ``nprobe``: an int or a sequence of ints (None: the store's); every value gives one entry of the report, values
        above ``nlist`` count as ``nlist`` (as in ``__call__``, and so reported).  ``k_factor``: as ``__call__`` takes it
        (None: the store's).  For every value the route is decided exactly as ``__call__`` decides it.  A call the list scan
        serves is searched as ``__call__`` searches it - with the re-ranking and candidate count of a ``Refine(Flat)`` store -
        and its keys are compared, by row number, with the exact top ``min(K, n)`` of the full image, which is searched once;
        only the per-query counts come back to the host.  A call that would be served exactly anyway (K > 56, rows too wide
        for the scan, more than 2 048 probes) is reported as recall 1.0 with ``served=False``, and nothing is launched for it.

        Needs an unsharded store with lists.  ``query_vectors`` as ``__call__`` takes them (device tensors included)."""
        run = self._recall_begin(query_vectors, K, k_factor, "recall")
        if nprobe is None:
            nprobes = [self.nprobe]
        elif isinstance(nprobe, (int, np.integer)) and not isinstance(nprobe, bool):
            nprobes = [nprobe]
        else:
            try:
                nprobes = list(nprobe)
            except TypeError:
                raise ValueError(f"nprobe must be an int >= 1 or a sequence of them, got {nprobe!r}") from None
            if not nprobes:
                raise ValueError("nprobe must name at least one value")
        return self._recall_measure(run, [self._check_nprobe(p) for p in nprobes])

    def _curve_width(self, ent: _Resident, max_nprobe) -> int:
        nlist = ent.ivf.nlist
        return min(nlist if max_nprobe is None else self._check_nprobe(max_nprobe), nlist, _capi.MAX_K)

    @_serialised
    def probe_recall_curve(self, query_vectors, K: int, max_nprobe: int | None = None) -> np.ndarray:
        """-> float64 [P + 1], ``P = min(max_nprobe or nlist, nlist, 2048)``: entry p is the share of the exact top-``K`` rows
        whose list is among the query's best p lists (entry 0 is 0) - the recall that probing alone allows at ``nprobe = p``.

        For an ``IVF<nlist>,Flat`` store, whose scan is exact over the probed lists, this IS ``recall(...).intersection`` at
        every ``nprobe <= P`` (up to near-ties: two rows whose scores the exact search and the list scan order differently can
        move one slot).  For the code modes it is a ceiling that no codec, ``k_factor`` or refiner lifts: a row whose list is
        not probed cannot be returned.  Costs one exact search, one coarse step at P (no list scan), one
        ``lvs_ivf_probe_ranks`` and a cumulative sum of P + 1 counts on the host.  Needs an unsharded store with lists."""
        run = self._recall_begin(query_vectors, K, None, "probe_recall_curve")
        _, hist = self._recall_ceiling(run, self._curve_width(run.ent, max_nprobe))
        return _curve_of(hist)

    @_serialised
    def tune_nprobe(self, query_vectors, K: int, target: float = 0.95, measure: str = "intersection",
                    k_factor: float | None = None, apply: bool = True):
        """-> ``(nprobe, RecallReport)``: the smallest ``nprobe`` found whose MEASURED recall of ``__call__(query_vectors, K)``
        reaches ``target``, and the one-entry report of that measurement.  ``measure``: ``"intersection"`` (share of the exact
        top K returned, the default) or ``"first"`` (share of queries whose true best row is returned).

        The search starts at the smallest p whose probe-limited ceiling (``probe_recall_curve``; for ``"first"``, the share
        of queries whose best row's list is among the p best) reaches the target: nothing below can, in any mode.  For an
        ``IVF<nlist>,Flat`` store that p is the answer - its recall is the ceiling - and no list scan is run; its report is
        made from the same ranks.  A code store is measured there, then at doubled values up to ``min(nlist, 2048)`` until the
        target is met, then bisected between the last miss and the first hit.  The coarse ranking behind the ceiling is
        taken 56 lists deep first - one pass over the centroids, a fraction of the exact search beside it - and four times
        deeper only while the ceiling stays below the target, so a Flat tune costs about one exact search.

        The guarantee is about the returned value: its measured recall on THESE queries is >= ``target`` (for a Flat store:
        up to near-ties, see ``probe_recall_curve``).  Measured recall of a code mode need not be monotone in ``nprobe``, so
        the value is minimal only up to that: a smaller one between two misses is not looked for.  The sample decides: the
        queries should look like the ones the store will serve.

        ``ValueError`` when the largest admissible ``nprobe`` misses the target; the message names the best measured value
        and the ceiling there - a ceiling below the target means the probes fall short (only reachable below ``nlist``); a
        ceiling above it means the codec does: raise ``k_factor`` on a ``Refine(Flat)`` store, or use one.  When the call
        would be served exactly whatever ``nprobe`` says (K > 56, rows too wide for the scan), the store's ``nprobe`` comes
        back unchanged with ``served=(False,)``.  ``apply=True`` sets ``self.nprobe`` to the result and nothing else."""
        if isinstance(target, bool) or not isinstance(target, (int, float, np.integer, np.floating)) or not 0 < target <= 1:
            raise ValueError(f"target must be a real number in (0, 1], got {target!r}")
        if measure not in ("intersection", "first"):
            raise ValueError(f"measure must be 'intersection' or 'first', got {measure!r}")
        if not isinstance(apply, (bool, np.bool_)):
            raise ValueError(f"apply must be a bool, got {apply!r}")
        target = float(target)
        run = self._recall_begin(query_vectors, K, k_factor, "tune_nprobe")
        if self._recall_plan(run, 1).route != "ivf":  # exact whatever nprobe says: nothing to tune, nothing launched
            return self.nprobe, self._recall_measure(run, [self.nprobe])
        pmax = self._curve_width(run.ent, None)
        known = {}  # the coarse ranking as far as it was needed: P, the ranks, the ceiling at every p <= P

        def widen(P: int) -> None:
            rank, hist = self._recall_ceiling(run, P)
            if measure == "first":  # the rank of each query's best row's list: nq counts
                r0 = _host(rank[:, 0]).astype(np.int64)
                hist = np.bincount(np.where(r0 < 0, P, r0), minlength=P + 1)
            known.update(P=P, rank=rank, ceiling=_curve_of(hist))

        # a ranking of 2 048 lists costs far more than the exact search beside it (a two-pass k = 2 048 search of the
        # centroids); the first 56 come from the one-pass search and settle most stores, wider ones only on demand
        widen(min(pmax, _capi.IVF_MAX_K))
        while not np.any(known["ceiling"] >= target) and known["P"] < pmax:
            widen(min(pmax, 4 * known["P"]))
        reports = {}

        def value(p: int) -> float:
            if p not in reports:
                reports[p] = self._recall_measure(run, [p])
            return float(getattr(reports[p], measure)[0])

        def fail(p: int):
            if p > known["P"]:
                widen(p)
            ceiling = known["ceiling"]
            if reports:
                best = max(reports, key=lambda v: (value(v), -v))
                got = f"the best measured is {value(best):.4f} at nprobe={best}"
            else:  # an IVF-Flat store: its recall is its ceiling
                got = f"the best measured is {ceiling[p]:.4f} at nprobe={p}"
            return ValueError(f"tune_nprobe: {measure} recall {target:g} at K={run.K} is not reached up to nprobe={p}: {got}, "
                              f"the probe-limited ceiling at nprobe={p} is {ceiling[p]:.4f}")

        reach = np.flatnonzero(known["ceiling"] >= target)
        if reach.size == 0:  # the probes fall short whatever the codec does; a code store is still measured once, to say by how much
            if self._mode.kind != "Flat":
                value(pmax)
            raise fail(pmax)
        rank = known["rank"]
        p = int(reach[0])
        if self._mode.kind == "Flat":  # exact over the probed lists: the ceiling is the recall
            inside = (rank >= 0) & (rank < p)
            hits = _host(inside.sum(dim=1)).astype(np.int32)[None, :]
            first = _host(inside[:, 0]).astype(np.float64)
            reports[p] = RecallReport(nprobes=(p,), intersection=np.array([_mean_ratio(hits[0], run.denom)], np.float64),
                                      first=np.array([first.mean()], np.float64), served=(True,), nq=run.queries.n, K=run.K,
                                      kc=run.K, hits=hits)
        else:
            lo = p - 1  # below p nothing reaches the target
            while value(p) < target:
                if p == pmax:
                    raise fail(pmax)
                lo, p = p, min(2 * p, pmax)
            while p - lo > 1:
                mid = (lo + p) // 2
                if value(mid) >= target:
                    p = mid
                else:
                    lo = mid
        if apply:
            self.nprobe = p
        return p, reports[p]

    def _range_args(self, ent: _Resident, ids, nprobe, what: str):
        """What ``range_search`` and ``ivf_self_pairs`` check alike -> (``ids`` as a vector or None for every row, lists probed
        per query or 0 without lists, whether the threshold scan takes the call).  Refused: a store whose rows or queries
        are in fact split over several ranks (``shard="auto"`` on one GPU splits nothing), ``ids`` that name a row twice (a
        bitmap holds a row once and a range result lists it once), an ``nprobe`` that is no int >= 1."""
        lay = self._layout()
        if lay[1] > 1 or lay[3] > 1:
            raise ValueError(f"{what} needs an unsharded store: this one is split over {lay[1]} x {lay[3]} ranks")
        sub = _ids_subset(ids, ent.n)
        if sub is not None and np.unique(sub).size != sub.size:
            raise ValueError("ids holds a row more than once: a threshold search returns a row once")
        if ent.ivf is None:
            return sub, 0, False
        be = self.backend
        nprobe = min(self._check_nprobe(self.nprobe if nprobe is None else nprobe), ent.ivf.nlist)
        return sub, nprobe, (nprobe <= _capi.MAX_K and hasattr(be, "ivf_range_search")
                             and be.ivf_range_fits(ent.d, ent.packed.mode))

    @_serialised
    def range_search(self, query_vectors, threshold: float, ids=None, nprobe: int | None = None, exact: bool = False):
        """faiss's ``range_search``: every row past a threshold for every query -> ``(lims int64 [nq + 1], D float32, I
        int64)``; query i's results are ``D[lims[i]:lims[i + 1]]`` / ``I[...]``, best first, ascending id among equal scores.
        ``METRIC_INNER_PRODUCT``: the rows with product ``> threshold``; ``METRIC_L2``: the rows with squared distance
        ``< threshold`` (faiss's radius), ``D`` the squared distances, ascending.  Both compares are strict, in fp32.

        An IVF store of any mode answers through its lists (``HipBackend.ivf_range_search``, faiss's
        ``IndexIVF::range_search``): the rows of each query's ``nprobe`` best lists (default: the store's) are scored EXACTLY
        from the full-precision image - the codes of an SQ8 / PQ store are not used - so the result is the exact one
        restricted to the probed lists, and ``nprobe = nlist`` is the exact result.  ``ids``: only those rows take part (a
        bitmap over the rows in the list scan); duplicates are a ``ValueError``.  ``exact=True``, ``"Flat"`` stores, rows too
        wide for the threshold scan (``HipBackend.ivf_range_fits``) and ``nprobe > 2048`` score every row, or every row of
        ``ids``, through ``HipBackend.range_join``.  Single GPU: a store split over several ranks is refused."""
        if not isinstance(exact, (bool, np.bool_)):
            raise ValueError(f"exact must be a bool, got {exact!r}")
        ent = self._current()
        q = self._query_matrix(query_vectors, ent)
        nq, be = int(q.shape[0]), self.backend
        threshold = float(threshold)
        if not np.isfinite(threshold):
            raise ValueError(f"threshold must be finite, got {threshold!r}")
        sub, nprobe, fits = self._range_args(ent, ids, nprobe, "range_search")
        use_lists = fits and not exact
        queries = be.pack(q, ent.packed.mode, normalize=self.normalize, exp=ent.packed.exp, check=True)
        empty = (np.zeros(nq + 1, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64))
        if nq == 0 or ent.n == 0 or (sub is not None and sub.size == 0):
            return empty
        # the kernels keep score > threshold with larger = better: a squared distance below the radius is -distance > -radius
        better = threshold if self.metric == METRIC_INNER_PRODUCT else -threshold
        if use_lists:
            sel = be.row_bitmap(sub, ent.n)[0] if sub is not None else None
            qi, j, s = be.ivf_range_search(ent.packed, ent.ivf, queries, better, self.metric, nprobe, sel=sel)
            qi, j, s = _host(qi), _host(j), _host(s)
        else:
            corpus = ent.packed if sub is None else be.gather(ent.packed, be.to_device(sub))
            qi, j, s = be.range_join(corpus, queries, better, self.metric)
            qi, j, s = _host(qi), _host(j), _host(s)
            j = j if sub is None else sub[j]
        order = np.lexsort((j, -s.astype(np.float64), qi))
        lims = np.zeros(nq + 1, np.int64)
        np.cumsum(np.bincount(qi, minlength=nq), out=lims[1:])
        s = s[order].astype(np.float32)
        return lims, (s if self.metric == METRIC_INNER_PRODUCT else np.float32(0.0) - s), j[order].astype(np.int64)

    @_serialised
    def ivf_self_pairs(self, threshold: float, ids=None, nprobe: int | None = None):
        """The store's own rows (all, or the rows ``ids``) as the queries of a threshold search through its lists -> host arrays
        ``(q, j, score)`` of ROW numbers: every ordered pair with ``q != j``, both in ``ids``, ``list(j)`` among the ``nprobe``
        lists row ``q`` probes, and score (the product, or minus the squared distance) ``> threshold``.  A pair usually comes
        back from both sides; ``dedup.threshold_pairs_ivf`` makes one record of the two.  The whole image is the query
        matrix as it stands (a view); a subset is gathered.  Needs an unsharded IVF store whose rows the threshold scan fits."""
        ent = self._ivf_current()
        be = self.backend
        sub, nprobe, fits = self._range_args(ent, ids, nprobe, "the list self-join")
        if not fits:
            raise ValueError(f"the threshold scan does not take d={ent.d} with nprobe={nprobe}: join exactly (nprobe=None)")
        if sub is None:
            queries, rows, sel = be.slice_rows(ent.packed, 0, ent.n), np.arange(ent.n, dtype=np.int64), None
        else:
            queries, rows, sel = be.gather(ent.packed, be.to_device(sub)), sub, be.row_bitmap(sub, ent.n)[0]
        if rows.size == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        q_rows = be.to_device(rows.astype(np.uint32).view(np.int32))
        q, j, s = be.ivf_range_search(ent.packed, ent.ivf, queries, float(threshold), self.metric, nprobe, q_rows=q_rows, sel=sel)
        return rows[_host(q)], _host(j).astype(np.int64), _host(s).astype(np.float32)

    @_serialised
    def sq8_codes(self):
        """-> (vmin float32 [d], vdiff float32 [d], codes uint8 [n, d] in ROW order, residual norms float32 [n]) of an
        IVF-SQ8 store, in the caller's units: row i decodes to ``c_l + vmin + (codes[i] + 0.5) * vdiff / 255`` (``l``: its
        list in ``ivf_lists()``, ``c_l`` its centroid there), and ``norms[i]`` is ``|vmin + (codes[i] + 0.5) * vdiff / 255|^2``
        as the device computed it in fp32."""
        return self._export_codes("SQ8", "SQ8")

    @_serialised
    def pq_codes(self):
        """-> (codebooks float32 [M, ksub, d / M], codes uint8 [n, M] in ROW order, beta float32 [n]) of an IVF-PQ store, in
        the caller's units: row i decodes to ``c_l + concat_m codebooks[m, codes[i, m]]`` (``l``: its list in
        ``ivf_lists()``, ``c_l`` its centroid there), and ``beta[i]`` is ``|rhat|^2 + 2 <c_l, rhat>`` of that decoded residual
        as the device computed it in fp32."""
        return self._export_codes("PQ", "PQ<M>")

    def _export_codes(self, kind: str, spelled: str):
        ent = self._ivf_current()
        if self._mode.kind != kind:
            raise ValueError(f"the loaded index has no {kind} codes (factory_string is not 'IVF<nlist>,{spelled}')")
        return self._mode.export(ent)

    def _check_width(self, d: int) -> None:
        if self._mode is not None:
            self._mode.check_width(d, self.factory_string)

    @staticmethod
    def _fp32_path(ent, q) -> bool:
        """fp32-accurate (hi|lo) operands take the certified one-pass search, which reads a count back mid-call: the staged
        pipeline is for the plain fp16 search."""
        return ent.packed.mode != _capi.PACK_F16

    def _check_queries(self, f: int, query_vectors, K, ids, kwargs):
        """Validation flags of the packed queries (``lvs_pack_rows_checked``).  inf / NaN raise.  Magnitudes that leave
        fp16's range under the INDEX's scale are searched again with an exponent of their own when the metric allows it
        (inner products; squared L2 needs one scale on both sides): the offending queries on their own, so that the rest
        of the batch keeps the index's exponent and its full precision - returns that result, else None.  The split is
        taken from the complete (replicated) query matrix, so every rank of a sharded store makes the same calls."""
        if not f:
            return None
        ent = self._current()
        if not (f & _capi.PACK_FLAG_RANGE and not f & _capi.PACK_FLAG_NONFINITE and self.metric == METRIC_INNER_PRODUCT
                and "_query_exp" not in kwargs and ent.packed.mode == _capi.PACK_SPLIT):
            self.backend.raise_for_flags(f, "query vectors")
            return None
        q = self._as_matrix(query_vectors, "query_vectors")
        big, pick = self._range_split(q, ent)
        kw = dict(kwargs)
        kw["_query_exp"] = "auto"
        if big is None:
            return self.__call__(q, K, ids, **kw)
        rest = self.__call__(pick(~big), K, ids, **kwargs)
        own = self.__call__(pick(big), K, ids, **kw)
        if self._is_device_tensor(rest.distances) or hasattr(rest.distances, "index_copy_"):  # return_device=True
            import torch

            D = torch.empty((len(big), K), dtype=rest.distances.dtype, device=rest.distances.device)
            I = torch.empty((len(big), K), dtype=rest.indices.dtype, device=rest.indices.device)
            for sel, part in ((~big, rest), (big, own)):
                at = torch.from_numpy(np.flatnonzero(sel)).to(D.device)
                D[at], I[at] = part.distances, part.indices
            return RMOutput(distances=D, indices=I)
        D, I = np.empty((len(big), K), np.float32), np.empty((len(big), K), np.int64)
        D[~big], I[~big] = rest.distances, rest.indices
        D[big], I[big] = own.distances, own.indices
        return RMOutput(distances=D, indices=I)

    def _range_split(self, q, ent):
        """-> (big, pick): ``big`` bool [nq], the queries with a component beyond fp16's range under the index's power-of-two
        scale, and ``pick(mask)``, the rows of ``q`` (a host array or a device tensor) under a mask like it.  ``big`` is None when
        all or none of them are: nothing to split, the batch goes to one call with ``_query_exp="auto"``."""
        on_device = self._is_device_tensor(q)
        rowmax = q.abs().amax(dim=1).float().cpu().numpy() if on_device else np.abs(q).max(axis=1, initial=0.0)
        big = np.asarray(rowmax, dtype=np.float64) * 2.0 ** ent.packed.exp > 65504.0
        if big.all() or not big.any():
            return None, None
        if on_device:
            import torch

            return big, lambda mask: q[torch.from_numpy(np.flatnonzero(mask)).to(q.device)]
        return big, lambda mask: q[mask]

    @_serialised
    def scores(self, query_vectors, ids: list[int] | None = None, _query_exp=None):
        """Similarity of every query to every indexed row (or to rows ``ids``, in that order) as one float32 matrix
        [Q, N] - what the K = N callers actually want (``sem_filter.py:491-497`` takes ``vec_scores`` of ALL rows,
        ``sem_join.py:343-373`` clips them to [0, 1]) without ranking anything.  Inner product:
        the product; L2: minus the squared distance.  On a sharded index every rank computes the columns of its
        shard and one all-gather completes the rows."""
        ent = self._current()
        q = self._query_matrix(query_vectors, ent)
        be = self.backend
        sub = _ids_subset(ids, ent.n)
        _, world = self._dist()
        queries = be.pack(q, ent.packed.mode, normalize=self.normalize,
                          exp=ent.packed.exp if _query_exp is None else _query_exp, check="lazy")
        f = int(queries.flags.item()) if getattr(queries, "flags", None) is not None else 0
        if (f & _capi.PACK_FLAG_RANGE and not f & _capi.PACK_FLAG_NONFINITE and self.metric == METRIC_INNER_PRODUCT
                and _query_exp is None and ent.packed.mode == _capi.PACK_SPLIT):
            # magnitudes outside fp16's range under the index's scale: inner products allow those queries an exponent of
            # their own (the rest of the batch keeps the index's, as in __call__)
            big, pick = self._range_split(q, ent)
            if big is None:
                return self.scores(q, ids, _query_exp="auto")
            rest, own = self.scores(pick(~big), ids), self.scores(pick(big), ids, _query_exp="auto")
            out = np.empty((len(big), rest.shape[1]), np.float32)
            out[~big], out[big] = rest, own
            return out
        if f:
            be.raise_for_flags(f, "query vectors")
        sc, order = self._score_rows(ent, queries, sub, world, want_ids=False)
        out = sc.cpu().numpy()
        if order is not None:  # columns arrived shard by shard: put them back into the order of `ids`
            res = np.empty_like(out)
            res[:, order] = out
            out = res
        return out

    def _score_rows(self, ent: _Resident, queries, sub, world: int, want_ids: bool = True):
        """Score rows [Q, n_eff] (device float32) of `queries` against all rows (``sub`` None) or the rows ``sub``.

        Returns ``(scores, order)``.  Unsharded: columns follow ``sub`` (``order`` = ``sub`` when ids are wanted, else
        None).  Sharded: every rank scores the requested rows that live in its shard, the blocks are all-gathered and
        laid side by side in rank order; ``order[j]`` then names column j - the global row id (``want_ids``) or its
        position in ``sub`` - and is None when the columns are simply rows 0..n-1."""
        be = self.backend
        if world == 1:
            corpus = ent.packed if sub is None else be.gather(ent.packed, be.to_device(sub))
            sc = be.scores(corpus, queries, self.metric)
            return sc, (sub if (sub is not None and want_ids) else None)
        from . import _dist

        per = -(-ent.n // world) if ent.n else 0
        bounds = [(min(ent.n, r * per), min(ent.n, (r + 1) * per)) for r in range(world)]
        if sub is None:
            pos = [np.arange(lo, hi, dtype=np.int64) for lo, hi in bounds]  # global rows per rank
            corpus = ent.packed
        else:
            pos = [np.flatnonzero((sub >= lo) & (sub < hi)) for lo, hi in bounds]  # positions in `sub` per rank
            mine = pos[bounds.index((ent.lo, ent.hi))]
            corpus = be.gather(ent.packed, be.to_device(sub[mine] - ent.lo))
        widths = [len(p_) for p_ in pos]
        wmax = max(widths) if widths else 0
        nq = queries.n
        import torch

        block = torch.full((nq, wmax), float("-inf"), dtype=torch.float32, device=queries.rows.device)
        if corpus.n:
            block[:, :corpus.n] = be.scores(corpus, queries, self.metric)
        parts = _dist.all_gather_rows(block, self._pg_corpus())  # [world, nq, wmax]
        sc = torch.cat([parts[r][:, :widths[r]] for r in range(world)], dim=1).contiguous()
        if sub is None:
            return sc, None
        cols = np.concatenate(pos) if pos else np.zeros(0, np.int64)
        return sc, (sub[cols] if want_ids else cols)

    def packed_rows(self, ids=None):
        """Device image (backend ``PackedRows``) of the current index restricted to positional ``ids`` (all rows
        when ``ids`` is None or covers them in order) - what the GPU-side operators (dedup, k-means) consume.
        Needs the whole index on this rank (``shard=False``)."""
        ent = self._current()
        if ent.lo != 0 or ent.hi != ent.n:
            raise ValueError("packed_rows needs an unsharded index")
        sub = _ids_subset(ids, ent.n)
        return ent.packed if sub is None else self.backend.gather(ent.packed, self.backend.to_device(sub))

    @_serialised
    def kmeans(self, vec_set, ncentroids: int, niter: int = 20, ids=None, return_result: bool = False, **kw):
        """faiss-parity k-means of the current index's rows ``ids`` (``lotus/utils.py:61-65``) on the GPU(s) that already
        hold them; returns the cluster id of every row (all rows on every rank).  ``vec_set`` is not needed (the device
        image is used) and only kept for the shape of the reference call.  On a row-sharded index every rank trains on
        and assigns the rows of its own shard (one all-reduce per iteration, one all-gather of the ids)."""
        from .cluster import kmeans as _kmeans

        ent = self._current()
        sub = _ids_subset(ids, ent.n)
        be = self.backend
        # the path is chosen from the group size - identical on every rank - never from this rank's share of the rows
        # (with ceil(n / world) >= n rank 0 holds everything while the others still enter the collectives)
        if self._dist()[1] == 1:  # the whole index lives on this rank
            packed = ent.packed if sub is None else be.gather(ent.packed, be.to_device(sub))
            res = _kmeans(None, ncentroids, niter=niter, backend=be, packed=packed, process_group=self._pg_corpus(), **kw)
        else:
            if sub is None:
                packed, local_pos, n_total = ent.packed, np.arange(ent.lo, ent.hi, dtype=np.int64), ent.n
            else:
                local_pos = np.flatnonzero((sub >= ent.lo) & (sub < ent.hi))  # positions in `ids`, ascending
                packed = be.gather(ent.packed, be.to_device(sub[local_pos] - ent.lo))
                n_total = int(sub.size)
            kw.pop("shard", None)
            res = _kmeans(None, ncentroids, niter=niter, backend=be, packed=packed, shard=True,
                          process_group=self._pg_corpus(), n_total=n_total, local_pos=local_pos, **kw)
        return res if return_result else res.assign

    # ------------------------------------------------------------------------------------------ multi-GPU
    def _pooled_seed_scores(self, ent: _Resident, queries, k: int, world: int):
        """Row-sharded join: every shard scores a small sample of its own rows and the blocks are all-gathered inside the
        corpus group, so that every shard starts from thresholds that know ALL shards' samples (an 8 x larger sample at no
        extra MFMA cost per GPU; ``lvs_flat_search_keys_seeded``).  None when the shape is not worth a collective; the
        decision depends on the call's arguments and the nominal shard size only, so every rank takes it alike."""
        be = self.backend
        if world <= 1 or not hasattr(be, "seed_tiles"):
            return None
        per = -(-ent.n // world) if ent.n else 0
        tiles = be.seed_tiles(queries.n, per, k, ent.packed.mode, queries.mode)
        if tiles <= 0:
            return None
        from . import _dist

        mine = be.seed_scores(ent.packed, queries, self.metric, tiles)                    # [tiles, nq]
        return _dist.all_gather_rows(mine, self._pg_corpus()).reshape(world * tiles, queries.n)

    def _allgather_merge(self, keys, world: int):
        """All-gather the per-shard candidate keys [Q,k] (8 B each; ONE RCCL all-gather over xGMI on a GPU node, staged
        through the host for any other process-group backend) and merge them on every rank (``lvs_merge_keys``)."""
        from . import _dist

        return self.backend.merge_keys(_dist.all_gather_rows(keys, self._pg_corpus()))
