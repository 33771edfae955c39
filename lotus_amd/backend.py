"""Device backend: torch provides HBM buffers, streams and (for multi-GPU) RCCL; every compute step is a C-ABI call
into liblotus_hip.so.  No CPU fallback - constructing the backend without a GPU raises."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import LotusHipError


@dataclass
class PackedRows:
    """Device image of an embedding matrix: fp16 rows [n, ld] (+ |x|^2 per row)."""

    rows: "object"  # torch.Tensor float16 [n, ld]
    norms: "object"  # torch.Tensor float32 [n]: |row|^2 of the STORED (scaled) values
    n: int
    d: int
    mode: int  # _capi.PACK_F16 | _capi.PACK_SPLIT
    exp: int = 0  # the rows hold x * 2^exp (an exact power-of-two scale chosen at pack time; 0 = as given)
    flags: "object" = None  # device int32 [1] of LVS_PACK_FLAG_* when the pack was validated lazily (check="lazy")


@dataclass
class IvfLists:
    """Inverted lists of an IVF-Flat index over a flat device image: row NUMBERS into that image, grouped by list."""

    centroids: "object"  # PackedRows [nlist, d], packed like the image (same mode, same scale exponent)
    offsets: "object"    # torch.Tensor int64 [nlist + 1]: list l = rows[offsets[l]:offsets[l + 1]]
    rows: "object"       # torch.Tensor int32 [n] holding uint32 row numbers, ascending inside a list
    nlist: int
    metric: int
    row_list: "object" = None  # torch.Tensor int32 [n]: the list of every row; made by ``ivf_row_lists`` on first use


def ivf_fits(d: int, k: int, mode: int) -> bool:
    """Host-only query of the library: does ``lvs_ivf_search_keys`` take this dimension, k and pack mode?"""
    return int(_capi.load().lvs_ivf_search_workspace_bytes(1, 1, 1, int(d), int(k), int(mode))) >= 0


def ivf_range_fits(d: int, mode: int) -> bool:
    """Host-only query of the library: does ``lvs_ivf_range_search`` take this dimension and pack mode?"""
    return int(_capi.load().lvs_ivf_range_workspace_bytes(1, 1, 1, int(d), int(mode))) >= 0


@dataclass
class IvfSq8Lists:
    """The 8-bit residual codes of an IVF-SQ8 index beside its ``IvfLists``, all in the image's stored scale (values x 2^exp)."""

    vmin: "object"       # torch.Tensor float32 [d]: per-dimension minimum of the training residuals
    vdiff: "object"      # torch.Tensor float32 [d]: vmax - vmin
    centroids: "object"  # torch.Tensor float32 [nlist, d]: the packed centroids' values
    codes: "object"      # torch.Tensor uint8 [n, ldc] in LIST order (position p of IvfLists.rows), ldc = d rounded up to 64
    rnorm: "object"      # torch.Tensor float32 [n]: |decoded residual|^2 per list position
    exp: int             # the image's pack exponent


def ivf_sq8_fits(d: int, k: int, mode: int) -> bool:
    """Host-only query of the library: does ``lvs_ivf_sq8_search_keys`` take this dimension, k and pack mode?"""
    return int(_capi.load().lvs_ivf_sq8_search_workspace_bytes(1, 1, 1, int(d), int(k), int(mode))) >= 0


@dataclass
class IvfPqLists:
    """The product-quantizer codes of an IVF-PQ index beside its ``IvfLists``, all in the image's stored scale (values x 2^exp)."""

    M: int               # subspaces (d % M == 0), dsub = d / M
    ksub: int            # codebook entries per subspace (256, fewer with fewer training rows)
    codebooks: "object"  # torch.Tensor float32 [M, ksub, dsub]
    centroids: "object"  # torch.Tensor float32 [nlist, d]: the packed centroids' values
    codes: "object"      # torch.Tensor uint8 [n, ldc] in LIST order (position p of IvfLists.rows), ldc = M rounded up to 16
    beta: "object"       # torch.Tensor float32 [n]: |rhat|^2 + 2 <c_l, rhat> per list position
    exp: int             # the image's pack exponent


def ivf_pq_fits(d: int, M: int, k: int, mode: int) -> bool:
    """Host-only query of the library: does ``lvs_ivf_pq_search_keys`` take this dimension, M, k and pack mode?"""
    return int(_capi.load().lvs_ivf_pq_search_workspace_bytes(1, 1, 1, int(d), int(M), int(k), int(mode))) >= 0


class _DevBytes:
    """A raw device pointer as something ``torch.as_tensor`` understands (the all-gather callback of ``lvs_search_sharded``)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def _operands(corpus: "PackedRows", queries: "PackedRows") -> dict:
    """A packed corpus and packed queries under the nine parameter names of the entry points that take both whole."""
    return dict(xb=_ptr(corpus.rows), xb_pack=corpus.mode, nb=corpus.n, xb_norms_sq=_ptr(corpus.norms), xq=_ptr(queries.rows),
                xq_pack=queries.mode, nq=queries.n, xq_norms_sq=_ptr(queries.norms), d=corpus.d)


class _Bounds:
    """The Hamerly bounds that a squared-L2 ``nearest`` call keeps beside its search: the caller's ``bounds`` tuple
    ``(assign, ub, lb, positions)``, the corpus statistics and the five coefficients of the search's own error bound."""

    def __init__(self, be, bounds, corpus_stats, coef, id_offset):
        self.be, self.corpus_stats, self.id_offset = be, corpus_stats, int(id_offset)
        self.assign, self.ub, self.lb, self.pos = bounds
        self.coef5 = (ctypes.c_float * 5)(*coef)

    def of_queries(self, q0: int, q1: int) -> "_Bounds":
        """The same bounds for the chunk [q0, q1) of the call's queries."""
        t = self.be.torch
        pos = self.pos[q0:q1] if self.pos is not None else t.arange(q0, q1, dtype=t.int64, device=self.be.device)
        return _Bounds(self.be, (self.assign, self.ub, self.lb, pos), self.corpus_stats, self.coef5, self.id_offset)

    def set(self, keys, sec, q_norms, nq: int) -> None:
        """Every query's bounds from the one-pass result (see ``HipBackend.nearest``)."""
        self.be._call("lvs_kmeans_bounds_set", keys=_ptr(keys), key_stride=1, second=_ptr(sec), q_norms_sq=_ptr(q_norms),
                   positions=_ptr(self.pos), m=nq, corpus_stats=_ptr(self.corpus_stats), coef5=ctypes.addressof(self.coef5),
                   id_offset=self.id_offset, assign=_ptr(self.assign), ub=_ptr(self.ub), lb=_ptr(self.lb), stream=self.be._stream())

    def fix(self, approx, exact, q_norms, sel) -> None:
        """The bounds of the queries ``sel`` again, from their one-pass keys ``approx`` and the ``exact`` keys that decided them."""
        # float32 rounding of |x|^2 + |c|^2 - 2 x.c (cancellation when the row sits on a centroid): a few ulps of
        # the largest term - 8e-6 R |x| + 4e-6 R^2; errors proportional to the distance itself are covered by the
        # relative margin of lvs_kmeans_bounds_step
        exact2 = (ctypes.c_float * 2)(8e-6, 4e-6)
        pos = sel if self.pos is None else self.pos[sel]
        self.be._call("lvs_kmeans_bounds_fix", approx_keys=_ptr(approx), exact_keys=_ptr(exact), q_norms_sq=_ptr(q_norms),
                   positions=_ptr(pos), m=int(sel.numel()), corpus_stats=_ptr(self.corpus_stats),
                   coef5=ctypes.addressof(self.coef5), exact_coef2=ctypes.addressof(exact2), id_offset=self.id_offset,
                   assign=_ptr(self.assign), ub=_ptr(self.ub), lb=_ptr(self.lb), stream=self.be._stream())


@dataclass
class _NearestHandle:
    """``nearest_begin`` -> ``nearest_finish``: finished keys, one handle per chunk, or ONE pending ``lvs_nearest3`` call."""

    queries: PackedRows
    done: "object" = None    # int64 [nq, 1]: nothing is pending
    chunks: list = None      # [(q0, q1, _NearestHandle of queries [q0, q1))]
    corpus: PackedRows = None
    metric: int = 0
    id_offset: int = 0
    exact_scores: bool = True
    bounds: _Bounds = None
    keys: "object" = None    # int64 [nq, 1]: the one-pass winners, decided in place by the finish
    keys2: "object" = None   # int64 [nq]: the runners-up
    pair_idx: "object" = None  # int64 [nq]: the queries only two rows can win, ``open_idx``: those to search again, and
    open_idx: "object" = None
    counts: "object" = None    # int64 [2]: how many of each (read by the finish: the call's one host round trip)


class HipBackend:
    PACK_CHUNK_ROWS = 262144
    NEAREST3_WS_BUDGET = 2 << 30  # bytes of scratch one lvs_nearest3 call may ask for; more queries go through in chunks
    MAX_STREAM_WORKSPACES = 4     # scratch buffers kept at a time (one per stream that has made a call)

    def __init__(self, device=None):
        import torch

        self.torch = torch
        self.lib = _capi.load()
        if not torch.cuda.is_available():
            raise LotusHipError("lotus_amd needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._ws = None
        # host -> device staging (see _h2d): a pinned buffer, a copy stream and a few threads that fill the buffer
        self._stage_buf = None   # pinned ring [H2D_SLOTS, H2D_SLICE_BYTES]; False: pinning failed, plain copies
        self._stage_done = None  # per ring slot: event of the last DMA that read it
        self._copy_stream = None
        self._pool = None
        import threading

        self._h2d_lock = threading.Lock()
        # one device workspace and one set of side streams per backend: stores that share a backend take this lock around
        # every plugin call (HipVS), so two threads never interleave the launches of two operations
        self._call_lock = threading.RLock()

    # ---- plumbing ----
    def _stream(self) -> int:
        return int(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _c(self, name: str, *args, **kw) -> None:
        """One C-ABI call on this backend's device: positional arguments as the header orders them, keywords by the header's
        parameter names (``_capi.bind``).  The library makes the stream's device current itself, but torch's default stream
        is the NULL handle, which names no device - so the device is also made current here."""
        args = _capi.bind(name, args, kw)
        with self.torch.cuda.device(self.device):
            _capi.check(getattr(self.lib, name)(*args), name)

    def _call(self, name: str, *args, **kw) -> None:
        """``_c`` as this module calls it: the keywords are bound here, so ``_c`` itself always sees one positional call in the
        header's order - what a wrapper put around ``_c`` (the tests record the entries called that way) can rely on."""
        self._c(name, *_capi.bind(name, args, kw))

    def _workspace(self, nbytes: int):
        """The scratch buffer of the CURRENT stream (one per stream: launches queued on a side stream - the k-means sums and
        certificates of one row range under the assignment search of the next - never share scratch memory with the main one)."""
        if self._ws is None:
            self._ws = {}
        key = self._stream()
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            if ws is None and len(self._ws) >= self.MAX_STREAM_WORKSPACES:
                # side streams come and go (one per k-means call): keep the default stream's buffer, drop the others - a dropped
                # buffer goes back to the allocator's pool of the stream it was allocated on, so work still queued there is safe
                for k_old in [k_ for k_ in self._ws if k_ != 0]:
                    del self._ws[k_old]
            ws = self._ws[key] = self.torch.empty(max(nbytes, 1 << 20), dtype=self.torch.uint8, device=self.device)
        return ws

    def synchronize(self) -> None:
        self.torch.cuda.synchronize(self.device)

    def to_device(self, arr: np.ndarray):
        return self.torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)

    # ---- host <-> device transfers at the boundary (VS.__call__ hands over host ndarrays, faiss_vs.py:43-77) ----
    H2D_SLICE_BYTES = 16 << 20
    H2D_SLOTS = 4       # pinned ring: H2D_SLOTS x H2D_SLICE_BYTES = 64 MB whatever the matrix (a pack chunk may be GBs)
    H2D_THREADS = 4

    def _h2d_ring(self):
        """The pinned staging ring, its copy stream and thread pool (created once; None when pinning fails - e.g. under a
        container's memlock limit - and the plain ``.to()`` path is used from then on)."""
        torch = self.torch
        if self._stage_buf is False:
            return None
        if self._stage_buf is None:
            try:
                self._stage_buf = torch.empty((self.H2D_SLOTS, self.H2D_SLICE_BYTES), dtype=torch.uint8, pin_memory=True)
            except Exception:  # cannot page-lock: fall back for good
                self._stage_buf = False
                return None
            from concurrent.futures import ThreadPoolExecutor

            self._pool = ThreadPoolExecutor(self.H2D_THREADS)
            self._copy_stream = torch.cuda.Stream(device=self.device)
            self._stage_done = [None] * self.H2D_SLOTS
        return self._stage_buf

    def _h2d(self, c: np.ndarray, out=None, after=None):
        """``out`` / ``after``: copy into this preallocated device tensor, the side stream waiting for the event ``after``
        (recorded when ``out`` was allocated) instead of for everything queued on the compute stream - a transfer that must
        overlap a search already in flight (``search_host_pipelined``).

        Device copy of a C-contiguous float16 / float32 host matrix.  A pageable ndarray reaches the GPU through a
        pinned staging buffer either way; doing that staging here, in 16 MB slices through a small ring - a few threads copy
        the next slices into free ring slots (numpy releases the GIL) while the DMA engine moves the finished ones on a side
        stream - makes the transfer run at the slower of (multi-threaded memcpy, PCIe) instead of a single-threaded memcpy
        followed by the DMA: 154 MB of queries in ~4 ms instead of ~15-25.  The compute stream waits on an event.  The ring
        is bounded (64 MB) and guarded by a lock: two threads sharing a backend take turns."""
        torch = self.torch
        nbytes = int(c.nbytes)
        ring = None
        if nbytes >= (4 << 20) and c.ndim == 2 and int(c.shape[1]) * c.itemsize <= self.H2D_SLICE_BYTES:
            with self._h2d_lock:
                ring = self._h2d_ring()
        if ring is None:
            import warnings

            with warnings.catch_warnings():  # a read-only memory map (store.py): the host view is only read by the copy
                warnings.simplefilter("ignore", UserWarning)
                t = torch.from_numpy(c)
            if out is not None:
                out.copy_(t)
                return out
            return t.to(self.device)
        tdt = torch.float16 if c.dtype == np.float16 else torch.float32
        rows, row_bytes = int(c.shape[0]), int(c.shape[1]) * c.itemsize
        per = max(1, self.H2D_SLICE_BYTES // row_bytes)
        bounds = [(a, min(rows, a + per)) for a in range(0, rows, per)]
        with self._h2d_lock:
            dev = out if out is not None else torch.empty(c.shape, dtype=tdt, device=self.device)
            cur = torch.cuda.current_stream(self.device)
            cs = self._copy_stream
            if out is not None and after is not None:
                cs.wait_event(after)
            else:
                cs.wait_stream(cur)  # `dev` was allocated on the compute stream
            slots = [ring[i][:per * row_bytes].view(tdt).reshape(per, int(c.shape[1])) for i in range(self.H2D_SLOTS)]
            slots_np = [t.numpy() for t in slots]
            pending, nxt = [], 0

            def submit():  # keep up to H2D_SLOTS host copies in flight; a slot is reused once its previous DMA has finished
                nonlocal nxt
                while nxt < len(bounds) and len(pending) < self.H2D_SLOTS:
                    slot = nxt % self.H2D_SLOTS
                    if self._stage_done[slot] is not None:
                        self._stage_done[slot].synchronize()
                    a, b = bounds[nxt]
                    pending.append((nxt, self._pool.submit(np.copyto, slots_np[slot][:b - a], c[a:b])))
                    nxt += 1

            last = None
            with torch.cuda.stream(cs):
                while nxt < len(bounds) or pending:
                    submit()
                    i, f = pending.pop(0)
                    f.result()
                    a, b = bounds[i]
                    dev[a:b].copy_(slots[i % self.H2D_SLOTS][:b - a], non_blocking=True)
                    last = self._stage_done[i % self.H2D_SLOTS] = cs.record_event()
            dev.record_stream(cs)
            if last is not None:
                cur.wait_event(last)
        return dev

    def to_host(self, *tensors):
        """Device tensors -> numpy arrays backed by pinned host memory (torch's caching host allocator: no page-locking
        per call), all copies in flight together, ONE stream synchronisation."""
        torch = self.torch
        outs = []
        for t in tensors:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            outs.append(h)
        torch.cuda.current_stream(self.device).synchronize()
        return tuple(h.numpy() for h in outs)

    CALL_PIPELINE_MIN_QUERIES = 32768
    CALL_CHUNK = 32768  # queries per launch of a chunked search (LVS_RQ_CHUNK_DEFAULT, lotus_amd/csrc/lvs_tile.h)
    CALL_PIPELINE = (0.1, 0.9)  # shares of the queries per stage: a short first stage (its H2D is the exposed one; measured at
    # 100 k x 1 M, tools/tcall_probe.py: one stage 144.0 ms, (0.1, 0.9) 139.2, (0.2, 0.8) 141.5, (0.5, 0.5) 145.1, three or four
    # stages 141.8-150.1 against 135.9 ms device-resident - shorter launches run further below the long-stream rate)

    def search_host_pipelined(self, corpus: PackedRows, q: np.ndarray, k: int, metric: int, id_offset: int = 0,
                              normalize: bool = False, exp: int = 0):
        """``VS.__call__`` for a large host query matrix (faiss_vs.py:75): the queries go through in two stages so that the
        host -> device copy of the second overlaps the search of the first and the device -> host copy of the first stage's
        results overlaps the search of the second (results are per query: staging is exact).  Only the first stage's H2D
        and the last stage's D2H are exposed.  -> (D float32 [nq,k], I int64 [nq,k] pinned-backed numpy arrays, flag word)."""
        torch = self.torch
        nq, d = int(q.shape[0]), int(q.shape[1])
        cuts = [0]
        if nq > 2 * self.CALL_CHUNK:
            # (r6) stages cut where the search cuts its chunks (lvs_flat_search_keys: launches of 32 768 queries, the remainder
            # last): a stage of the remainder (copy: a few MB), one chunk, then everything else - no stage splits a chunk into
            # the smaller, slower launches, and every copy but the first tiny one runs under a search
            r = nq % self.CALL_CHUNK
            cuts += [r, r + self.CALL_CHUNK] if r >= 256 else [self.CALL_CHUNK]
        else:
            for share in self.CALL_PIPELINE[:-1]:
                cuts.append(min(nq, (int(nq * share) + cuts[-1] + 255) // 256 * 256))
        cuts.append(nq)
        stages = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        tdt = torch.float16 if q.dtype == np.float16 else torch.float32
        cur = torch.cuda.current_stream(self.device)
        # every stage's device buffer exists before the first search is queued: its copy need not wait for that search
        bufs = [torch.empty((b - a, d), dtype=tdt, device=self.device) for a, b in stages]
        allocated = cur.record_event()
        if getattr(self, "_d2h_stream", None) is None:
            self._d2h_stream = torch.cuda.Stream(device=self.device)
        Dh = torch.empty((nq, k), dtype=torch.float32, pin_memory=True)
        Ih = torch.empty((nq, k), dtype=torch.int64, pin_memory=True)
        flags = torch.zeros((1,), dtype=torch.int32, device=self.device)
        mode = corpus.mode
        for (a, b), buf in zip(stages, bufs):
            c = np.ascontiguousarray(q[a:b], dtype=np.float16 if q.dtype == np.float16 else np.float32)
            self._h2d(c, out=buf, after=allocated)
            queries = self.pack(buf, mode, normalize=normalize, exp=exp, check="lazy")
            if queries.flags is not None:
                flags |= queries.flags
            keys = self.search_keys(corpus, queries, k, metric, id_offset=id_offset)
            Dd, Id = self.keys_to_result(keys, metric, None, score_exp=self.score_exp_of(corpus, queries))
            done = cur.record_event()
            with torch.cuda.stream(self._d2h_stream):
                self._d2h_stream.wait_event(done)
                Dh[a:b].copy_(Dd, non_blocking=True)
                Ih[a:b].copy_(Id, non_blocking=True)
            Dd.record_stream(self._d2h_stream)
            Id.record_stream(self._d2h_stream)
        fh = torch.empty((1,), dtype=torch.int32, pin_memory=True)
        fh.copy_(flags, non_blocking=True)
        cur.synchronize()
        self._d2h_stream.synchronize()
        return Dh.numpy(), Ih.numpy(), int(fh[0])

    # ---- packing ----
    SCALE_TARGET_EXP = 6  # exp="auto": the largest |x| lands in [2^6, 2^7) - components ~10x smaller still have their lo half
                          # in fp16's normal range, values up to 500x larger than the sampled maximum still fit

    def absmax(self, x) -> float:
        """Largest |value| of a device tensor (float16 / float32) through ``lvs_absmax``."""
        torch = self.torch
        bits = torch.zeros((1,), dtype=torch.int32, device=self.device)
        t = x.contiguous()
        if t.dtype not in (torch.float16, torch.float32):
            t = t.to(torch.float32)
        n, d = (int(t.shape[0]), int(t.shape[1])) if t.dim() == 2 else (1, int(t.numel()))
        self._call("lvs_absmax", src=_ptr(t), src_dtype=_capi.DTYPE_F16 if t.dtype == torch.float16 else _capi.DTYPE_F32, n=n, d=d,
                inout_bits=_ptr(bits), stream=self._stream())
        return float(np.array([int(bits.item())], np.uint32).view(np.float32)[0])

    @classmethod
    def exp_for(cls, absmax: float) -> int:
        """The pack exponent that moves ``absmax`` to [2^SCALE_TARGET_EXP, 2^(SCALE_TARGET_EXP + 1))."""
        if not np.isfinite(absmax) or absmax <= 0.0:
            return 0
        return int(np.clip(cls.SCALE_TARGET_EXP - int(np.floor(np.log2(absmax))), -60, 60))

    def pack(self, x, mode: int, normalize: bool = False, check=False, exp=0) -> PackedRows:
        """x: numpy [n,d] (float16/32/64) or a torch CUDA tensor (float16/float32).

        ``exp``: every value is multiplied by 2^exp before it is rounded (exact).  ``"auto"`` picks the exponent from the
        data (hi|lo rows only: fp32-accurate rows keep ~22 significant bits whatever the embeddings' magnitude; fp16 rows
        are stored as given): from the first chunk's largest magnitude, with 500x headroom - should a later chunk exceed
        it, everything is packed again with the exponent of the true maximum.
        ``check``: validate the values on the device while packing.  ``True`` raises ``ValueError`` for inf / NaN or for
        magnitudes beyond fp16's range (one read-back of a flag word; faiss itself accepts any float32, the fp16-based
        rows here do not - DESIGN.md section 7); ``"lazy"`` leaves the flag word on the device (``PackedRows.flags``) for
        the caller to read together with its results (``raise_for_flags``)."""
        torch = self.torch
        is_tensor = torch.is_tensor(x)
        n, d = int(x.shape[0]), int(x.shape[1])
        ld = int(self.lib.lvs_packed_ld(d, mode))
        if ld <= 0:
            raise LotusHipError(f"bad dimension d={d}")
        auto = isinstance(exp, str)
        if auto and exp != "auto":
            raise ValueError("exp must be an int or 'auto'")
        if auto and normalize and mode == _capi.PACK_SPLIT:
            auto, exp = False, self.SCALE_TARGET_EXP + 2  # unit rows: components <= 1, typically ~3 / sqrt(d)
        if auto and (mode != _capi.PACK_SPLIT or n == 0):
            auto, exp = False, 0
        rows = torch.empty((n, ld), dtype=torch.float16, device=self.device)
        norms = torch.empty((n,), dtype=torch.float32, device=self.device)
        flags = torch.zeros((1,), dtype=torch.int32, device=self.device) if (check or auto) else None
        amax_bits = torch.zeros((1,), dtype=torch.int32, device=self.device) if auto else None
        step = self.PACK_CHUNK_ROWS

        def chunk_of(r0, r1):
            if is_tensor:
                chunk = x[r0:r1].contiguous()
                if chunk.dtype not in (torch.float16, torch.float32):
                    chunk = chunk.to(torch.float32)
                if chunk.device != self.device:
                    chunk = chunk.to(self.device)
                return chunk
            c = x[r0:r1]
            c = np.ascontiguousarray(c, dtype=np.float16 if c.dtype == np.float16 else np.float32)
            return self._h2d(c)

        def run(e: int):
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                chunk = chunk_of(r0, r1)
                src_dtype = _capi.DTYPE_F16 if chunk.dtype == torch.float16 else _capi.DTYPE_F32
                if auto:
                    self._call("lvs_absmax", src=_ptr(chunk), src_dtype=src_dtype, n=r1 - r0, d=d, inout_bits=_ptr(amax_bits),
                            stream=self._stream())
                    if r0 == 0 and e is None:  # the exponent comes from the first chunk (one read-back per index build)
                        e = self.exp_for(float(np.array([int(amax_bits.item())], np.uint32).view(np.float32)[0]))
                self._call("lvs_pack_rows_checked", src=_ptr(chunk), src_dtype=src_dtype, n=r1 - r0, d=d, pack_mode=mode,
                        normalize=int(bool(normalize)), scale_exp=int(e), dst=_ptr(rows[r0:r1]), out_norms_sq=_ptr(norms[r0:r1]),
                        out_flags=_ptr(flags), stream=self._stream())
                del chunk
            return e

        e = run(None if auto else int(exp))
        if auto and n > step:  # a later chunk may have exceeded the first chunk's range: pack again with the true maximum's
            f = int(flags.item())
            if f & _capi.PACK_FLAG_RANGE and not f & _capi.PACK_FLAG_NONFINITE:
                flags.zero_()
                e = run(self.exp_for(float(np.array([int(amax_bits.item())], np.uint32).view(np.float32)[0])))
        out = PackedRows(rows=rows, norms=norms, n=n, d=d, mode=mode, exp=int(e or 0), flags=flags if check == "lazy" else None)
        if check is True or (auto and check != "lazy"):
            self.raise_for_flags(int(flags.item()))
        return out

    @staticmethod
    def raise_for_flags(f: int, what: str = "embeddings") -> None:
        if f & _capi.PACK_FLAG_NONFINITE:
            raise ValueError(f"{what} contain inf or NaN")
        if f & _capi.PACK_FLAG_RANGE:
            raise ValueError(f"{what}: values exceed fp16's range (|x| > 65504 after the index's power-of-two scale): "
                             "rescale them (the device rows are fp16 or fp16 hi|lo pairs)")

    def gather(self, src: PackedRows, ids_dev) -> PackedRows:
        torch = self.torch
        m = int(ids_dev.numel())
        ld = int(src.rows.shape[1])
        rows = torch.empty((m, ld), dtype=torch.float16, device=self.device)
        norms = torch.empty((m,), dtype=torch.float32, device=self.device)
        self._call("lvs_gather_rows", src=_ptr(src.rows), ld=ld, ids=_ptr(ids_dev), n_ids=m, dst=_ptr(rows), stream=self._stream())
        self._call("lvs_gather_f32", _ptr(src.norms), _ptr(ids_dev), m, _ptr(norms), self._stream())
        return PackedRows(rows=rows, norms=norms, n=m, d=src.d, mode=src.mode, exp=src.exp)

    def unpack(self, src: PackedRows, ids_dev=None, raw: bool = False):
        """float32 values [m, d] of the packed rows ``ids_dev`` (all rows when None), as a device tensor - the caller's
        values (pack scale undone); ``raw=True``: the stored values x 2^exp as they are (k-means works on those)."""
        torch = self.torch
        m = src.n if ids_dev is None else int(ids_dev.numel())
        out = torch.empty((m, src.d), dtype=torch.float32, device=self.device)
        self._call("lvs_unpack_rows", src=_ptr(src.rows), d=src.d, pack_mode=src.mode, ids=_ptr(ids_dev), n=m,
                scale_exp=0 if raw else int(src.exp), dst=_ptr(out), stream=self._stream())
        return out

    @staticmethod
    def slice_rows(src: PackedRows, r0: int, r1: int) -> PackedRows:
        """Rows [r0, r1) of a packed matrix (a view: same HBM)."""
        return PackedRows(rows=src.rows[r0:r1], norms=src.norms[r0:r1], n=r1 - r0, d=src.d, mode=src.mode, exp=src.exp)

    # ---- search ----
    CERT_MIN_PAIRS = 1 << 26  # below this many (query, row) pairs the extra launches cost more than the two passes saved
    CERT_MAX_K = 48
    CERT_SPARE_SMALL_K = 5  # spare list slots of the one-pass search for k <= 10 (k1 = k + spare <= 15)
    # largest k served by the 15-slot lists of the 256-query geometry.  fp32 10 k x 1 M, same box (profiles/r06l_fp32_k12_probe.log):
    # k = 11: 15.9 ms (0.4 % of the queries open) against 20.5 ms with k + 8 slots on the 128-query geometry; k = 12: 17.0 (3.8 % open)
    # against 20.6; k = 13: 21.7 (17 % open) against 20.7
    CERT_MAX_K_SMALL_LISTS = 12
    CERT_RJ_MIN_QUERIES = 4097  # from here on the certified search's one pass takes the chunked lvs_rj_kernel path (plain lists)
    CERT_BAND_SEARCH = 2.05   # banded lists: rows further than this many error bounds below the k-th one-pass score are not
    CERT_BAND_CERTIFY = 2.02  # listed; the certificate assumes a slightly narrower band (> 2 is what its proof needs)

    SEED_EXCHANGE_MIN_QUERIES = 2048  # below this a sharded call is too short for an extra collective (see seed_tiles)

    def seed_tiles(self, nq: int, shard_rows: int, k: int, corpus_mode: int, query_mode: int) -> int:
        """Sample tiles every shard of a row-sharded join contributes to the pooled starting thresholds (0: no exchange).
        A function of the arguments only - every rank computes it from the NOMINAL shard size, so all ranks agree on the
        shape of the exchange.  fp32-accurate operands (hi|lo rows) are searched through the certified one-pass path, whose
        certificate reads a short list as "this shard holds no more rows": no pooled thresholds there."""
        if nq < self.SEED_EXCHANGE_MIN_QUERIES or corpus_mode != _capi.PACK_F16 or query_mode != _capi.PACK_F16:
            return 0
        if not 1 <= k <= 56:
            return 0
        return max(0, int(self.lib.lvs_flat_search_seed_tiles(int(nq), int(shard_rows), int(k))))

    def seed_scores(self, corpus: PackedRows, queries: PackedRows, metric: int, tiles: int):
        """-> float32 [tiles, nq]: best score of every query over each of the first ``tiles`` 256-row tiles of this shard
        (``lvs_flat_search_seed_scores``; -inf rows where the shard is shorter)."""
        torch = self.torch
        out = torch.empty((int(tiles), queries.n), dtype=torch.float32, device=self.device)
        if tiles and queries.n:
            self._call("lvs_flat_search_seed_scores", **_operands(corpus, queries), metric=metric, tiles=int(tiles),
                    out_scores=_ptr(out), stream=self._stream())
        return out

    def search_keys(self, corpus: PackedRows, queries: PackedRows, k: int, metric: int, id_offset: int = 0,
                    row_ids=None, one_pass: bool | None = None, stats: dict | None = None, seed_scores=None):
        """-> int64 tensor [nq, k] holding the uint64 result keys (bit pattern).

        ``seed_scores`` (float32 [rows, nq], optional): scores of rows of the WHOLE searched set - the all-gathered
        ``seed_scores`` blocks of every corpus shard - whose k-th largest per query becomes the launch's starting threshold
        (``lvs_flat_search_keys_seeded``); a shard may then return fewer than k keys (key 0 slots).

        fp32-accurate operands (fp16 hi|lo rows) need 2-3 MFMA passes in the plain search.  For large calls with
        k <= 48 the same exact result comes from ONE pass (``one_pass``: None = decide by size, False = never):
        ``lvs_flat_search_keys_hi`` with a few spare list slots, exact rescoring of the candidates, a per-query
        certificate (``lvs_certify_topk``) and the plain search for the few uncertified queries only."""
        torch = self.torch
        if corpus.d != queries.d:
            raise ValueError("corpus / query dimension mismatch")
        if metric == _capi.METRIC_L2 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        split = corpus.mode == _capi.PACK_SPLIT or queries.mode == _capi.PACK_SPLIT
        if one_pass is None:
            one_pass = queries.n * corpus.n >= self.CERT_MIN_PAIRS
        if (one_pass and split and row_ids is None and 1 <= k <= self.CERT_MAX_K and corpus.n >= 4 * (k + 8)
                and queries.n > 0):
            if k == 1:  # the winner + runner-up certificate is the cheaper one-pass form for a single neighbour
                return self.nearest(corpus, queries, metric, id_offset=id_offset, stats=stats)
            return self._search_keys_certified(corpus, queries, k, metric, id_offset, stats)
        if seed_scores is not None and int(seed_scores.shape[0]) > 0:
            if seed_scores.dim() != 2 or int(seed_scores.shape[1]) != queries.n or seed_scores.dtype != torch.float32:
                raise ValueError("seed_scores must be float32 [rows, nq]")
            seed_scores = seed_scores.contiguous()
            return self._search_call("lvs_flat_search_keys_seeded", corpus, queries, k, metric, id_offset, row_ids,
                                     seed_scores=_ptr(seed_scores), seed_rows=int(seed_scores.shape[0]))
        return self._search_call("lvs_flat_search_keys", corpus, queries, k, metric, id_offset, row_ids)

    @staticmethod
    def _cached_max(pk: PackedRows, name: str, compute) -> float:
        """``compute()`` once per device image: the value is cached on the image where it accepts attributes."""
        v = getattr(pk, name, None)
        if v is None:
            v = compute()
            try:
                setattr(pk, name, v)
            except Exception:
                pass
        return v

    def lo_norm_max(self, pk: PackedRows) -> float:
        """Largest |lo part of a row| of a device image (0 for fp16 rows), computed once per image and cached on it."""
        if pk.mode != _capi.PACK_SPLIT or pk.n == 0:
            return 0.0

        def compute():
            torch, dpad = self.torch, int(pk.rows.shape[1]) // 2
            m = torch.zeros((), dtype=torch.float32, device=self.device)
            for r0 in range(0, pk.n, 1 << 18):  # in chunks: the float32 copy of 2^18 x 768 lo parts is 0.8 GB
                m = torch.maximum(m, pk.rows[r0:r0 + (1 << 18), dpad:].float().square().sum(dim=1).max())
            return float(m.sqrt().item())

        return self._cached_max(pk, "_lo_norm_max", compute)

    def row_norm_max(self, pk: PackedRows) -> float:
        """Largest |row| of a device image, computed once per image and cached on it."""
        if pk.n == 0:
            return 0.0
        return self._cached_max(pk, "_row_norm_max", lambda: float(pk.norms.max().sqrt().item()))

    def _search_call(self, name: str, corpus, queries, k, metric, id_offset, row_ids=None, **extra):
        """One flat search (``lvs_flat_search_keys`` / ``_seeded`` / ``_hi`` / ``_hi_banded``) -> keys [nq, k].  ``extra``: what the
        entry declares beyond the plain search (``kc``, ``band_scale``, ``band_slack``; ``seed_scores``, ``seed_rows``)."""
        keys = self.torch.empty((queries.n, k), dtype=self.torch.int64, device=self.device)
        need = int(self.lib.lvs_flat_search_workspace_bytes(queries.n, corpus.n, corpus.d, k, corpus.mode, queries.mode))
        if need < 0:
            raise LotusHipError("the flat search's workspace query rejected the shape")
        ws = self._workspace(need)
        self._call(name, **_operands(corpus, queries), metric=metric, k=k, id_offset=int(id_offset), row_ids=_ptr(row_ids),
                out_keys=_ptr(keys), workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream(), **extra)
        return keys

    def _rescore(self, corpus, queries, metric, id_offset, keys) -> None:
        """Put the exact scores into the keys [nq, k] of every query, in place (one wave per query, HBM-bound)."""
        self._call("lvs_rescore_keys", xb=_ptr(corpus.rows), xb_pack=corpus.mode, xq=_ptr(queries.rows), xq_pack=queries.mode,
                nq=queries.n, d=corpus.d, metric=metric, xb_norms_sq=_ptr(corpus.norms), xq_norms_sq=_ptr(queries.norms),
                id_offset=int(id_offset), k=int(keys.shape[1]), keys=_ptr(keys), stream=self._stream())

    @staticmethod
    def _count(stats: dict | None, **counts) -> None:
        """Add the named counts into ``stats`` (when the caller gave one)."""
        if stats is not None:
            for name, v in counts.items():
                stats[name] = stats.get(name, 0) + v

    def _cert_bound(self, corpus, queries, metric):
        """-> (scale, slack), Python floats (float64): the certified top-k search's error bound is scale |q| + slack."""
        # |s - s_hi| <= |q| |lo_row| + |lo_q| |row| + |lo_q| |lo_row| (Cauchy-Schwarz) with the MEASURED largest lo-part norms
        # E_c, E_q of the two operands (cached per device image; ~0.4 x the worst case 2^-11 |x|, so fewer queries stay open than
        # under round 3's a-priori bound; being measured, they also cover components in fp16's subnormal range), + float32
        # accumulation noise relative to |q| |row|
        R, E_c, E_q = self.row_norm_max(corpus), self.lo_norm_max(corpus), self.lo_norm_max(queries)
        c = 1.0 if metric == _capi.METRIC_IP else 2.0
        scale = c * (E_c * (1.0 + 1e-3) + 8e-6 * R)
        slack = 1e-6 * (2.0 ** (corpus.exp + queries.exp) + R * R) + c * E_q * (R + E_c) * (1.0 + 1e-3)
        return scale, slack

    def _search_keys_certified(self, corpus, queries, k, metric, id_offset, stats, k1=None):
        """Exact top-k of fp32-accurate operands from one MFMA pass (see ``search_keys``).

        The one-pass score of a pair differs from the exact one by at most ``|q| |lo_row| + |lo_q| |row| <= 2^-11 |q| R``
        per split operand (``R`` = largest row norm; every component is rounded to 11 significant bits).  With k1 > k
        list slots, a row that is NOT among a query's k1 candidates has a one-pass score <= the list's last one, so its
        exact score is at most that + the bound; if the k-th EXACT score of the candidates is strictly higher, their
        exact top k is the exact top k."""
        torch = self.torch
        nq = queries.n
        first_round = k1 is None
        if first_round:
            # k <= 12 stays on the 256-query geometry (15 slots): banded lists make spare slots cheap, and the 128-query geometry
            # of deeper lists is 25-45 % slower - a few more open queries for the second round are the smaller price
            k1 = min(15, k + self.CERT_SPARE_SMALL_K) if k <= 10 else (15 if k <= self.CERT_MAX_K_SMALL_LISTS else min(56, k + 8))
        k1 = min(k1, corpus.n)
        scale, slack = self._cert_bound(corpus, queries, metric)
        # BANDED lists: with bound = scale |q| + slack, a row whose one-pass score is more than 2 bound below the k-th best
        # one-pass score cannot reach the exact top k (k-th exact >= k-th one-pass - bound).  So the kernel admits a row only
        # above max(last slot, k-th slot - CERT_BAND_SEARCH x bound): the k1-deep lists then cost the insertions of k-deep
        # ones, and a query stays open only when more than k1 - k rows crowd that band.  The certificate assumes the slightly
        # narrower CERT_BAND_CERTIFY (rounding of the two evaluations of the band can never make it claim too much).
        banded = k1 > k
        # (r6) joins of fp32 embeddings: the one pass over the hi parts runs on the register-resident-queries kernel
        # (lvs_rj_kernel: chunks of <= 32 768 queries, 0.5 instead of 0.43 of the MFMA roof) whenever the shape is its - that kernel
        # has no banded admission, so the lists are plain k1-deep ones (k1 <= 16 there) and the certificate the plain one
        dpad = int(corpus.rows.shape[1]) // (2 if corpus.mode == _capi.PACK_SPLIT else 1)
        if (banded and first_round and k1 <= 16 and nq >= self.CERT_RJ_MIN_QUERIES and corpus.n >= 65536
                and dpad in (256, 384, 512, 768) and corpus.mode == queries.mode == _capi.PACK_SPLIT):
            banded = False
        if banded:
            approx = self._search_call("lvs_flat_search_keys_hi_banded", corpus, queries, k1, metric, id_offset,
                                       kc=k, band_scale=float(self.CERT_BAND_SEARCH * scale),
                                       band_slack=float(self.CERT_BAND_SEARCH * slack))
        else:
            approx = self._search_call("lvs_flat_search_keys_hi", corpus, queries, k1, metric, id_offset)
        exact = approx.clone()
        self._rescore(corpus, queries, metric, id_offset, exact)
        self._call("lvs_sort_keys_desc", _ptr(exact), nq, k1, self._stream())
        idx = torch.empty((nq,), dtype=torch.int64, device=self.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._call("lvs_certify_topk_banded", approx_keys=_ptr(approx), exact_keys=_ptr(exact), q_norms_sq=_ptr(queries.norms), nq=nq,
                k1=k1, k=k, scale=float(scale), slack=float(slack), band=float(self.CERT_BAND_CERTIFY if banded else 0.0),
                out_idx=_ptr(idx), out_count=_ptr(cnt), stream=self._stream())
        keys = exact[:, :k].contiguous()
        n_open = int(cnt.item())
        n_plain = 0
        if n_open:
            sel = idx[:n_open]
            sub = self.gather(queries, sel)
            if first_round and k1 < min(56, corpus.n):
                # second round for the few open queries: the same one-pass search with the longest lists (56 slots) - a row
                # outside a 56-deep list is far below the k-th exact score unless the query sits in a dense tie - before
                # anyone pays the 2-3 segment plain search (1 % of 10 k x 1 M fp32 queries: 1.2 ms of plain search -> 0.4 ms)
                inner = {}
                keys[sel] = self._search_keys_certified(corpus, sub, k, metric, id_offset, inner, k1=56)
                n_plain = inner.get("plain", 0)
            else:
                keys[sel] = self.search_keys(corpus, sub, k, metric, id_offset=id_offset, one_pass=False)
                n_plain = n_open
        if first_round:
            self._count(stats, uncertified=n_open, queries=nq)
        self._count(stats, plain=n_plain)
        return keys

    def nearest(self, corpus: PackedRows, queries: PackedRows, metric: int, id_offset: int = 0, stats: dict | None = None,
                exact_scores: bool = True, corpus_stats=None, bounds=None):
        """Nearest corpus row of every query (k = 1) -> int64 key tensor [nq, 1], same winner as ``search_keys(.., 1, ..)``
        (two rows whose exact scores agree to within float32 rounding may come out in either order: a certified winner needs no
        second look, a PAIR is settled by ``lvs_resolve_pairs``' scalar float32 dot products, an OPEN query by the multi-segment
        MFMA search - three summation orders; ``stats`` counts ``pairs`` and ``open`` separately, ``uncertified`` is their sum).

        fp32-accurate operands (fp16 hi|lo rows) cost two or three MFMA passes in the exact search.  Here ONE pass over
        the hi parts (``lvs_nearest_hi``) gives every query a winner and its margin over the runner-up; the true score
        of a pair differs from the hi-only score by at most |q| |lo_row| + |lo_q| |row| (Cauchy-Schwarz), so a margin
        above twice that bound certifies the winner.  Only the uncertified queries (``lvs_margin_select``: ties,
        near-ties) are searched again exactly.  This is the k-means assignment step (``lotus/utils.py:62,65``) with
        fp32-accurate centroids at the cost of fp16 ones.  ``exact_scores=False`` leaves the one-pass scores inside the
        keys of certified queries (the ids are exact either way) and saves one pass over the queries.  ``corpus_stats``:
        device float32 [2] = (largest |row|^2, largest |lo part of a row|^2) of the corpus as ``kmeans_pack_centroids`` /
        ``kmeans_finish`` leave it - the certificate's bound is then evaluated on the device (no host round trip for it).
        ``bounds``: ``(assign int32, ub float32, lb float32, positions int64 or None)`` device tensors - squared-L2 searches
        only, needs ``corpus_stats``: the rows ``positions`` (None: rows 0..nq) also get their Hamerly bounds from this
        search (``_Bounds.set``): the winner, an upper bound of its distance and a lower bound of the distance to
        every other corpus row, the search's own error bound included."""
        torch = self.torch
        if bounds is not None and (corpus_stats is None or metric != _capi.METRIC_L2):
            raise ValueError("bounds need the squared-L2 metric and the corpus statistics")
        if corpus.mode == _capi.PACK_F16 and queries.mode == _capi.PACK_F16 and bounds is None:
            return self.search_keys(corpus, queries, 1, metric, id_offset=id_offset)  # nothing to certify: already exact
        if corpus.d != queries.d:
            raise ValueError("corpus / query dimension mismatch")
        nq = queries.n
        keys = torch.empty((nq, 1), dtype=torch.int64, device=self.device)
        if nq == 0 or corpus.n == 0:
            return self.search_keys(corpus, queries, 1, metric, id_offset=id_offset, one_pass=False)
        # bound = (coef[0] E + coef[1] R) |q| + coef[2] + coef[3] R + coef[4] R^2 (E = largest lo-part norm, R = largest norm over
        # the corpus rows): derived where the library states it, csrc/lvs_bound.h
        coef, dpad = self._nearest_coef(corpus, queries, metric)
        if bounds is not None:
            bounds = _Bounds(self, bounds, corpus_stats, coef, id_offset)
        if corpus.n <= _capi.NEAREST3_MAX_ROWS:
            # a small corpus (k-means centroids): queries streaming past resident corpus tiles + the two-candidate certificate.
            # Its scratch is 20 B per (corpus tile, query): the queries go through in chunks that keep it below a fixed budget
            # (10 M rows x 16 384 centroids would ask for 12.8 GB in one call - ADVICE r04); results are per query, so
            # chunking changes nothing.  Every chunk is begun AND finished before the next (one chunk's tensors alive at a time)
            for q0, q1, qs, bs in self._nearest3_chunks(corpus, queries, bounds):
                part = self._nearest3_finish(
                    self._nearest3_begin(corpus, qs, metric, id_offset, exact_scores, corpus_stats, bs, coef, dpad), stats)
                if q1 - q0 == nq:
                    return part
                keys[q0:q1] = part
            return keys
        if corpus_stats is None:
            R = float(corpus.norms.max().sqrt().item())
            E = self.lo_norm_max(corpus)
            scale = coef[0] * E + coef[1] * R
            slack = coef[2] + coef[3] * R + coef[4] * R * R
        sec = torch.empty((nq,), dtype=torch.float32, device=self.device)
        need = int(self.lib.lvs_nearest_hi_workspace_bytes(nq, corpus.n, corpus.d))
        ws = self._workspace(need)
        self._call("lvs_nearest_hi", **_operands(corpus, queries), metric=metric, id_offset=int(id_offset), out_keys=_ptr(keys),
                out_second=_ptr(sec), workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream())
        idx = torch.empty((nq,), dtype=torch.int64, device=self.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=self.device)
        if corpus_stats is None:
            self._call("lvs_margin_select", keys=_ptr(keys), second=_ptr(sec), q_norms_sq=_ptr(queries.norms), nq=nq,
                    scale=float(scale), slack=float(slack), out_idx=_ptr(idx), out_count=_ptr(cnt), stream=self._stream())
        else:
            coef5 = (ctypes.c_float * 5)(*coef)
            self._call("lvs_margin_select_stats", keys=_ptr(keys), second=_ptr(sec), q_norms_sq=_ptr(queries.norms), nq=nq,
                    corpus_stats=_ptr(corpus_stats), coef5=ctypes.addressof(coef5), out_idx=_ptr(idx), out_count=_ptr(cnt),
                    stream=self._stream())
        if bounds is not None:  # every row's bounds from the one-pass result first; the uncertified rows are redone below
            bounds.set(keys, sec, queries.norms, nq)
        n_open = int(cnt.item())  # the call's one host round trip: the exact search below is sized by it
        # the winners are certified, their scores are still the one-pass approximations: put the exact scores in
        # (one HBM-bound pass over the queries; the k-means objective sums them)
        if exact_scores:
            self._rescore(corpus, queries, metric, id_offset, keys)
        if n_open:
            sel = idx[:n_open]
            sub = self.gather(queries, sel)
            exact_keys = self.search_keys(corpus, sub, 1, metric, id_offset=id_offset, one_pass=False)  # with or without bounds
            if bounds is not None:
                bounds.fix(keys[sel].contiguous(), exact_keys, sub.norms, sel)
            keys[sel] = exact_keys
        self._count(stats, uncertified=n_open, queries=nq)
        return keys

    @staticmethod
    def _nearest_coef(corpus, queries, metric):
        """-> (the five coefficients of the one-pass error bound, stated in ``csrc/lvs_bound.h``, dpad).  Needs no device."""
        coef5 = (ctypes.c_float * 5)()
        _capi.check(_capi.load().lvs_nearest_bound_coef(int(metric), queries.mode, corpus.d, corpus.exp + queries.exp,
                                                        ctypes.addressof(coef5)), "lvs_nearest_bound_coef")
        return list(coef5), int(corpus.rows.shape[1]) // (2 if corpus.mode == _capi.PACK_SPLIT else 1)

    def _nearest3_step(self, corpus) -> int:
        """Most queries one ``lvs_nearest3`` call may take inside the scratch budget (20 B per corpus tile and query)."""
        per_q = max(1, int(self.lib.lvs_nearest3_workspace_bytes(1 << 20, corpus.n, corpus.d)) >> 20)
        return max(1 << 16, (self.NEAREST3_WS_BUDGET // per_q) >> 16 << 16)

    def _nearest3_chunks(self, corpus, queries, bounds):
        """The queries in chunks of ``_nearest3_step``: yields (q0, q1, queries [q0, q1), the bounds of those queries).  Queries
        that fit one call come back as they are."""
        step = self._nearest3_step(corpus)
        if queries.n <= step:
            yield 0, queries.n, queries, bounds
            return
        for q0 in range(0, queries.n, step):
            q1 = min(queries.n, q0 + step)
            yield q0, q1, self.slice_rows(queries, q0, q1), (None if bounds is None else bounds.of_queries(q0, q1))

    def _nearest3_begin(self, corpus, queries, metric, id_offset, exact_scores, corpus_stats, bounds, coef, dpad):
        """``nearest`` for a corpus of at most 16 384 rows (``lvs_nearest3``): the one-pass search also returns the runner-up's
        id and the THIRD score, so a query whose best-second margin is inside the error bound but whose best-third margin is
        not has only two possible winners - two exact dot products (``lvs_resolve_pairs``) decide it instead of an exact
        search over every row; only queries with three or more rows inside the bound take that search.  The three-way split
        depends on a query's own scores and the corpus alone, never on which other queries share the call.

        Launches only: the one-pass search and the three-way split; nothing is read back.  -> handle for ``_nearest3_finish``
        (which may run on another stream once these launches are done - ``nearest_begin`` / ``nearest_finish``)."""
        torch = self.torch
        nq = queries.n
        if corpus_stats is None:  # (largest |row|^2, largest |lo part|^2) of the corpus, left on the device
            E2 = (corpus.rows[:, dpad:].float().square().sum(dim=1).max() if corpus.mode == _capi.PACK_SPLIT
                  else torch.zeros((), dtype=torch.float32, device=self.device))
            corpus_stats = torch.stack([corpus.norms.max(), E2]).to(torch.float32)
        i64 = dict(dtype=torch.int64, device=self.device)
        keys, keys2 = torch.empty((nq, 1), **i64), torch.empty((nq,), **i64)
        sec, third = (torch.empty((nq,), dtype=torch.float32, device=self.device) for _ in range(2))
        need = int(self.lib.lvs_nearest3_workspace_bytes(nq, corpus.n, corpus.d))
        if need < 0:
            raise LotusHipError("lvs_nearest3_workspace_bytes rejected the shape")
        ws = self._workspace(need)
        self._call("lvs_nearest3", **_operands(corpus, queries), metric=metric, id_offset=int(id_offset), out_keys=_ptr(keys),
                out_keys2=_ptr(keys2), out_second=_ptr(sec), out_third=_ptr(third), workspace=_ptr(ws),
                workspace_bytes=int(ws.numel()), stream=self._stream())
        pair_idx, open_idx, counts = torch.empty((nq,), **i64), torch.empty((nq,), **i64), torch.zeros((2,), **i64)
        coef5 = (ctypes.c_float * 5)(*coef)
        self._call("lvs_nearest3_select", keys=_ptr(keys), keys2=_ptr(keys2), second=_ptr(sec), third=_ptr(third),
                q_norms_sq=_ptr(queries.norms), nq=nq, corpus_stats=_ptr(corpus_stats), coef5=ctypes.addressof(coef5),
                out_pair_idx=_ptr(pair_idx), out_open_idx=_ptr(open_idx), out_counts=_ptr(counts), stream=self._stream())
        if bounds is not None:  # every row's bounds from the one-pass result first; the uncertified rows are redone below
            bounds.set(keys, sec, queries.norms, nq)
        return _NearestHandle(queries=queries, corpus=corpus, metric=metric, id_offset=id_offset, exact_scores=exact_scores,
                              bounds=bounds, keys=keys, keys2=keys2, pair_idx=pair_idx, open_idx=open_idx, counts=counts)

    def _nearest3_finish(self, h, stats):
        """The call's one host round trip (how many queries are pairs / open) and what follows from it: two exact dot products
        for the pairs, the exact search for the open queries.  -> keys [nq, 1]."""
        corpus, queries, metric, id_offset, bounds, keys = h.corpus, h.queries, h.metric, h.id_offset, h.bounds, h.keys
        pair_idx, open_idx = h.pair_idx, h.open_idx
        n_pair, n_open = (int(v) for v in h.counts.tolist())  # the call's one host round trip
        psel = pair_idx[:n_pair]
        # the one-pass keys of the rows decided below, as the bounds' fix needs them (taken before any exact score goes in)
        approx_pair = keys[psel].contiguous() if (bounds is not None and n_pair) else None
        approx_open = keys[open_idx[:n_open]].contiguous() if (bounds is not None and n_open) else None
        if h.exact_scores:
            self._rescore(corpus, queries, metric, id_offset, keys)
        if n_pair:
            self._call("lvs_resolve_pairs", xb=_ptr(corpus.rows), xb_pack=corpus.mode, xq=_ptr(queries.rows), xq_pack=queries.mode,
                    d=corpus.d, metric=metric, xb_norms_sq=_ptr(corpus.norms), xq_norms_sq=_ptr(queries.norms),
                    id_offset=int(id_offset), pair_idx=_ptr(pair_idx), pair_count=_ptr(h.counts), capacity=n_pair, keys=_ptr(keys),
                    keys2=_ptr(h.keys2), stream=self._stream())
            if bounds is not None:
                bounds.fix(approx_pair, keys[psel].contiguous(), queries.norms[psel].contiguous(), psel)
        if n_open:
            sel = open_idx[:n_open]
            sub = self.gather(queries, sel)
            exact_keys = self.search_keys(corpus, sub, 1, metric, id_offset=id_offset, one_pass=False)
            if bounds is not None:
                bounds.fix(approx_open, exact_keys, sub.norms, sel)
            keys[sel] = exact_keys
        self._count(stats, uncertified=n_open + n_pair, pairs=n_pair, open=n_open, queries=queries.n)
        return keys

    def nearest_begin(self, corpus: PackedRows, queries: PackedRows, metric: int, id_offset: int = 0, exact_scores: bool = True,
                      corpus_stats=None):
        """``nearest`` in two halves, for callers that keep the launch stream busy: ``nearest_begin`` queues the one-pass search and
        the certificate's three-way split and returns at once (no host round trip); ``nearest_finish(handle)`` - on this or on
        another stream that waits for an event recorded after ``nearest_begin`` - reads the two counts and queues the exact work
        for the uncertified queries.  Same launches, same arithmetic, same keys as ``nearest``.  Keep the handle alive until the
        stream ``nearest_finish`` ran on has been joined (its tensors were allocated on the stream of ``nearest_begin``)."""
        small = corpus.n <= _capi.NEAREST3_MAX_ROWS and not (corpus.mode == _capi.PACK_F16 and queries.mode == _capi.PACK_F16)
        if not small or queries.n == 0 or corpus.n == 0 or corpus.d != queries.d:
            return _NearestHandle(queries=queries, done=self.nearest(corpus, queries, metric, id_offset=id_offset,
                                                                     exact_scores=exact_scores, corpus_stats=corpus_stats))
        coef, dpad = self._nearest_coef(corpus, queries, metric)
        # the same scratch budget as nearest() (a 3 M-row range x 16 384 centroids asked for 3.8 GB in one call):
        # the queries go through in chunks, one handle each; the launches of chunk i + 1 reuse the stream's scratch behind chunk
        # i's (same stream: ordered)
        chunks = [(q0, q1, self._nearest3_begin(corpus, qs, metric, id_offset, exact_scores, corpus_stats, None, coef, dpad))
                  for q0, q1, qs, _ in self._nearest3_chunks(corpus, queries, None)]
        return chunks[0][2] if len(chunks) == 1 else _NearestHandle(queries=queries, chunks=chunks)

    def nearest_finish(self, handle, stats: dict | None = None):
        if handle.done is not None:
            self._count(stats, queries=handle.queries.n)
            return handle.done
        if handle.chunks is None:
            return self._nearest3_finish(handle, stats)
        keys = self.torch.empty((handle.queries.n, 1), dtype=self.torch.int64, device=self.device)
        for q0, q1, h in handle.chunks:
            keys[q0:q1] = self._nearest3_finish(h, stats)
        return keys

    def kmeans_centroid_shift(self, c_old, c_new):
        """-> (delta float32 [k], top2 float32 [3]): how far every centroid moved, the largest and second largest shift."""
        torch = self.torch
        k, d = int(c_new.shape[0]), int(c_new.shape[1])
        delta = torch.empty((k,), dtype=torch.float32, device=self.device)
        top2 = torch.empty((3,), dtype=torch.float32, device=self.device)
        self._call("lvs_kmeans_centroid_shift", c_old=_ptr(c_old), c_new=_ptr(c_new), k=k, d=d, out_delta=_ptr(delta),
                out_top2=_ptr(top2), stream=self._stream())
        return delta, top2

    def kmeans_bounds_step(self, assign, ub, lb, delta, top2):
        """Move the bounds by the centroid shifts; -> int64 device tensor of the rows that need a new search."""
        torch = self.torch
        n = int(assign.numel())
        idx = torch.empty((n,), dtype=torch.int64, device=self.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._call("lvs_kmeans_bounds_step", assign=_ptr(assign), ub=_ptr(ub), lb=_ptr(lb), delta=_ptr(delta), top2=_ptr(top2), n=n,
                out_idx=_ptr(idx), out_count=_ptr(cnt), stream=self._stream())
        return idx[:int(cnt.item())]

    def search_sharded(self, shard: PackedRows, queries: PackedRows, k: int, metric: int, id_offset: int, world: int,
                       seed_tiles: int, all_gather):
        """This rank's share of a row-sharded search with the exchange steps run INSIDE the C ABI (``lvs_search_sharded``, ABI 6):
        sample scores -> all-gather -> seeded shard search -> all-gather of the key lists -> merge, all enqueued on the current
        stream.  ``all_gather``: callable(device uint8 tensor [n]) -> device uint8 tensor [world, n] (rank order), called by the
        library for its two exchanges - ``lotus_amd._dist.all_gather_rows`` over any ``torch.distributed`` backend.  (A host with
        an ``ncclComm_t`` of its own calls ``lvs_search_sharded_rccl`` and needs no callback at all.)  -> int64 keys [nq, k],
        identical on every rank and equal to what ``search_keys`` + ``merge_keys`` give."""
        torch = self.torch
        nq = queries.n
        if shard.d != queries.d:
            raise ValueError("corpus / query dimension mismatch")
        errors = []

        def transport(_ctx, send, recv, nbytes, _stream):
            try:  # the library's stream is torch's current stream (self._stream()): torch work queued here stays in order
                src = torch.as_tensor(_DevBytes(send, nbytes), device=self.device)
                out = all_gather(src)
                torch.as_tensor(_DevBytes(recv, world * nbytes), device=self.device).copy_(out.reshape(-1))
                return 0
            except Exception as e:  # noqa: BLE001 - reported through the status code
                errors.append(e)
                return _capi.EDEVICE

        cb = _capi.CALLBACKS["lvs_all_gather_fn"](transport)
        need = int(self.lib.lvs_search_sharded_workspace_bytes(world, nq, shard.n, shard.d, k, shard.mode, queries.mode,
                                                               int(seed_tiles)))
        if need < 0:
            raise LotusHipError("lvs_search_sharded_workspace_bytes rejected the shape")
        ws = self._workspace(need)
        keys = torch.zeros((nq, k), dtype=torch.int64, device=self.device)
        try:
            self._call("lvs_search_sharded", all_gather=ctypes.cast(cb, ctypes.c_void_p), all_gather_ctx=None, nranks=world,
                    xb=_ptr(shard.rows) if shard.n else None, xb_pack=shard.mode, nb_local=shard.n, xq=_ptr(queries.rows),
                    xq_pack=queries.mode, nq=nq, d=shard.d, metric=metric, k=k, xb_norms_sq=_ptr(shard.norms) if shard.n else None,
                    xq_norms_sq=_ptr(queries.norms), id_offset=int(id_offset), seed_tiles=int(seed_tiles), out_keys=_ptr(keys),
                    workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream())
        except LotusHipError:  # the library hands back the status its all-gather returned: what the callback raised is the cause
            if errors:
                raise errors[0]
            raise
        return keys

    # ---- IVF-Flat ----
    IVF_ASSIGN_CHUNK_ROWS = 262144  # rows assigned to their list per search call while the lists are built

    def ivf_build(self, packed: PackedRows, centroids, metric: int, offsets=None, rows=None) -> IvfLists:
        """Inverted lists of ``packed`` around ``centroids`` (float32 [nlist, d], the caller's units).  Every row goes to its
        best centroid under ``metric`` (faiss's IVF quantizer: an ``IndexFlatIP`` / ``IndexFlatL2`` over the centroids; ties
        to the lower list id), then a stable counting sort groups the row numbers by list (``lvs_ivf_build_lists``).  The
        image itself is not copied.  ``offsets`` / ``rows`` (host arrays): lists built before (a persisted sidecar) - only
        uploaded."""
        torch = self.torch
        c = centroids if torch.is_tensor(centroids) else np.ascontiguousarray(centroids, dtype=np.float32)
        nlist = int(c.shape[0])
        cpk = self.pack(c, packed.mode, exp=int(packed.exp))
        if offsets is not None:
            return IvfLists(centroids=cpk, offsets=self.to_device(np.asarray(offsets, dtype=np.int64)),
                            rows=self.to_device(np.asarray(rows, dtype=np.uint32).view(np.int32)), nlist=nlist, metric=metric)
        n = packed.n
        assign = torch.empty((n,), dtype=torch.int64, device=self.device)
        step = self.IVF_ASSIGN_CHUNK_ROWS
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            keys = self.search_keys(cpk, self.slice_rows(packed, r0, r1), 1, metric).reshape(-1)
            assign[r0:r1] = 0xFFFFFFFF - (keys & 0xFFFFFFFF)
        off = torch.empty((nlist + 1,), dtype=torch.int64, device=self.device)
        out_rows = torch.empty((n,), dtype=torch.int32, device=self.device)
        need = int(self.lib.lvs_ivf_build_workspace_bytes(n, nlist))
        if need < 0:
            raise LotusHipError("lvs_ivf_build_workspace_bytes rejected the shape")
        ws = self._workspace(need)
        self._call("lvs_ivf_build_lists", assign=_ptr(assign), n=n, nlist=nlist, out_offsets=_ptr(off), out_rows=_ptr(out_rows),
                workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream())
        return IvfLists(centroids=cpk, offsets=off, rows=out_rows, nlist=nlist, metric=metric)

    def ivf_fits(self, d: int, k: int, mode: int) -> bool:
        """Can the list scan serve queries of dimension ``d`` packed with ``mode`` at this ``k``?  It keeps a tile's queries
        in LDS, which bounds d (``lvs_ivf_search_workspace_bytes`` answers LVS_EUNSUPPORTED beyond); callers search the other
        shapes exactly."""
        return ivf_fits(d, k, mode)

    def row_bitmap(self, ids, n: int):
        """-> (device uint32 tensor [ceil(n / 32)], distinct ids): the row selector of the three ``sel=`` searches.  Row r
        is selected iff bit ``r & 31`` of word ``r >> 5`` is set; bits at or past ``n`` are clear.  ``ids``: host int64 row
        numbers in [0, n), any order, duplicates allowed (the count is of distinct rows).  Built on the host - a boolean mask
        packed little-endian, 125 KB per million rows to upload, far less than the ids - so the count needs no device sync."""
        mask = np.zeros(-(-int(n) // 32) * 32, dtype=bool)
        mask[np.asarray(ids, dtype=np.int64).reshape(-1)] = True
        words = np.packbits(mask, bitorder="little").view(np.uint32)  # (a little-endian host: byte 0 is bits 0-7 of word 0)
        return self.to_device(words), int(mask.sum())

    def ivf_search(self, corpus: PackedRows, lists: IvfLists, queries: PackedRows, k: int, metric: int, nprobe: int,
                   want_probe: bool = False, sel=None):
        """-> int64 key tensor [nq, k] (and, ``want_probe``, int32 [nq, nprobe] list ids of the probes, best first): the exact
        top k over the rows of each query's ``nprobe`` best lists (``lvs_ivf_search_keys``); key 0 past those rows.  ``sel``
        (``row_bitmap``'s tensor): only the selected rows of those lists take part (``lvs_ivf_search_keys_sel``)."""
        need = self.lib.lvs_ivf_search_workspace_bytes(queries.n, lists.nlist, nprobe, corpus.d, k, queries.mode)
        return self._ivf_search("lvs_ivf_search", need, corpus, lists, queries, k, metric, nprobe, want_probe, sel,
                                xb=_ptr(corpus.rows), xb_pack=corpus.mode, xb_norms_sq=_ptr(corpus.norms))

    def _ivf_search(self, entry: str, need: int, corpus: PackedRows, lists: IvfLists, queries: PackedRows, k: int, metric: int,
                    nprobe: int, want_probe: bool, sel=None, **mode):
        """What the three IVF searches share: ``<entry>_keys`` on ``need`` bytes of scratch, the answer of its
        ``<entry>_workspace_bytes``.  ``mode``: the parameters only this mode's entry declares.  ``sel``: a row selector - the
        call goes to ``<entry>_keys_sel``, which takes it as ``sel_bits``."""
        torch = self.torch
        if metric == _capi.METRIC_L2 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        nq, cpk = queries.n, lists.centroids
        keys = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        probe = torch.empty((nq, nprobe), dtype=torch.int32, device=self.device) if want_probe else None
        if need < 0:
            m = f" M={mode['M']}" if "M" in mode else ""
            raise LotusHipError(f"{entry}_workspace_bytes rejected nq={nq} nlist={lists.nlist} nprobe={nprobe}{m} k={k}")
        ws = self._workspace(int(need))
        name = entry + "_keys"
        if sel is not None:
            if int(sel.numel()) != -(-corpus.n // 32):
                raise ValueError(f"the row selector has {int(sel.numel())} words for {corpus.n} rows")
            name, mode["sel_bits"] = name + "_sel", _ptr(sel)
        self._call(name, offsets=_ptr(lists.offsets), rows=_ptr(lists.rows), nb=corpus.n, nlist=lists.nlist, centroids=_ptr(cpk.rows),
                c_pack=cpk.mode, c_norms_sq=_ptr(cpk.norms), xq=_ptr(queries.rows), xq_pack=queries.mode, nq=nq,
                xq_norms_sq=_ptr(queries.norms), d=corpus.d, metric=metric, nprobe=int(nprobe), k=int(k), out_keys=_ptr(keys),
                out_probe=_ptr(probe), workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream(), **mode)
        return (keys, probe) if want_probe else keys

    # ---- threshold search through the lists ----
    IVF_RANGE_CHUNK_ROWS = 65536  # query rows per C call, each with its own pair buffer (as RANGE_CHUNK_ROWS)

    def ivf_range_fits(self, d: int, mode: int) -> bool:
        """Can ``lvs_ivf_range_kernel`` serve queries of dimension ``d`` packed with ``mode``?  Its LDS image holds a tile's
        queries and no lists, so the bound is wider than ``ivf_fits``'s; callers join the other shapes exactly."""
        return ivf_range_fits(d, mode)

    def ivf_range_search(self, corpus: PackedRows, lists: IvfLists, queries: PackedRows, threshold: float, metric: int,
                         nprobe: int, q_rows=None, sel=None, capacity: int = 1 << 22):
        """All (query, row, score) with score > threshold over the rows of each query's ``nprobe`` best lists
        (``lvs_ivf_range_search``): three device tensors (int64, int64, float32), order unspecified.  The score is the inner
        product or minus the squared distance, exact whatever codes the store keeps.  ``q_rows`` (device int32 tensor holding
        uint32 row numbers, [nq]): query i is that row and is not paired with it.  ``sel``: ``row_bitmap``'s selector.

        The queries go through in chunks with ``range_join``'s count-then-rerun protocol: a chunk that counted more than
        ``capacity`` pairs - and only that chunk - runs again with buffers of the counted size."""
        torch = self.torch
        if metric == _capi.METRIC_L2 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        if sel is not None and int(sel.numel()) != -(-corpus.n // 32):
            raise ValueError(f"the row selector has {int(sel.numel())} words for {corpus.n} rows")
        if q_rows is not None and int(q_rows.numel()) != queries.n:
            raise ValueError(f"q_rows names {int(q_rows.numel())} rows for {queries.n} queries")
        cpk = lists.centroids
        step = self.IVF_RANGE_CHUNK_ROWS
        outs = []
        cnt = torch.zeros((1,), dtype=torch.int64, device=self.device)
        oq = oj = os_ = None
        for c0 in range(0, queries.n, step):
            c1 = min(queries.n, c0 + step)
            qs = self.slice_rows(queries, c0, c1)
            need = int(self.lib.lvs_ivf_range_workspace_bytes(qs.n, lists.nlist, int(nprobe), corpus.d, qs.mode))
            if need < 0:
                raise LotusHipError(f"lvs_ivf_range_workspace_bytes rejected nq={qs.n} nlist={lists.nlist} nprobe={nprobe} "
                                    f"d={corpus.d}")
            ws = self._workspace(need)
            cap = int(capacity)
            while True:
                if oq is None or oq.numel() < cap:
                    oq = torch.empty((cap,), dtype=torch.int64, device=self.device)
                    oj = torch.empty((cap,), dtype=torch.int64, device=self.device)
                    os_ = torch.empty((cap,), dtype=torch.float32, device=self.device)
                cnt.zero_()
                self._call("lvs_ivf_range_search", **_operands(corpus, qs), offsets=_ptr(lists.offsets), rows=_ptr(lists.rows),
                        sel_bits=_ptr(sel), nlist=lists.nlist, centroids=_ptr(cpk.rows), c_pack=cpk.mode, c_norms_sq=_ptr(cpk.norms),
                        q_rows=_ptr(q_rows[c0:c1]) if q_rows is not None else None, metric=metric, nprobe=int(nprobe),
                        threshold=float(threshold), score_exp=self.score_exp_of(corpus, qs), capacity=cap, out_q=_ptr(oq),
                        out_j=_ptr(oj), out_s=_ptr(os_), out_count=_ptr(cnt), workspace=_ptr(ws), workspace_bytes=int(ws.numel()),
                        stream=self._stream())
                n = int(cnt.item())
                if n <= cap:
                    break
                cap = n  # counted but not stored: size the buffers and run this chunk again
            if n:
                outs.append((oq[:n] + c0, oj[:n].clone(), os_[:n].clone()))
        if not outs:
            e = torch.empty((0,), dtype=torch.int64, device=self.device)
            return e, e.clone(), torch.empty((0,), dtype=torch.float32, device=self.device)
        return (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), torch.cat([o[2] for o in outs]))

    # ---- IVF-SQ8 ----
    SQ8_TRAIN_CHUNK_ROWS = 65536  # training rows unpacked at a time while the residual ranges are taken

    def _list_of_rows(self, lists: IvfLists, n: int):
        """int64 [n]: the list of every row (-1 for rows in no list)."""
        torch = self.torch
        sizes = lists.offsets[1:] - lists.offsets[:-1]
        lid = torch.repeat_interleave(torch.arange(lists.nlist, device=self.device), sizes)
        out = torch.full((n,), -1, dtype=torch.int64, device=self.device)
        out[lists.rows.to(torch.int64) & 0xFFFFFFFF] = lid
        return out

    def _train_residuals(self, packed: PackedRows, lists: IvfLists, ids_dev):
        """float32 [len(ids_dev), d], stored scale: the residuals x - c_l of the rows ``ids_dev`` against their lists' centroids."""
        c = self.unpack(lists.centroids, raw=True)
        return self.unpack(packed, ids_dev, raw=True) - c[self._list_of_rows(lists, packed.n)[ids_dev]]

    def ivf_sq8_train(self, packed: PackedRows, lists: IvfLists, train_ids):
        """-> (vmin, vdiff) float32 [d] device tensors in the stored scale: per-dimension range of the residuals x - c_l of the
        training rows ``train_ids`` (host int64; faiss trains the scalar quantizer on the coarse quantizer's training set)."""
        torch = self.torch
        ids = np.asarray(train_ids, dtype=np.int64)
        vmin = torch.full((packed.d,), float("inf"), dtype=torch.float32, device=self.device)
        vmax = torch.full((packed.d,), float("-inf"), dtype=torch.float32, device=self.device)
        for r0 in range(0, len(ids), self.SQ8_TRAIN_CHUNK_ROWS):
            r = self._train_residuals(packed, lists, self.to_device(ids[r0:r0 + self.SQ8_TRAIN_CHUNK_ROWS]))
            vmin = torch.minimum(vmin, r.amin(dim=0))
            vmax = torch.maximum(vmax, r.amax(dim=0))
        return vmin, vmax - vmin

    def ivf_sq8_encode(self, packed: PackedRows, lists: IvfLists, vmin, vdiff, codes=None, rnorm=None) -> IvfSq8Lists:
        """Codes of every list position (``lvs_ivf_sq8_encode``).  ``codes`` / ``rnorm`` (host arrays, list order, codes
        [n, d]): encoded before (a persisted sidecar) - only uploaded."""
        torch = self.torch
        d = packed.d
        ldc = -(-d // 64) * 64
        vmin = torch.as_tensor(np.asarray(vmin, np.float32) if not torch.is_tensor(vmin) else vmin, device=self.device)
        vdiff = torch.as_tensor(np.asarray(vdiff, np.float32) if not torch.is_tensor(vdiff) else vdiff, device=self.device)
        c = self.unpack(lists.centroids, raw=True).contiguous()
        n = int(lists.rows.numel())
        if codes is not None:
            out = torch.zeros((n, ldc), dtype=torch.uint8, device=self.device)
            out[:, :d] = self.to_device(np.ascontiguousarray(codes, dtype=np.uint8))
            rn = self.to_device(np.ascontiguousarray(rnorm, dtype=np.float32))
        else:
            out = torch.empty((n, ldc), dtype=torch.uint8, device=self.device)
            rn = torch.empty((n,), dtype=torch.float32, device=self.device)
            self._call("lvs_ivf_sq8_encode", xb=_ptr(packed.rows), xb_pack=packed.mode, n=n, d=d, offsets=_ptr(lists.offsets),
                    rows=_ptr(lists.rows), nlist=lists.nlist, centroids=_ptr(c), vmin=_ptr(vmin), vdiff=_ptr(vdiff),
                    out_codes=_ptr(out), out_residual_norms_sq=_ptr(rn), stream=self._stream())
        return IvfSq8Lists(vmin=vmin.contiguous(), vdiff=vdiff.contiguous(), centroids=c, codes=out, rnorm=rn,
                           exp=int(packed.exp))

    def ivf_sq8_fits(self, d: int, k: int, mode: int) -> bool:
        """Can the SQ8 list scan serve queries of dimension ``d`` at this ``k``?  Its LDS image bounds d (d <= 2368);
        callers search the other shapes exactly."""
        return ivf_sq8_fits(d, k, mode)

    def ivf_sq8_search(self, corpus: PackedRows, lists: IvfLists, sq8: IvfSq8Lists, queries: PackedRows, k: int, metric: int,
                       nprobe: int, want_probe: bool = False, sel=None):
        """-> int64 key tensor [nq, k] (and, ``want_probe``, int32 [nq, nprobe] probes): the top k of the DECODED rows of each
        query's ``nprobe`` best lists (``lvs_ivf_sq8_search_keys``); key 0 past those rows.  ``sel``: as ``ivf_search``."""
        need = self.lib.lvs_ivf_sq8_search_workspace_bytes(queries.n, lists.nlist, nprobe, corpus.d, k, queries.mode)
        return self._ivf_search("lvs_ivf_sq8_search", need, corpus, lists, queries, k, metric, nprobe, want_probe, sel,
                                codes=_ptr(sq8.codes), residual_norms_sq=_ptr(sq8.rnorm), vmin=_ptr(sq8.vmin), vdiff=_ptr(sq8.vdiff),
                                centroids_f32=_ptr(sq8.centroids))

    # ---- IVF-PQ ----
    PQ_SEED = 1234          # faiss's ClusteringParameters default, the same for every subspace
    PQ_NITER = 25           # faiss's ProductQuantizer training defaults
    PQ_MAX_POINTS_PER_CENTROID = 256

    def ivf_pq_train(self, packed: PackedRows, lists: IvfLists, train_ids, M: int):
        """-> codebooks float32 [M, ksub, d / M] device tensor in the stored scale: per subspace one k-means (squared L2,
        ``ksub = min(256, training rows)`` centroids, 25 iterations, fixed seed) over the sub-vectors of the residuals x - c_l
        of the training rows ``train_ids`` (host int64).  The subsample of 256 points per centroid is drawn once, as every
        subspace's k-means would draw it with the same seed."""
        from . import cluster

        torch = self.torch
        d = packed.d
        dsub = d // M
        ids = np.asarray(train_ids, dtype=np.int64)
        ksub = min(256, len(ids))
        cap = ksub * self.PQ_MAX_POINTS_PER_CENTROID
        if len(ids) > cap:
            ids = ids[self.rand_perm(len(ids), self.PQ_SEED, cap)]
        r = self._train_residuals(packed, lists, self.to_device(ids)).cpu().numpy()
        books = np.empty((M, ksub, dsub), np.float32)
        for m in range(M):
            res = cluster.kmeans(np.ascontiguousarray(r[:, m * dsub:(m + 1) * dsub]), ksub, niter=self.PQ_NITER,
                                 seed=self.PQ_SEED, max_points_per_centroid=self.PQ_MAX_POINTS_PER_CENTROID, backend=self,
                                 final_assign=False)
            books[m] = res.centroids
        return torch.as_tensor(books, device=self.device)

    def ivf_pq_encode(self, packed: PackedRows, lists: IvfLists, codebooks, codes=None, beta=None) -> IvfPqLists:
        """Codes of every list position (``lvs_ivf_pq_encode``) against ``codebooks`` [M, ksub, dsub] (stored scale).
        ``codes`` / ``beta`` (host arrays, list order, codes [n, M]): encoded before (a persisted sidecar) - only uploaded."""
        torch = self.torch
        d = packed.d
        books = codebooks if torch.is_tensor(codebooks) else torch.as_tensor(np.asarray(codebooks, np.float32))
        books = books.to(device=self.device, dtype=torch.float32).contiguous()
        if books.ndim != 3 or books.shape[0] < 1 or d % books.shape[0] != 0 or books.shape[2] != d // books.shape[0]:
            raise ValueError(f"codebooks of shape {tuple(books.shape)} do not split d={d} into equal subspaces")
        M, ksub = int(books.shape[0]), int(books.shape[1])
        if not 1 <= ksub <= 256:
            raise ValueError(f"ksub={ksub} must be in [1, 256] (8-bit codes)")
        ldc = -(-M // 16) * 16
        c = self.unpack(lists.centroids, raw=True).contiguous()
        n = int(lists.rows.numel())
        if codes is not None:
            out = torch.zeros((n, ldc), dtype=torch.uint8, device=self.device)
            out[:, :M] = self.to_device(np.ascontiguousarray(codes, dtype=np.uint8))
            bt = self.to_device(np.ascontiguousarray(beta, dtype=np.float32))
        else:
            out = torch.empty((n, ldc), dtype=torch.uint8, device=self.device)
            bt = torch.empty((n,), dtype=torch.float32, device=self.device)
            self._call("lvs_ivf_pq_encode", xb=_ptr(packed.rows), xb_pack=packed.mode, n=n, d=d, offsets=_ptr(lists.offsets),
                    rows=_ptr(lists.rows), nlist=lists.nlist, centroids=_ptr(c), M=M, ksub=ksub, codebooks=_ptr(books),
                    out_codes=_ptr(out), out_beta=_ptr(bt), stream=self._stream())
        return IvfPqLists(M=M, ksub=ksub, codebooks=books, centroids=c, codes=out, beta=bt, exp=int(packed.exp))

    def ivf_pq_fits(self, d: int, M: int, k: int, mode: int) -> bool:
        """Can the PQ list scan serve this shape?  Its LDS image (one query's fp32 table, M KB) bounds M (M <= 159);
        callers search the other shapes exactly."""
        return ivf_pq_fits(d, M, k, mode)

    def ivf_pq_search(self, corpus: PackedRows, lists: IvfLists, pq: IvfPqLists, queries: PackedRows, k: int, metric: int,
                      nprobe: int, want_probe: bool = False, sel=None):
        """-> int64 key tensor [nq, k] (and, ``want_probe``, int32 [nq, nprobe] probes): the top k of the DECODED rows of each
        query's ``nprobe`` best lists (``lvs_ivf_pq_search_keys``); key 0 past those rows.  ``sel``: as ``ivf_search``."""
        need = self.lib.lvs_ivf_pq_search_workspace_bytes(queries.n, lists.nlist, nprobe, corpus.d, pq.M, k, queries.mode)
        return self._ivf_search("lvs_ivf_pq_search", need, corpus, lists, queries, k, metric, nprobe, want_probe, sel,
                                codes=_ptr(pq.codes), beta=_ptr(pq.beta), codebooks=_ptr(pq.codebooks), M=pq.M, ksub=pq.ksub,
                                centroids_f32=_ptr(pq.centroids))

    # ---- exact re-ranking ("...,Refine(Flat)") ----
    REFINE_MAX_CANDIDATES = 64  # candidate slots per query of lvs_refine_keys: one per lane of the query's wave

    def refine_keys(self, corpus: PackedRows, queries: PackedRows, cand_keys, k: int, metric: int):
        """cand_keys int64 [nq, kc] (a first stage's result keys, kc <= 64) -> int64 keys [nq, k], k <= kc: the best ``k`` of
        every query's candidate rows by their EXACT score against the stored rows of ``corpus`` (``lvs_refine_keys``), best
        first, equal scores in ascending row order.  Only the row number of a candidate key is read; key 0 (and a row
        number past the corpus) is an empty slot, and the result is padded with key 0 when fewer than ``k`` slots hold a row."""
        torch = self.torch
        if metric == _capi.METRIC_L2 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        nq, kc = int(cand_keys.shape[0]), int(cand_keys.shape[1])
        if nq != queries.n:
            raise ValueError(f"cand_keys has {nq} rows for {queries.n} queries")
        cand = cand_keys.contiguous()
        out = torch.empty((nq, int(k)), dtype=torch.int64, device=self.device)
        self._call("lvs_refine_keys", **_operands(corpus, queries), metric=metric, cand_keys=_ptr(cand), kc=kc, k=int(k),
                out_keys=_ptr(out), stream=self._stream())
        return out

    # ---- recall measurement on resident keys ----
    def keys_overlap(self, truth, got):
        """truth int64 keys [nq, kt], got int64 keys [nq, kg] -> (hits, first), int32 device tensors [nq]: how many of a
        query's non-empty ``truth`` rows are among its ``got`` rows, and whether its first ``truth`` row is
        (``lvs_keys_overlap``).  Only row numbers are compared - the score halves may come from different arithmetic."""
        torch = self.torch
        nq, kt, kg = int(truth.shape[0]), int(truth.shape[1]), int(got.shape[1])
        if int(got.shape[0]) != nq:
            raise ValueError(f"got has {int(got.shape[0])} rows for {nq} queries")
        truth, got = truth.contiguous(), got.contiguous()
        hits = torch.empty((nq,), dtype=torch.int32, device=self.device)
        first = torch.empty((nq,), dtype=torch.int32, device=self.device)
        self._call("lvs_keys_overlap", truth_keys=_ptr(truth), kt=kt, got_keys=_ptr(got), kg=kg, nq=nq, out_hits=_ptr(hits),
                out_first=_ptr(first), stream=self._stream())
        return hits, first

    def ivf_row_lists(self, lists: IvfLists):
        """-> int32 device tensor [n]: the list of every row, -1 for a row in no list (``lvs_ivf_row_lists``, the inverse of
        ``lists.rows``).  Computed on first use and kept on the ``IvfLists`` object."""
        cached = lists.row_list
        if cached is None:
            n = int(lists.rows.numel())
            cached = self.torch.full((n,), -1, dtype=self.torch.int32, device=self.device)
            self._call("lvs_ivf_row_lists", offsets=_ptr(lists.offsets), rows=_ptr(lists.rows), n=n, nlist=lists.nlist,
                    out_row_list=_ptr(cached), stream=self._stream())
            lists.row_list = cached
        return cached

    def ivf_probe_ranks(self, truth, row_list, probe):
        """truth int64 keys [nq, kt], row_list (``ivf_row_lists``), probe int32 [nq, P] (best first, -1 padded) -> (rank int32
        [nq, kt], hist int64 [P + 1]), device tensors: the position in ``probe[q]`` of the list of every ``truth`` row (P:
        not probed, -1: empty slot) and how many non-empty entries have each rank (``lvs_ivf_probe_ranks``)."""
        torch = self.torch
        nq, kt, P = int(truth.shape[0]), int(truth.shape[1]), int(probe.shape[1])
        if int(probe.shape[0]) != nq:
            raise ValueError(f"probe has {int(probe.shape[0])} rows for {nq} queries")
        truth, probe = truth.contiguous(), probe.contiguous()
        rank = torch.empty((nq, kt), dtype=torch.int32, device=self.device)
        hist = torch.zeros((P + 1,), dtype=torch.int64, device=self.device)
        self._call("lvs_ivf_probe_ranks", truth_keys=_ptr(truth), kt=kt, row_list=_ptr(row_list), n=int(row_list.numel()),
                probe=_ptr(probe), P=P, nq=nq, out_rank=_ptr(rank), out_hist=_ptr(hist), stream=self._stream())
        return rank, hist

    def merge_keys(self, parts):
        """parts int64 [P, nq, k] -> [nq, k]."""
        torch = self.torch
        P, nq, k = (int(s) for s in parts.shape)
        out = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        self._call("lvs_merge_keys", parts=_ptr(parts.contiguous()), nparts=P, nq=nq, k=k, out_keys=_ptr(out), stream=self._stream())
        return out

    def keys_to_result(self, keys, metric: int, id_map=None, score_exp: int = 0):
        """keys -> (D float32, I int64) device tensors.  ``score_exp``: sum of the two operands' pack exponents - the scores
        inside the keys are 2^score_exp x the caller's (``score_exp_of``)."""
        torch = self.torch
        nq, k = int(keys.shape[0]), int(keys.shape[1])
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        self._call("lvs_keys_to_result", keys=_ptr(keys), nq=nq, k=k, metric=metric, id_map=_ptr(id_map), score_exp=int(score_exp),
                out_D=_ptr(D), out_I=_ptr(I), stream=self._stream())
        return D, I

    @staticmethod
    def score_exp_of(corpus: PackedRows, queries: PackedRows) -> int:
        return int(corpus.exp) + int(queries.exp)

    def scores(self, corpus: PackedRows, queries: PackedRows, metric: int):
        torch = self.torch
        out = torch.empty((queries.n, corpus.n), dtype=torch.float32, device=self.device)
        if metric == _capi.METRIC_L2 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        self._call("lvs_scores", **_operands(corpus, queries), metric=metric, score_exp=self.score_exp_of(corpus, queries),
                out=_ptr(out), ld_out=corpus.n, stream=self._stream())
        return out

    def rank_scores(self, sc, id_offset: int = 0):
        """Rank every float32 score row best-first: ``sc`` [nq, nb] (larger = better) -> int64 key tensor [nq, nb].
        The device sort handles < 2^32 scores per launch, so the queries go through in chunks."""
        torch = self.torch
        nq, nb = int(sc.shape[0]), int(sc.shape[1])
        keys = torch.empty((nq, nb), dtype=torch.int64, device=self.device)
        if nq == 0 or nb == 0:
            return keys
        step = max(1, min(nq, (2**32 - 2) // nb))
        for q0 in range(0, nq, step):
            q1 = min(nq, q0 + step)
            need = int(self.lib.lvs_sort_rows_workspace_bytes(q1 - q0, nb))
            if need < 0:
                raise LotusHipError("lvs_sort_rows_workspace_bytes rejected the shape")
            ws = self._workspace(need)
            self._call("lvs_sort_rows_desc", scores=_ptr(sc[q0:q1]), nq=q1 - q0, nb=nb, ld=int(sc.stride(0)), id_offset=int(id_offset),
                    out_keys=_ptr(keys[q0:q1]), workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream())
        return keys

    def rank_all(self, corpus: PackedRows, queries: PackedRows, metric: int, id_offset: int = 0):
        """Every corpus row ranked for every query (K = N callers): int64 key tensor [nq, nb], best first."""
        if corpus.n >= 2**32 - 2:
            raise ValueError("K = N ranking needs fewer than 2^32 - 2 rows")
        return self.rank_scores(self.scores(corpus, queries, metric), id_offset)

    # ---- threshold join (sem_dedup) ----
    RANGE_CHUNK_ROWS = 65536  # query rows per launch (a multiple of 256 x any rank count that divides it)

    def range_join(self, corpus: PackedRows, queries: PackedRows, threshold: float, metric: int = _capi.METRIC_IP,
                   q_row0: int = -1, id_offset: int = 0, stride: int = 1, phase: int = 0, capacity: int = 1 << 22):
        """All (query, corpus id, score) with score > threshold.  q_row0 >= 0: self-join, pairs with id > query row
        only.  Returns three device tensors (int64, int64, float32); order unspecified.

        The query rows go through in chunks, each with its own pair buffer: when a chunk finds more than `capacity`
        pairs only that chunk is run again with a buffer of the counted size (the kernel keeps counting past the
        capacity) - a 5 M-row self-join repeats at most 1/77 of its work, not all of it."""
        torch = self.torch
        step = max(256 * stride, self.RANGE_CHUNK_ROWS // (256 * stride) * (256 * stride))
        # (r6) several ranks and a join the register-resident kernel's RANGE mode takes (fp16 rows, inner product, a long corpus):
        # whole CHUNKS of query rows are dealt to the ranks instead of 256-query tiles inside every launch - each chunk then runs
        # on that kernel as on one GPU.  Snake order (0 .. w-1, w-1 .. 0, ...): a self-join's early chunks see more rows than its
        # late ones, and plain round-robin would hand rank 0 the heavier chunk of every round.  Every rank applies the same rule,
        # so the ranks' pair lists partition the result.
        deal_chunks = (stride > 1 and metric == _capi.METRIC_IP and corpus.mode == queries.mode == _capi.PACK_F16
                       and corpus.n >= 2 * self.RANGE_CHUNK_ROWS and queries.n >= 2 * self.RANGE_CHUNK_ROWS
                       and int(corpus.rows.shape[1]) in (256, 384, 512, 768))
        if deal_chunks:
            step = self.RANGE_CHUNK_ROWS
        outs = []
        cnt = torch.zeros((1,), dtype=torch.int64, device=self.device)
        oq = oj = os_ = None
        for ci, c0 in enumerate(range(0, max(queries.n, 1), step)):
            c1 = min(queries.n, c0 + step)
            if c1 <= c0:
                break
            if deal_chunks:
                rnd, pos = divmod(ci, stride)
                if (pos if rnd % 2 == 0 else stride - 1 - pos) != phase:
                    continue
            qs = self.slice_rows(queries, c0, c1)
            cap = capacity
            while True:
                if oq is None or oq.numel() < cap:
                    oq = torch.empty((cap,), dtype=torch.int64, device=self.device)
                    oj = torch.empty((cap,), dtype=torch.int64, device=self.device)
                    os_ = torch.empty((cap,), dtype=torch.float32, device=self.device)
                cnt.zero_()
                self._call("lvs_range_join", **_operands(corpus, qs), metric=metric, threshold=float(threshold),
                        score_exp=self.score_exp_of(corpus, qs), q_row0=int(q_row0 + c0) if q_row0 >= 0 else -1,
                        id_offset=int(id_offset), qt_stride=1 if deal_chunks else int(stride),
                        qt_phase=0 if deal_chunks else int(phase), capacity=int(cap), out_q=_ptr(oq), out_j=_ptr(oj),
                        out_s=_ptr(os_), out_count=_ptr(cnt), stream=self._stream())
                n = int(cnt.item())
                if n <= cap:
                    break
                cap = n  # counted but not stored: size the buffers and run this chunk again
            if n:
                outs.append((oq[:n] + c0, oj[:n].clone(), os_[:n].clone()))
        if not outs:
            e = torch.empty((0,), dtype=torch.int64, device=self.device)
            return e, e.clone(), torch.empty((0,), dtype=torch.float32, device=self.device)
        return (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), torch.cat([o[2] for o in outs]))

    # ---- k-means pieces ----
    def kmeans_accumulate(self, x: PackedRows, assign, k: int):
        """-> (sums float32 [k,d], counts float32 [k]) of the rows of x grouped by assign (int64 device tensor)."""
        torch = self.torch
        sums = torch.zeros((k, x.d), dtype=torch.float32, device=self.device)
        counts = torch.zeros((k,), dtype=torch.float32, device=self.device)
        need = int(self.lib.lvs_kmeans_accumulate_workspace_bytes(x.n, k))
        ws = self._workspace(need)
        self._call("lvs_kmeans_accumulate", x=_ptr(x.rows), n=x.n, d=x.d, pack_mode=x.mode, assign=_ptr(assign), k=k, sums=_ptr(sums),
                counts=_ptr(counts), workspace=_ptr(ws), workspace_bytes=int(ws.numel()), stream=self._stream())
        return sums, counts

    def kmeans_accumulate_keys(self, x: PackedRows, keys, k: int, id_offset: int = 0):
        """The same straight from the assignment search's result keys [n(,1)] (no decode pass in between)."""
        sums = self.torch.zeros((k, x.d), dtype=self.torch.float32, device=self.device)
        counts = self.torch.zeros((k,), dtype=self.torch.float32, device=self.device)
        self.kmeans_accumulate_keys_into(x, keys, k, sums, counts, id_offset)
        return sums, counts

    def kmeans_accumulate_keys_into(self, x: PackedRows, keys, k: int, sums, counts, id_offset: int = 0, workspace=None) -> None:
        """Add the rows of ``x`` to ``sums`` / ``counts`` CONTINUING the in-row-order sums that are there (zeros before the first
        rows): handing the rows over in consecutive ranges gives bit for bit what one call over all rows gives.  ``workspace``: a
        uint8 device tensor of ``lvs_kmeans_accumulate_workspace_bytes`` for a call that runs on a side stream next to launches
        using the backend's own workspace."""
        need = int(self.lib.lvs_kmeans_accumulate_workspace_bytes(x.n, k))
        ws = workspace if workspace is not None else self._workspace(need)
        if int(ws.numel()) < need:
            raise ValueError("workspace too small")
        self._call("lvs_kmeans_accumulate_keys", x=_ptr(x.rows), n=x.n, d=x.d, pack_mode=x.mode, keys=_ptr(keys),
                id_offset=int(id_offset), k=k, sums=_ptr(sums), counts=_ptr(counts), workspace=_ptr(ws),
                workspace_bytes=int(ws.numel()), stream=self._stream())

    def kmeans_objective(self, centroids, sums, counts, x2, out) -> None:
        """out[0] (device float64) = x2[0] - 2 sum_j <c_j, S_j> + sum_j n_j |c_j|^2: faiss's objective of the iteration
        (sum of the assignment distances) from the sums, with the centroids BEFORE the update; float64 on the device."""
        k, d = int(centroids.shape[0]), int(centroids.shape[1])
        need = int(self.lib.lvs_kmeans_objective_workspace_bytes(k))
        if getattr(self, "_obj_ws", None) is None or self._obj_ws.numel() < need:
            self._obj_ws = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
        self._call("lvs_kmeans_objective", centroids=_ptr(centroids), sums=_ptr(sums), counts=_ptr(counts), k=k, d=d,
                x_norms_sq_sum=_ptr(x2), out_obj=_ptr(out), workspace=_ptr(self._obj_ws),
                workspace_bytes=int(self._obj_ws.numel()), stream=self._stream())

    def _centroid_image(self, centroids, mode: int, exp: int):
        """-> (PackedRows for the image of ``centroids`` [k,d], float32 [2] for its statistics), both still to be written."""
        torch = self.torch
        k, d = int(centroids.shape[0]), int(centroids.shape[1])
        rows = torch.empty((k, int(self.lib.lvs_packed_ld(d, mode))), dtype=torch.float16, device=self.device)
        norms = torch.empty((k,), dtype=torch.float32, device=self.device)
        cstats = torch.empty((2,), dtype=torch.float32, device=self.device)
        return PackedRows(rows=rows, norms=norms, n=k, d=d, mode=mode, exp=int(exp)), cstats

    def kmeans_pack_centroids(self, centroids, mode: int, exp: int = 0):
        """-> (PackedRows of the centroids, device float32 [2] = (largest |c|^2, largest |lo part|^2)).  ``centroids`` are
        in the points' scaled domain already (``exp``: the points' pack exponent, recorded on the result)."""
        pk, cstats = self._centroid_image(centroids, mode, exp)
        self._call("lvs_kmeans_pack_centroids", centroids=_ptr(centroids), k=pk.n, d=pk.d, pack_mode=mode, packed_out=_ptr(pk.rows),
                norms_out=_ptr(pk.norms), stats_out=_ptr(cstats), stream=self._stream())
        return pk, cstats

    def kmeans_finish(self, sums, counts, centroids, n_train: int, mode: int, nsplit_out=None, exp: int = 0):
        """The rest of a faiss iteration after the sums, one C-ABI call, nothing read back: centroids (device float32
        [k,d], in place) = sums / counts where counts > 0 (compute_centroids), faiss's empty-cluster split on the device
        (``nsplit_out``: device int32 [1]), and the repacked centroids -> (PackedRows, stats) as ``kmeans_pack_centroids``."""
        pk, cstats = self._centroid_image(centroids, mode, exp)
        self._call("lvs_kmeans_update_centroids", sums=_ptr(sums), counts=_ptr(counts), k=pk.n, d=pk.d, n_train=int(n_train),
                centroids=_ptr(centroids), out_nsplit=_ptr(nsplit_out), pack_mode=mode, packed_out=_ptr(pk.rows),
                norms_out=_ptr(pk.norms), stats_out=_ptr(cstats), stream=self._stream())
        return pk, cstats

    def kmeans_iteration(self, x: PackedRows, x2, k: int, n_train_total: int, centroids, cpk: PackedRows, cstats, keys_out,
                         obj_out, nsplit_out=None, all_reduce=None, stats: dict | None = None) -> None:
        """ONE exhaustive Lloyd iteration as one C-ABI call (``lvs_kmeans_iteration``, ABI 7): the certified assignment of the
        rows ``x`` against the centroids, the in-row-order sums, the objective, [``all_reduce(tensor)``: the in-place sum over the
        ranks of a float32 / float64 device tensor], division + faiss's split + repack - ``centroids`` (float32 [k,d]), ``cpk``
        (their hi|lo image) and ``cstats`` are updated in place, ``keys_out`` [n] receives the assignment, ``obj_out`` (float64
        [1]) the objective, ``nsplit_out`` (int32 [1]) the split count.  Bit-identical to ``nearest`` + ``kmeans_accumulate_keys``
        + ``kmeans_objective`` + ``kmeans_finish``.  One host round trip inside (the open rows' count)."""
        torch = self.torch
        need = int(self.lib.lvs_kmeans_iteration_workspace_bytes(x.n, x.d, int(k), x.mode, cpk.mode))
        if need < 0:
            raise LotusHipError("lvs_kmeans_iteration_workspace_bytes rejected the shape")
        ws = self._workspace(need)
        cb, errors = None, []
        if all_reduce is not None:
            def transport(_ctx, buf, count, dtype, _stream):
                try:  # the library's stream is torch's current stream: torch work queued here stays in order
                    dt, size = (torch.float32, 4) if dtype == 0 else (torch.float64, 8)
                    all_reduce(torch.as_tensor(_DevBytes(buf, int(count) * size), device=self.device).view(dt))
                    return 0
                except Exception as e:  # noqa: BLE001 - reported through the status code
                    errors.append(e)
                    return _capi.EDEVICE

            fn = _capi.CALLBACKS["lvs_all_reduce_fn"](transport)
            cb = ctypes.cast(fn, ctypes.c_void_p)
        host_counts = (ctypes.c_int64 * 2)()
        try:
            self._call("lvs_kmeans_iteration", all_reduce=cb, all_reduce_ctx=None, x=_ptr(x.rows), x_pack=x.mode, n=x.n, d=x.d,
                    x_norms_sq=_ptr(x.norms), x_norms_sq_sum=_ptr(x2), exp_sum=int(x.exp) + int(cpk.exp), k=int(k),
                    n_train_total=int(n_train_total), centroids=_ptr(centroids), c_pack=cpk.mode, c_packed=_ptr(cpk.rows),
                    c_norms=_ptr(cpk.norms), c_stats=_ptr(cstats), out_keys=_ptr(keys_out), out_obj=_ptr(obj_out),
                    out_nsplit=_ptr(nsplit_out), out_host_counts=ctypes.addressof(host_counts), workspace=_ptr(ws),
                    workspace_bytes=int(ws.numel()), stream=self._stream())
        except LotusHipError:
            if errors:
                raise errors[0]
            raise
        n_pair, n_open = int(host_counts[0]), int(host_counts[1])
        self._count(stats, uncertified=n_open + n_pair, pairs=n_pair, open=n_open, queries=x.n)

    def kmeans_update_centroids(self, sums, counts, centroids) -> None:
        """centroids (device float32 [k,d], in place) = sums / counts where counts > 0 (faiss compute_centroids) - the
        division alone, for callers that split empty clusters on the host (``split_clusters``)."""
        k, d = int(centroids.shape[0]), int(centroids.shape[1])
        self._call("lvs_kmeans_update_centroids", sums=_ptr(sums), counts=_ptr(counts), k=k, d=d, n_train=0, centroids=_ptr(centroids),
                out_nsplit=None, pack_mode=0, packed_out=None, norms_out=None, stats_out=None, stream=self._stream())

    def rand_perm(self, n: int, seed: int, m: int | None = None) -> np.ndarray:
        """faiss ``rand_perm(n, seed)``; with ``m`` only its first ``m`` entries (O(m) host time instead of O(n))."""
        if m is not None and m < n:
            out = np.empty(m, np.int64)
            _capi.check(self.lib.lvs_rand_perm_prefix_host(n, seed, m, out.ctypes.data), "lvs_rand_perm_prefix_host")
            return out
        out = np.empty(n, np.int64)
        _capi.check(self.lib.lvs_rand_perm_host(n, seed, out.ctypes.data), "lvs_rand_perm_host")
        return out

    def split_clusters(self, n: int, hassign: np.ndarray, centroids: np.ndarray) -> int:
        assert hassign.dtype == np.float32 and centroids.dtype == np.float32 and centroids.flags.c_contiguous
        k, d = centroids.shape
        ns = ctypes.c_int32(0)
        _capi.check(self.lib.lvs_kmeans_split_clusters_host(d, k, n, hassign.ctypes.data, centroids.ctypes.data,
                                                            ctypes.byref(ns)), "lvs_kmeans_split_clusters_host")
        return int(ns.value)

    # ---- measurement ----
    def timing_enable(self, on: bool) -> None:
        _capi.check(self.lib.lvs_timing_enable(int(on)))

    KERNEL_NAMES = {0: "lvs_tile_kernel", 1: "lvs_stream_kernel", 2: "lvs_rq_kernel", 3: "lvs_rj_kernel", 4: "lvs_ivf_scan_kernel",
                    5: "lvs_ivf_sq8_scan_kernel", 6: "lvs_ivf_pq_scan_kernel", 7: "lvs_refine_kernel", 8: "lvs_ivf_range_kernel"}

    def timing_read(self):
        """-> (total ms of the dominant kernel's launches, searches that timed at least one): total / searches = kernel time per
        search whether it ran as one launch or - beyond 4 096 queries on the register-resident kernels - as one per chunk."""
        t = self.timing_read_full()
        return t["total_ms"], t["calls"]

    def timing_read_full(self) -> dict:
        tot, cnt, calls, kern = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        _capi.check(self.lib.lvs_timing_read_calls(ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(calls), ctypes.byref(kern)))
        return {"total_ms": float(tot.value), "launches": int(cnt.value), "calls": int(calls.value),
                "kernel": self.KERNEL_NAMES.get(int(kern.value), str(int(kern.value)))}
