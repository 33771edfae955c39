"""``RefineOracleBackend`` with numpy twins of ``HipBackend.row_bitmap`` and of the ``sel=`` argument of the three IVF
searches, so that the host side of ``HipVS(ids_probe=True)`` runs without a GPU.  The rule the GPU tests hold the selected
scans to needs no new arithmetic: drop the unselected row numbers from every list, recompute the offsets
(``filter_lists``), and apply the existing reference - ``ivf_reference`` / ``sq8_reference`` / ``pq_reference`` - to those
lists, with the probes of the UNFILTERED index (the coarse step does not see the selector)."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from ivf_oracle_backend import ivf_reference, probe_lists
from ivf_pq_oracle_backend import pq_decode, pq_reference
from ivf_refine_oracle_backend import RefineOracleBackend
from ivf_sq8_oracle_backend import list_of_rows, sq8_decode, sq8_reference


def bitmap_words(ids, n: int) -> np.ndarray:
    """uint32 [ceil(n / 32)]: bit ``r & 31`` of word ``r >> 5`` set for every row r of ``ids``, written bit by bit."""
    words = np.zeros(-(-int(n) // 32), np.uint32)
    for r in np.unique(np.asarray(ids, np.int64)):
        words[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return words


def bitmap_mask(words, n: int) -> np.ndarray:
    """bool [n]: the rows a selector selects; bits at or past ``n`` are not rows."""
    w = np.ascontiguousarray(np.asarray(words).view(np.uint32))
    return np.array([(int(w[r >> 5]) >> (r & 31)) & 1 for r in range(int(n))], dtype=bool)


def filter_lists(offsets, rows, mask):
    """(offsets int64 [nlist + 1], rows uint32): the lists without their unselected rows, order kept."""
    rows = np.asarray(rows, np.uint32)
    keep = mask[rows.astype(np.int64)]
    nlist = len(offsets) - 1
    lid = np.repeat(np.arange(nlist), np.diff(offsets))
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(lid[keep], minlength=nlist), out=off[1:])
    return off, rows[keep]


def _keys(D, I, metric):
    better = D if metric == 0 else -D
    keys = np.where(I >= 0, oracle.pack_keys(better, np.where(I >= 0, I, 0)), np.uint64(0))
    return torch.from_numpy(np.array(keys, dtype=np.uint64, order="C", copy=True).view(np.int64))


class SelectOracleBackend(RefineOracleBackend):
    def row_bitmap(self, ids, n):
        ids = np.asarray(ids, np.int64).reshape(-1)
        self.calls.append(("row_bitmap", int(ids.size), int(n)))
        return torch.from_numpy(bitmap_words(ids, n)), int(np.unique(ids).size)

    def _selected(self, sel, corpus, lists):
        if int(sel.numel()) != -(-corpus.n // 32):
            raise AssertionError(f"the device would read {-(-corpus.n // 32)} selector words, given {int(sel.numel())}")
        mask = bitmap_mask(sel.numpy(), corpus.n)
        off, rows = lists.offsets.numpy(), lists.rows.numpy().view(np.uint32)
        return off, rows, filter_lists(off, rows, mask), int(mask.sum())

    def ivf_search(self, corpus, lists, queries, k, metric, nprobe, want_probe=False, sel=None):
        if sel is None:
            return super().ivf_search(corpus, lists, queries, k, metric, nprobe, want_probe)
        if not self.ivf_fits(corpus.d, k, queries.mode) or nprobe > lists.nlist or nprobe > 2048:
            raise AssertionError(f"the device would refuse d={corpus.d} k={k} nprobe={nprobe}")
        _, _, (off_f, rows_f), nsel = self._selected(sel, corpus, lists)
        self.calls.append(("ivf_search_sel", queries.n, k, nprobe, nsel))
        xq = queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        D, I = ivf_reference(corpus.rows.numpy(), xq, k, metric, None, off_f, rows_f, probe)
        return (_keys(D, I, metric), torch.from_numpy(probe.astype(np.int32))) if want_probe else _keys(D, I, metric)

    def ivf_sq8_search(self, corpus, lists, sq8, queries, k, metric, nprobe, want_probe=False, sel=None):
        if sel is None:
            return super().ivf_sq8_search(corpus, lists, sq8, queries, k, metric, nprobe, want_probe)
        if not self.ivf_sq8_fits(corpus.d, k, queries.mode) or nprobe > lists.nlist or nprobe > 2048:
            raise AssertionError(f"the device would refuse d={corpus.d} k={k} nprobe={nprobe}")
        off, rows, (off_f, rows_f), nsel = self._selected(sel, corpus, lists)
        self.calls.append(("ivf_sq8_search_sel", queries.n, k, nprobe, nsel))
        xq = queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        codes = np.empty((corpus.n, corpus.d), np.uint8)
        codes[rows.astype(np.int64)] = sq8.codes.numpy()[:, :corpus.d]
        xhat = sq8_decode(sq8.centroids.numpy(), list_of_rows(off, rows, corpus.n), sq8.vmin.numpy(), sq8.vdiff.numpy(), codes)
        D, I = sq8_reference(xhat, xq, k, metric, off_f, rows_f, probe)
        return (_keys(D, I, metric), torch.from_numpy(probe.astype(np.int32))) if want_probe else _keys(D, I, metric)

    def ivf_pq_search(self, corpus, lists, pq, queries, k, metric, nprobe, want_probe=False, sel=None):
        if sel is None:
            return super().ivf_pq_search(corpus, lists, pq, queries, k, metric, nprobe, want_probe)
        if not self.ivf_pq_fits(corpus.d, pq.M, k, queries.mode) or nprobe > lists.nlist or nprobe > 2048:
            raise AssertionError(f"the device would refuse d={corpus.d} M={pq.M} k={k} nprobe={nprobe}")
        off, rows, (off_f, rows_f), nsel = self._selected(sel, corpus, lists)
        self.calls.append(("ivf_pq_search_sel", queries.n, k, nprobe, nsel))
        xq = queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        codes = np.empty((corpus.n, pq.M), np.uint8)
        codes[rows.astype(np.int64)] = pq.codes.numpy()[:, :pq.M]
        xhat = pq_decode(pq.centroids.numpy(), list_of_rows(off, rows, corpus.n), pq.codebooks.numpy(), codes)
        D, I = pq_reference(xhat, xq, k, metric, off_f, rows_f, probe)
        return (_keys(D, I, metric), torch.from_numpy(probe.astype(np.int32))) if want_probe else _keys(D, I, metric)
