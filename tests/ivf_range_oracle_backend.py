"""``IvfOracleBackend`` (through ``SelectOracleBackend``, so that stores of every IVF mode build) with a numpy twin of
``HipBackend.ivf_range_search`` / ``ivf_range_fits``, so that the host side of ``HipVS.range_search``,
``dedup.threshold_pairs_ivf`` and ``ops.sem_dedup(nprobe=...)`` runs without a GPU.  Also the rule the GPU tests hold
``lvs_ivf_range_kernel`` to: ``ivf_range_reference`` = every (query, row) of the probed lists whose float64 score clears the
threshold, with the pairs too close to the threshold to call set apart."""
from __future__ import annotations

import numpy as np
import torch

from ivf_oracle_backend import probe_lists
from ivf_select_oracle_backend import SelectOracleBackend, bitmap_mask
from ivf_sq8_oracle_backend import list_of_rows
from lotus_amd.backend import ivf_range_fits


def _allowed(nb, offsets, rows, probe, sel):
    """-> (inprobe bool [nq, nlist + 1], list of every row with nlist for rows in no list or not selected)."""
    nlist = len(offsets) - 1
    lid = np.asarray(list_of_rows(np.asarray(offsets), np.asarray(rows, np.uint32), nb), np.int64).copy()
    lid[lid < 0] = nlist
    if sel is not None:
        lid[~np.asarray(sel, bool)] = nlist
    probe = np.asarray(probe, np.int64)
    inprobe = np.zeros((probe.shape[0], nlist + 1), bool)
    qq = np.repeat(np.arange(probe.shape[0]), probe.shape[1])
    ok = probe.reshape(-1) >= 0
    inprobe[qq[ok], probe.reshape(-1)[ok]] = True
    return inprobe, lid


def ivf_range_reference(xb, xq, thr, metric, offsets, rows, probe, sel=None, eps=2e-5, block=2048):
    """-> (want, near), int64 arrays [m, 2] of (query, row): with float64 scores of the stored values over the rows of each
    query's probed lists (``probe`` [nq, nprobe]; ``sel``: bool [nb], only those rows), ``want`` clears the threshold by more
    than ``eps`` and ``near`` lies within ``eps`` of it.  ``thr`` as ``HipVS.range_search`` takes it: inner product - score >
    thr; squared L2 - distance < thr."""
    xb64, xq64 = np.asarray(xb, np.float64), np.asarray(xq, np.float64)
    inprobe, lid = _allowed(xb64.shape[0], offsets, rows, probe, sel)
    bn = np.einsum("ij,ij->i", xb64, xb64)
    want, near = [], []
    for q0 in range(0, xq64.shape[0], block):
        q = xq64[q0:q0 + block]
        s = q @ xb64.T
        if metric == 1:
            s = np.einsum("ij,ij->i", q, q)[:, None] + bn[None, :] - 2.0 * s
            margin = thr - s  # positive: inside the radius
        else:
            margin = s - thr
        ok = inprobe[q0:q0 + block][:, lid]
        for out, m in ((want, ok & (margin > eps)), (near, ok & (np.abs(margin) <= eps))):
            qi, ri = np.nonzero(m)
            out.append(np.stack([qi + q0, ri], axis=1))
    return np.concatenate(want).astype(np.int64), np.concatenate(near).astype(np.int64)


def float64_scores(xb, xq, metric, pairs):
    """The float64 score (product, or squared distance) of every (query, row) of ``pairs`` [m, 2]."""
    out = np.empty(len(pairs), np.float64)
    for a in range(0, len(pairs), 1 << 16):
        q = np.asarray(xq[pairs[a:a + (1 << 16), 0]], np.float64)
        b = np.asarray(xb[pairs[a:a + (1 << 16), 1]], np.float64)
        out[a:a + (1 << 16)] = np.einsum("ij,ij->i", q, b) if metric == 0 else np.einsum("ij,ij->i", q - b, q - b)
    return out


def codes(pairs, nb):
    """(query, row) pairs as one sortable int64 each."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return pairs[:, 0] * np.int64(nb) + pairs[:, 1]


def check_pairs(got, want, near, nb):
    """want <= got <= want + near, and no (query, row) twice."""
    g, w, n = codes(got, nb), codes(want, nb), codes(near, nb)
    assert np.unique(g).size == g.size, "a (query, row) pair came back twice"
    missing = np.setdiff1d(w, g)
    extra = np.setdiff1d(g, np.union1d(w, n))
    assert missing.size == 0 and extra.size == 0, (missing.size, extra.size, missing[:5], extra[:5])


class IvfRangeOracleBackend(SelectOracleBackend):
    @staticmethod
    def ivf_range_fits(d, mode):
        return ivf_range_fits(d, mode)  # the library's own answer (host-only), as HipBackend.ivf_range_fits

    def range_join(self, corpus, queries, threshold, *a, **kw):
        self.calls.append(("range_join", queries.n, corpus.n))
        return super().range_join(corpus, queries, threshold, *a, **kw)

    def ivf_range_search(self, corpus, lists, queries, threshold, metric, nprobe, q_rows=None, sel=None, capacity=1 << 22):
        if not self.ivf_range_fits(corpus.d, queries.mode) or nprobe > lists.nlist or nprobe > 2048 or nprobe < 1:
            raise AssertionError(f"the device would refuse d={corpus.d} nprobe={nprobe}")
        if metric == 1 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        mask = None
        if sel is not None:
            if int(sel.numel()) != -(-corpus.n // 32):
                raise AssertionError(f"the device would read {-(-corpus.n // 32)} selector words, given {int(sel.numel())}")
            mask = bitmap_mask(sel.numpy(), corpus.n)
        self.calls.append(("ivf_range_search", queries.n, nprobe, q_rows is not None, None if mask is None else int(mask.sum())))
        xb, xq = corpus.rows.numpy(), queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        inprobe, lid = _allowed(corpus.n, lists.offsets.numpy(), lists.rows.numpy().view(np.uint32), probe, mask)
        s = xq @ xb.T
        if metric == 1:
            s = -np.maximum((queries.norms.numpy()[:, None] + corpus.norms.numpy()[None, :]) - 2 * s, 0)
        s = s.astype(np.float32)
        e = self.score_exp_of(corpus, queries)
        hit = inprobe[:, lid] & (s > np.float32(threshold) * np.float32(2.0 ** e))  # the device compares in the scaled domain
        if q_rows is not None:
            own = q_rows.numpy().view(np.uint32).astype(np.int64)
            hit[np.arange(queries.n), own] = False
        q, j = np.nonzero(hit)
        out_s = (s[q, j] * np.float32(2.0 ** -e)).astype(np.float32)
        return torch.from_numpy(q.astype(np.int64)), torch.from_numpy(j.astype(np.int64)), torch.from_numpy(out_s)
