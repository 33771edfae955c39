"""``IvfOracleBackend`` with numpy twins of ``HipBackend.ivf_sq8_train`` / ``ivf_sq8_encode`` / ``ivf_sq8_search``, so that the
host side of an IVF-SQ8 ``HipVS`` runs without a GPU.  Also the rule the GPU tests hold the device to: ``sq8_reference`` =
the exact top k, in float64, over the DECODED rows of the probed lists.

The codec is faiss's ``ScalarQuantizer`` ``QT_8bit`` (per-dimension ranges) with ``by_residual``, as recalled:
  * training takes vmin_j / vmax_j over the residuals of the training rows (range statistic "min-max", no expansion);
  * encode: code = int(255 * clamp((r - vmin) / vdiff, 0, 1)) - truncation, so only r == vmax reaches 255;
  * decode: vmin + (code + 0.5) * vdiff / 255 (the middle of the code's cell).
Where vdiff_j == 0 faiss would divide by zero; here the code is 0 and the value decodes to vmin_j."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from ivf_oracle_backend import IvfOracleBackend, probe_lists
from lotus_amd.backend import IvfSq8Lists, ivf_sq8_fits

FLT_MAX = np.float32(3.4028234663852886e38)


def list_of_rows(offsets, rows, n) -> np.ndarray:
    """int64 [n]: the list of every row."""
    where = np.full(n, -1, np.int64)
    where[np.asarray(rows, np.uint32).astype(np.int64)] = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return where


def sq8_train(x, c, where, train_ids):
    """(vmin, vdiff) float32 [d] over the residuals x - c[where] of the training rows (float32 arithmetic, as the device)."""
    ids = np.asarray(train_ids, np.int64)
    r = np.asarray(x, np.float32)[ids] - np.asarray(c, np.float32)[where[ids]]
    vmin, vmax = r.min(axis=0), r.max(axis=0)
    return vmin.astype(np.float32), (vmax - vmin).astype(np.float32)


def sq8_encode(x, c, where, vmin, vdiff):
    """(codes uint8 [n, d], |rhat|^2 float32 [n]) in ROW order, float32 arithmetic as the device."""
    r = np.asarray(x, np.float32) - np.asarray(c, np.float32)[where]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip((r - vmin) / vdiff, np.float32(0), np.float32(1)).astype(np.float32)
    codes = np.where(vdiff > 0, np.floor(np.float32(255) * t), 0).astype(np.uint8)
    b = (vdiff / np.float32(255)).astype(np.float32)
    rh = (vmin + np.float32(0.5) * b) + b * codes.astype(np.float32)
    return codes, np.einsum("ij,ij->i", rh, rh, dtype=np.float32)


def sq8_boundary_distance(x, c, where, vmin, vdiff):
    """float64 [n, d]: how far 255 (r - vmin) / vdiff is from the nearest integer (inf where vdiff == 0) - the codes of a
    device and of this twin may differ only where it is tiny."""
    r = np.asarray(x, np.float64) - np.asarray(c, np.float64)[where]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 255.0 * np.clip((r - vmin) / vdiff.astype(np.float64), 0.0, 1.0)
    return np.where(vdiff > 0, np.abs(t - np.round(t)), np.inf)


def sq8_decode(c, where, vmin, vdiff, codes) -> np.ndarray:
    """float64 [n, d]: c_l + vmin + (code + 0.5) * vdiff / 255 of every row (row-order codes)."""
    vmin, vdiff = np.asarray(vmin, np.float64), np.asarray(vdiff, np.float64)
    return np.asarray(c, np.float64)[where] + vmin + (codes.astype(np.float64) + 0.5) * vdiff / 255.0


def sq8_reference(xhat, xq, k, metric, offsets, rows, probe):
    """(D float32, I int64) of the exact float64 search of every query over the decoded rows of its probed lists; ties to the
    lower row number; -1 / -+FLT_MAX past those rows (the oracle's padding)."""
    nq = xq.shape[0]
    D = np.full((nq, k), FLT_MAX if metric == 1 else -FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    rows = np.asarray(rows, np.uint32)
    for q in range(nq):
        ids = np.concatenate([rows[offsets[l]:offsets[l + 1]] for l in probe[q] if l >= 0] + [np.zeros(0, np.uint32)])
        ids = np.sort(ids.astype(np.int64))
        qv = np.asarray(xq[q], np.float64)
        if metric == 1:
            s = ((xhat[ids] - qv) ** 2).sum(axis=1)
            order = np.lexsort((ids, s))
        else:
            s = xhat[ids] @ qv
            order = np.lexsort((ids, -s))
        m = min(k, len(ids))
        D[q, :m] = s[order[:m]]
        I[q, :m] = ids[order[:m]]
    return D, I


class Sq8OracleBackend(IvfOracleBackend):
    @staticmethod
    def ivf_sq8_fits(d, k, mode):
        return ivf_sq8_fits(d, k, mode)  # the library's own answer (host-only), as HipBackend.ivf_sq8_fits

    def ivf_sq8_train(self, packed, lists, train_ids):
        self.calls.append(("ivf_sq8_train", len(train_ids)))
        x = packed.rows.numpy()
        where = list_of_rows(lists.offsets.numpy(), lists.rows.numpy().view(np.uint32), packed.n)
        vmin, vdiff = sq8_train(x, lists.centroids.rows.numpy(), where, train_ids)
        return torch.from_numpy(vmin), torch.from_numpy(vdiff)

    def ivf_sq8_encode(self, packed, lists, vmin, vdiff, codes=None, rnorm=None):
        self.calls.append(("ivf_sq8_encode", codes is not None))
        vmin = np.asarray(vmin.numpy() if torch.is_tensor(vmin) else vmin, np.float32)
        vdiff = np.asarray(vdiff.numpy() if torch.is_tensor(vdiff) else vdiff, np.float32)
        off, rows = lists.offsets.numpy(), lists.rows.numpy().view(np.uint32)
        c = lists.centroids.rows.numpy().astype(np.float32)
        d = packed.d
        ldc = -(-d // 64) * 64
        if codes is None:
            where = list_of_rows(off, rows, packed.n)
            cr, rn = sq8_encode(packed.rows.numpy(), c, where, vmin, vdiff)
            codes, rnorm = cr[rows.astype(np.int64)], rn[rows.astype(np.int64)]
        full = np.zeros((len(rows), ldc), np.uint8)
        full[:, :d] = codes
        return IvfSq8Lists(vmin=torch.from_numpy(vmin.copy()), vdiff=torch.from_numpy(vdiff.copy()), centroids=torch.from_numpy(c),
                           codes=torch.from_numpy(full), rnorm=torch.from_numpy(np.asarray(rnorm, np.float32).copy()),
                           exp=int(packed.exp))

    def ivf_sq8_search(self, corpus, lists, sq8, queries, k, metric, nprobe, want_probe=False):
        if not self.ivf_sq8_fits(corpus.d, k, queries.mode) or nprobe > lists.nlist or nprobe > 2048:
            raise AssertionError(f"the device would refuse d={corpus.d} k={k} nprobe={nprobe}")
        self.calls.append(("ivf_sq8_search", queries.n, k, nprobe))
        xq = queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        off, rows = lists.offsets.numpy(), lists.rows.numpy().view(np.uint32)
        where = list_of_rows(off, rows, corpus.n)
        codes = np.empty((corpus.n, corpus.d), np.uint8)
        codes[rows.astype(np.int64)] = sq8.codes.numpy()[:, :corpus.d]
        xhat = sq8_decode(sq8.centroids.numpy(), where, sq8.vmin.numpy(), sq8.vdiff.numpy(), codes)
        D, I = sq8_reference(xhat, xq, k, metric, off, rows, probe)
        better = D if metric == 0 else -D
        keys = np.where(I >= 0, oracle.pack_keys(better, np.where(I >= 0, I, 0)), np.uint64(0))
        keys = torch.from_numpy(np.array(keys, dtype=np.uint64, order="C", copy=True).view(np.int64))
        return (keys, torch.from_numpy(probe.astype(np.int32))) if want_probe else keys
