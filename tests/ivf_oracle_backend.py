"""``OracleBackend`` with numpy twins of ``HipBackend.ivf_build`` / ``ivf_search``, so that the host side of an IVF
``HipVS`` (factory strings, fallbacks, the ``ivf.npz`` sidecar) runs without a GPU.  Also the rule the GPU tests hold the
device to: ``ivf_reference`` = the exact top k over the rows of the probed lists."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from lotus_amd.backend import IvfLists, ivf_fits
from oracle_backend import OracleBackend


def assign_lists(xb: np.ndarray, centroids: np.ndarray, metric: int) -> np.ndarray:
    """Best centroid of every row under ``metric`` (ties to the lower list id), int64 [n]."""
    _, I = oracle.flat_search(np.asarray(centroids, np.float32), np.asarray(xb, np.float32), 1, metric)
    return I[:, 0].astype(np.int64)


def group_rows(assign: np.ndarray, nlist: int):
    """(offsets int64 [nlist + 1], rows uint32 [n]): a stable sort of the row numbers by list."""
    order = np.argsort(assign, kind="stable")
    counts = np.bincount(assign, minlength=nlist)
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off, order.astype(np.uint32)


def probe_lists(centroids: np.ndarray, xq: np.ndarray, nprobe: int, metric: int) -> np.ndarray:
    _, I = oracle.flat_search(np.asarray(centroids, np.float32), np.asarray(xq, np.float32), nprobe, metric)
    return I


def ivf_reference(xb, xq, k, metric, centroids, offsets, rows, probe):
    """(D, I) of the exact search of every query over the union of the rows of its probed lists (oracle conventions: -1 /
    -+FLT_MAX past them)."""
    nq = xq.shape[0]
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    for q in range(nq):
        ids = np.sort(np.concatenate([rows[offsets[l]:offsets[l + 1]] for l in probe[q] if l >= 0] + [np.zeros(0, np.uint32)]))
        ids = ids.astype(np.int64)
        d1, i1 = oracle.flat_search(np.asarray(xb[ids], np.float32), xq[q:q + 1], k, metric)  # = flat_search(.., ids=ids)
        D[q], I[q] = d1[0], (np.where(i1[0] >= 0, ids[np.maximum(i1[0], 0)], -1) if ids.size else i1[0])
    return D, I


class IvfOracleBackend(OracleBackend):
    @staticmethod
    def ivf_fits(d, k, mode):
        return ivf_fits(d, k, mode)  # the library's own answer (host-only), as HipBackend.ivf_fits

    def ivf_build(self, packed, centroids, metric, offsets=None, rows=None):
        c = centroids.numpy() if torch.is_tensor(centroids) else np.asarray(centroids, np.float32)
        cpk = self.pack(c, packed.mode, exp=int(packed.exp))
        self.calls.append(("ivf_build", int(c.shape[0]), offsets is not None))
        if offsets is None:
            offsets, rows = group_rows(assign_lists(packed.rows.numpy(), cpk.rows.numpy(), metric), int(c.shape[0]))
        return IvfLists(centroids=cpk, offsets=torch.from_numpy(np.asarray(offsets, np.int64).copy()),
                        rows=torch.from_numpy(np.asarray(rows, np.uint32).view(np.int32).copy()), nlist=int(c.shape[0]),
                        metric=metric)

    def ivf_search(self, corpus, lists, queries, k, metric, nprobe, want_probe=False):
        if not self.ivf_fits(corpus.d, k, queries.mode) or nprobe > lists.nlist or nprobe > 2048:
            raise AssertionError(f"the device would refuse d={corpus.d} k={k} nprobe={nprobe}")
        self.calls.append(("ivf_search", queries.n, k, nprobe))
        xb, xq = corpus.rows.numpy(), queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        off, rows = lists.offsets.numpy(), lists.rows.numpy().view(np.uint32)
        D, I = ivf_reference(xb, xq, k, metric, None, off, rows, probe)
        better = D if metric == 0 else -D
        keys = np.where(I >= 0, oracle.pack_keys(better, np.where(I >= 0, I, 0)), np.uint64(0))
        keys = torch.from_numpy(np.array(keys, dtype=np.uint64, order="C", copy=True).view(np.int64))
        return (keys, torch.from_numpy(probe.astype(np.int32))) if want_probe else keys
