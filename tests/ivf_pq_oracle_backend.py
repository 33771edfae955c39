"""``Sq8OracleBackend`` with numpy twins of ``HipBackend.ivf_pq_train`` / ``ivf_pq_encode`` / ``ivf_pq_search``, so that the
host side of an IVF-PQ ``HipVS`` runs without a GPU.  The rule the GPU tests hold the device to is ``sq8_reference`` applied
to the PQ-decoded rows: the exact top k, in float64, over the DECODED rows of the probed lists.

The codec is faiss's ``ProductQuantizer`` (nbits = 8) with ``by_residual``, as recalled:
  * training: per subspace m one k-means (squared L2, 25 iterations, seed 1234, 256 points per centroid) over the sub-vectors
    r[:, m dsub:(m + 1) dsub] of the residuals x - c_l of the training rows; ksub = min(256, training rows) - faiss refuses
    fewer than 256 training rows, here the codebooks shrink instead;
  * encode: code_m = argmin_j |r_m - cb[m][j]|^2 over the ksub entries, ties to the smaller j;
  * decode: c_l + concat_m cb[m][code_m]; beta = |rhat|^2 + 2 <c_l, rhat>, the per-row term of faiss's precomputed L2 table."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from ivf_oracle_backend import probe_lists
from ivf_sq8_oracle_backend import Sq8OracleBackend, list_of_rows, sq8_reference
from lotus_amd.backend import IvfPqLists, ivf_pq_fits

PQ_SEED, PQ_NITER, PQ_MPPC = 1234, 25, 256


def pq_train(x, c, where, train_ids, M, backend):
    """codebooks float32 [M, ksub, d / M] over the residuals of the training rows (the k-means of ``lotus_amd.cluster`` on
    ``backend``, as the device)."""
    from lotus_amd import cluster

    ids = np.asarray(train_ids, np.int64)
    ksub = min(256, len(ids))
    if len(ids) > ksub * PQ_MPPC:
        ids = ids[backend.rand_perm(len(ids), PQ_SEED, ksub * PQ_MPPC)]
    r = np.asarray(x, np.float32)[ids] - np.asarray(c, np.float32)[where[ids]]
    dsub = r.shape[1] // M
    books = np.empty((M, ksub, dsub), np.float32)
    for m in range(M):
        res = cluster.kmeans(np.ascontiguousarray(r[:, m * dsub:(m + 1) * dsub]), ksub, niter=PQ_NITER, seed=PQ_SEED,
                             max_points_per_centroid=PQ_MPPC, backend=backend, final_assign=False)
        books[m] = res.centroids
    return books


def _sub_dists(r, books, m):
    """float32 [n, ksub]: |r_m - cb[m][j]|^2 in float32 arithmetic."""
    dsub = books.shape[2]
    diff = r[:, None, m * dsub:(m + 1) * dsub] - books[m][None, :, :]
    return np.einsum("njt,njt->nj", diff, diff, dtype=np.float32)


def pq_encode(x, c, where, books):
    """(codes uint8 [n, M], beta float32 [n]) in ROW order: per subspace the nearest entry (ties to the smaller j)."""
    books = np.asarray(books, np.float32)
    r = np.asarray(x, np.float32) - np.asarray(c, np.float32)[where]
    M = books.shape[0]
    codes = np.empty((r.shape[0], M), np.uint8)
    for m in range(M):
        codes[:, m] = np.argmin(_sub_dists(r, books, m), axis=1)  # argmin: the first of equal minima
    rh = pq_residuals(books, codes).astype(np.float32)
    cl = np.asarray(c, np.float32)[where]
    beta = (np.einsum("ij,ij->i", rh, rh, dtype=np.float32)
            + np.float32(2) * np.einsum("ij,ij->i", cl, rh, dtype=np.float32)).astype(np.float32)
    return codes, beta


def pq_margin(x, c, where, books):
    """float64 [n, M]: second-best minus best sub-distance of every (row, subspace) - the codes of a device and of this twin
    may differ only where it is tiny (inf with a single entry)."""
    books = np.asarray(books, np.float64)
    r = np.asarray(x, np.float64) - np.asarray(c, np.float64)[where]
    M, ksub, dsub = books.shape
    out = np.full((r.shape[0], M), np.inf)
    if ksub < 2:
        return out
    for m in range(M):
        diff = r[:, None, m * dsub:(m + 1) * dsub] - books[m][None, :, :]
        dist = np.sort(np.einsum("njt,njt->nj", diff, diff), axis=1)
        out[:, m] = dist[:, 1] - dist[:, 0]
    return out


def pq_residuals(books, codes) -> np.ndarray:
    """float64 [n, d]: concat_m cb[m][codes[:, m]]."""
    books = np.asarray(books, np.float64)
    return np.concatenate([books[m][codes[:, m].astype(np.int64)] for m in range(books.shape[0])], axis=1)


def pq_decode(c, where, books, codes) -> np.ndarray:
    """float64 [n, d]: c_l + concat_m cb[m][code_m] of every row (row-order codes)."""
    return np.asarray(c, np.float64)[where] + pq_residuals(books, codes)


pq_reference = sq8_reference  # the exact float64 top k over given decoded rows of the probed lists


class PqOracleBackend(Sq8OracleBackend):
    @staticmethod
    def ivf_pq_fits(d, M, k, mode):
        return ivf_pq_fits(d, M, k, mode)  # the library's own answer (host-only), as HipBackend.ivf_pq_fits

    def ivf_pq_train(self, packed, lists, train_ids, M):
        self.calls.append(("ivf_pq_train", len(train_ids), M))
        where = list_of_rows(lists.offsets.numpy(), lists.rows.numpy().view(np.uint32), packed.n)
        books = pq_train(packed.rows.numpy(), lists.centroids.rows.numpy(), where, train_ids, M, self)
        return torch.from_numpy(books)

    def ivf_pq_encode(self, packed, lists, codebooks, codes=None, beta=None):
        self.calls.append(("ivf_pq_encode", codes is not None))
        books = np.asarray(codebooks.numpy() if torch.is_tensor(codebooks) else codebooks, np.float32)
        M, ksub = books.shape[0], books.shape[1]
        if packed.d % M != 0 or books.shape[2] != packed.d // M:
            raise ValueError("codebooks do not split d into equal subspaces")
        off, rows = lists.offsets.numpy(), lists.rows.numpy().view(np.uint32)
        c = lists.centroids.rows.numpy().astype(np.float32)
        if codes is None:
            where = list_of_rows(off, rows, packed.n)
            cr, bt = pq_encode(packed.rows.numpy(), c, where, books)
            codes, beta = cr[rows.astype(np.int64)], bt[rows.astype(np.int64)]
        ldc = -(-M // 16) * 16
        full = np.zeros((len(rows), ldc), np.uint8)
        full[:, :M] = codes
        return IvfPqLists(M=int(M), ksub=int(ksub), codebooks=torch.from_numpy(books.copy()), centroids=torch.from_numpy(c),
                          codes=torch.from_numpy(full), beta=torch.from_numpy(np.asarray(beta, np.float32).copy()),
                          exp=int(packed.exp))

    def ivf_pq_search(self, corpus, lists, pq, queries, k, metric, nprobe, want_probe=False):
        if not self.ivf_pq_fits(corpus.d, pq.M, k, queries.mode) or nprobe > lists.nlist or nprobe > 2048:
            raise AssertionError(f"the device would refuse d={corpus.d} M={pq.M} k={k} nprobe={nprobe}")
        self.calls.append(("ivf_pq_search", queries.n, k, nprobe))
        xq = queries.rows.numpy()
        probe = probe_lists(lists.centroids.rows.numpy(), xq, nprobe, metric)
        off, rows = lists.offsets.numpy(), lists.rows.numpy().view(np.uint32)
        where = list_of_rows(off, rows, corpus.n)
        codes = np.empty((corpus.n, pq.M), np.uint8)
        codes[rows.astype(np.int64)] = pq.codes.numpy()[:, :pq.M]
        xhat = pq_decode(pq.centroids.numpy(), where, pq.codebooks.numpy(), codes)
        D, I = pq_reference(xhat, xq, k, metric, off, rows, probe)
        better = D if metric == 0 else -D
        keys = np.where(I >= 0, oracle.pack_keys(better, np.where(I >= 0, I, 0)), np.uint64(0))
        keys = torch.from_numpy(np.array(keys, dtype=np.uint64, order="C", copy=True).view(np.int64))
        return (keys, torch.from_numpy(probe.astype(np.int32))) if want_probe else keys
