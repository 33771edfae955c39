"""``PqOracleBackend`` with a numpy twin of ``HipBackend.refine_keys``, so that the host side of a ``"...,Refine(Flat)"``
``HipVS`` runs without a GPU, and the float64 rule the GPU tests hold ``lvs_refine_kernel`` to.

The rule: the result is the best k of a query's candidate rows by their EXACT score - float64 arithmetic over the stored
values of the flat image - in the project's total order (score best first, then ascending row).  Only the row number of a
candidate key counts; key 0 and a row number past the corpus are empty slots, wherever they stand."""
from __future__ import annotations

import numpy as np
import torch

import oracle
from ivf_pq_oracle_backend import PqOracleBackend

FLT_MAX = np.float64(np.finfo(np.float32).max)


def candidate_rows(cand_keys, nb: int) -> np.ndarray:
    """int64 [nq, kc]: the row number of every candidate key, -1 for an empty slot (key 0, or a row >= nb)."""
    keys = np.asarray(cand_keys).view(np.uint64)
    rows = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return np.where((keys == 0) | (rows >= nb), np.int64(-1), rows)


def exact_scores(xb, xq_row, ids, metric: int) -> np.ndarray:
    """float64 "larger is better" scores of rows ``ids`` against one query: the product, or minus the squared distance."""
    X = np.asarray(xb, np.float64)[np.asarray(ids, np.int64)]
    qv = np.asarray(xq_row, np.float64)
    return X @ qv if metric == 0 else -((X - qv) ** 2).sum(axis=1)


def refine_reference(xb, xq, cand, k: int, metric: int):
    """(D float64 [nq, k], I int64 [nq, k]): per query the best k of its candidate rows ``cand`` [nq, kc] (-1: empty slot) by
    float64 score over the stored values ``xb`` / ``xq``, ties to the lower row; D as the stores report it (squared L2
    positive), missing slots -1 / -FLT_MAX (inner product) or +FLT_MAX (L2)."""
    cand = np.asarray(cand, np.int64)
    nq = cand.shape[0]
    D = np.full((nq, k), -FLT_MAX if metric == 0 else FLT_MAX, np.float64)
    I = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        ids = cand[q][cand[q] >= 0]
        if ids.size == 0:
            continue
        s = exact_scores(xb, xq[q], ids, metric)
        take = np.lexsort((ids, -s))[:k]
        I[q, :take.size] = ids[take]
        D[q, :take.size] = s[take] if metric == 0 else -s[take]
    return D, I


def refine_keys_reference(xb, xq, cand_keys, k: int, metric: int) -> np.ndarray:
    """uint64 [nq, k]: what ``lvs_refine_keys`` returns for stored values ``xb`` / ``xq`` (the caller's or the stored scale: the
    keys carry the scores of the values given) - float64 scores rounded to float32, ranked as keys."""
    cand = candidate_rows(cand_keys, np.asarray(xb).shape[0])
    nq, kc = cand.shape
    keys = np.zeros((nq, kc), np.uint64)
    for q in range(nq):
        at = cand[q] >= 0
        if at.any():
            s = exact_scores(xb, xq[q], cand[q][at], metric).astype(np.float32)
            keys[q, at] = oracle.pack_keys(s, cand[q][at])
    return np.ascontiguousarray(np.sort(keys, axis=1)[:, ::-1][:, :k])


class RefineOracleBackend(PqOracleBackend):
    def refine_keys(self, corpus, queries, cand_keys, k, metric):
        if metric == 1 and corpus.exp != queries.exp:
            raise ValueError("squared L2 needs both operands packed with the same scale exponent")
        kc = int(cand_keys.shape[1])
        if not 1 <= k <= kc <= 64 or int(cand_keys.shape[0]) != queries.n:
            raise AssertionError(f"the device would refuse nq={queries.n} kc={kc} k={k}")
        self.calls.append(("refine_keys", queries.n, kc, k))
        keys = refine_keys_reference(corpus.rows.numpy(), queries.rows.numpy(), cand_keys.numpy(), k, metric)
        return torch.from_numpy(np.array(keys, dtype=np.uint64, order="C", copy=True).view(np.int64))
