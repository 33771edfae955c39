"""``IvfRangeOracleBackend`` with numpy twins of ``HipBackend.keys_overlap`` / ``ivf_row_lists`` / ``ivf_probe_ranks``, so that
the host side of ``HipVS.recall`` / ``probe_recall_curve`` / ``tune_nprobe`` runs without a GPU.  The twins are plain set and
index arithmetic on the row numbers - no staging, no bisection - and are also the rule the GPU tests hold the three kernels to
(``overlap_reference``, ``row_lists_reference``, ``probe_ranks_reference``)."""
from __future__ import annotations

import numpy as np
import torch

from ivf_range_oracle_backend import IvfRangeOracleBackend

LOW = np.uint64(0xFFFFFFFF)


def key_rows(keys) -> list:
    """Per query, the row numbers of the non-empty keys in slot order, None in an empty slot (key 0, or a low half of 0: row
    2^32 - 1, which no image has)."""
    k = np.asarray(keys).view(np.uint64)
    return [[None if (v == 0 or (v & LOW) == 0) else int(LOW - (v & LOW)) for v in row] for row in k]


def overlap_reference(truth, got):
    """(hits, first) int32 [nq] by set membership of the row numbers."""
    hits, first = [], []
    for t, g in zip(key_rows(truth), key_rows(got)):
        have = {r for r in g if r is not None}
        hits.append(sum(1 for r in t if r is not None and r in have))
        first.append(int(t[0] is not None and t[0] in have))
    return np.asarray(hits, np.int32), np.asarray(first, np.int32)


def row_lists_reference(offsets, rows, n: int) -> np.ndarray:
    """int32 [n]: list of every row, -1 for a row that no list holds."""
    offsets = np.asarray(offsets, np.int64)
    out = np.full(n, -1, np.int32)
    for l in range(len(offsets) - 1):
        out[np.asarray(rows[offsets[l]:offsets[l + 1]], np.int64)] = l
    return out


def probe_ranks_reference(truth, row_list, probe):
    """(rank int32 [nq, kt], hist int64 [P + 1]): position of each true row's list in the query's probes (dict lookup)."""
    probe = np.asarray(probe)
    P, n = probe.shape[1], len(row_list)
    rank = np.full((probe.shape[0], np.asarray(truth).shape[1]), -1, np.int32)
    hist = np.zeros(P + 1, np.int64)
    for q, t in enumerate(key_rows(truth)):
        where = {}
        for pos, l in enumerate(probe[q].tolist()):
            if l >= 0:
                where.setdefault(l, pos)
        for j, r in enumerate(t):
            if r is None or r >= n:
                continue
            rank[q, j] = where.get(int(row_list[r]), P) if row_list[r] >= 0 else P
            hist[rank[q, j]] += 1
    return rank, hist


class IvfRecallOracleBackend(IvfRangeOracleBackend):
    def keys_overlap(self, truth, got):
        self.calls.append(("keys_overlap", int(truth.shape[0]), int(truth.shape[1]), int(got.shape[1])))
        hits, first = overlap_reference(truth.numpy(), got.numpy())
        return torch.from_numpy(hits), torch.from_numpy(first)

    def ivf_row_lists(self, lists):
        if lists.row_list is None:
            self.calls.append(("ivf_row_lists", lists.nlist))
            rows = lists.rows.numpy().view(np.uint32)
            lists.row_list = torch.from_numpy(row_lists_reference(lists.offsets.numpy(), rows, len(rows)))
        return lists.row_list

    def ivf_probe_ranks(self, truth, row_list, probe):
        self.calls.append(("ivf_probe_ranks", int(truth.shape[0]), int(truth.shape[1]), int(probe.shape[1])))
        rank, hist = probe_ranks_reference(truth.numpy(), row_list.numpy(), probe.numpy())
        return torch.from_numpy(rank), torch.from_numpy(hist)
