"""Flat searches at the widths users index (d = 192 .. 4 096): the case table, the float64 reference and the checker shared by
tests/test_widths_host.py (planner classes, teeth; no GPU) and tests/test_gpu_widths.py (the kernels).  Imports no GPU module.

Bars are the project's (BASELINE north_star): a returned score within ``BAR`` = 1e-5 of the float64 score of the stored values,
order and membership exact up to ``GAP`` = 2e-5 (``synth.compare_topk``'s tie_gap).  Rows are unit vectors; for L2 the corpus is
multiplied by 1.3 (tests/test_gpu_random_parity.py), so squared distances are of magnitude <= 5.3.

``check_topk_exact`` replaces ``synth.compare_topk`` here because that one excuses every slot whose reference neighbours are
closer than the gap, and at these widths the top scores crowd together (300 x 3 000 x 4 096, k = 56, IP: 16 % of the slots
lie inside a 2e-5 gap).  The properties below need no excusal: each is true of ANY result whose scores are within the bar of
the float64 ones and that was selected by those scores (BAR <= GAP / 2)."""
from collections import namedtuple

import numpy as np

import synth

F16, SPLIT = 0, 1  # lotus_amd._capi.PACK_F16 / PACK_SPLIT
IP, L2 = 0, 1      # lotus_amd._capi.METRIC_IP / METRIC_L2
BAR, GAP = 1e-5, 2e-5
L2_CORPUS_SCALE = np.float32(1.3)


def stored64(x, mode):
    """The float64 value of what the device stores: fp16(x), or hi + lo with hi = fp16(x), lo = fp16(x - hi)."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    if mode == F16:
        return hi.astype(np.float64)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64)


def split64(x):
    """(hi, lo) of a hi|lo row image, both float64."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    return hi.astype(np.float64), (x - hi.astype(np.float32)).astype(np.float16).astype(np.float64)


def scores_from_products(qb, qn, bn, metric):
    """Score matrix (larger is better) from the products q.b [nq, nb] and the squared norms of both sides."""
    if metric == IP:
        return qb
    return -np.maximum(qn[:, None] + bn[None, :] - 2.0 * qb, 0.0)


def scores64(xb_s, xq_s, metric):
    """The full float64 score matrix [nq, nb] of stored values, larger is better: q.b, or -max(|q|^2 + |b|^2 - 2 q.b, 0)."""
    xb_s, xq_s = np.asarray(xb_s, np.float64), np.asarray(xq_s, np.float64)
    return scores_from_products(xq_s @ xb_s.T, (xq_s * xq_s).sum(1), (xb_s * xb_s).sum(1), metric)


def topk64(S, k):
    """The reference's own top k of a score matrix in the project's total order: best score first, equal scores by
    ascending id; -1 behind the last row.  -> (D [nq, k] float64, I [nq, k] int64)"""
    nq, nb = S.shape
    n = min(k, nb)
    I = np.full((nq, k), -1, np.int64)
    D = np.full((nq, k), -np.inf)
    for q in range(nq):
        if n < nb:
            cut = np.partition(S[q], nb - n)[nb - n]
            cand = np.flatnonzero(S[q] >= cut)
        else:
            cand = np.arange(nb)
        order = cand[np.lexsort((cand, -S[q, cand]))][:n]
        I[q, :n] = order
        D[q, :n] = S[q, order]
    return D, I


def check_topk_exact(S, D, I, k, bar=BAR, gap=GAP):
    """Assert that (D, I) [nq, k] is a top-k of the float64 score matrix S [nq, nb]; D in S's sense (larger is better: pass -D
    for squared L2 distances).  Per query, nothing excused:
      1. min(k, nb) ids, all in range, none repeated, and -1 only behind them;
      2. |D[q, r] - S[q, I[q, r]]| <= bar;
      3. D is non-increasing, and equal D come in ascending id order;
      4. every row not returned has S <= min(S of the returned) + gap;
      5. for r < s, S[I[q, r]] >= S[I[q, s]] - gap.
    Returns the largest error of (2)."""
    S = np.asarray(S, np.float64)
    D, I = np.asarray(D, np.float64), np.asarray(I).astype(np.int64)
    nq, nb = S.shape
    assert D.shape == (nq, k) and I.shape == (nq, k), (D.shape, I.shape, (nq, k))
    n = min(k, nb)
    worst = 0.0
    for q in range(nq):
        ids = I[q, :n]
        assert (I[q, n:] == -1).all(), f"query {q}: ids behind slot {n}: {I[q, n:].tolist()}"
        assert ((ids >= 0) & (ids < nb)).all(), f"query {q}: ids out of range: {ids.tolist()}"
        assert np.unique(ids).size == n, f"query {q}: an id repeats: {ids.tolist()}"
        s, dq = S[q, ids], D[q, :n]
        err = np.abs(dq - s)
        assert (err <= bar).all(), f"query {q}: score error {err.max():.3e} at slot {int(err.argmax())} (bar {bar:.1e})"
        worst = max(worst, float(err.max())) if n else worst
        step = np.diff(dq)
        assert (step <= 0).all(), f"query {q}: D rises at slot {int(np.argmax(step > 0)) + 1}"
        tied = step == 0
        assert (np.diff(ids)[tied] > 0).all(), f"query {q}: equal scores out of id order: {ids.tolist()}"
        if n < nb:
            rest = S[q].copy()
            rest[ids] = -np.inf
            over = rest.max() - s.min()
            assert over <= gap, f"query {q}: row {int(rest.argmax())} left out, {over:.3e} above the weakest returned (gap {gap:.1e})"
        if n > 1:
            low = np.minimum.accumulate(s)[:-1] - s[1:]  # the weakest of the slots before s, against slot s
            assert (low >= -gap).all(), f"query {q}: slot {int(low.argmin()) + 1} is {-low.min():.3e} better than one before it"
    return worst


# ---- the cases -----------------------------------------------------------------------------------------------------------
# Stream class: U = fragments per inner-loop iteration of lvs_stream_kernel's instantiation ("general": jper a multiple of none
# of 16 / 24 / 8 - the fragment state machine with 16), nqb = 32-query blocks per workgroup, groups = sibling workgroups per
# corpus range, seed = U of the SEED instantiation that scans the sample first (None: no sample), jper = 16-half fragments per
# K segment, nseg = K segments, nj = jper * nseg fragments per 32-row block.
StreamClass = namedtuple("StreamClass", "U nqb groups seed jper nseg")
Case = namedtuple("Case", "name d bmode qmode nq nb k metric kernel cls seed")
STREAM, TILE = "lvs_stream_kernel", "lvs_tile_kernel"


def _s(d, bmode, qmode, nq, k, metric, cls, nb=4133, seed=0):
    name = f"stream-d{d}-{'FS'[bmode]}{'FS'[qmode]}-q{nq}-k{k}-{'IL'[metric]}-nb{nb}"
    return Case(name, d, bmode, qmode, nq, nb, k, metric, STREAM, cls, seed)


def _t(d, bmode, qmode, nq, nb, k, metric, seed=0):
    name = f"tile-d{d}-{'FS'[bmode]}{'FS'[qmode]}-q{nq}-nb{nb}-k{k}-{'IL'[metric]}"
    return Case(name, d, bmode, qmode, nq, nb, k, metric, TILE, None, seed)


G = "general"
STREAM_CASES = [
    _s(192, F16, F16, 1, 10, IP, StreamClass(G, 1, 1, None, 12, 1)),         # nj 12 < 16: no wrap inside a block
    _s(312, F16, F16, 20, 16, L2, StreamClass(G, 1, 1, None, 20, 1)),        # nj 20 -> 32 steps, 12 of padding
    _s(192, SPLIT, SPLIT, 7, 5, IP, StreamClass(G, 1, 1, None, 12, 3)),      # three segments, nj 36
    _s(312, SPLIT, F16, 32, 10, IP, StreamClass(G, 1, 1, None, 20, 2)),      # two segments, nj 40
    _s(448, F16, F16, 64, 10, IP, StreamClass(G, 2, 1, None, 28, 1)),        # two query blocks, eight waves
    _s(448, F16, F16, 96, 15, L2, StreamClass(G, 3, 1, None, 28, 1)),        # three query blocks
    _s(640, F16, F16, 1, 56, IP, StreamClass(8, 1, 1, None, 40, 1)),         # U8, five iterations per run, 64 slots
    _s(1100, F16, F16, 5, 10, IP, StreamClass(24, 1, 1, None, 72, 1)),       # U24, three iterations per run
    _s(1100, F16, F16, 40, 16, L2, StreamClass(8, 2, 1, None, 72, 1)),       # two blocks: no U24 -> U8, nine iterations
    _s(1024, F16, F16, 1, 10, IP, StreamClass(16, 1, 1, None, 64, 1)),       # U16, four iterations
    _s(1024, F16, F16, 33, 10, IP, StreamClass(16, 2, 1, None, 64, 1)),
    _s(1024, SPLIT, SPLIT, 1, 10, L2, StreamClass(16, 1, 1, None, 64, 3)),   # 128 query fragments, ~148 KB of LDS
    _s(1536, F16, F16, 1, 10, IP, StreamClass(16, 1, 1, None, 96, 1)),
    _s(1536, F16, F16, 33, 10, IP, StreamClass(16, 1, 2, None, 96, 1)),      # two sibling groups of one block
    _s(1920, F16, F16, 3, 30, IP, StreamClass(24, 1, 1, None, 120, 1)),      # U24, five iterations
    _s(2240, F16, F16, 1, 56, IP, StreamClass(G, 1, 1, None, 140, 1)),       # the last fp16 width that fits the LDS
    _s(1088, SPLIT, SPLIT, 1, 56, L2, StreamClass(G, 1, 1, None, 68, 3)),    # the last hi|lo width that fits
    _s(1024, F16, F16, 8, 10, IP, StreamClass(16, 1, 1, 16, 64, 1), nb=33000),
    _s(312, F16, F16, 40, 10, L2, StreamClass(G, 2, 1, G, 20, 1), nb=33000),
    _s(1100, F16, F16, 2, 10, IP, StreamClass(24, 1, 1, 8, 72, 1), nb=33000),  # the SEED instantiation has no U24 -> U8
]
TILE_CASES = [
    _t(2241, F16, F16, 1, 5000, 10, IP),       # one past the stream kernel's LDS edge
    _t(1089, SPLIT, SPLIT, 1, 5000, 10, IP),   # one past the hi|lo edge
    # the literal single-query call with float32 embeddings.  Ten slots: a dropped lo segment moves a score by about 4.4e-6 rms
    # here, and the largest of the ten is 7.1e-6 .. 1.18e-5 over seeds 0 .. 7: on seeds 0, 1, 3 and 4 the checker accepts that
    # answer, so the case runs on seed 5, the one with the largest (tests/test_widths_host.py asserts the rejection)
    _t(1536, SPLIT, SPLIT, 1, 20000, 10, IP, seed=5),
    _t(1024, F16, F16, 300, 3001, 10, IP),
    _t(1536, SPLIT, SPLIT, 130, 3000, 10, L2),
    _t(1536, F16, SPLIT, 260, 3000, 7, IP),
    _t(1536, F16, SPLIT, 260, 3000, 7, L2),
    _t(1536, SPLIT, F16, 260, 3000, 7, IP),
    _t(1536, SPLIT, F16, 260, 3000, 7, L2),
    _t(3072, SPLIT, SPLIT, 300, 3000, 15, L2),  # 144 K-steps
    _t(4096, F16, F16, 300, 3000, 16, IP),      # 128-query geometry
    _t(4096, SPLIT, SPLIT, 40, 2000, 56, IP),
    _t(1536, F16, F16, 64, 3000, 100, IP),      # selection passes
    _t(1024, F16, F16, 32, 60000, 100, IP),     # two-phase
]
# one-pass certified search (search_keys(one_pass=True)): nq = 300, nb = 4 000, hi|lo on both sides
CERT_CASES = [Case(f"cert-d{d}-k{k}-{'IL'[m]}", d, SPLIT, SPLIT, 300, 4000, k, m, None, None, 0)
              for d in (1536, 3072) for k in (1, 10) for m in (IP, L2)]
TOPK_CASES = STREAM_CASES + TILE_CASES + CERT_CASES

_DATA = {}


def case_data(c):
    """(xb, xq) float32 as the caller holds them (fp16-representable for F16 operands) - made once per shape and seed."""
    key = (c.nb, c.nq, c.d, c.seed)
    if key not in _DATA:
        if len(_DATA) >= 2:
            _DATA.clear()  # (the widest pair is 125 MB)
        xb = synth.corpus(c.nb, c.d, seed=100 + c.seed)
        xq, _ = synth.queries(xb, c.nq, seed=200 + c.seed)
        _DATA[key] = (xb, xq)
    xb, xq = _DATA[key]
    if c.metric == L2:
        xb = xb * L2_CORPUS_SCALE
    return xb, xq


def case_scores(c, xb, xq):
    return scores64(stored64(xb, c.bmode), stored64(xq, c.qmode), c.metric)
