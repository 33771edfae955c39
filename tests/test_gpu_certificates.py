"""The kernels that decide what the exact paths may skip - lvs_certify_topk[_banded], lvs_margin_select[_stats],
lvs_nearest3_select - called through the C ABI on synthetic arrays and compared with the float64 restatements of their rules
(tests/cert_rules.py): at the decision boundary itself with inputs for which every float32 operation is exact, on edge
contents (empty keys, infinities, NaN, NULL norms), on random inputs wherever the float64 slack is outside float32 rounding,
and the compaction of the listed indices at every block / wave edge.  Plus the two small kernels the certified search
depends on, lvs_sort_keys_desc and lvs_rescore_keys, and lvs_resolve_pairs, which claims the latter's arithmetic."""
import ctypes
import itertools

import numpy as np
import pytest

import cert_rules as cr
from lotus_amd import _capi
from lotus_amd.backend import _ptr
from oracle.flat import pack_keys, unpack_keys

pytestmark = pytest.mark.gpu
F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
SENT = cr.SENT
U = 2.0 ** -6               # the score step of the exact cases
ROUND = 8 * 2.0 ** -24      # random cases: a query is decided by the rule when |slack| > ROUND * (|best| + |other| + bound)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _keys_dev(be, keys):
    return be.to_device(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))


def _f32_dev(be, a):
    return None if a is None else be.to_device(np.ascontiguousarray(a, dtype=np.float32))


_lists = cr.index_lists


def _certify(be, approx, exact, qn, k1, k, scale, slack, band, entry="lvs_certify_topk_banded"):
    nq = approx.shape[0]
    a, e, q = _keys_dev(be, approx), _keys_dev(be, exact), _f32_dev(be, qn)
    tail = (float(band),) if entry.endswith("banded") else ()
    return _lists(be, nq, 1, lambda out, cnt: be._c(entry, _ptr(a), _ptr(e), _ptr(q), nq, k1, k, float(scale), float(slack),
                                                    *tail, _ptr(out), _ptr(cnt), be._stream()))[0]


def _margin(be, keys, sec, qn, scale, slack):
    nq = keys.shape[0]
    kd, s, q = _keys_dev(be, keys), _f32_dev(be, sec), _f32_dev(be, qn)
    return _lists(be, nq, 1, lambda out, cnt: be._c("lvs_margin_select", _ptr(kd), _ptr(s), _ptr(q), nq, float(scale),
                                                    float(slack), _ptr(out), _ptr(cnt), be._stream()))[0]


def _coef(coef5):
    return (ctypes.c_float * 5)(*[float(c) for c in coef5])


def _margin_stats(be, keys, sec, qn, stats, coef5):
    nq = keys.shape[0]
    kd, s, q, st = _keys_dev(be, keys), _f32_dev(be, sec), _f32_dev(be, qn), _f32_dev(be, stats)
    c = _coef(coef5)
    return _lists(be, nq, 1, lambda out, cnt: be._c("lvs_margin_select_stats", _ptr(kd), _ptr(s), _ptr(q), nq, _ptr(st),
                                                    ctypes.addressof(c), _ptr(out), _ptr(cnt), be._stream()))[0]


def _nearest3(be, keys1, keys2, sec, third, qn, stats, coef5):
    """-> class per query (cert_rules.CERTIFIED / PAIR / OPEN); a query in both lists fails"""
    nq = keys1.shape[0]
    k1, k2 = _keys_dev(be, keys1), _keys_dev(be, keys2)
    s, t, q, st = _f32_dev(be, sec), _f32_dev(be, third), _f32_dev(be, qn), _f32_dev(be, stats)
    c = _coef(coef5)
    pair, opn = _lists(be, nq, 2, lambda po, oo, cnt: be._c("lvs_nearest3_select", _ptr(k1), _ptr(k2), _ptr(s), _ptr(t), _ptr(q),
                                                            nq, _ptr(st), ctypes.addressof(c), _ptr(po), _ptr(oo), _ptr(cnt),
                                                            be._stream()))
    assert not (pair & opn).any()
    return np.where(pair, cr.PAIR, np.where(opn, cr.OPEN, cr.CERTIFIED))


def _exact32(a):
    """float64 values that must be float32 numbers already (the exact cases rest on it)"""
    a = np.asarray(a, dtype=np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return a.astype(np.float32)


QNS = (1.0, 4.0, 16.0)
BASES = (-3.5, -0.25, 0.0, 0.75, 2.0 + U)   # negative scores: squared L2
STEPS = (-1, 0, 1)                          # margin == bound - ulp | == bound | == bound + ulp
STATS = [((1.0, 0.0), (0.5, 0.25, 0.125, 0.0625, 0.03125)), ((4.0, 0.25), (0.5, 0.25, 0.125, 0.0625, 0.03125)),
         ((4.0, 0.25), (0.25, 0.0, 0.0, 0.0, 0.0)), ((1.0, 0.25), (0.0, 0.0, 0.0, 0.0, 0.0)), ((4.0, 0.0), (0.0, 0.0, 1.0, 0.0, 0.5))]


def _grid(*axes):
    g = np.array(list(itertools.product(*axes)), dtype=np.float64)
    return [g[:, i].copy() for i in range(g.shape[1])]


# ---- exact boundary cases: no tolerance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_qn", [True, False])
def test_margin_select_at_the_boundary(hip_backend, with_qn):
    """best - second == bound - 2^-6 | bound | bound + 2^-6 with every float32 operation exact (|q| in {1, 2, 4}, power-of-two
    coefficients, scores that are multiples of 2^-6): the rule is strict, equality is listed."""
    be = hip_backend
    qn, sec, j = _grid(QNS, BASES, STEPS)
    qn_arg = _exact32(qn) if with_qn else None
    norm = np.sqrt(qn) if with_qn else np.ones_like(qn)
    ids = np.arange(qn.size) + 3
    for scale, slack in itertools.product((0.0, 0.25), (0.0, 0.125)):
        best = _exact32(sec + (scale * norm + slack) + j * U)
        keys = pack_keys(best, ids)
        rule, sl = cr.margin(keys, sec, qn_arg, scale, slack)
        assert np.array_equal(sl, j * U) and np.array_equal(rule, j <= 0)
        assert np.array_equal(_margin(be, keys, sec, qn_arg, scale, slack), rule), (scale, slack)
    for stats, coef in STATS:
        sc, sk = cr.stats_scale_slack(stats, coef)
        best = _exact32(sec + (sc * norm + sk) + j * U)
        keys = pack_keys(best, ids)
        rule, sl = cr.margin_stats(keys, sec, qn_arg, stats, coef)
        assert np.array_equal(sl, j * U) and np.array_equal(rule, j <= 0)
        assert np.array_equal(_margin_stats(be, keys, sec, qn_arg, stats, coef), rule), (stats, coef)


@pytest.mark.parametrize("with_qn", [True, False])
def test_nearest3_select_at_both_boundaries(hip_backend, with_qn):
    """The same for the three-way split: best - second around the bound decides certified | pair (the third score far below),
    best - third around it decides pair | open (the second score equal to the best)."""
    be = hip_backend
    qn, base, j = _grid(QNS, BASES, STEPS)
    qn_arg = _exact32(qn) if with_qn else None
    norm = np.sqrt(qn) if with_qn else np.ones_like(qn)
    n = qn.size
    keys2 = pack_keys(np.zeros(n, np.float32), np.arange(n) + 1000)
    for stats, coef in STATS:
        sc, sk = cr.stats_scale_slack(stats, coef)
        bound = sc * norm + sk
        # certified | pair: second = base, best = base + bound + j ulp, third = base - 1 - bound (a clear pair margin)
        best = _exact32(base + bound + j * U)
        keys1 = pack_keys(best, np.arange(n))
        third = _exact32(base - 1 - bound)
        cls, s2, _ = cr.nearest3(keys1, keys2, base, third, qn_arg, stats, coef)
        assert np.array_equal(s2, j * U) and np.array_equal(cls, np.where(j > 0, cr.CERTIFIED, cr.PAIR))
        assert np.array_equal(_nearest3(be, keys1, keys2, base, third, qn_arg, stats, coef), cls), (stats, coef)
        # pair | open: best = second = base, third = base - bound - j ulp
        keys1 = pack_keys(_exact32(base), np.arange(n))
        third = _exact32(base - bound - j * U)
        cls, s2, s3 = cr.nearest3(keys1, keys2, base, third, qn_arg, stats, coef)
        assert np.array_equal(s3, j * U) and np.array_equal(cls, np.where(j > 0, cr.PAIR, cr.OPEN))
        assert np.array_equal(_nearest3(be, keys1, keys2, base, third, qn_arg, stats, coef), cls), (stats, coef)


def _certify_case(k1, k, band, variant, qn, base, j, scale, slack, norm):
    """approx / exact [nq, k1] whose decisive scores sit j score steps from the boundary.  variant: which term is the largest
    one-pass score a row outside the list may have had - 'last' (the last slot), 'band' (k-th slot - band * bound, the last
    slot lower) or 'empty' (the same with an EMPTY last slot)."""
    n = qn.size
    bound = scale * norm + slack
    approx, exact = np.full((n, k1), 100.0), np.full((n, k1), 100.0)
    if band == 0 or k1 == k:
        s_min = base.copy()
        approx[:, k1 - 1] = base
        if k1 > k:
            approx[:, k - 1:k1 - 1] = (base + 3)[:, None]   # the k-th one-pass slot is NOT the slot band 0 reads
    elif variant == "last":
        s_min = base.copy()
        approx[:, k:] = base[:, None]
        approx[:, k - 1] = base + 0.5 * band * bound         # k-th slot - band * bound is below the last slot
    else:
        s_min = base - band * bound
        approx[:, k - 1:] = base[:, None]
        approx[:, k1 - 1] = s_min - 1
    s_k = s_min + bound + j * U
    exact[:, k - 1] = s_k
    exact[:, k:] = (s_k - 1)[:, None]
    ids = np.arange(n * k1).reshape(n, k1)
    ak, ek = pack_keys(_exact32(approx), ids), pack_keys(_exact32(exact), ids)
    if variant == "empty" and band > 0 and k1 > k:
        ak[:, k1 - 1] = 0
    return ak, ek


@pytest.mark.parametrize("k1,k", [(3, 2), (4, 4), (2, 1), (1, 1), (6, 3)])
def test_certify_topk_at_the_boundary(hip_backend, k1, k):
    """k-th exact score == largest possible outside score + bound - 2^-6 | + 0 | + 2^-6, all float32 operations exact:
    band 0 (both entry points) and bands 2 and 2.5, with the last slot / the band term / the band term and an empty last
    slot deciding, k1 == k and k == 1 included.  Equality is open."""
    be = hip_backend
    qn, base, j = _grid(QNS, BASES, STEPS)
    for with_qn, scale, slack in itertools.product((True, False), (0.0, 0.25), (0.0, 0.125)):
        qn_arg = _exact32(qn) if with_qn else None
        norm = np.sqrt(qn) if with_qn else np.ones_like(qn)
        for band, variant in [(0.0, "last"), (2.0, "last"), (2.0, "band"), (2.5, "band"), (2.5, "empty"), (2.0, "empty")]:
            ak, ek = _certify_case(k1, k, band, variant, qn, base, j, scale, slack, norm)
            rule, sl = cr.certify(ak, ek, qn_arg, k1, k, scale, slack, band)
            assert np.array_equal(sl, j * U) and np.array_equal(rule, j <= 0), (band, variant)
            assert np.array_equal(_certify(be, ak, ek, qn_arg, k1, k, scale, slack, band), rule), (band, variant, scale, slack)
            if band == 0:
                assert np.array_equal(_certify(be, ak, ek, qn_arg, k1, k, scale, slack, band, entry="lvs_certify_topk"), rule)


# ---- edge contents ---------------------------------------------------------------------------------------------------------
def test_certify_topk_edge_contents(hip_backend):
    """Empty last slot with a filled k-th slot and the reverse, a banded list with an empty last slot or an empty k-th
    one-pass slot, negative (squared L2) scores, NaN |q|^2, q_norms_sq == NULL - as the rule decides them."""
    be = hip_backend
    k1, k = 3, 2
    nan = np.nan
    #        approx (0: empty)       exact                   |q|^2
    rows = [((9, 8, 0), (9, 1, 0.5), 4.0),         # 0 unfilled list: band 0 never opens it; banded: 1 > 8 - band * bound + bound ?
            ((9, 8, 1), (9, 0, 0), 4.0),           # 1 k-th exact slot empty (fewer than k rows): never open
            ((9, 8, 1), (9, 1.75, 0), 4.0),        # 2 band 0: 1.75 > 1 + 0.625
            ((9, 8, 1), (9, 1.625, 0), 4.0),       # 3 band 0: equality -> open
            ((9, 8, 1), (9, 8.5, 1), nan),         # 4 NaN bound: open
            ((-7, -7.5, -8), (-7, -7.25, -9), 4.0),    # 5 negative scores: -7.25 > -8 + 0.625
            ((-7, -7.5, -8), (-7, -7.375, -9), 4.0),   # 6 equality
            ((9, 5, 0), (9, 4.5, 0), 4.0),         # 7 band 2, empty last: 4.5 > 5 - 1.25 + 0.625 = 4.375
            ((9, 5, 0), (9, 4.375, 0), 4.0),       # 8 equality
            ((9, 0, 0), (9, 4, 0), 4.0),           # 9 k-th one-pass slot empty: never open
            ((9, 5, 4.5), (9, 5.125, 0), 4.0),     # 10 band 2: last slot 4.5 > 5 - 1.25: 5.125 > 4.5 + 0.625 is false
            ((9, 5, 4.5), (9, 5.25, 0), 4.0)]      # 11 ... 5.25 > 5.125
    n = len(rows)
    ids = np.arange(n * k1).reshape(n, k1) + 1
    av, ev = np.float32([r[0] for r in rows]), np.float32([r[1] for r in rows])
    ak = np.where(av == 0, np.uint64(0), pack_keys(av, ids))
    ek = np.where(ev == 0, np.uint64(0), pack_keys(ev, ids))
    qn = np.float32([r[2] for r in rows])
    scale, slack = 0.25, 0.125
    want = {0.0: [0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0], 2.0: [1, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1, 0]}
    for band in (0.0, 2.0):
        rule, _ = cr.certify(ak, ek, qn, k1, k, scale, slack, band)
        assert list(rule.astype(int)) == want[band], band
        assert np.array_equal(_certify(be, ak, ek, qn, k1, k, scale, slack, band), rule)
    assert np.array_equal(_certify(be, ak, ek, qn, k1, k, scale, slack, 0.0, entry="lvs_certify_topk"),
                          cr.certify(ak, ek, qn, k1, k, scale, slack, 0.0)[0])
    for band in (0.0, 2.0, 2.5):   # q_norms_sq == NULL: |q| = 1 (the NaN row is then decided by its scores)
        rule, _ = cr.certify(ak, ek, None, k1, k, scale, slack, band)
        assert not rule[4]
        assert np.array_equal(_certify(be, ak, ek, None, k1, k, scale, slack, band), rule)


def test_margin_and_nearest3_edge_contents(hip_backend):
    """Empty winner key (never listed), second = -inf (one corpus row: certified), second = +inf, NaN second, NaN |q|^2,
    inf - inf (always listed), third = -inf without a runner-up key (never a pair), negative scores, q_norms_sq == NULL."""
    be = hip_backend
    inf, nan = np.inf, np.nan
    #          best   second third  key2  |q|^2
    rows = [(1.0, 0.0, -1.0, 1, 4.0),      # 0 1 > 0.625 certified
            (0.0, 0.0, 0.0, 1, 4.0),       # 1 EMPTY winner key (set below)
            (1.0, -inf, -inf, 0, 4.0),     # 2 one corpus row
            (1.0, inf, 0.0, 1, 4.0),       # 3 second = +inf: listed; best - third = 1 > bound: a pair
            (1.0, nan, nan, 1, 4.0),       # 4 NaN second and third: open
            (1.0, 0.0, -1.0, 1, nan),      # 5 NaN |q|^2: open
            (inf, inf, inf, 1, 4.0),       # 6 inf - inf: open
            (1.0, 1.0, -inf, 0, 4.0),      # 7 a tie, third = -inf but NO runner-up key: open, never a pair
            (1.0, 1.0, -inf, 1, 4.0),      # 8 two corpus rows that tie: a pair
            (-4.0, -4.5, -4.75, 1, 4.0),   # 9 negative scores: 0.5 <= 0.625 listed; 0.75 > 0.625 pair
            (-4.0, -4.625, -6.0, 1, 4.0),  # 10 equality: listed, pair
            (-4.0, -4.75, -6.0, 1, 4.0),   # 11 certified
            (-4.0, -4.5, -4.625, 1, 4.0)]  # 12 third at equality: open
    best, sec, third = (np.float32([r[i] for r in rows]) for i in range(3))
    n = len(rows)
    keys1 = pack_keys(best, np.arange(n) + 7)
    keys1[1] = 0
    keys2 = np.where(np.array([r[3] for r in rows]) == 1, pack_keys(sec, np.arange(n) + 100), np.uint64(0))
    qn = np.float32([r[4] for r in rows])
    stats, coef = (4.0, 0.25), (0.25, 0.0625, 0.125, 0.0, 0.0)   # scale 0.25, slack 0.125: bound 0.625 at |q| = 2
    assert cr.stats_scale_slack(stats, coef) == (0.25, 0.125)
    rule, _ = cr.margin(keys1, sec, qn, 0.25, 0.125)
    assert list(rule.astype(int)) == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]
    assert np.array_equal(_margin(be, keys1, sec, qn, 0.25, 0.125), rule)
    assert np.array_equal(_margin_stats(be, keys1, sec, qn, stats, coef), rule)
    cls, _, _ = cr.nearest3(keys1, keys2, sec, third, qn, stats, coef)
    C, P, O = cr.CERTIFIED, cr.PAIR, cr.OPEN
    assert list(cls) == [C, C, C, P, O, O, O, O, P, P, P, C, O]
    assert np.array_equal(_nearest3(be, keys1, keys2, sec, third, qn, stats, coef), cls)
    # q_norms_sq == NULL: |q| = 1, bound 0.375
    rule, _ = cr.margin(keys1, sec, None, 0.25, 0.125)
    assert not rule[5] and not rule[9]
    assert np.array_equal(_margin(be, keys1, sec, None, 0.25, 0.125), rule)
    assert np.array_equal(_margin_stats(be, keys1, sec, None, stats, coef), rule)
    cls, _, _ = cr.nearest3(keys1, keys2, sec, third, None, stats, coef)
    assert np.array_equal(_nearest3(be, keys1, keys2, sec, third, None, stats, coef), cls)


# ---- random cases: the rule decides wherever float32 rounding cannot --------------------------------------------------------
def _random_margins(rng, n, bound):
    """(other, best): float32 scores over four decades whose margin best - other lies a relative 1e-6 .. 0.3 of
    (|best| + |other| + bound) on either side of `bound` - far more often near the boundary than random data ever is, yet
    (almost always) outside the zone float32 rounding may decide"""
    other = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    off = 0.3 * 10.0 ** rng.uniform(-5.5, 0, n) * rng.choice([-1.0, 1.0], n) * (2 * np.abs(other) + bound)
    return other, (other.astype(np.float64) + bound + off).astype(np.float32)


def _decided(slack, *magnitudes):
    zone = ROUND * sum(np.abs(np.asarray(m, dtype=np.float64)) for m in magnitudes)
    out = np.abs(slack) > zone
    assert (~out).mean() <= 0.01, (~out).mean()   # the case is about the rule, not about rounding
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_margin_select_on_random_inputs(hip_backend, seed):
    """Every query whose float64 slack exceeds 8 * 2^-24 * (|best| + |second| + bound) - the float32 roundings of sqrt, scale *
    |q| + slack (three) and best - second (one) - is decided as the rule decides it; at most 1 % may lie inside that zone."""
    be = hip_backend
    rng = np.random.default_rng(seed)
    n = 20_000
    qn = (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    scale, slack = float(np.float32(0.37)), float(np.float32(0.011))
    bound = scale * np.sqrt(qn.astype(np.float64)) + slack
    sec, best = _random_margins(rng, n, bound)
    keys = pack_keys(best, rng.integers(0, 1 << 31, n))
    rule, sl = cr.margin(keys, sec, qn, scale, slack)
    ok = _decided(sl, best, sec, bound)
    assert 0.3 < rule.mean() < 0.7
    assert np.array_equal(_margin(be, keys, sec, qn, scale, slack)[ok], rule[ok])
    stats = np.float32([2.3, 1.7e-4])
    coef = np.float32([4.0, 2e-3, 1e-6, 1e-5, 1.6e-5])
    sc, sk = cr.stats_scale_slack(stats, coef)
    bound = sc * np.sqrt(qn.astype(np.float64)) + sk
    sec, best = _random_margins(rng, n, bound)
    keys = pack_keys(best, rng.integers(0, 1 << 31, n))
    rule, sl = cr.margin_stats(keys, sec, qn, stats, coef)
    ok = _decided(sl, best, sec, bound)
    assert np.array_equal(_margin_stats(be, keys, sec, qn, stats, coef)[ok], rule[ok])


@pytest.mark.parametrize("seed", [0, 1])
def test_nearest3_select_on_random_inputs(hip_backend, seed):
    be = hip_backend
    rng = np.random.default_rng(10 + seed)
    n = 20_000
    qn = (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    stats = np.float32([1.9, 3.1e-4])
    coef = np.float32([4.0, 2e-3, 1e-6, 1e-5, 1.6e-5])
    sc, sk = cr.stats_scale_slack(stats, coef)
    bound = sc * np.sqrt(qn.astype(np.float64)) + sk
    sec, best = _random_margins(rng, n, bound)
    # the third score: the same construction against the SAME best (second >= third is not needed by the rule)
    third = (best.astype(np.float64) - bound - 0.3 * 10.0 ** rng.uniform(-5.5, 0, n) * rng.choice([-1.0, 1.0], n)
             * (2 * np.abs(best) + bound)).astype(np.float32)
    keys1 = pack_keys(best, rng.integers(0, 1 << 31, n))
    keys2 = np.where(rng.random(n) < 0.9, pack_keys(sec, rng.integers(0, 1 << 31, n)), np.uint64(0))
    cls, s2, s3 = cr.nearest3(keys1, keys2, sec, third, qn, stats, coef)
    ok = _decided(s2, best, sec, bound) & _decided(s3, best, third, bound)
    assert min((cls == c).mean() for c in (cr.CERTIFIED, cr.PAIR, cr.OPEN)) > 0.1
    assert np.array_equal(_nearest3(be, keys1, keys2, sec, third, qn, stats, coef)[ok], cls[ok])


@pytest.mark.parametrize("band", [0.0, 2.0])
def test_certify_topk_on_random_inputs(hip_backend, band):
    """Random lists with the k-th exact score a relative 1e-6 .. 0.3 on either side of the boundary.  Band 2: the band term is
    a_k - 2 bound (the product is exact), so the expression carries the three roundings of the bound (net once: -2 e + e), one of
    the subtraction and one of the sum - inside 8 * 2^-24 * (|s_k| + |outside score| + bound) like the plain certificate."""
    be = hip_backend
    rng = np.random.default_rng(int(band) + 20)
    n, k1, k = 20_000, 5, 3
    qn = (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    scale, slack = float(np.float32(0.013)), float(np.float32(2e-3))
    bound = scale * np.sqrt(qn.astype(np.float64)) + slack
    last = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    a_k = (last + rng.uniform(0, 2, n) * (band if band else 1.0) * bound).astype(np.float32)   # either term may be the larger
    s_min = np.maximum(a_k.astype(np.float64) - band * bound, last) if band else last.astype(np.float64)
    off = 0.3 * 10.0 ** rng.uniform(-5.5, 0, n) * rng.choice([-1.0, 1.0], n) * (2 * np.abs(s_min) + bound)
    s_k = (s_min + bound + off).astype(np.float32)
    approx = np.stack([a_k + 2, a_k + 1, a_k, a_k, last], axis=1).astype(np.float32)
    exact = np.stack([s_k + 2, s_k + 1, s_k, s_k - 1, s_k - 2], axis=1).astype(np.float32)
    ids = rng.integers(0, 1 << 31, (n, k1))
    ak, ek = pack_keys(approx, ids), pack_keys(exact, ids)
    rule, sl = cr.certify(ak, ek, qn, k1, k, scale, slack, band)
    s_min = s_k.astype(np.float64) - sl - bound   # the restatement's own outside score
    ok = _decided(sl, s_k, s_min, bound)
    assert 0.3 < rule.mean() < 0.7
    assert np.array_equal(_certify(be, ak, ek, qn, k1, k, scale, slack, band)[ok], rule[ok])


# ---- compaction ------------------------------------------------------------------------------------------------------------
_patterns = cr.open_patterns


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_certify_topk_compaction(hip_backend, nq):
    """256 queries per block, one ballot and one atomic per wave: the listed SET equals the rule's at every wave / block edge
    and open pattern; no duplicates, the counter is added to, nothing beyond the count is written (checked in _lists)."""
    be = hip_backend
    k1, k = 3, 2
    ids = np.arange(nq * k1).reshape(nq, k1)
    ak = pack_keys(np.tile(np.float32([9, 8, 1]), (nq, 1)), ids)
    for name, want in _patterns(nq, np.random.default_rng(nq)):
        ek = pack_keys(np.stack([np.full(nq, 9.0), np.where(want, 0.0, 8.0), np.full(nq, -1.0)], axis=1).astype(np.float32), ids)
        for band in (0.0, 2.0):
            assert np.array_equal(cr.certify(ak, ek, None, k1, k, 0.5, 0.0, band)[0], want)
            assert np.array_equal(_certify(be, ak, ek, None, k1, k, 0.5, 0.0, band), want), (name, band)
        assert np.array_equal(_certify(be, ak, ek, None, k1, k, 0.5, 0.0, 0.0, entry="lvs_certify_topk"), want), name


SELECT_SIZES = cr.SELECT_SIZES


@pytest.mark.parametrize("nq", SELECT_SIZES)
def test_margin_select_compaction(hip_backend, nq):
    """Two sweeps per workgroup of `per_block` queries, one reservation each: both forms at the block edges, with blocks that
    list nothing, everything, their first / last query only."""
    be = hip_backend
    keys = pack_keys(np.full(nq, 2.0, np.float32), np.arange(nq))
    stats, coef = (4.0, 0.25), (0.5, 0.25, 0.0, 0.0, 0.0)   # scale 0.75, slack 0
    for name, want in _patterns(nq, np.random.default_rng(nq)):
        sec = np.where(want, 2.0, 0.0).astype(np.float32)
        assert np.array_equal(cr.margin(keys, sec, None, 0.5, 0.0)[0], want)
        assert np.array_equal(cr.margin_stats(keys, sec, None, stats, coef)[0], want)
        assert np.array_equal(_margin(be, keys, sec, None, 0.5, 0.0), want), name
        assert np.array_equal(_margin_stats(be, keys, sec, None, stats, coef), want), name


@pytest.mark.parametrize("nq", SELECT_SIZES)
def test_nearest3_select_compaction(hip_backend, nq):
    """Both lists and both counters of one launch: pairs only, open only, every query in one of the two, and two unrelated
    patterns - one list empty and the other full included."""
    be = hip_backend
    rng = np.random.default_rng(nq + 1)
    keys1 = pack_keys(np.full(nq, 4.0, np.float32), np.arange(nq))
    keys2 = pack_keys(np.full(nq, 4.0, np.float32), np.arange(nq) + 1)
    stats, coef = (4.0, 0.25), (0.5, 0.25, 0.125, 0.0625, 0.03125)   # bound 1.125 at |q| = 1
    none = np.zeros(nq, bool)
    pats = _patterns(nq, rng)
    cases = []
    for name, p in pats:
        cases += [(name + " | none", p, none), ("none | " + name, none, p), (name + " | the rest", p, ~p)]
    cases.append(("random | every 64th", pats[6][1], pats[4][1] & ~pats[6][1]))
    if nq > 2049:   # the large size: the patterns that tell blocks apart are enough
        cases = [c for c in cases if c[0] in ("all | none", "none | all", "alternating | the rest", "random 0.4 % | the rest",
                                              "first | the rest", "none | last", "every 64th | none", "random | every 64th")]
    for name, pair, opn in cases:
        want = np.where(pair, cr.PAIR, np.where(opn, cr.OPEN, cr.CERTIFIED))
        sec = np.where(pair | opn, 4.0, 0.0).astype(np.float32)
        third = np.where(opn, 4.0, 0.0).astype(np.float32)
        assert np.array_equal(cr.nearest3(keys1, keys2, sec, third, None, stats, coef)[0], want)
        assert np.array_equal(_nearest3(be, keys1, keys2, sec, third, None, stats, coef), want), name


# ---- argument checks -------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(hip_backend):
    import torch

    be = hip_backend
    buf = torch.zeros((64,), dtype=torch.int64, device=be.device)
    f = torch.ones((8,), dtype=torch.float32, device=be.device)
    p, s = _ptr(buf), be._stream()
    einval = dict(match="status %d" % _capi.EINVAL)

    def certify(k1, k, scale, slack, band):
        be._c("lvs_certify_topk_banded", p, p, _ptr(f), 2, k1, k, scale, slack, band, p, p, s)

    certify(3, 2, 0.5, 0.5, 2.0)
    for bad in [(2, 3, 0.5, 0.5, 2.0), (3, 0, 0.5, 0.5, 2.0), (3, 2, -0.5, 0.5, 2.0), (3, 2, 0.5, -0.5, 2.0), (3, 2, 0.5, 0.5, -2.0)]:
        with pytest.raises(_capi.LotusHipError, **einval):
            certify(*bad)
    for bad in [(2, 3, 0.5, 0.5), (3, 0, 0.5, 0.5), (3, 2, -0.5, 0.5), (3, 2, 0.5, -0.5)]:
        with pytest.raises(_capi.LotusHipError, **einval):
            be._c("lvs_certify_topk", p, p, _ptr(f), 2, *bad, p, p, s)
    for scale, slack in [(-0.5, 0.5), (0.5, -0.5)]:
        with pytest.raises(_capi.LotusHipError, **einval):
            be._c("lvs_margin_select", p, _ptr(f), _ptr(f), 2, scale, slack, p, p, s)
    for neg in range(5):
        c = _coef([-1.0 if i == neg else 0.5 for i in range(5)])
        with pytest.raises(_capi.LotusHipError, **einval):
            be._c("lvs_margin_select_stats", p, _ptr(f), _ptr(f), 2, _ptr(f), ctypes.addressof(c), p, p, s)
        with pytest.raises(_capi.LotusHipError, **einval):
            be._c("lvs_nearest3_select", p, p, _ptr(f), _ptr(f), _ptr(f), 2, _ptr(f), ctypes.addressof(c), p, p, p, s)
    with pytest.raises(_capi.LotusHipError, **einval):
        be._c("lvs_sort_keys_desc", p, 1, 65, s)
    be.synchronize()
    assert int(buf.abs().sum()) == 0   # the refused calls wrote nothing (the accepted one certified both all-empty queries)


# ---- the two small kernels of the certified search --------------------------------------------------------------------------
def test_sort_keys_desc(hip_backend):
    """One wave per list: every k up to the wave width, query counts around the four lists of a block, duplicates and empty
    keys; nothing beyond nq * k is written."""
    import torch

    be = hip_backend
    rng = np.random.default_rng(5)
    for k, nq in itertools.product([1, 2, 15, 63, 64], [1, 3, 4, 5, 257]):
        keys = pack_keys(rng.standard_normal((nq, k)).astype(np.float32), rng.integers(0, 1000, (nq, k)))
        keys[rng.random((nq, k)) < 0.2] = 0
        if k > 1:
            keys[:, 1] = keys[:, 0]                     # a duplicate in every list
        if nq > 1:
            keys[1, :] = keys[1, 0]                     # one list of equal keys
        buf = torch.full((nq * k + 64,), SENT, dtype=torch.int64, device=be.device)
        buf[:nq * k] = _keys_dev(be, keys).reshape(-1)
        be._c("lvs_sort_keys_desc", _ptr(buf), nq, k, be._stream())
        h = buf.cpu().numpy()
        assert (h[nq * k:] == SENT).all()
        assert np.array_equal(h[:nq * k].view(np.uint64).reshape(nq, k), np.sort(keys, axis=1)[:, ::-1]), (k, nq)


@pytest.mark.parametrize("d", [8, 64, 200, 520])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("qmode,bmode", [(F16, F16), (F16, SPLIT), (SPLIT, F16), (SPLIT, SPLIT)])
def test_rescore_keys(hip_backend, qmode, bmode, metric, d):
    """Shuffled candidate lists with empty slots: ids, empty slots and the order stay as they are; every new score is the
    float64 score of the STORED values within the float32 accumulation bound (dpad / 64 + 10) 2^-24 |q| |row| (+ 3 * 2^-24 (|q|^2
    + |row|^2) for the three float32 operations of the squared distance).  d = 520 (dpad 576) is the smallest width at which
    some lanes (0 - 7) take a second trip of the scorer's stride-512 loop and the others do not."""
    be = hip_backend
    rng = np.random.default_rng(d + 7 * metric + 3 * qmode + bmode)
    nb, nq, k, off = 50, 9, 6, 11
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    xq = (xb[rng.integers(0, nb, nq)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    cb = be.pack(xb.astype(np.float16) if bmode == F16 else xb, bmode)
    cq = be.pack(xq.astype(np.float16) if qmode == F16 else xq, qmode)
    sb, sq = be.unpack(cb).cpu().numpy().astype(np.float64), be.unpack(cq).cpu().numpy().astype(np.float64)
    rows = np.stack([rng.permutation(nb)[:k] for _ in range(nq)])
    keys = pack_keys(rng.standard_normal((nq, k)).astype(np.float32), rows + off)   # stale scores, in no order
    empty = rng.random((nq, k)) < 0.25
    empty[0, 0] = True
    keys[empty] = 0
    kd = _keys_dev(be, keys)
    be._c("lvs_rescore_keys", _ptr(cb.rows), cb.mode, _ptr(cq.rows), cq.mode, nq, d, metric, _ptr(cb.norms), _ptr(cq.norms), off, k,
          _ptr(kd), be._stream())
    got, ids, e = unpack_keys(kd.cpu().numpy().view(np.uint64))
    assert np.array_equal(e, empty) and np.array_equal(ids[~empty], (rows + off)[~empty])
    q2, b2 = (sq ** 2).sum(1), (sb ** 2).sum(1)
    want = np.einsum("qd,qkd->qk", sq, sb[rows])
    dpad = int(cb.rows.shape[1]) // (2 if bmode == SPLIT else 1)
    tol = (dpad / 64 + 10) * 2.0 ** -24 * np.sqrt(q2)[:, None] * np.sqrt(b2)[rows]
    if metric == L2:
        want = -(q2[:, None] + b2[rows] - 2 * want)
        tol = tol + 3 * 2.0 ** -24 * (q2[:, None] + b2[rows])
    err = np.abs(got.astype(np.float64) - want)[~empty]
    print("rescore", qmode, bmode, metric, d, "max err / tol", float((err / tol[~empty]).max()))
    assert (err <= tol[~empty]).all()


@pytest.mark.parametrize("d", [8, 200, 520])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("qmode,bmode", [(F16, F16), (F16, SPLIT), (SPLIT, F16), (SPLIT, SPLIT)])
def test_resolve_pairs(hip_backend, qmode, bmode, metric, d):
    """lvs_resolve_pairs on its own: 64 queries, 300 rows, ids from 11; the index list names 48 of the queries in shuffled order
    and the device count says 30 of a capacity of 48, then 60 of a capacity of 25.  A query that is not listed, listed beyond
    min(count, capacity) or has an empty key keeps its key bit for bit; every other keys[q] is, bit for bit, the larger of the
    two keys lvs_rescore_keys makes of the same two rows ("the arithmetic of lvs_rescore_keys") - the higher exact score and,
    among equal scores (duplicated corpus rows), the lower id.

    Before the two kernels shared one scorer with its multiply-adds fused by name (csrc/lvs_certify.h) the last assertion failed for
    16 of the 24 cases: the compiler fused one kernel's multiply-adds and not the other's, and with a lo part in an operand 1 to
    22 of the 22 to 27 settled keys were 1 to 32 float32 ulps from lvs_rescore_keys' (never another winner)."""
    import torch

    be = hip_backend
    rng = np.random.default_rng(1000 + d + 7 * metric + 3 * qmode + bmode)
    nb, nq, off, listed_n = 300, 64, 11, 48
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    xb[1::2][:20] = xb[0::2][:20]                       # rows 2 i and 2 i + 1 (i < 20) are equal: equal exact scores
    xq = (xb[rng.integers(0, nb, nq)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    cb = be.pack(xb.astype(np.float16) if bmode == F16 else xb, bmode)
    cq = be.pack(xq.astype(np.float16) if qmode == F16 else xq, qmode)
    rows = np.stack([rng.permutation(nb)[:2] for _ in range(nq)])
    twins = 2 * rng.integers(0, 20, 24)
    rows[:24, 0], rows[:24, 1] = twins, twins + 1       # 24 ties ...
    rows[:12] = rows[:12, ::-1]                         # ... half of them with the higher id in keys1
    keys = pack_keys(rng.standard_normal((nq, 2)).astype(np.float32), rows + off)   # stale scores, in no order
    keys[[3, 30, 40, 50], 1] = 0                        # no runner-up
    keys[[4, 31, 41, 51], 0] = 0                        # no winner
    keys[5] = 0
    exact = _keys_dev(be, keys)                         # [nq, 2] -> the two exact keys of every query
    be._c("lvs_rescore_keys", _ptr(cb.rows), cb.mode, _ptr(cq.rows), cq.mode, nq, d, metric, _ptr(cb.norms), _ptr(cq.norms), off, 2,
          _ptr(exact), be._stream())
    exact = exact.cpu().numpy().view(np.uint64)
    s, ids, _ = unpack_keys(exact)
    first_wins = (s[:, 0] > s[:, 1]) | ((s[:, 0] == s[:, 1]) & (ids[:, 0] < ids[:, 1]))
    both = (keys != 0).all(axis=1)
    ties = both & (s[:, 0] == s[:, 1])
    assert ties[:12].any() and ties[12:24].any() and not ties[24:].any()
    idx = np.array([q for q in rng.permutation(nq) if q not in (3, 4, 5)])
    idx = np.insert(idx, [1, 7, 20], [3, 4, 5])         # three of the queries with an empty key among the first 25 listed
    k2 = _keys_dev(be, keys[:, 1].copy())
    idx_dev = be.to_device(idx.astype(np.int64))        # past the list: the queries that are not listed (they stay untouched)
    for count, cap in [(30, listed_n), (60, 25)]:
        k1 = torch.full((nq + 64,), SENT, dtype=torch.int64, device=be.device)
        k1[:nq] = _keys_dev(be, keys[:, 0].copy())
        cnt = be.to_device(np.array([count], np.int64))
        be._c("lvs_resolve_pairs", _ptr(cb.rows), cb.mode, _ptr(cq.rows), cq.mode, d, metric, _ptr(cb.norms), _ptr(cq.norms), off,
              _ptr(idx_dev), _ptr(cnt), cap, _ptr(k1), _ptr(k2), be._stream())
        h = k1.cpu().numpy()
        assert (h[nq:] == SENT).all() and int(cnt.cpu()[0]) == count
        got = h[:nq].view(np.uint64)
        done = np.zeros(nq, bool)
        done[idx[:min(count, cap)]] = True
        done &= both
        assert 10 <= done.sum() < min(count, cap) and (done & ties).sum() >= 2
        want = exact[done].max(axis=1)
        ulps = np.abs((got[done] >> np.uint64(32)).astype(np.int64) - (want >> np.uint64(32)).astype(np.int64))
        print("resolve_pairs", qmode, bmode, metric, d, (count, cap), "settled", int(done.sum()), "keys that differ", int((got[done] != want).sum()),
              "other winner", int(((got[done] ^ want) & np.uint64(0xFFFFFFFF) != 0).sum()), "largest score distance in ulps", int(ulps.max()))
        assert np.array_equal(got[~done], keys[~done, 0])
        low = np.uint64(0xFFFFFFFF)   # the id half: the row with the higher exact score and, among equal scores, the lower id
        assert np.array_equal(got[done] & low, np.where(first_wins, exact[:, 0], exact[:, 1])[done] & low)
        assert np.array_equal(got[done], want)
