"""The float64 restatements in tests/cert_rules.py against brute force (no GPU): the Hamerly chain set -> shift -> step never
skips a row whose nearest centroid changed, the certify restatement agrees with the host model of test_exactness_rules.py,
and the select rules treat empty keys, NaN and infinities as the header says.  The one-pass bound's coefficients: the header
lvs_bound.h, the library entry lvs_nearest_bound_coef and a float64 restatement agree bit for bit."""
import ctypes

import numpy as np
import pytest

import cert_rules as cr
import plan_native
from lotus_amd import _capi
from lotus_amd.backend import HipBackend, PackedRows
from oracle.flat import pack_keys
from test_exactness_rules import certified


@pytest.mark.parametrize("seed", range(4))
def test_hamerly_chain_never_skips_a_row_whose_nearest_centroid_changed(seed):
    rng = np.random.default_rng(seed)
    skipped = listed_n = changed_n = 0
    for move in range(150):
        n, K, d = 300, int(rng.integers(2, 12)), int(rng.integers(1, 6))
        C = rng.standard_normal((K, d))
        X = C[rng.integers(0, K, n)] + 0.3 * rng.standard_normal((n, d))
        D = np.sqrt(((X[:, None, :] - C[None, :, :]) ** 2).sum(-1))
        order = np.argsort(D, axis=1, kind="stable")
        a = order[:, 0]
        rows = np.arange(n)
        ub, lb = cr.bounds_from_sq(D[rows, a] ** 2, D[rows, order[:, 1]] ** 2, 0.0)   # set with err = 0
        size = 10.0 ** rng.uniform(-4, 0)
        C2 = C + size * rng.standard_normal((K, d)) * (rng.random((K, 1)) < 0.7)         # some centroids do not move
        if move % 3 == 0:
            C2[int(rng.integers(K))] += 3 * size * rng.standard_normal(d)                # one moves far
        true, g1, gi, g2 = cr.shift(C, C2)
        assert true[gi] == g1 and g2 <= g1 and (np.delete(true, gi) <= g2).all()
        ub2, lb2, listed, slack = cr.bounds_step(a, ub, lb, true, (g1, gi, g2))
        D2 = np.sqrt(((X[:, None, :] - C2[None, :, :]) ** 2).sum(-1))
        # the bounds stay bounds (up to float64 rounding of the distances themselves)
        assert (ub2 >= D2[rows, a] * (1 - 1e-12)).all()
        other = D2.copy()
        other[rows, a] = np.inf
        assert (lb2 <= other.min(axis=1) * (1 + 1e-12) + 1e-12).all()
        changed = D2.argmin(axis=1) != a
        assert listed[changed].all(), (seed, move)
        assert np.array_equal(listed, ~(slack < 0))
        skipped += int((~listed).sum())
        listed_n += int(listed.sum())
        changed_n += int(changed.sum())
    assert skipped > 1000 and listed_n > 1000 and changed_n > 100, (skipped, listed_n, changed_n)  # all outcomes exercised


def test_bounds_step_leaves_unassigned_rows_alone_and_lists_them():
    ub, lb, listed, _ = cr.bounds_step([-1, 0, 1], [1.0, 1.0, 1.0], [9.0, 9.0, 9.0], [0.5, 2.0], (2.0, 1, 0.5))
    assert list(ub) == [1.0, 1.5, 3.0] and list(lb) == [9.0, 7.0, 8.5] and list(listed) == [True, False, False]
    # the guard is strict: ub (1 + 1e-5) == lb is listed
    _, _, listed, slack = cr.bounds_step([0], [1.0], [1.0 + 1e-5], [0.0], (0.0, 0, 0.0))
    assert slack[0] == 0.0 and listed[0]


@pytest.mark.parametrize("seed", range(3))
def test_certify_restatement_agrees_with_the_host_model(seed):
    rng = np.random.default_rng(40 + seed)
    n_open = n_cert = 0
    for trial in range(400):
        k = int(rng.integers(1, 6))
        k1 = k + int(rng.integers(0, 5))
        n = int(rng.integers(0, k1 + 1))                     # candidates in the list: short, or full lists
        band = float(rng.choice([2.0, 2.02, 2.5]))
        scale, slack = float(rng.choice([0.0, 0.01])), float(rng.choice([0.0, 0.02]))
        qn = np.float32(rng.uniform(0.5, 4.0))
        bound = scale * np.sqrt(np.float64(qn)) + slack
        exact = rng.normal(0, 0.05, n).astype(np.float32)
        hi = (exact + rng.uniform(-bound, bound, n)).astype(np.float32)
        cand = np.arange(n)
        approx_keys = np.zeros((1, k1), np.uint64)
        exact_keys = np.zeros((1, k1), np.uint64)
        oa, oe = np.argsort(-hi, kind="stable"), np.argsort(-exact, kind="stable")
        approx_keys[0, :n] = pack_keys(hi[oa], oa)
        exact_keys[0, :n] = pack_keys(exact[oe], oe)
        is_open, sl = cr.certify(approx_keys, exact_keys, np.array([qn]), k1, k, scale, slack, band)
        want = certified(hi.astype(np.float64), exact.astype(np.float64), cand, k, k1, bound, band)
        assert bool(is_open[0]) == (not want), (seed, trial)
        assert (sl[0] > 0) == (not is_open[0])
        n_open += int(is_open[0])
        n_cert += int(not is_open[0])
    assert n_open >= 40 and n_cert >= 40


def test_certify_band_zero_reads_the_last_slot_and_an_unfilled_list_holds_every_row():
    k1, k = 4, 2
    a = pack_keys(np.float32([5, 4, 3, 1]), np.arange(4)).reshape(1, 4)
    e = pack_keys(np.float32([5, 2, 1, 0]), np.arange(4)).reshape(1, 4)
    assert not cr.certify(a, e, None, k1, k, 0.5, 0.25, 0.0)[0][0]       # 2 > 1 + 0.75
    assert cr.certify(a, e, None, k1, k, 0.5, 0.5, 0.0)[0][0]            # 2 > 1 + 1 is false: strict
    assert cr.certify(a, e, np.float32([4.0]), k1, k, 0.5, 0.0, 0.0)[0][0]   # |q| = 2
    a2 = a.copy()
    a2[0, 3] = 0
    assert not cr.certify(a2, e, None, k1, k, 100.0, 0.0, 0.0)[0][0]    # unfilled list: every row is in it
    assert cr.certify(a2, e, None, k1, k, 1.0, 0.0, 2.0)[0][0]           # banded: 2 > (4 - 2) + 1 is false
    assert not cr.certify(a2, e, None, k1, k, 0.25, 0.0, 16.0)[0][0]    # 2 > (4 - 4) + 0.25
    e2 = e.copy()
    e2[0, 1] = 0
    assert not cr.certify(a, e2, None, k1, k, 100.0, 0.0, 0.0)[0][0] and not cr.certify(a, e2, None, k1, k, 100.0, 0.0, 2.0)[0][0]


def test_margin_rules_on_empty_keys_nan_and_infinities():
    inf, nan = np.inf, np.nan
    best = np.float32([1, 1, 1, 1, 1, inf, 1, 1])
    sec = np.float32([0, 1, -inf, inf, nan, inf, 0, 0.5])
    keys = pack_keys(best, np.arange(8))
    keys[6] = 0
    listed, slack = cr.margin(keys, sec, None, 0.25, 0.25)
    #                 1>.5   0      inf    -inf   nan   inf-inf empty  .5>.5 strict
    assert list(listed) == [False, True, False, True, True, True, False, True]
    assert slack[0] == 0.5 and slack[7] == 0.0 and slack[6] == np.inf
    listed, _ = cr.margin(keys[:1], sec[:1], np.float32([nan]), 0.25, 0.25)
    assert listed[0]
    stats, coef = np.float32([4.0, 0.25]), np.float32([0.5, 0.25, 0.125, 0.0625, 0.03125])
    assert cr.stats_scale_slack(stats, coef) == (0.75, 0.375)
    assert np.array_equal(cr.margin_stats(keys, sec, None, stats, coef)[0], cr.margin(keys, sec, None, 0.75, 0.375)[0])
    # three-way split: certified | pair (needs a runner-up key) | open
    k2 = np.uint64([7, 7, 0, 7, 7])
    cls, s2, s3 = cr.nearest3(pack_keys(np.float32([4, 4, 4, 4, 4]), np.arange(5)), k2, np.float32([1, 3, 3, 3, nan]),
                              np.float32([0, 1, -inf, 3, 0]), None, stats, coef)
    assert list(cls) == [cr.CERTIFIED, cr.PAIR, cr.OPEN, cr.OPEN, cr.PAIR] and s2[1] == 1 - 1.125 and s3[1] == 3 - 1.125


def _coef_restated(metric, pack, d, exp_sum):
    """The five coefficients of the one-pass bound (c[0] E + c[1] R) |q| + c[2] + c[3] R + c[4] R^2, restated in float64 from the
    comment of lvs_margin_select_stats (include/lotus_hip.h) and the text HipBackend._nearest_coef had before the library
    stated them: written here once, never imported from the product.  -> float32 [5]."""
    ip, qsplit = metric == _capi.METRIC_IP, 1.0 if pack == _capi.PACK_SPLIT else 0.0
    c = 2.0 if ip else 4.0
    dpad = (d + 63) // 64 * 64
    return np.array([c, c * ((2.0 ** -11) * qsplit + 8e-6) + 2.0 ** -16 * (1.0 if ip else 2.0), 1e-6 * 2.0 ** exp_sum,
                     qsplit * c * (dpad ** 0.5) * 2.0 ** -25, 1e-6 + (0.0 if ip else 2.0 ** -16)], np.float64).astype(np.float32)


_COEF_GRID = [(m, p, d, e) for m in (_capi.METRIC_IP, _capi.METRIC_L2) for p in (_capi.PACK_F16, _capi.PACK_SPLIT)
              for d in (1, 8, 63, 64, 65, 100, 768, 1536, 4096) for e in (-40, -1, 0, 3, 40)]


def _lib_coef(lib, metric, pack, d, exp_sum, out=True):
    buf = (ctypes.c_float * 5)()
    rc = lib.lvs_nearest_bound_coef(metric, pack, d, exp_sum, ctypes.addressof(buf) if out else None)
    return rc, np.array(buf, np.float32)


def test_bound_coefficients_header_library_and_restatement_agree_bit_for_bit():
    lib = _capi.load()  # no GPU: the entry touches no device
    from_header = plan_native.bound_coefs(_COEF_GRID)
    for case, bits in zip(_COEF_GRID, from_header):
        metric, pack, d, exp_sum = case
        want = _coef_restated(*case)
        assert bits is not None and np.array_equal(np.array(bits, np.uint32), want.view(np.uint32)), (case, bits, want)
        rc, got = _lib_coef(lib, *case)
        assert rc == _capi.OK and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case, got, want)
        # HipBackend._nearest_coef on stand-in operands: the same numbers (as Python floats), dpad from the rows' width
        dpad = (d + 63) // 64 * 64
        corpus = PackedRows(rows=np.empty((0, 2 * dpad), np.float16), norms=None, n=0, d=d, mode=_capi.PACK_SPLIT, exp=exp_sum - 7)
        queries = PackedRows(rows=np.empty((0, dpad * (1 + pack)), np.float16), norms=None, n=0, d=d, mode=pack, exp=7)
        coef, got_dpad = HipBackend._nearest_coef(corpus, queries, metric)
        assert got_dpad == dpad and len(coef) == 5 and all(type(v) is float for v in coef)
        assert np.array_equal(np.array(coef, np.float64), want.astype(np.float64)), (case, coef, want)
    # every argument moves the answer: 2 metrics x 5 exponents x (fp16 queries: no width term | hi|lo queries: 5 padded widths)
    assert len(set(from_header)) == 2 * 5 * (1 + 5)


def test_bound_coefficients_refuse_bad_arguments():
    lib = _capi.load()
    for bad in [(2, 0, 64, 0), (-1, 0, 64, 0), (0, 2, 64, 0), (1, -1, 64, 0), (0, 1, 0, 0), (1, 1, -5, 0)]:
        assert _lib_coef(lib, *bad)[0] == _capi.EINVAL, bad
        assert plan_native.bound_coefs([bad]) == [None], bad
    assert _lib_coef(lib, 1, 1, 64, 0, out=False)[0] == _capi.EINVAL  # a NULL output
    assert _lib_coef(lib, 1, 1, 64, 0)[0] == _capi.OK


def test_shift_and_top2():
    true, g1, gi, g2 = cr.shift(np.zeros((4, 2)), np.array([[3, 4], [0, 0], [5, 0], [0, 1]], float))
    assert list(true) == [5, 0, 5, 1] and (g1, gi, g2) == (5.0, 0, 5.0)       # a tie: first index, second == largest
    assert cr.top2([2.0]) == (2.0, 0, 0.0) and cr.top2([0.0, 0.0]) == (0.0, 0, 0.0)


def test_bounds_set_and_fix_restatements():
    stats, coef = np.float32([4.0, 0.0]), np.float32([0, 0.5, 0, 0, 0])          # err = |x|
    keys = pack_keys(np.float32([-9, -16, 0]), np.array([12, 10, 11]))
    keys[2] = 0
    a, u, l = cr.bounds_set(keys, 1, np.float32([-25, -np.inf, -4]), np.float32([16, 9, 1]), np.array([4, 0, 2]), stats, coef, 10,
                            np.full(5, 7), np.full(5, 70.0), np.full(5, 700.0))
    assert list(a) == [0, 7, -1, 7, 2] and list(u) == [np.sqrt(19), 70, np.inf, 70, np.sqrt(13)]
    assert list(l) == [np.inf, 700, np.sqrt(3), 700, np.sqrt(21)]
    two = np.stack([keys, pack_keys(np.float32([-25, -36, -4]), np.array([10, 11, 12]))], axis=1)
    a2, u2, l2 = cr.bounds_set(two, 2, None, np.float32([16, 9, 1]), None, stats, coef, 10, np.zeros(3), np.zeros(3), np.zeros(3))
    assert list(a2) == [2, 0, -1] and list(l2) == [np.sqrt(21), np.sqrt(33), np.sqrt(3)]
    # fix: same winner keeps lb; another winner lowers it below the one-pass winner's distance; an empty exact key: untouched
    approx = pack_keys(np.float32([-9, -9, -9]), np.array([12, 12, 12]))
    exact = pack_keys(np.float32([-4, -1, -1]), np.array([12, 11, 11]))
    exact[2] = 0
    a3, u3, l3 = cr.bounds_fix(approx, exact, np.float32([16, 16, 16]), np.array([0, 1, 2]), stats, coef, np.float32([0.25, 0.5]),
                               10, np.full(3, 5), np.full(3, 50.0), np.array([1.0, 8.0, 8.0]))
    assert list(a3) == [2, 1, 5] and list(u3) == [np.sqrt(4 + 2 + 2), np.sqrt(1 + 2 + 2), 50.0]
    assert list(l3) == [1.0, np.sqrt(5), 8.0]
