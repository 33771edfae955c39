"""The Hamerly bound kernels of k-means - lvs_kmeans_centroid_shift, lvs_kmeans_bounds_set, lvs_kmeans_bounds_fix,
lvs_kmeans_bounds_step - called through the C ABI and compared with float64 (tests/cert_rules.py): every bound must be SOUND
(ub never below, lb never above the true distance; a moved centroid's shift never under-reported; no row skipped whose
nearest centroid changed) and TIGHT (within the kernels' own 1e-6 / 1e-5 factors plus float32 rounding of the truth)."""
import ctypes

import numpy as np
import pytest

import cert_rules as cr
from lotus_amd import _capi
from lotus_amd.backend import _ptr
from oracle.flat import pack_keys, unpack_keys

pytestmark = pytest.mark.gpu
SPLIT, L2 = _capi.PACK_SPLIT, _capi.METRIC_L2
F32_GUARD = np.float32(1.0 + 1e-5)   # the step's guard as the float32 number the rule is evaluated with


def _dev(be, a, dtype):
    return None if a is None else be.to_device(np.ascontiguousarray(a, dtype=dtype))


def _keys_dev(be, keys):
    return be.to_device(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))


def _coef(c):
    return (ctypes.c_float * len(c))(*[float(v) for v in c])


def _shift(be, c_old, c_new):
    delta, top2 = be.kmeans_centroid_shift(_dev(be, c_old, np.float32), _dev(be, c_new, np.float32))
    be.synchronize()
    return delta.cpu().numpy(), top2.cpu().numpy()


def _top2_fields(top2):
    return float(top2[0]), int(top2[1:2].view(np.int32)[0]), float(top2[2])


def _check_top2(delta, top2):
    """largest value, the index of that value, second largest (0 when there is one centroid)"""
    g1, gi, g2 = _top2_fields(top2)
    assert 0 <= gi < delta.size
    assert g1 == delta.max() and delta[gi] == g1
    assert g2 == (np.delete(delta, gi).max() if delta.size > 1 else 0.0)


# ---- lvs_kmeans_centroid_shift ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 63, 64, 65, 200, 768])
def test_centroid_shift_is_never_below_and_hardly_above_the_true_move(hip_backend, d):
    """delta[j] against the float64 norm of the difference of the float32 inputs, k around the four centroids of a block and
    the 256 threads of the top-2 pass, moves of relative size 1e-4, 1e-2 and 1: true <= delta (soundness) and delta <= true (1 +
    1e-6 + (d / 64 + 10) 2^-23) (the kernel's factor plus its accumulation error).
    Measured on the MI355X over all d of this test: delta / true in 1 + [7.4e-7, 1.11e-6]."""
    be = hip_backend
    rng = np.random.default_rng(d)
    lo, hi = np.inf, 0.0
    for k in [1, 2, 3, 4, 5, 255, 256, 257, 1024]:
        for rel in (1e-4, 1e-2, 1.0):
            c_old = (rng.standard_normal((k, d)) * 10.0 ** rng.uniform(-1, 1, (k, 1))).astype(np.float32)
            c_new = (c_old + rel * np.abs(c_old).max(axis=1, keepdims=True) * rng.standard_normal((k, d))).astype(np.float32)
            if k > 2:
                c_new[1] = c_old[1]   # a centroid that does not move
            delta, top2 = _shift(be, c_old, c_new)
            true = cr.shift(c_old, c_new)[0]
            assert (true <= delta).all(), (k, rel, float((true - delta).max()))
            assert (delta <= true * (1 + 1e-6 + (d / 64 + 10) * 2.0 ** -23)).all(), (k, rel, float((delta / true).max()))
            assert (delta[true == 0] == 0).all()
            r = delta[true > 0] / true[true > 0]
            lo, hi = min(lo, float(r.min())), max(hi, float(r.max()))
            _check_top2(delta, top2)
    print("centroid shift d=%d: delta / true - 1 in [%.3g, %.3g]" % (d, lo - 1, hi - 1))


def test_centroid_shift_top2(hip_backend):
    """top2 = (largest, its centroid, second largest): ties for the largest (second == largest), all-zero moves, one centroid
    (second = 0), the largest at index 0, at k - 1 and at an index >= 256 (a thread's second-round element), the second largest
    in the same thread as the largest and in another one."""
    be = hip_backend

    def run(moves):
        moves = np.asarray(moves, dtype=np.float32)
        delta, top2 = _shift(be, np.zeros((moves.size, 1), np.float32), moves[:, None])
        assert (delta >= np.abs(moves)).all() and (delta <= np.abs(moves) * (1 + 2e-6)).all()
        _check_top2(delta, top2)
        return delta, _top2_fields(top2)

    for k in (1, 2, 5, 256, 257, 1024):
        _, (g1, gi, g2) = run(np.zeros(k))                       # nothing moved
        assert (g1, g2) == (0.0, 0.0) and 0 <= gi < k
    delta, (g1, gi, g2) = run([-3.0])                             # one centroid
    assert gi == 0 and g1 == delta[0] > 0 and g2 == 0.0
    base = np.linspace(0.1, 1.0, 1024)
    for k, at in [(2, 0), (2, 1), (5, 0), (5, 4), (257, 256), (1024, 0), (1024, 1023), (1024, 700), (1024, 255), (1024, 256)]:
        for second_at in {(at + 256) % k, (at + 1) % k, (at - 256) % k}:
            moves = base[:k].copy()
            moves[at] = 7.0
            if second_at != at:
                moves[second_at] = 5.0
            delta, (g1, gi, g2) = run(moves)
            assert gi == at and g1 == delta[at]
            assert g2 == (delta[second_at] if second_at != at else np.delete(delta, at).max()), (k, at, second_at)
    for k, ties in [(2, (0, 1)), (1024, (100, 300)), (1024, (300, 556)), (1024, (0, 1023)), (257, (0, 256))]:
        moves = base[:k].copy() * 0.5
        moves[list(ties)] = 2.0
        delta, (g1, gi, g2) = run(moves)
        assert gi in ties and g1 == g2 == delta[ties[0]]          # a tie: the second largest IS the largest


# ---- lvs_kmeans_bounds_set / lvs_kmeans_bounds_fix on synthetic keys ---------------------------------------------------------
STATS = np.float32([2.3, 1.7e-4])
COEF5 = np.float32([4.0, 2e-3, 1e-6, 1e-5, 1.6e-5])
EXACT2 = np.float32([8e-6, 4e-6])
REL = 3e-6                    # the kernels' 1e-6 factor plus about ten float32 roundings
A_SENT, U_SENT, L_SENT = -9, -1.5, -2.5
ID_OFFSET = 1000


def _set_inputs(rng, m):
    """squared distances d1 <= d2 and |x|^2 such that the search's error bound err is either <= 0.49 d2 or >= 1.01 d2, and
    either <= d1 / 2.05 or >= d1 / 0.99 (in between d - err is ill-conditioned in float32: the reference says nothing there) -
    by construction, nothing is filtered"""
    scale, slack = cr.stats_scale_slack(STATS, COEF5)
    d2 = 10.0 ** rng.uniform(-2.5, 2, m)
    small = rng.random(m) < 0.7
    f = np.where(small, rng.uniform(0.06, 0.45, m), rng.uniform(1.01, 3.0, m))
    err = f * d2
    above = small & (rng.random(m) < 0.6)                       # d1 = h err with h in [2.05, 1 / f] or [0, min(0.99, 1 / f)]
    h = np.where(above, rng.uniform(2.05, 1.0 / np.minimum(f, 0.45)), rng.uniform(0, np.minimum(0.99, 1.0 / f)))
    d1 = h * err
    d1[rng.random(m) < 0.05] = 0.0                              # rows that sit on their centroid
    qn = (((err - slack) / scale) ** 2).astype(np.float32)
    d1, d2 = d1.astype(np.float32), d2.astype(np.float32)
    e = cr.search_error(qn, STATS, COEF5)                       # what the float32 inputs really say
    assert ((e <= d2 / 2) | (e >= d2 * (1 + 1e-3))).all() and ((e <= d1 / 2) | (e >= d1 * (1 + 1e-3))).all()
    return d1, d2, qn


def _call_set(be, keys, stride, second, qn, pos, m, assign, ub, lb):
    c, stats = _coef(COEF5), _dev(be, STATS, np.float32)   # every device buffer stays referenced until the kernel has run
    be._c("lvs_kmeans_bounds_set", _ptr(keys), stride, _ptr(second), _ptr(qn), _ptr(pos), m, _ptr(stats), ctypes.addressof(c),
          ID_OFFSET, _ptr(assign), _ptr(ub), _ptr(lb), be._stream())
    be.synchronize()


def _sentinels(be, N):
    import torch

    return (torch.full((N,), A_SENT, dtype=torch.int32, device=be.device),
            torch.full((N,), U_SENT, dtype=torch.float32, device=be.device),
            torch.full((N,), L_SENT, dtype=torch.float32, device=be.device))


def _within(got, ref, upper):
    """got on the sound side of ref and within REL of it (ref = 0 or inf: equal)"""
    got, ref = got.astype(np.float64), np.asarray(ref, dtype=np.float64)
    if upper:
        return (got >= ref) & (got <= ref * (1 + REL))
    return (got <= ref) & (got >= ref * (1 - REL))


@pytest.mark.parametrize("scattered", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
def test_bounds_set_on_synthetic_keys(hip_backend, stride, scattered):
    """ub >= sqrt(d1 + err) and lb <= sqrt(max(d2 - err, 0)) in float64, both within 3e-6 relative; rows 0..m or a scattered
    subset, the runner-up as a score vector or as the second key of an exact k = 2 result, a non-zero id offset, an empty winner
    (assign -1, a huge ub), a -inf runner-up (lb = +inf); rows that are not named keep their values."""
    be = hip_backend
    rng = np.random.default_rng(10 * stride + scattered)
    N, m = 1000, 700
    d1, d2, qn = _set_inputs(rng, m)
    ids = rng.integers(0, 300, m) + ID_OFFSET
    keys = np.zeros((m, stride), np.uint64)
    keys[:, 0] = pack_keys(-d1, ids)
    keys[3, 0] = keys[400, 0] = 0                                # empty winners
    second = None
    if stride == 2:
        keys[:, 1] = pack_keys(-d2, ids + 1)
    else:
        second = -d2
        second[[5, 600]] = -np.inf                               # a single centroid: no runner-up
    pos = rng.permutation(N)[:m] if scattered else None
    assign, ub, lb = _sentinels(be, N)
    _call_set(be, _keys_dev(be, keys), stride, _dev(be, second, np.float32), _dev(be, qn, np.float32), _dev(be, pos, np.int64), m,
              assign, ub, lb)
    a, u, l = assign.cpu().numpy(), ub.cpu().numpy(), lb.cpu().numpy()
    ra, ru, rl = cr.bounds_set(keys, stride, second, qn, pos, STATS, COEF5, ID_OFFSET, np.full(N, A_SENT), np.full(N, U_SENT),
                               np.full(N, L_SENT))
    named = np.zeros(N, bool)
    named[np.arange(m) if pos is None else pos] = True
    assert np.array_equal(a, ra)
    assert (a[~named] == A_SENT).all() and (u[~named] == np.float32(U_SENT)).all() and (l[~named] == np.float32(L_SENT)).all()
    empty = named & (ra == -1)
    assert empty.sum() == 2 and (u[empty] >= 1e18).all()
    live = named & ~empty
    assert _within(u[live], ru[live], True).all(), float((u[live] / ru[live]).max())
    assert _within(l[named], rl[named], False).all()
    assert (rl[named] == 0).sum() > 50 and (np.isinf(l[named]).sum() == (0 if stride == 2 else 2))


@pytest.mark.parametrize("scattered", [False, True])
def test_bounds_fix_on_synthetic_keys(hip_backend, scattered):
    """After a set: rows the exact search gave the SAME winner keep lb bit for bit and get ub from the exact key (+ the float32
    rounding allowance exact_coef2); rows with ANOTHER winner also get lb <= sqrt(max(d1a - err, 0)), the distance to the
    one-pass winner; rows with an empty exact key and rows that are not named are untouched."""
    be = hip_backend
    rng = np.random.default_rng(30 + scattered)
    N, m, m2 = 1000, 700, 300
    d1, d2, qn = _set_inputs(rng, m)
    ids = rng.integers(0, 300, m) + ID_OFFSET
    keys = pack_keys(-d1, ids)
    pos = rng.permutation(N)[:m] if scattered else np.arange(m)
    assign, ub, lb = _sentinels(be, N)
    _call_set(be, _keys_dev(be, keys), 1, _dev(be, -d2, np.float32), _dev(be, qn, np.float32),
              _dev(be, pos if scattered else None, np.int64), m, assign, ub, lb)
    a0, u0, l0 = assign.cpu().numpy(), ub.cpu().numpy(), lb.cpu().numpy()
    sel = rng.permutation(m)[:m2]                                 # the rows the exact search decided
    kind = rng.integers(0, 3, m2)                                 # 0 same winner, 1 another, 2 empty exact key
    d1e = (d1[sel] * rng.uniform(0.5, 1.0, m2)).astype(np.float32)
    exact = pack_keys(-d1e, np.where(kind == 0, ids[sel], ids[sel] + 1))
    exact[kind == 2] = 0
    approx = keys[sel]
    fix_pos = pos[sel]
    c5, c2 = _coef(COEF5), _coef(EXACT2)
    # (every device buffer stays referenced until the kernel has run)
    ka, ke, q, p, st = (_keys_dev(be, approx), _keys_dev(be, exact), _dev(be, qn[sel], np.float32), _dev(be, fix_pos, np.int64),
                        _dev(be, STATS, np.float32))
    be._c("lvs_kmeans_bounds_fix", _ptr(ka), _ptr(ke), _ptr(q), _ptr(p), m2, _ptr(st), ctypes.addressof(c5), ctypes.addressof(c2),
          ID_OFFSET, _ptr(assign), _ptr(ub), _ptr(lb), be._stream())
    be.synchronize()
    a, u, l = assign.cpu().numpy(), ub.cpu().numpy(), lb.cpu().numpy()
    ra, ru, rl = cr.bounds_fix(approx, exact, qn[sel], fix_pos, STATS, COEF5, EXACT2, ID_OFFSET, a0, u0, l0)
    assert np.array_equal(a, ra)
    rows = {kd: fix_pos[kind == kd] for kd in range(3)}
    touched = np.zeros(N, bool)
    touched[np.concatenate([rows[0], rows[1]])] = True
    assert np.array_equal(a[~touched], a0[~touched]) and np.array_equal(u[~touched], u0[~touched])
    assert np.array_equal(l[~touched], l0[~touched])              # empty exact keys and rows not named included
    assert len(rows[2]) > 50 and np.array_equal(l[rows[0]], l0[rows[0]])   # same winner: lb is kept
    assert _within(u[touched], ru[touched], True).all()
    assert _within(l[rows[1]], rl[rows[1]], False).all()
    lowered = l[rows[1]] < l0[rows[1]]
    assert lowered.sum() > 20 and (l[rows[1]] <= l0[rows[1]]).all()


# ---- lvs_kmeans_bounds_step ------------------------------------------------------------------------------------------------
def _step(be, assign, ub, lb, delta, top2):
    """-> (ub, lb, listed mask) as the device leaves them; the list's own invariants are checked in cert_rules.index_lists"""
    n = assign.size
    a, u, l = _dev(be, assign, np.int32), _dev(be, ub, np.float32), _dev(be, lb, np.float32)
    dl, t2 = _dev(be, delta, np.float32), _dev(be, top2, np.float32)
    listed = cr.index_lists(be, n, 1, lambda out, cnt: be._c("lvs_kmeans_bounds_step", _ptr(a), _ptr(u), _ptr(l), _ptr(dl), _ptr(t2),
                                                              n, _ptr(out), _ptr(cnt), be._stream()))[0]
    assert np.array_equal(a.cpu().numpy(), assign)
    return u.cpu().numpy(), l.cpu().numpy(), listed


def _top2_array(delta):
    g1, gi, g2 = cr.top2(delta)
    t = np.float32([g1, 0, g2])
    t[1:2].view(np.int32)[0] = gi
    return t, np.float32(g1), gi, np.float32(g2)


def _f32_listed(assign, ub, lb):
    """the rule on the float32 values the device returned"""
    return (assign < 0) | ~((ub * F32_GUARD).astype(np.float32) < lb)


@pytest.mark.parametrize("n", cr.SELECT_SIZES)
def test_bounds_step_bookkeeping_is_bit_exact(hip_backend, n):
    """ub + delta[a] and lb - (second largest delta if a is the largest mover, else the largest) are one float32 rounding each:
    bit-exact against numpy; rows without an assignment are unchanged and listed; the listed set is the float32 rule on the
    returned arrays - at the block edges of the two-sweep compaction and for every open pattern."""
    be = hip_backend
    rng = np.random.default_rng(n)
    K = 300
    delta = (0.05 * rng.random(K)).astype(np.float32)
    top2, g1, gi, g2 = _top2_array(delta)
    for name, want in cr.open_patterns(n, rng):
        assign = rng.integers(0, K, n).astype(np.int32)
        assign[rng.random(n) < 0.2] = gi                          # rows of the largest mover: the other shift applies
        unassigned = want & (np.arange(n) % 3 == 0)
        assign[unassigned] = -1
        ub = rng.uniform(0.5, 2.0, n).astype(np.float32)
        a = np.maximum(assign, 0)
        u1 = (ub + delta[a]).astype(np.float32)
        sub = np.where(a == gi, g2, g1).astype(np.float32)
        lb = ((u1 * np.where(want, np.float32(0.5), np.float32(3.0))).astype(np.float32) + sub).astype(np.float32)
        l1 = (lb - sub).astype(np.float32)
        u_ref, l_ref = np.where(assign >= 0, u1, ub), np.where(assign >= 0, l1, lb)
        u, l, listed = _step(be, assign, ub, lb, delta, top2)
        assert np.array_equal(u, u_ref) and np.array_equal(l, l_ref), name
        assert np.array_equal(listed, _f32_listed(assign, u, l)) and np.array_equal(listed, want), name
        if n <= 2049:
            assert np.array_equal(cr.bounds_step(assign, ub, lb, delta, (g1, gi, g2))[2], want)


def test_bounds_step_guard_is_strict(hip_backend):
    """lb a few float32 steps around ub (1 + 1e-5): a row is skipped only while ub (1 + 1e-5) < lb - equality is listed - and
    the float64 rule agrees wherever its slack is outside the two float32 roundings."""
    be = hip_backend
    rng = np.random.default_rng(4)
    n = 4096
    ub = (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    edge = (ub * F32_GUARD).astype(np.float32)
    j = rng.integers(-3, 4, n)
    lb = edge.copy()
    for _ in range(3):
        lb = np.where(j > 0, np.nextafter(lb, np.float32(np.inf)), np.where(j < 0, np.nextafter(lb, np.float32(-np.inf)), lb))
        j = j - np.sign(j)
    assign = np.zeros(n, np.int32)
    delta = np.zeros(1, np.float32)
    u, l, listed = _step(be, assign, ub, lb, delta, _top2_array(delta)[0])
    assert np.array_equal(u, ub) and np.array_equal(l, lb)
    assert np.array_equal(listed, ~(edge < lb)) and (listed & (edge == lb)).sum() > 300 and (~listed).sum() > 1000
    _, _, rule, slack = cr.bounds_step(assign, ub, lb, delta, (0.0, 0, 0.0))
    clear = np.abs(slack) > 2.0 ** -23 * ub    # one rounding of the product, and 1 + 1e-5 itself as a float32 number
    assert clear.sum() > 500 and np.array_equal(listed[clear], rule[clear])


@pytest.mark.parametrize("L", [2.0, 0.37])
def test_bounds_step_on_the_collinear_move(hip_backend, L):
    """Where the triangle inequality is tight: centroids a = 0 and b = L e1 move along e1 towards the rows t e1 between them,
    t chosen so that the gap d_b' / d_a' - 1 AFTER the move sweeps 0 and +-10^(-7.5 .. -3); a far centroid stands still; ub and
    lb as a sound search leaves them (distance (1 +- 1e-6), float32), delta and top2 from the device.  Every row whose new gap is
    <= 0 must be listed (soundness); every row whose new gap is > 3e-5 (the 1e-5 guard, three 1e-6 factors, rounding) must not
    be (tightness).  With a fourth centroid that moves the most of all, lb drops by THAT centroid's shift (half of L here), so
    the rule lists every row and no gap threshold applies; there the device must still list what the float64 rule lists.
    Measured on the MI355X, both L, every configuration: the largest gap of a listed row is 1.01e-5, the smallest gap of a
    skipped row 1.77e-5 - the switch lies between two neighbours of the quarter-decade sweep, 1e-5 and 1.78e-5."""
    be = hip_backend
    rng = np.random.default_rng(int(L * 100))
    d = 64
    g0 = 10.0 ** np.arange(-7.5, -2.99, 0.25)
    g = np.repeat(np.concatenate([[0.0], g0, -g0]), 200)
    g = g * (1 + 1e-3 * rng.uniform(-1, 1, g.size))
    lo_unlisted, hi_listed = np.inf, -np.inf
    for (da, db), big in [(c, False) for c in [(1e-3, 0), (0, 1e-3), (3e-2, 1e-3), (1e-3, 3e-2), (0.0125, 0.0125), (0.2, 0.1)]] + \
                         [((1e-3, 3e-2), True), ((3e-2, 1e-3), True)]:
        K = 4 if big else 3
        C = np.zeros((K, d), np.float32)
        C[1, 0], C[2, 1] = L, 10 * L
        C2 = C.copy()
        C2[0, 0], C2[1, 0] = -da * L, L - db * L
        if big:
            C[3, 1] = C2[3, 1] = -10 * L
            C2[3, 2] = 0.5 * L                                    # far away, and the largest mover of all
        ca2, cb2 = float(C2[0, 0]), float(C2[1, 0])
        x = ((cb2 + (1 + g) * ca2) / (2 + g)).astype(np.float32)  # t = (L - db - (1 + g) da) / (2 + g)
        x64 = x.astype(np.float64)
        d_a, d_b = x64 - float(C[0, 0]), float(C[1, 0]) - x64
        d_far = np.sqrt(x64 ** 2 + float(C[2, 1]) ** 2)
        assert (d_a > 0).all() and (d_a < d_b).all() and (d_b < d_far).all()   # every row is assigned to a before the move
        ub, lb = (d_a * (1 + 1e-6)).astype(np.float32), (d_b * (1 - 1e-6)).astype(np.float32)
        assign = np.zeros(x.size, np.int32)
        delta, top2 = _shift(be, C, C2)
        g1, gi, g2 = _top2_fields(top2)
        assert gi == 3 if big else (da == db or gi == (0 if da > db else 1))
        u, l, listed = _step(be, assign, ub, lb, delta, top2)
        gap = (cb2 - x64) / (x64 - ca2) - 1
        assert listed[gap <= 0].all(), ((da, db), big)
        _, _, rule, slack = cr.bounds_step(assign, ub, lb, delta, (g1, gi, g2))
        clear = np.abs(slack) > 2.0 ** -21 * (u + l)              # ub + delta, lb - g, ub (1 + 1e-5): three roundings
        assert np.array_equal(listed[clear], rule[clear])
        if big:
            assert listed.all()
            continue
        assert not listed[gap > 3e-5].any(), ((da, db), float(gap[listed].max()))
        assert listed.any() and not listed.all()
        lo_unlisted, hi_listed = min(lo_unlisted, float(gap[~listed].min())), max(hi_listed, float(gap[listed].max()))
    print("bounds step L=%g: smallest skipped gap %.3g, largest listed gap %.3g" % (L, lo_unlisted, hi_listed))


# ---- the real pipeline at the smallest shapes ------------------------------------------------------------------------------
def _distances(X, C, assign):
    """float64: distance of every row to its assigned centroid and to the nearest OTHER centroid, the nearest centroid of all.
    The three nearest by the Gram expansion are measured again from the differences (exact for rows that sit on a centroid)."""
    rows = np.arange(X.shape[0])
    G = (X ** 2).sum(1)[:, None] + (C ** 2).sum(1)[None, :] - 2 * X @ C.T
    cand = np.argsort(G, axis=1, kind="stable")[:, :min(3, C.shape[0])]
    dc = np.sqrt(((X[:, None, :] - C[cand]) ** 2).sum(-1))
    own = np.sqrt(((X - C[assign]) ** 2).sum(-1))
    other = np.where(cand == assign[:, None], np.inf, dc).min(axis=1)
    nearest = cand[rows, dc.argmin(axis=1)]
    return own, other, nearest, dc.min(axis=1)


@pytest.mark.parametrize("d", [32, 200])
@pytest.mark.parametrize("K", [2, 3, 17, 300])
def test_bounds_of_the_real_search_hold_before_and_after_a_move(hip_backend, K, d):
    """be.nearest(..., bounds=...) with fp32 (hi|lo) operands on blob rows plus rows that are exact copies of a centroid, rows
    half way between two centroids and a centroid pair that differs only in the lo half (so that lvs_kmeans_bounds_fix runs):
    ub >= the float64 distance of the STORED values to the assigned centroid, lb <= the distance to every other centroid; then
    three moves (all centroids a little, one far, one not at all) through lvs_kmeans_centroid_shift + lvs_kmeans_bounds_step: both
    inequalities hold against the new centroids and every row that is not listed still has its assigned centroid nearest."""
    import torch

    be = hip_backend
    rng = np.random.default_rng(K * 1000 + d)
    n = 3000
    C = rng.standard_normal((K, d)).astype(np.float32)
    C[0] = C[0].astype(np.float16).astype(np.float32)
    if K >= 3:                                                    # a twin of centroid 0 below fp16 resolution
        C[K - 1] = C[0]
        C[K - 1, :8] += 0.3 * np.spacing(np.abs(C[0, :8].astype(np.float16))).astype(np.float32)
        assert np.array_equal(C[0].astype(np.float16), C[K - 1].astype(np.float16)) and not np.array_equal(C[0], C[K - 1])
    X = (C[rng.integers(0, K, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    X[:20] = C[rng.integers(0, K, 20)]                            # exact copies of a centroid
    pa = rng.integers(0, K, 20)
    X[20:40] = 0.5 * (C[pa] + C[(pa + 1) % K])                    # half way between two centroids
    X[40:60] = C[K - 1]
    cq = be.pack(X, SPLIT)
    cb, cstats = be.kmeans_pack_centroids(be.to_device(C), SPLIT)
    assign = torch.full((n,), -1, dtype=torch.int32, device=be.device)
    ub = torch.zeros((n,), dtype=torch.float32, device=be.device)
    lb = torch.zeros((n,), dtype=torch.float32, device=be.device)
    stats = {}
    keys = be.nearest(cb, cq, L2, exact_scores=False, corpus_stats=cstats, stats=stats, bounds=(assign, ub, lb, None))
    assert stats["uncertified"] > 0, stats                        # some rows took the fix path
    a = assign.cpu().numpy().astype(np.int64)
    assert np.array_equal(a, unpack_keys(keys.cpu().numpy().view(np.uint64).reshape(-1))[1])
    c_old = be.unpack(cb)
    Xs, Cs = be.unpack(cq).cpu().numpy().astype(np.float64), c_old.cpu().numpy().astype(np.float64)
    own, other, _, _ = _distances(Xs, Cs, a)
    u, l = ub.cpu().numpy().astype(np.float64), lb.cpu().numpy().astype(np.float64)
    assert (u >= own).all(), float((own - u).max())
    assert (l <= other).all(), float((l - other).max())
    far = np.zeros((K, d), np.float32)
    far[1] = 0.25 * np.sqrt(2 * d) * (lambda v: v / np.linalg.norm(v))(rng.standard_normal(d))
    still = 1e-3 * rng.standard_normal((K, d)).astype(np.float32)
    still[K // 2] = 0
    for name, move in [("small", 1e-3 * rng.standard_normal((K, d)).astype(np.float32)), ("one far", far), ("one still", still)]:
        cb2, _ = be.kmeans_pack_centroids(be.to_device((C + move).astype(np.float32)), SPLIT)
        c_new = be.unpack(cb2)
        delta, top2 = be.kmeans_centroid_shift(c_old, c_new)
        if name == "one still":
            assert float(delta[K // 2]) == 0.0
        ub2, lb2 = ub.clone(), lb.clone()
        idx = be.kmeans_bounds_step(assign, ub2, lb2, delta, top2).cpu().numpy()
        listed = np.zeros(n, bool)
        listed[idx] = True
        assert idx.size == listed.sum() and 0 < idx.size < n, (name, idx.size)
        own2, other2, nearest2, _ = _distances(Xs, c_new.cpu().numpy().astype(np.float64), a)
        u2, l2 = ub2.cpu().numpy().astype(np.float64), lb2.cpu().numpy().astype(np.float64)
        assert (u2 >= own2).all(), (name, float((own2 - u2).max()))
        assert (l2 <= other2).all(), (name, float((l2 - other2).max()))
        assert np.array_equal(nearest2[~listed], a[~listed]), name
