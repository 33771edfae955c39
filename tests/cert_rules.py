"""Plain float64 restatements of the rules that decide what the exact paths skip, written from the header comments of
include/lotus_hip.h (not from the kernels): the top-k certificates, the nearest-row margin rules and the Hamerly bounds of
k-means.  Every function returns the decision per query / row and the float64 SLACK: how far the float64 margin is from the
float64 bound (select rules), or ub (1 + 1e-5) - lb (bounds step).  The GPU tests compare the kernels with these wherever the
slack is outside float32 rounding; tests/test_cert_rules_host.py checks the restatements themselves against brute force."""
import numpy as np

from oracle.flat import unpack_keys

CERTIFIED, PAIR, OPEN = 0, 1, 2
STEP_GUARD = 1e-5  # lvs_kmeans_bounds_step lists a row unless ub (1 + 1e-5) < lb


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _scores(keys):
    """keys -> (float64 scores, empty mask)"""
    better, _, empty = unpack_keys(np.asarray(keys, dtype=np.uint64))
    return better.astype(np.float64), empty


def query_norm(qn, nq):
    """|q| per query; q_norms_sq == NULL means |q| = 1"""
    with np.errstate(invalid="ignore"):
        return np.ones(nq) if qn is None else np.sqrt(_f64(qn))


def stats_scale_slack(stats, coef5):
    """bound = (c0 E + c1 R) |q| + c2 + c3 R + c4 R^2 with R = sqrt(stats[0]), E = sqrt(stats[1]) -> (scale, slack)"""
    R, E = np.sqrt(float(stats[0])), np.sqrt(float(stats[1]))
    c = [float(v) for v in coef5]
    return c[0] * E + c[1] * R, c[2] + c[3] * R + c[4] * R * R


def certify(approx, exact, qn, k1, k, scale, slack, band):
    """lvs_certify_topk (band == 0) / lvs_certify_topk_banded.  approx, exact: uint64 [nq, k1].
    -> (open [nq] bool, slack [nq] = s_k - (s_min + bound); +inf where the rule does not look at the scores)."""
    approx = np.asarray(approx, dtype=np.uint64).reshape(-1, k1)
    exact = np.asarray(exact, dtype=np.uint64).reshape(-1, k1)
    nq = approx.shape[0]
    bound = float(scale) * query_norm(qn, nq) + float(slack)
    s_last, e_last = _scores(approx[:, k1 - 1])
    s_k, e_k = _scores(exact[:, k - 1])
    a_k, e_ak = _scores(approx[:, k - 1])
    if band > 0:
        looked = ~e_k & ~e_ak
        s_min = a_k - float(band) * bound
        s_min = np.where(e_last, s_min, np.fmax(s_min, s_last))
    else:
        looked = ~e_last & ~e_k
        s_min = s_last
    with np.errstate(invalid="ignore"):
        margin = s_k - (s_min + bound)
        is_open = looked & ~(s_k > s_min + bound)
    return is_open, np.where(looked, margin, np.inf)


def margin(keys, second, qn, scale, slack):
    """lvs_margin_select: listed = score(key) - second <= scale |q| + slack; an empty key is never listed, whatever cannot be
    compared (NaN, inf - inf) always is.  -> (listed [nq] bool, slack [nq] = (best - second) - bound)."""
    best, empty = _scores(keys)
    nq = best.shape[0]
    bound = float(scale) * query_norm(qn, nq) + float(slack)
    with np.errstate(invalid="ignore"):
        m = best - _f64(second)
        listed = ~empty & ~(m > bound)
        sl = m - bound
    return listed, np.where(empty, np.inf, sl)


def margin_stats(keys, second, qn, stats, coef5):
    """lvs_margin_select_stats: the same test with the bound from the corpus statistics."""
    scale, slack = stats_scale_slack(stats, coef5)
    return margin(keys, second, qn, scale, slack)


def nearest3(keys1, keys2, second, third, qn, stats, coef5):
    """lvs_nearest3_select -> (class [nq] in {CERTIFIED, PAIR, OPEN}, slack2 = (best - second) - bound, slack3 = (best - third)
    - bound).  An empty winner key is never listed; a pair needs a runner-up key."""
    best, empty = _scores(keys1)
    nq = best.shape[0]
    has2 = np.asarray(keys2, dtype=np.uint64) != 0
    scale, slack = stats_scale_slack(stats, coef5)
    bound = scale * query_norm(qn, nq) + slack
    with np.errstate(invalid="ignore"):
        m2, m3 = best - _f64(second), best - _f64(third)
        cert = empty | (m2 > bound)
        pair = ~cert & has2 & (m3 > bound)
    cls = np.where(cert, CERTIFIED, np.where(pair, PAIR, OPEN))
    return cls, np.where(empty, np.inf, m2 - bound), np.where(empty, np.inf, m3 - bound)


def top2(delta):
    """(largest, index of the first largest, second largest; 0 when there is one value) of a delta vector"""
    delta = _f64(delta)
    i = int(np.argmax(delta))
    rest = np.delete(delta, i)
    return float(delta[i]), i, float(rest.max()) if rest.size else 0.0


def shift(c_old, c_new):
    """lvs_kmeans_centroid_shift -> (true |c_new_j - c_old_j| [k], largest, index of the first largest, second largest)"""
    true = np.sqrt(((_f64(c_new) - _f64(c_old)) ** 2).sum(axis=1))
    return (true,) + top2(true)


def search_error(qn, stats, coef5):
    """the search's own error bound of a squared distance: (c0 E + c1 R) |x| + c2 + c3 R + c4 R^2"""
    scale, slack = stats_scale_slack(stats, coef5)
    return scale * np.sqrt(_f64(qn)) + slack


def bounds_from_sq(d1, d2, err):
    """ub = sqrt(d1 + err), lb = sqrt(max(d2 - err, 0)) from squared distances to the winner / the runner-up"""
    d1, d2, err = _f64(d1), _f64(d2), _f64(err)
    return np.sqrt(d1 + err), np.sqrt(np.maximum(d2 - err, 0.0))


def bounds_set(keys, key_stride, second, qn, positions, stats, coef5, id_offset, assign, ub, lb):
    """lvs_kmeans_bounds_set.  keys uint64 [m * key_stride]; second [m] or None (then the runner-up is keys[i][1]).
    -> new (assign int64, ub float64, lb float64); rows not named keep their values; an empty winner: assign -1, ub +inf."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, key_stride)
    m = keys.shape[0]
    rows = np.arange(m) if positions is None else np.asarray(positions, dtype=np.int64)
    s1, empty = _scores(keys[:, 0])
    _, ids, _ = unpack_keys(keys[:, 0])
    s2 = _f64(second) if second is not None else _scores(keys[:, 1])[0]
    err = search_error(qn, stats, coef5)
    u, l = bounds_from_sq(np.maximum(-s1, 0.0), np.maximum(-s2, 0.0), err)
    assign, ub, lb = np.array(assign, dtype=np.int64), np.array(ub, dtype=np.float64), np.array(lb, dtype=np.float64)
    assign[rows] = np.where(empty, -1, ids - int(id_offset))
    ub[rows] = np.where(empty, np.inf, u)
    lb[rows] = l
    return assign, ub, lb


def bounds_fix(approx, exact, qn, positions, stats, coef5, exact_coef2, id_offset, assign, ub, lb):
    """lvs_kmeans_bounds_fix: ub renewed from the exact distance (+ e0 R |x| + e1 R^2); lb kept when the winner is the same
    centroid, otherwise also below the distance to the one-pass winner; an empty exact key leaves the row as it is."""
    approx, exact = np.asarray(approx, dtype=np.uint64), np.asarray(exact, dtype=np.uint64)
    m = exact.shape[0]
    rows = np.arange(m) if positions is None else np.asarray(positions, dtype=np.int64)
    sa, _ = _scores(approx)
    se, e_empty = _scores(exact)
    _, ia, _ = unpack_keys(approx)
    _, ie, _ = unpack_keys(exact)
    R = np.sqrt(float(stats[0]))
    x = np.sqrt(_f64(qn))
    err1 = search_error(qn, stats, coef5)
    err2 = float(exact_coef2[0]) * R * x + float(exact_coef2[1]) * R * R
    assign, ub, lb = np.array(assign, dtype=np.int64), np.array(ub, dtype=np.float64), np.array(lb, dtype=np.float64)
    live = ~e_empty
    r = rows[live]
    assign[r] = ie[live] - int(id_offset)
    ub[r] = np.sqrt(np.maximum(-se[live], 0.0) + err2[live])
    other = live & (ia != ie)
    r = rows[other]
    lb[r] = np.minimum(lb[r], np.sqrt(np.maximum(np.maximum(-sa[other], 0.0) - err1[other], 0.0)))
    return assign, ub, lb


def bounds_step(assign, ub, lb, delta, top2_):
    """lvs_kmeans_bounds_step: ub += delta[assign]; lb -= the largest delta among the OTHER centroids (the second largest for
    rows assigned to the largest mover); top2_ = (largest, its centroid, second largest).  Rows with no assignment are left
    alone and listed.  -> (ub, lb, listed, slack = ub (1 + 1e-5) - lb), float64."""
    assign = np.asarray(assign, dtype=np.int64)
    ub, lb, delta = np.array(ub, dtype=np.float64), np.array(lb, dtype=np.float64), _f64(delta)
    g1, gi, g2 = float(top2_[0]), int(top2_[1]), float(top2_[2])
    has = assign >= 0
    a = np.where(has, assign, 0)
    ub = np.where(has, ub + delta[a], ub)
    lb = np.where(has, lb - np.where(a == gi, g2, g1), lb)
    with np.errstate(invalid="ignore"):
        slack = ub * (1.0 + STEP_GUARD) - lb
        listed = ~has | ~(ub * (1.0 + STEP_GUARD) < lb)
    return ub, lb, listed, slack


# ---- plumbing shared by the GPU tests of the kernels that append indices to a list ------------------------------------------
SENT, PRE = -77, 5   # sentinel of the index buffers; the counters start at PRE: the kernels must ADD to them
SELECT_SIZES = [1, 1023, 1024, 1025, 2049, 2_100_001]   # two-sweep kernels: block edges; the last takes per_block off its floor


def index_lists(be, nq, nlists, call):
    """Run `call(out_0, .., out_{nlists-1}, counters)` with sentinel-filled index buffers of nq + 64 entries and counters
    preloaded with PRE.  -> one bool mask [nq] per list, after checking: the counter was added to, the entries are written from
    the counter's old value on, nothing else was touched, every index is in range and none comes twice."""
    import torch

    outs = [torch.full((nq + 64,), SENT, dtype=torch.int64, device=be.device) for _ in range(nlists)]
    cnt = torch.full((nlists,), PRE, dtype=torch.int64, device=be.device)
    call(*outs, cnt)
    be.synchronize()
    masks = []
    for o, c in zip(outs, cnt.cpu().numpy()):
        h = o.cpu().numpy()
        n = int(c) - PRE
        assert 0 <= n <= nq, n
        assert (h[:PRE] == SENT).all() and (h[PRE + n:] == SENT).all()
        got = h[PRE:PRE + n]
        assert ((got >= 0) & (got < nq)).all()
        seen = np.bincount(got, minlength=nq)
        assert seen.max(initial=0) <= 1  # no duplicates
        masks.append(seen.astype(bool))
    return masks


def open_patterns(nq, rng):
    i = np.arange(nq)
    return [("none", np.zeros(nq, bool)), ("all", np.ones(nq, bool)), ("first", i == 0), ("last", i == nq - 1),
            ("every 64th", i % 64 == 0), ("alternating", i % 2 == 0), ("random 0.4 %", rng.random(nq) < 0.004)]
