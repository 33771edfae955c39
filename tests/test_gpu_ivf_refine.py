"""Exact re-ranking on the device (lvs_refine_keys / lvs_refine_kernel) against the float64 rule of
tests/ivf_refine_oracle_backend.py: the best k of a query's candidate rows by exact score over the stored values, in the
project's total order; only a candidate key's row number counts, key 0 is an empty slot.

Bars: scores within 1e-5 of the float64 score of the stored values, ids identical wherever the
reference's neighbouring scores are more than 2e-5 apart, at most 15 % of the slots inside such a gap.  The rows are unit
vectors, so scores are of magnitude <= 1 (inner product) or <= 4 (squared L2) and fp32 accumulation stays two orders of
magnitude inside the bar; operands scaled by s carry bars scaled by s^2, as the scores are (the rule of the scaled IVF
edge cases)."""
import numpy as np
import pytest

import synth
from ivf_refine_oracle_backend import exact_scores, refine_reference
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
NB, NQ = 3000, 67  # 67 queries: not a multiple of the four waves of a workgroup
BAR, TIE_GAP, TIE_CAP = 1e-5, 2e-5, 0.15

_OPERANDS = {}


def _operands(be, d, mode):
    """Packed unit Gaussian rows and queries of one (d, pack mode), made once, with their stored values in float64."""
    if (d, mode) not in _OPERANDS:
        while len(_OPERANDS) >= 6:  # (the wide ones hold 77 MB of float64 each)
            _OPERANDS.pop(next(iter(_OPERANDS)))
        xb, xq = synth.corpus(NB, d, seed=d), synth.corpus(NQ, d, seed=d + 1)
        if mode == F16:
            xb, xq = xb.astype(np.float16), xq.astype(np.float16)
        pb, pq = be.pack(xb, mode), be.pack(xq, mode)
        xb_s, xq_s = be.unpack(pb).cpu().numpy().astype(np.float64), be.unpack(pq).cpu().numpy().astype(np.float64)
        _OPERANDS[(d, mode)] = (pb, pq, xb_s, xq_s)
    return _OPERANDS[(d, mode)]


def _keys_of(rng, rows):
    """Candidate keys naming ``rows`` (-1: an empty slot, key 0) under RANDOM score bits: the kernel must not read them."""
    bits = rng.integers(1, 1 << 32, rows.shape, dtype=np.uint64)
    keys = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.where(rows >= 0, rows, 0).astype(np.uint64))
    return np.where(rows >= 0, keys, np.uint64(0))


def _draw(rng, nq, kc, nb):
    return np.stack([rng.choice(nb, kc, replace=False) for _ in range(nq)]).astype(np.int64)


def _refine(be, pb, pq, keys, k, metric, score_exp=0):
    out = be.refine_keys(pb, pq, be.to_device(keys.view(np.int64)), k, metric)
    D, I = be.keys_to_result(out, metric, score_exp=score_exp)
    be.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), out.cpu().numpy().view(np.uint64)


def _check(xb_s, xq_s, rows, k, metric, D, I, bar=BAR, tie_gap=TIE_GAP, what=""):
    D_ref, I_ref = refine_reference(xb_s, xq_s, rows, k, metric)
    err, hard, _ = synth.compare_topk(D_ref, I_ref, D, I, atol=bar, tie_gap=tie_gap)
    valid = I_ref >= 0
    gaps = np.abs(np.diff(D_ref, axis=1))
    near = np.zeros_like(valid)
    near[:, 1:] |= gaps <= tie_gap
    near[:, :-1] |= gaps <= tie_gap
    share = float((near & valid).sum()) / max(1, int(valid.sum()))
    print(f"{what} k={k}: max score error {err:.3e} (bar {bar:.1e}), hard id mismatches {hard}, near-tie share {share:.4f}")
    assert err <= bar and hard == 0, (what, err, hard)
    assert share <= TIE_CAP, (what, share)
    assert np.array_equal(I == -1, I_ref == -1)

    def score_fn(q, ids):
        s = exact_scores(xb_s, xq_s[q], ids, metric)
        return s if metric == IP else -s

    synth.check_ids_by_rescoring(score_fn, D, I, [r[r >= 0] for r in rows], bar)
    return D_ref, I_ref


# ---- the kernel alone ----------------------------------------------------------------------------------------------------
# fewer lanes than a wave, a padded width, a pass and a half, passes; then the instantiations with 4 passes of 512 halfs, with 5 (on
# the six-pass kernel), with 6 (hi|lo queries: its own launch bounds) and the one that reads the query again per group of rows (dpad
# > 3 072).  The reference's near-tie share at the four wide ones, computed on the CPU, is at most 4.4 % (cap 15 %).
@pytest.mark.parametrize("d", [64, 100, 192, 768, 1536, 2048, 2500, 3072, 3200])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_planted_candidates_come_back_in_exact_order(hip_backend, mode, metric, d):
    be = hip_backend
    pb, pq, xb_s, xq_s = _operands(be, d, mode)
    rng = np.random.default_rng(1000 * d + 10 * mode + metric)
    for kc in (1, 7, 56, 64):
        rows = _draw(rng, NQ, kc, NB)
        keys = _keys_of(rng, rows)
        for k in sorted({1, kc // 2 + 1, kc}):
            D, I, _ = _refine(be, pb, pq, keys, k, metric)
            _check(xb_s, xq_s, rows, k, metric, D, I, what=f"mode={mode} metric={metric} d={d} kc={kc}")


@pytest.mark.parametrize("d", [192, 3072])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("qmode,bmode", [(F16, SPLIT), (SPLIT, F16)])
def test_mixed_operands_come_back_in_exact_order(hip_backend, qmode, bmode, metric, d):
    """fp16 queries against hi|lo rows and hi|lo queries against fp16 rows: the kernel's instantiations with different query and
    row pack modes, at one pass and a half and at six."""
    be = hip_backend
    pb, _, xb_s, _ = _operands(be, d, bmode)
    _, pq, _, xq_s = _operands(be, d, qmode)
    rng = np.random.default_rng(1000 * d + 100 * qmode + 10 * bmode + metric)
    for kc in (7, 64):
        rows = _draw(rng, NQ, kc, NB)
        keys = _keys_of(rng, rows)
        for k in sorted({1, kc // 2 + 1, kc}):
            D, I, _ = _refine(be, pb, pq, keys, k, metric)
            _check(xb_s, xq_s, rows, k, metric, D, I, what=f"queries mode={qmode} rows mode={bmode} metric={metric} d={d} kc={kc}")


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_empty_slots_equal_rows_and_the_corpus_ends(hip_backend, mode, metric):
    be = hip_backend
    d, kc, k = 192, 56, 20
    rng = np.random.default_rng(77 + mode + 2 * metric)
    xb, xq = synth.corpus(NB, d, seed=5), synth.corpus(NQ, d, seed=6)
    dup = np.sort(rng.choice(np.arange(1, NB - 1), 10, replace=False))
    xb[dup] = xb[dup[0]]  # ten identical rows
    xq[3] = xb[dup[0]]    # ... which are query 3's best
    if mode == F16:
        xb, xq = xb.astype(np.float16), xq.astype(np.float16)
    pb, pq = be.pack(xb, mode), be.pack(xq, mode)
    xb_s, xq_s = be.unpack(pb).cpu().numpy().astype(np.float64), be.unpack(pq).cpu().numpy().astype(np.float64)
    rows = _draw(rng, NQ, kc, NB)
    rows[rng.random(rows.shape) < 0.3] = -1  # empty slots scattered through the lists
    others = np.setdiff1d(np.arange(1, NB - 1), dup)
    rows[3] = rng.permutation(np.concatenate([dup, rng.choice(others, kc - 10, replace=False)]))
    rows[3][rng.choice(np.flatnonzero(~np.isin(rows[3], dup)), 8, replace=False)] = -1
    rows[5] = -1  # a query without a candidate
    rows[7][np.isin(rows[7], (0, NB - 1))] = -1
    rows[7, :2] = (NB - 1, 0)  # the corpus' last and first row
    rows[9] = -1
    rows[9, [4, 30, 55]] = (17, 2999, 1234)  # fewer candidates than k, anywhere in the list
    keys = _keys_of(rng, rows)
    D, I, out = _refine(be, pb, pq, keys, k, metric)
    D_ref, I_ref = _check(xb_s, xq_s, rows, k, metric, D, I, what=f"planted mode={mode} metric={metric}")
    assert np.array_equal((out != 0).sum(axis=1), np.minimum(k, (rows >= 0).sum(axis=1)))  # non-empty in -> non-empty out
    assert (out[5] == 0).all() and (I[5] == -1).all()
    assert (out[9, 3:] == 0).all() and sorted(I[9, :3]) == [17, 1234, 2999]
    assert np.array_equal(I[3, :10], dup) and (D[3, :10] == D[3, 0]).all()  # ascending rows, bit-equal scores
    assert np.array_equal(np.isin([0, NB - 1], I[7]), np.isin([0, NB - 1], I_ref[7]))
    sc = exact_scores(xb_s, xq_s[7], [0, NB - 1], metric)
    for r, s in zip((0, NB - 1), sc if metric == IP else -sc):
        if r in I[7]:
            assert abs(D[7][list(I[7]).index(r)] - s) <= BAR
    assert (out[:, :-1] >= out[:, 1:]).all()  # best first, empty slots last
    # one query and five: a workgroup with idle waves; every wave scores as in the full launch, bit for bit
    for n in (1, 5):
        Dn, In, outn = _refine(be, pb, be.slice_rows(pq, 0, n), np.ascontiguousarray(keys[:n]), k, metric)
        assert np.array_equal(outn, out[:n]) and np.array_equal(In, I[:n]) and np.array_equal(Dn, D[:n])


def test_scaled_hi_lo_rows_in_the_callers_units(hip_backend):
    """hi|lo rows of magnitude 1 000 are stored with a pack exponent; squared L2 comes back in the caller's units."""
    be = hip_backend
    d, kc, k, s = 100, 56, 10, 1000.0
    rng = np.random.default_rng(9)
    xb, xq = synth.corpus(NB, d, seed=11) * np.float32(s), synth.corpus(NQ, d, seed=12) * np.float32(s)
    pb = be.pack(xb, SPLIT, exp="auto")
    assert pb.exp != 0
    pq = be.pack(xq, SPLIT, exp=pb.exp)
    xb_s, xq_s = be.unpack(pb).cpu().numpy().astype(np.float64), be.unpack(pq).cpu().numpy().astype(np.float64)
    assert np.abs(xb_s - xb).max() <= 1e-3 * s
    rows = _draw(rng, NQ, kc, NB)
    D, I, _ = _refine(be, pb, pq, _keys_of(rng, rows), k, L2, score_exp=be.score_exp_of(pb, pq))
    assert 0.5 * s * s < D.max() < 4 * s * s
    _check(xb_s, xq_s, rows, k, L2, D, I, bar=BAR * s * s, tie_gap=TIE_GAP * s * s, what="scaled x1000 hi|lo L2")
    with pytest.raises(ValueError, match="scale exponent"):
        be.refine_keys(pb, be.pack(xq, SPLIT, exp=0), be.to_device(_keys_of(rng, rows).view(np.int64)), k, L2)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _clustered(n, d, centers, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d)).astype(np.float32)
    x = c[rng.integers(0, centers, n)] + 0.5 * rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


@pytest.mark.parametrize("metric", [METRIC_INNER_PRODUCT, METRIC_L2])
@pytest.mark.parametrize("codec", ["PQ8", "SQ8"])
def test_hipvs_refined_search(hip_backend, tmp_path, codec, metric):
    xb, xq = _clustered(4000, 64, 20, seed=31), _clustered(50, 64, 20, seed=32)
    K, path = 10, str(tmp_path / "idx")
    vr = HipVS(factory_string=f"IVF16,{codec},Refine(Flat)", nprobe=4, metric=metric, k_factor=5, device="cuda:0")
    vr.index(None, xb, path)
    vp = HipVS(factory_string=f"IVF16,{codec}", nprobe=4, metric=metric, device="cuda:0")
    vp.load_index(path)
    kc = vr.refine_candidates(K)
    assert kc == 50
    be = vr.backend
    be.timing_enable(True)
    out = vr(xq, K)
    t = be.timing_read_full()
    be.timing_enable(False)
    assert t["kernel"] == "lvs_refine_kernel" and t["calls"] == 2, t  # the scan, then the re-ranking: no exact fall-back
    cand = vp(xq, kc).indices
    ent = vr._current()
    xb_s = be.unpack(ent.packed).cpu().numpy().astype(np.float64)
    xq_s = be.unpack(be.pack(xq, ent.packed.mode, exp=ent.packed.exp)).cpu().numpy().astype(np.float64)
    _check(xb_s, xq_s, cand, K, metric, out.distances, out.indices, what=f"HipVS {codec} metric={metric}")
    dev = vr(xq, K, return_device=True)
    assert np.array_equal(dev.distances.cpu().numpy(), out.distances) and np.array_equal(dev.indices.cpu().numpy(), out.indices)
    # the re-ranking finds more of the true neighbours than the codes alone
    flat = HipVS(metric=metric, device="cuda:0")
    flat.load_index(path)
    truth, plain = flat(xq, K).indices, vp(xq, K).indices
    hits = lambda got: sum(len(set(a) & set(b)) for a, b in zip(got, truth))  # noqa: E731
    assert hits(out.indices) >= hits(plain)
