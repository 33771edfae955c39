"""Host half of the width tests (tests/width_cases.py; the kernels run in tests/test_gpu_widths.py).

* The case table is honest about the branch each stream case reaches: the compiled planner (lvs_flat_plan + lvs_flat_route through
  tests/native/plan_check.cpp's ``route`` question) gives the launch shape, the instantiation follows from it exactly as
  ``stream_launch_nqb`` / ``stream_launch_mode`` (lvs_stream.hip) choose it, and the classes reached must cover every branch the
  narrow widths of the other GPU tests never take.
* Both LDS edges of the stream kernel are pinned.
* Teeth: ``check_topk_exact`` rejects, for every top-k case, the answer of a kernel that skips one 16-column A fragment and of
  one that skips a hi|lo cross segment."""
import numpy as np
import pytest

import plan_native
import width_cases as wc
from width_cases import F16, SPLIT, G

KIND_STREAM, KIND_LIST = 2, 3


def _route(nq, nb, d, k, bmode, qmode):
    kind, nbfrag, kcap, nqb, groups, sample, jper, nseg = plan_native.ask([f"route {nq} {nb} {d} {k} {bmode} {qmode}"])[0]
    return dict(kind=kind, nbfrag=nbfrag, kcap=kcap, nqb=nqb, groups=groups, sample=sample, jper=jper, nseg=nseg)


def _unroll(jper, nqb, seed):
    """stream_launch_nqb: the largest of 16 / 24 / 8 that divides the fragments per K segment (24: one query block, not SEED)."""
    if jper % 16 == 0:
        return 16
    if nqb == 1 and not seed and jper % 24 == 0:
        return 24
    if jper % 8 == 0:
        return 8
    return G


def stream_class(c):
    r = _route(c.nq, c.nb, c.d, c.k, c.bmode, c.qmode)
    assert r["kind"] == KIND_STREAM, (c.name, r)
    assert r["nqb"] in (1, 2, 3) and r["kcap"] >= c.k  # stream_launch_mode: 1 -> four waves, 2 and 3 -> eight
    assert r["jper"] * 16 == -(-c.d // 64) * 64
    seed = _unroll(r["jper"], r["nqb"], True) if r["sample"] > 0 else None
    return wc.StreamClass(_unroll(r["jper"], r["nqb"], False), r["nqb"], r["groups"], seed, r["jper"], r["nseg"]), r


def test_every_stream_case_reaches_its_class_and_the_classes_cover_the_branches():
    reached = []
    for c in wc.STREAM_CASES:
        cls, r = stream_class(c)
        assert cls == c.cls, (c.name, cls, c.cls)
        assert r["nbfrag"] * 1024 * r["nqb"] + r["nqb"] * 32 * (r["kcap"] * 8 + 4) <= 160 * 1024
        reached.append(cls)
    nj = lambda s: s.jper * s.nseg  # noqa: E731
    gen = [s for s in reached if s.U == G]
    for nseg in (1, 2, 3):  # the general stream wraps inside a block (nj > UNROLL), for every count of K segments
        assert any(s.nseg == nseg and nj(s) > 16 for s in gen), nseg
    assert any(nj(s) < 16 for s in gen)                    # ... and the one shape the narrow tests did run
    assert {2, 3} <= {s.nqb for s in gen}
    assert any(s.seed == G for s in gen)
    assert any(s.U == 24 and s.jper > 24 for s in reached)  # the pointer hand-over inside a run
    assert any(s.U == 8 and s.jper > 8 and s.nqb == 1 for s in reached)
    assert any(s.U == 8 and s.jper > 8 and s.nqb == 2 for s in reached)
    assert any(s.seed == 8 and s.jper > 8 for s in reached)
    assert any(s.U == 16 and s.jper >= 64 for s in reached)
    assert any(s.seed == 16 and s.jper >= 64 for s in reached)
    assert any(s.groups == 2 for s in reached)
    assert any(s.jper == 140 for s in reached) and any(s.jper == 68 and s.nseg == 3 for s in reached)  # the widest that fit


def test_tile_cases_go_to_the_list_kernel():
    for c in wc.TILE_CASES:
        assert _route(c.nq, c.nb, c.d, c.k, c.bmode, c.qmode)["kind"] == KIND_LIST, c.name


def test_the_stream_kernels_lds_edge():
    """One 32-query block with 64 list slots beside nbfrag KB of query fragments in 160 KiB: 140 fragments fit (159 872 B), 144
    do not (163 968 B) - fp16 queries up to dpad 2 240, hi|lo queries up to dpad 1 088."""
    nq, nb, k = 1, 4133, 56
    for mode, last in ((F16, 2240), (SPLIT, 1088)):
        fits, beyond = _route(nq, nb, last, k, mode, mode), _route(nq, nb, last + 1, k, mode, mode)
        assert fits["kind"] == KIND_STREAM and (fits["nqb"], fits["groups"], fits["kcap"]) == (1, 1, 64), fits
        assert fits["nbfrag"] == 140 - 4 * mode and beyond["kind"] == KIND_LIST, (fits, beyond)
        assert fits["nbfrag"] * 1024 + 32 * 64 * 8 + 32 * 4 <= 160 * 1024 < (fits["nbfrag"] + 4 * (1 + mode)) * 1024 + 32 * 64 * 8 + 32 * 4
    # the literal sem_search call with float32 embeddings of d = 1 536: no stream launch, whatever the corpus
    for nb in (4133, 20000, 1000000):
        assert _route(1, nb, 1536, 10, SPLIT, SPLIT)["kind"] == KIND_LIST


def test_the_route_question_is_the_dump():
    """``route`` goes through the same lvs_flat_plan + lvs_flat_route as the pinned dump (tests/test_plan_pins.py)."""
    r = _route(96, 1000000, 768, 10, F16, F16)  # "route 2 48 16 3 1"
    assert (r["kind"], r["nbfrag"], r["kcap"], r["nqb"], r["groups"]) == (2, 48, 16, 3, 1)
    assert r["sample"] == 32768 and (r["jper"], r["nseg"]) == (48, 1)
    assert _route(1, 1000000, 768, 10, F16, F16)["sample"] == 0  # one query runs unseeded
    assert _route(96, 1000000, 768, 10, SPLIT, SPLIT)["kind"] == KIND_LIST
    assert _route(100000, 1000000, 768, 100, F16, F16)["kind"] == KIND_LIST  # the two-phase search's fallback


# ---- the checker itself -----------------------------------------------------------------------------------------------------
def test_check_topk_exact_on_small_hand_made_results():
    S = np.array([[0.9, 0.5, 0.5, 0.1, 0.50001]])
    D, I = wc.topk64(S, 3)
    assert I.tolist() == [[0, 4, 1]]
    assert wc.check_topk_exact(S, D, I, 3) == 0.0
    wc.check_topk_exact(S, [[0.9, 0.5, 0.5]], [[0, 1, 2]], 3)          # row 4 left out, 1e-5 above the weakest: inside the gap
    wc.check_topk_exact(S, [[0.9, 0.500005, 0.500004]], [[0, 1, 4]], 3)  # two rows 1e-5 apart in either order
    for D, I in (([[0.9, 0.5, 0.5]], [[0, 2, 1]]),                     # equal scores out of id order
                 ([[0.9, 0.5, 0.50001]], [[0, 1, 4]]),                 # D rises
                 ([[0.9, 0.50001, 0.1]], [[0, 4, 3]]),                 # rows 1 and 2 left out, 0.4 above the weakest
                 ([[0.9, 0.50001, 0.50001]], [[0, 4, 4]]),             # an id twice
                 ([[0.9, 0.50001, 0.5]], [[0, 4, 5]]),                 # out of range
                 ([[0.9, 0.50001, 0.5]], [[0, 4, -1]]),                # a hole although rows remain
                 ([[0.90002, 0.50001, 0.5]], [[0, 4, 1]]),             # a score 2e-5 off
                 ([[0.5, 0.5, 0.5]], [[1, 2, 0]])):                    # the best row last (with its score bent to hide it)
        with pytest.raises(AssertionError):
            wc.check_topk_exact(S, D, I, 3)
    D, I = wc.topk64(S, 7)  # k > nb: five ids, then -1
    assert I[0, 5:].tolist() == [-1, -1]
    wc.check_topk_exact(S, D, I, 7)
    I[0, 4] = -1
    with pytest.raises(AssertionError):
        wc.check_topk_exact(S, D, I, 7)


def test_stored64_is_what_the_device_stores():
    x = np.array([[1.0 + 2.0 ** -12, 0.1, -3.3e-5, 0.0]], np.float32)
    assert np.array_equal(wc.stored64(x, F16), x.astype(np.float16).astype(np.float64))
    hi, lo = wc.split64(x)
    assert np.array_equal(wc.stored64(x, SPLIT), hi + lo) and np.abs(wc.stored64(x, SPLIT) - x).max() <= 2.0 ** -22
    assert lo[0, 0] == 2.0 ** -12 and hi[0, 0] == 1.0


# ---- teeth ------------------------------------------------------------------------------------------------------------------
def wrong_products(c, xb, xq):
    """q.b of every pair as a kernel with one piece of its K loop missing would sum it -> [(what, products)].
    The fragment: the last 16 columns that hold data (the last A fragment of dpad wherever that one is not all padding - at
    d = 1 100, 1 089 and 2 241 it is, and skipping it would change nothing).  The segment: hi . lo of the corpus' lo parts
    (hi|lo corpus), else lo . hi of the queries' lo parts."""
    xb_s, xq_s = wc.stored64(xb, c.bmode), wc.stored64(xq, c.qmode)
    qb = xq_s @ xb_s.T
    c0 = (c.d - 1) // 16 * 16
    out = [("fragment", qb - xq_s[:, c0:c0 + 16] @ xb_s[:, c0:c0 + 16].T)]
    if c.bmode == SPLIT:
        out.append(("segment", qb - wc.split64(xq)[0] @ wc.split64(xb)[1].T if c.qmode == SPLIT else qb - xq_s @ wc.split64(xb)[1].T))
    elif c.qmode == SPLIT:
        out.append(("segment", qb - wc.split64(xq)[1] @ xb_s.T))
    return xb_s, xq_s, qb, out


@pytest.mark.parametrize("c", wc.TOPK_CASES, ids=lambda c: c.name)
def test_the_checker_rejects_a_dropped_fragment_and_a_dropped_segment(c):
    xb, xq = wc.case_data(c)
    xb_s, xq_s, qb, wrong = wrong_products(c, xb, xq)
    qn, bn = (xq_s * xq_s).sum(1), (xb_s * xb_s).sum(1)
    S = wc.scores_from_products(qb, qn, bn, c.metric)
    D, I = wc.topk64(S, c.k)
    assert wc.check_topk_exact(S, D, I, c.k) == 0.0  # the reference's own answer passes
    for what, products in wrong:
        Dw, Iw = wc.topk64(wc.scores_from_products(products, qn, bn, c.metric), c.k)
        with pytest.raises(AssertionError):
            wc.check_topk_exact(S, Dw, Iw, c.k)
            print(f"{c.name}: the answer with the {what} dropped passes: the case does not discriminate")
