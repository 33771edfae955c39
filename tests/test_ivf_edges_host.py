"""Every case of ivf_edge_cases.py through ``PqOracleBackend``, without a GPU: the construction runs, the case's
preconditions hold (it is what it claims to be, the reference stays inside every cap, at most 15 % of its slots are near
ties), and the assertions the GPU test makes pass on a backend that is right by construction.  Large cases are checked on
fewer queries here; the case itself is never changed."""
import numpy as np
import pytest

import ivf_edge_cases as E
import plan_native
import synth
from ivf_pq_oracle_backend import PqOracleBackend
from lotus_amd import _capi


@pytest.mark.parametrize("name,mode", E.PARAMS, ids=[f"{n}-{m}" for n, m in E.PARAMS])
def test_case_is_what_it_claims(name, mode):
    be = PqOracleBackend()
    case = E.build(name)
    pick = np.arange(case.xq.shape[0]) if case.pick is None else case.pick
    if case.host_queries is not None and case.post is None:
        pick = pick[:case.host_queries]
    res = E.run_case(be, case, mode, pick=pick, only_picked=True)
    E.preconditions(be, case, mode, res)
    E.check_result(case, mode, res)


def test_every_family_meets_every_mode():
    by_mode = {m: {n.split("-")[0] for n, mm in E.PARAMS if mm == m} for m in (E.FLAT, E.SQ8, E.PQ)}
    for m, fams in by_mode.items():
        assert {"planted", "hot", "ramp", "tied", "wide", "k1", "k56", "scaled", "common", "signs"} <= fams, (m, fams)
    assert [k for k in E.KS if f"k{k}" in E.CASES] == E.KS


def test_shapes_beyond_the_scans_are_refused():
    """"Refused": the workspace function answers LVS_EUNSUPPORTED and the backend's *_fits returns False."""
    be = PqOracleBackend()
    lib = _capi.load()
    for pack, dmax in E.FLAT_DMAX.items():
        assert E.largest_flat_d(be, pack) == dmax and be.ivf_fits(dmax, 56, pack)
        assert not be.ivf_fits(dmax + 64, 56, pack)
        assert lib.lvs_ivf_search_workspace_bytes(1, 1, 1, dmax + 64, 56, pack) == _capi.EUNSUPPORTED
    for pack in (E.F16, E.SPLIT):
        assert be.ivf_sq8_fits(2368, 56, pack) and not be.ivf_sq8_fits(2369, 56, pack)
        assert lib.lvs_ivf_sq8_search_workspace_bytes(1, 1, 1, 2369, 56, pack) == _capi.EUNSUPPORTED
        assert be.ivf_pq_fits(636, 159, 56, pack) and not be.ivf_pq_fits(640, 160, 56, pack)
        assert lib.lvs_ivf_pq_search_workspace_bytes(1, 1, 1, 640, 160, 56, pack) == _capi.EUNSUPPORTED


def test_budget_cases_halve_the_chunk():
    """The two cases meant to exceed the 512 MB scratch budget do: all their queries at once need more than the planner ever
    asks for, so it runs them in chunks of min(nq, 16 384) halved (rounding up) until one fits: 3 001 -> 1 501 -> 751 -> 376
    queries for the two tiled modes, 10 001 -> 5 001 -> 2 501 under the tables of M = 159."""
    lib = _capi.load()
    for need, plan, chunk in (
            (lib.lvs_ivf_search_workspace_bytes(3001, 8200, 2048, 64, 56, E.F16), ("Flat", 3001, 8200, 2048, 64, 56, E.F16), 376),
            (lib.lvs_ivf_sq8_search_workspace_bytes(3001, 8200, 2048, 64, 56, E.F16), ("SQ8", 3001, 8200, 2048, 64, 56, E.F16), 376),
            (lib.lvs_ivf_pq_search_workspace_bytes(10001, 40, 4, 636, 159, 56, E.SPLIT), ("PQ", 10001, 40, 4, 636, 56, E.SPLIT, 159), 2501)):
        assert 0 < need <= E.WS_BUDGET
        assert plan_native.ivf_chunk(*plan) == (chunk, plan[1] % chunk, need)
    assert 3001 * 2048 * 56 * 8 > E.WS_BUDGET and 10001 * 159 * 256 * 4 > E.WS_BUDGET
    # the planner never arrives below 128 queries: every halving sequence from 256 or more has an element in [128, 255],
    # and a chunk of 255 fits unhalved (its scratch is more than that of 128, and within the budget)
    for fn, args in ((lib.lvs_ivf_search_workspace_bytes, (8200, 2048, 64, 56, E.F16)),
                     (lib.lvs_ivf_sq8_search_workspace_bytes, (8200, 2048, 64, 56, E.F16)),
                     (lib.lvs_ivf_pq_search_workspace_bytes, (8200, 2048, 64, 8, 56, E.F16)),
                     (lib.lvs_ivf_pq_search_workspace_bytes, (40, 4, 636, 159, 56, E.SPLIT))):
        assert 0 < fn(128, *args) < fn(255, *args) <= E.WS_BUDGET
    pick = E.chunk_boundary_sample(3001, 404)
    for b in (3000, 1501, 751, 752, 376, 375, 188, 189, 2 * 376, 7 * 376 + 1):
        assert b in pick
    assert 300 <= len(pick) <= 700


def test_grouped_reference_is_the_per_query_reference():
    """The batched float64 reference of the 5 000-query cases against sq8_reference, query by query."""
    from ivf_sq8_oracle_backend import sq8_reference

    rng = np.random.default_rng(1)
    x = rng.standard_normal((3000, 16))
    x[100:140] = x[100]  # exact ties
    off, rows = E.deal([0, 700, 1, 2299], 2)
    q = rng.standard_normal((40, 16)).astype(np.float32)
    probe = np.stack([rng.choice(4, 2, replace=False) for _ in range(40)])
    for metric in (E.IP, E.L2):
        D, I = E.grouped_reference(x, q, 56, metric, off, rows, probe)
        D1, I1 = sq8_reference(x, q, 56, metric, off, rows, probe)
        assert np.array_equal(I, I1)
        np.testing.assert_allclose(np.where(I >= 0, D, 0), np.where(I1 >= 0, D1, 0), rtol=1e-6)


def test_rescoring_catches_what_compare_topk_excuses():
    """A right score beside a neighbouring row's number passes compare_topk at k = 1 and fails the rescoring check."""
    xb = synth.corpus(500, 32, seed=1).astype(np.float64)
    xq = synth.queries(xb.astype(np.float32), 6, seed=2)[0]
    S = xq.astype(np.float64) @ xb.T
    I = np.argmax(S, axis=1)[:, None]
    D = np.take_along_axis(S, I, axis=1)
    off, rows = np.array([0, 500]), np.arange(500, dtype=np.uint32)
    fn, allowed = E.rescoring_args(xb, xq, E.IP, off, rows, np.zeros((6, 1), np.int64))
    synth.check_ids_by_rescoring(fn, D, I, allowed, 1e-5)
    wrong = (I + 1) % 500
    assert synth.compare_topk(D, I, D, wrong)[:2] == (0.0, 0)
    with pytest.raises(AssertionError):
        synth.check_ids_by_rescoring(fn, D, wrong, allowed, 1e-5)
    with pytest.raises(AssertionError):  # a repeated id
        synth.check_ids_by_rescoring(fn, np.repeat(D, 2, axis=1), np.repeat(I, 2, axis=1), allowed, 1e-5)
    with pytest.raises(AssertionError):  # a row of no probed list
        synth.check_ids_by_rescoring(fn, D, I, [np.setdiff1d(rows, I[q]) for q in range(6)], 1e-5)
