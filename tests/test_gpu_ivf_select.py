"""The row selector of the three IVF list scans (``*_keys_sel``) on the planted inputs of ivf_select_cases.py: random
selections over list lengths around every scan's block size, a lone selected last row, skipped blocks, selector word edges
with garbage past the last row, fewer selected rows than k, complements, several tiles per list and re-ranking.  Per case:
scores within the bar of the float64 reference over the FILTERED probed lists, ids equal outside near ties, the -1 pattern,
every returned id selected and rescored on the CPU, and the mode's scan kernel named by the timing - an exact fall-back
cannot make a case pass.  test_ivf_select_host.py proves on the CPU that each case is what it claims to be.  Then one
end-to-end search per mode through ``HipVS(ids_probe=True)``."""
import numpy as np
import pytest

import ivf_edge_cases as E
import ivf_select_cases as S
import synth
from ivf_oracle_backend import ivf_reference
from ivf_select_oracle_backend import filter_lists
from ivf_sq8_oracle_backend import list_of_rows, sq8_decode, sq8_reference
from ivf_pq_oracle_backend import pq_decode
from lotus_amd import HipVS, METRIC_INNER_PRODUCT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,mode", S.PARAMS, ids=[f"{n}-{m}" for n, m in S.PARAMS])
def test_selected_scan_matches_the_filtered_reference(hip_backend, name, mode):
    sc = S.build(name)
    res = S.run_sel(hip_backend, sc, mode)
    print(f"{name}-{mode}: bar {res['bar']:.3g}, {int(res['mask'].sum())} rows selected, kernel {res['kernel']}")
    assert res["kernel"] == E.SCAN_KERNEL[mode]
    S.preconditions(hip_backend, sc, mode, res)
    S.check_result(sc, mode, res)


@pytest.mark.parametrize("mode", S.MODES)
def test_all_selected_is_bit_identical_to_the_plain_search(hip_backend, mode):
    plain, full = S.all_selected_is_the_plain_search(hip_backend, mode)
    assert plain["kernel"] == full["kernel"] == E.SCAN_KERNEL[mode]


@pytest.mark.parametrize("mode", S.MODES)
def test_a_selection_and_its_complement_merge_to_the_plain_search(hip_backend, mode):
    for res in S.complement_merges_to_the_plain_search(hip_backend, mode):
        assert res["kernel"] == E.SCAN_KERNEL[mode]


@pytest.mark.parametrize("mode", (S.SQ8, S.PQ))
def test_refine_over_a_selection(hip_backend, mode):
    res = S.refine_over_a_selection(hip_backend, mode)
    assert res["kernel"] == E.SCAN_KERNEL[mode]


@pytest.mark.parametrize("fs,mode", [("IVF32,Flat", S.FLAT), ("IVF32,SQ8", S.SQ8), ("IVF32,PQ8", S.PQ)])
def test_hipvs_ids_probe_end_to_end(hip_backend, fs, mode):
    """``HipVS(ids_probe=True)`` -> ``index`` -> ``__call__(ids=...)`` against the filtered-lists rule over ``ivf_probe``'s
    lists and the store's own codes."""
    be = hip_backend
    n, d, nq, k, nprobe = 6000, 64, 100, 10, 4
    xb = synth.corpus(n, d, seed=41)
    xq = synth.queries(xb, nq, seed=42)[0]
    ids = np.sort(np.random.default_rng(43).choice(n, 2400, replace=False))  # 40 %: 2 400 * 32 > 6 000 * 4
    vs = HipVS(backend=be, factory_string=fs, nprobe=nprobe, ids_probe=True, storage="fp16")
    vs.index(None, xb.astype(np.float16), "e2e-" + mode, persist=False)
    be.timing_enable(True)
    try:
        out = vs(xq.astype(np.float16), k, ids=ids)
        kernel = be.timing_read_full()["kernel"]
    finally:
        be.timing_enable(False)
    assert kernel == E.SCAN_KERNEL[mode]
    D, I = np.asarray(out.distances), np.asarray(out.indices)
    c, off, rows = vs.ivf_lists()
    probe = vs.ivf_probe(xq.astype(np.float16))
    mask = np.zeros(n, bool)
    mask[ids] = True
    off_f, rows_f = filter_lists(off, rows, mask)
    x16 = xb.astype(np.float16).astype(np.float32)
    q16 = xq.astype(np.float16).astype(np.float32)
    if mode == S.FLAT:
        D_ref, I_ref = ivf_reference(x16, q16, k, METRIC_INNER_PRODUCT, c, off_f, rows_f, probe)
        xref = x16
    else:
        where = list_of_rows(off, rows, n)
        if mode == S.SQ8:
            vmin, vdiff, codes, _ = vs.sq8_codes()
            xref = sq8_decode(c, where, vmin, vdiff, codes)
        else:
            books, codes, _ = vs.pq_codes()
            xref = pq_decode(c, where, books, codes)
        D_ref, I_ref = sq8_reference(xref, q16, k, METRIC_INNER_PRODUCT, off_f, rows_f, probe)
    assert E.near_tie_share(D_ref, I_ref, 2e-5) <= E.NEAR_TIE_CAP
    err, hard, _ = synth.compare_topk(D_ref, I_ref, D, I, atol=1e-5, tie_gap=2e-5)
    print(f"{fs}: max score error {err:.3g}, hard id mismatches {hard}")
    assert err <= 1e-5 and hard == 0
    assert np.array_equal(I == -1, I_ref == -1) and np.isin(I[I >= 0], ids).all()
    score_fn, allowed = E.rescoring_args(xref, q16, METRIC_INNER_PRODUCT, off_f, rows_f, probe)
    synth.check_ids_by_rescoring(score_fn, D, I, allowed, 1e-5)
