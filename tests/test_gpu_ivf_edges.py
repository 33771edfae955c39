"""The three IVF list scans on the planted inputs of ivf_edge_cases.py: list lengths around the kernels' block sizes, a hot
list, maximal insertion pressure, mass ties, nlist beyond one round of lvs_ivf_tiles_kernel, nprobe up to 2 048, chunks
halved by the scratch budget, every k around the kcap switches, the row widths at and beside each scan's limits, and
values away from unit Gaussians.  Per case: scores within the bar of the float64 reference over the probed lists and ids
equal outside near ties (compare_topk), the -1 pattern, the probes, every returned id rescored on the CPU
(check_ids_by_rescoring), and the mode's scan kernel named by the timing - an exact fall-back cannot make a case pass.
test_ivf_edges_host.py proves on the CPU that each case is what it claims to be."""
import numpy as np
import pytest

import ivf_edge_cases as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,mode", E.PARAMS, ids=[f"{n}-{m}" for n, m in E.PARAMS])
def test_scan_matches_the_reference(hip_backend, name, mode):
    case = E.build(name)
    res = E.run_case(hip_backend, case, mode)
    print(f"{name}-{mode}: bar {res['bar']:.3g} checked {len(res['pick'])} queries, kernel {res['kernel']}")
    assert res["kernel"] == E.SCAN_KERNEL[mode]
    E.preconditions(hip_backend, case, mode, res)
    E.check_result(case, mode, res)


def test_shapes_beyond_the_scans_are_refused(hip_backend):
    be = hip_backend
    for pack, dmax in E.FLAT_DMAX.items():
        assert be.ivf_fits(dmax, 56, pack) and not be.ivf_fits(dmax + 64, 56, pack)
    for pack in (E.F16, E.SPLIT):
        assert be.ivf_sq8_fits(2368, 56, pack) and not be.ivf_sq8_fits(2369, 56, pack)
        assert be.ivf_pq_fits(636, 159, 56, pack) and not be.ivf_pq_fits(640, 160, 56, pack)
