"""Every flat search route, the threshold join, the score rows and the nearest search on the device, bit for bit, on inputs
whose float32 arithmetic is exact in any summation order (tests/lattice_cases.py: small integers times a power of two, full
of natural ties).  Each leg's only comparison is an equality - of keys, of pair sets, of score bits - with the CPU oracle's
result: no tie gap, no excused last rank, no score tolerance.  tests/test_lattice_host.py checks on the CPU that the inputs are
exact, that the ties are there, which kernel the planner sends each case to, and that every leg passes on the oracle's backend.

Every top-k and join test asserts the kernel the timing hook reports (the last timed launch of the call), and the launches
where the case is about chunking, and prints both (run with -s)."""
import pytest

import lattice_cases as lc
from lattice_cases import IP, L2
from lotus_amd import _capi

pytestmark = pytest.mark.gpu

assert (lc.F16, lc.SPLIT, IP, L2) == (_capi.PACK_F16, _capi.PACK_SPLIT, _capi.METRIC_IP, _capi.METRIC_L2)


@pytest.mark.parametrize("c", lc.TOPK_CASES, ids=lambda c: c.name)
def test_lattice_topk(hip_backend, c):
    out = lc.run_topk(hip_backend, c)
    print(f"\n{c.name}: {out['kernel']} launches {out['launches']} calls {out['calls']} {out['stats'] or ''}", end="")
    if c.one_pass:  # the last timed launch is the plain search of the queries the certificate left open: a few of them, any kernel
        assert out["kernel"] in (lc.TILE, lc.STREAM, lc.RQ) and out["calls"] >= 1, out
        return
    assert out["kernel"] == c.kernel and out["calls"] >= 1, out
    if c.launches:
        assert out["launches"] == c.launches and out["calls"] == 1, out


def test_lattice_shards(hip_backend):
    lc.run_shards(hip_backend)


@pytest.mark.parametrize("c", lc.JOIN_CASES, ids=lambda c: c.name)
def test_lattice_join(hip_backend, c):
    out = lc.run_join(hip_backend, c)
    print(f"\n{c.name}: {out['pairs']} pairs, {out['kernel']} launches {out['launches']}", end="")
    if c.stride == 1:
        runs = 1 if out["pairs"] <= c.capacity else 2  # beyond the capacity: counted, then run again
        assert out["kernel"] == c.kernel and out["launches"] == runs * len(c.plan), out


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("bpack,qpack", lc.SCORES_PACKS)
def test_lattice_scores(hip_backend, bpack, qpack, metric):
    lc.run_scores(hip_backend, bpack, qpack, metric)


@pytest.mark.parametrize("metric", [IP, L2])
def test_lattice_rank_all(hip_backend, metric):
    lc.run_rank_all(hip_backend, metric)


@pytest.mark.parametrize("bpack,qpack", lc.NEAREST_PACKS)
@pytest.mark.parametrize("nq,nb,d", lc.NEAREST_SHAPES)
def test_lattice_nearest(hip_backend, nq, nb, d, bpack, qpack):
    stats = lc.run_nearest(hip_backend, nq, nb, d, bpack, qpack)
    print(f"\nnearest {nq} x {nb} x {d} packs {bpack}/{qpack}: {stats}", end="")
    assert (bpack, qpack) == (lc.F16, lc.F16) or stats.get("queries") == nq, stats  # the certified one-pass route ran
