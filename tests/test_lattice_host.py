"""Host half of the exact-arithmetic tests (tests/lattice_cases.py; the kernels run in tests/test_gpu_lattice.py).  Per case:

* the guards - conditions on the inputs and the reference alone: float32 arithmetic on the case is exact in any summation order,
  and the ties are there (at least half of a top-k case's queries have equal k-th and (k + 1)-th reference scores, 0.1 for the
  dense cases; at least a tenth as many pairs exactly at a join's threshold as above it, 1 000 .. 200 000 above);
* the route - the compiled planner (tests/native/plan_check.cpp) confirms the kernel, chunks and geometry the case declares;
* every ``run_*`` on the CPU oracle's backend: the case and its assertions are what they claim before the device sees them."""
import numpy as np
import pytest

import lattice_cases as lc
from lattice_cases import F16, IP, L2, SPLIT


@pytest.fixture(scope="module")
def be():
    return lc.ExactOracleBackend()


def test_the_generator_gives_fp16_lattice_values():
    for dense in (False, True):
        x = lc.lattice(500, 96, 3, **lc.flavour(96, dense))
        assert x.dtype == np.float32 and np.array_equal(x, x.astype(np.float16).astype(np.float32)) and not lc.split_lo(x).any()
        assert set(np.unique(x / lc.STEP)) == ({-2.0, -1.0, 0.0, 1.0, 2.0} if dense else {-1.0, 0.0, 1.0})
    assert abs((lc.lattice(500, 64, 3, **lc.flavour(64, False)) != 0).mean() - 0.5 * 2 / 3) < 0.02
    lo = np.float32(lc.STEP + lc.LO_STEP)  # the real-lo leg's 12-bit value: hi = 2^-3, lo = 2^-14
    assert lo == np.float32((1 + 2.0 ** -11) * 2.0 ** -3) and np.float16(lo) == lc.STEP and lc.split_lo([lo])[0] == lc.LO_STEP


def test_ref_keys_is_pack_keys_of_the_oracles_result():
    xb, xq = lc.lattice(9, 8, 1, 1, 0.5), lc.lattice(2, 8, 2, 1, 0.5)
    keys = lc.ref_keys(xb, xq, 12, L2, id_offset=100)
    assert keys.dtype == np.uint64 and keys.shape == (2, 12) and (keys[:, 9:] == 0).all() and (keys[:, :9] != 0).all()
    better, ids, empty = lc.oracle.flat.unpack_keys(keys)
    s = lc.scores64(xb, xq, L2)
    for q in range(2):
        order = np.lexsort((np.arange(9), -s[q]))
        assert np.array_equal(ids[q, :9], order + 100) and np.array_equal(better[q, :9], s[q, order])


def test_the_case_table_names_every_route_once():
    names = [c.name for c in lc.TOPK_CASES] + [c.name for c in lc.JOIN_CASES]
    assert len(set(names)) == len(names)
    assert {c.kernel for c in lc.TOPK_CASES} == {lc.TILE, lc.STREAM, lc.RQ, lc.RJ}
    assert max(c.nq * c.nb * c.d for c in lc.TOPK_CASES) == 65536 * 32768 * 256  # the largest launch
    assert all(c.m <= 512 for c in lc.TOPK_CASES)


@pytest.mark.parametrize("c", lc.TOPK_CASES, ids=lambda c: c.name)
def test_topk_case_guards_route_and_oracle(be, c):
    tied = lc.topk_guards(c)
    plan = lc.planned(c)
    assert {k: plan.get(k) for k, _ in c.plan} == dict(c.plan), (c.name, plan)
    assert {lc.ROUTE_STREAM: lc.STREAM, lc.ROUTE_LIST: lc.TILE}.get(plan["kind"], c.kernel) == c.kernel
    if "chunk_kernels" in plan:  # the hook reports the LAST chunk's kernel
        assert c.kernel == (lc.RQ if plan["chunk_kernels"][-1] == lc.CHUNK_RQ else lc.RJ)
        assert not c.launches or c.launches == len(plan["chunks"])
    out = lc.run_topk(be, c, host=True)
    print(f"\n{c.name}: tied at rank k {tied}, plan {plan}, oracle stats {out['stats']}", end="")


def test_shards_on_the_oracle(be):
    assert lc.SHARD_BOUNDS[0] == (0, 200) and lc.SHARD_BOUNDS[1][0] == lc.SHARD_BOUNDS[1][1] and lc.SHARD_BOUNDS[-1][1] == lc.SHARD_CASE.nb
    assert all(a[1] == b[0] for a, b in zip(lc.SHARD_BOUNDS, lc.SHARD_BOUNDS[1:]))
    assert any((hi - lo) % 256 for lo, hi in lc.SHARD_BOUNDS[2:])
    lc.run_shards(be)


@pytest.mark.parametrize("c", lc.JOIN_CASES, ids=lambda c: c.name)
def test_join_case_guards_route_and_oracle(be, c):
    thr, above, at = lc.join_guards(c)
    assert lc.join_planned(c) == c.plan, (c.name, lc.join_planned(c))
    assert c.kernel == lc.TILE  # every plan here ends with a launch of the list kernel (the rj launches' 29-row tail)
    out = lc.run_join(be, c)
    assert out["pairs"] == above
    print(f"\n{c.name}: thr {thr}, {above} pairs above, {at} at the threshold", end="")


def test_a_join_that_is_not_strict_fails_by_the_pairs_at_the_threshold(be):
    """Teeth: ``>=`` instead of ``>`` is a difference of tens of thousands of pairs, and the leg's assertion sees it."""
    c = lc.JOIN_CASES[0]
    S, thr, above, at = lc.join_reference(c.nq, c.nb, c.d, c.metric, c.q_row0)
    assert at >= 10_000
    q, j = np.nonzero(S >= np.float32(thr))
    import torch

    with pytest.raises(AssertionError):
        lc._assert_pairs((torch.from_numpy(q), torch.from_numpy(j), torch.from_numpy(S[q, j])), S, thr, "not strict")


def test_a_wrong_tie_order_at_the_last_rank_fails():
    """Teeth: the later of two equal rows in a list's last slot changes one key, and the leg's assertion sees it."""
    c = lc.SHARD_CASE
    D, I = lc._topk_ref(c)
    want = lc.topk_ref_keys(c)
    q = int(np.argmax(D[:, c.k - 1] == D[:, c.k]))
    wrong = want.copy()
    wrong[q, c.k - 1] = lc._keys_of(D[q:q + 1, c.k:], I[q:q + 1, c.k:], c.metric)[0, 0]  # the (k + 1)-th row: same score, higher id
    assert (wrong[q, c.k - 1] >> np.uint64(32)) == (want[q, c.k - 1] >> np.uint64(32))
    with pytest.raises(AssertionError):
        lc._assert_keys(wrong, want, "tie order")


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("bpack,qpack", lc.SCORES_PACKS)
def test_scores_on_the_oracle(be, bpack, qpack, metric):
    lc.run_scores(be, bpack, qpack, metric)


@pytest.mark.parametrize("metric", [IP, L2])
def test_rank_all_on_the_oracle(be, metric):
    assert lc.RANK_SHAPE[1] > 2048  # K = N beyond LVS_MAX_K
    lc.run_rank_all(be, metric)


@pytest.mark.parametrize("nq,nb,d", lc.NEAREST_SHAPES)
def test_nearest_on_the_oracle(be, nq, nb, d):
    tied = lc.nearest_guards(nq, nb, d)
    for bpack, qpack in lc.NEAREST_PACKS:
        lc.run_nearest(be, nq, nb, d, bpack, qpack)
    print(f"\nnearest {nq} x {nb} x {d}: best two scores equal for {tied:.2f} of the queries", end="")
