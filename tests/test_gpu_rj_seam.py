"""GPU parity of `lvs_rj_kernel` at the seam between two 32-row corpus blocks: the block's filter ("does any lane of either query
block hold a candidate?", then per query block), the visit behind it, the drains, and the head of the next block's first unit
(barrier + first fragment read) that follows them.  Same oracle and bars as `test_gpu_rj.py` - scores within 1e-5,
no id mismatch outside 2e-5 near-ties - but on the smallest launch the kernel takes with more than one group: 300 queries (two
groups, the second ragged: its waves hold one query block or none) x 65 600 rows = 2 050 whole blocks in 121 ranges of 17, so
EVERY query of the call is checked, and planted rows sit exactly where a seam can go wrong:

  * a wave's two query blocks are blocks w and w + 4 of its group: wave 0 holds queries 0 .. 31 and 128 .. 159.  Queries 3, 35 and
    131 are copies of rows 0 and 31 (the first block of the first range; 3 and 131: both query blocks of ONE wave at once), 4 / 36 /
    132 the same on the first block of the launch's second range, 5 / 37 / 133 on its last block;
  * queries 170 (second query block of wave 1) and 40 (its first) alone on rows in the last blocks of two other ranges: the branch
    that decides per query block.  Whether the other query block holds a candidate in that very block depends on the thresholds
    of the moment in a k-NN run; the threshold join below has ONE constant threshold and random rows 14 sigma below it, so there
    a planted pair's block holds a candidate in exactly one query block;
  * 400 equal rows from a row with row % 32 == 31 on: the candidate buffer overflows (the drain inside the visit) in a burst
    that straddles seams; the duplicate's top k comes back in ascending id order, as the oracle's.

A planted query is an exact copy of a unit row rounded to fp16: every component is off by at most 2^-11 relative, so its score
with itself is within 2^-10 of 1 (squared L2: exactly 0) - the bar for "rank 1 with score 1"; the 1e-5 oracle bar holds besides."""
import numpy as np
import pytest

import oracle
import synth
from lotus_amd import _capi
from oracle.dedup import range_self_join

pytestmark = pytest.mark.gpu
F16 = _capi.PACK_F16
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
NQ, NB = 300, 65_600
EQ0, EQN = 32 * 1000 + 31, 400  # the block of equal rows: starts on the last row of a 32-row block

_CACHE = {}


def _range_rows(nb, nq):
    """Rows per corpus range of one launch: lvs_rq_ranges_for's rule and lvs_grouped_geometry's rounding (lvs_plan.h)."""
    groups = max(1, -(-nq // 256))
    ranges = 256 if groups <= 1 else (8 * (32 // groups) if groups <= 32 else 256 // groups)
    nblocks = nb // 32
    ranges = max(1, min(ranges, (nblocks + 3) // 4))
    return -(-nblocks // ranges) * 32


def _plants():
    r = _range_rows(NB, NQ)  # first row of the second range; its last row is 2 r - 1
    assert r == 17 * 32 and NB % 32 == 0 and EQ0 % 32 == 31
    return {3: 0, 35: 31, 131: 31,                      # first block of range 0
            4: r, 36: r + 31, 132: r + 31,              # first block of range 1
            5: 2 * r - 1, 37: 2 * r - 32, 133: 2 * r - 32,  # last block of range 1
            170: 9 * r - 5,                             # only the second query block of wave 1 ... (last block of range 8)
            40: 30 * r - 20,                            # ... and only its first (last block of range 29)
            299: NB - 1}                                # the ragged group's last query on the corpus' last whole-block row


def _data(be, d):
    """One corpus of NB + 13 rows per width (the first NB are the whole-block corpus), its queries and device images - built once."""
    if d not in _CACHE:
        xb = synth.corpus(NB + 13, d, seed=61).astype(np.float16)
        xb[EQ0:EQ0 + EQN] = xb[EQ0]
        xb32 = xb.astype(np.float32)
        xq, _ = synth.queries(xb32, NQ, seed=62)
        xq = xq.astype(np.float16)
        for q, row in _plants().items():
            xq[q] = xb[row]
        xq[7] = xb[EQ0]
        _CACHE[d] = {"xb": xb32, "xq": xq.astype(np.float32), "cq": be.pack(xq, F16),
                     NB: be.pack(xb[:NB], F16), NB + 13: be.pack(xb, F16), "ref": {}}
    return _CACHE[d]


def _reference(c, nb, k, metric):
    key = (nb, k, metric)
    if key not in c["ref"]:
        c["ref"][key] = oracle.flat_search(c["xb"][:nb], c["xq"], k, metric)
    return c["ref"][key]


@pytest.mark.parametrize("nb", [NB, NB + 13])  # whole blocks only / + a 13-row tail (one more list per query from lvs_rq_kernel)
@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [256, 768])
def test_every_query_of_a_two_group_launch_with_rows_planted_on_the_seams(hip_backend, d, metric, k, nb):
    be = hip_backend
    c = _data(be, d)
    be.timing_enable(True)
    keys = be.search_keys(c[nb], c["cq"], k, metric, id_offset=11)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    assert t["kernel"] == "lvs_rj_kernel", t  # (also with a tail: its lvs_rq_kernel launch for the last nb % 32 rows is not timed)
    D, I = be.keys_to_result(keys, metric)
    Dg, Ig = D.cpu().numpy(), I.cpu().numpy() - 11
    Dr, Ir = _reference(c, nb, k, metric)
    err, hard, recall = synth.compare_topk(Dr, Ir, Dg, Ig, atol=1e-5)
    print(f"d={d} metric={metric} k={k} nb={nb}: score error {err:.2e}, hard id mismatches {hard}, recall {recall:.6f}")
    assert err <= 1e-5, f"score error {err}"
    assert hard == 0, f"{hard} id mismatches outside near-ties"
    assert recall >= 0.9999, recall
    for q, row in _plants().items():
        assert Ig[q, 0] == row, (q, row, Ig[q, :3])
        want = 1.0 if metric == IP else 0.0
        assert abs(float(Dg[q, 0]) - want) <= 2.0 ** -10, (q, Dg[q, 0])
    # the queried duplicate: k of the 400 equal rows, in ascending id order as the oracle's
    assert np.array_equal(Ig[7], np.arange(EQ0, EQ0 + k)), Ig[7]
    assert np.array_equal(Ig[7], Ir[7])


def test_threshold_join_with_pairs_planted_in_first_and_last_blocks_of_ranges(hip_backend):
    """`lvs_range_join` (the RANGE epilogue of the same kernel frame) as a self-join of 65 600 unit rows, d = 256: 50 pairs at
    cosine 0.95 against a threshold of 0.9, random rows at cosine 0 +- 1/16.  The 65 536 query rows go through in two launches of
    128 groups x 2 ranges - rows [0, 65 600) and [32 768, 65 600) - and every pair's later row lies in the first or last block of
    one of those ranges; the earlier rows fall into both query blocks of their waves.  The pair set is the CPU oracle's."""
    be = hip_backend
    n, d, npairs = NB, 256, 50
    x = synth.corpus(n, d, seed=71)
    r0 = _range_rows(n, 32768)            # launch 1: ranges [0, r0) and [r0, n)
    r1 = 32768 + _range_rows(n - 32768, 32768)  # launch 2: [32 768, r1) and [r1, n)
    assert (r0, r1) == (1025 * 32, 32768 + 513 * 32)
    rng = np.random.default_rng(72)
    # (first block, last block) of each range, as the later row j of a pair; the earlier row i is drawn below j, inside the
    # launch that meets j: launch 1 for j < 32 768 + ..., launch 2 only for i >= 32 768
    blocks1 = [0, r0 - 32, r0, n - 32]
    blocks2 = [32768, r1 - 32, r1, n - 32]
    pairs = set()
    used = set()
    while len(pairs) < npairs:
        two = len(pairs) % 2 == 1
        b = int(rng.choice(blocks2 if two else blocks1))
        j = b + int(rng.integers(0, 32))
        lo = 32768 if two else 0
        if j <= lo + 1:
            j = lo + 31
        i = int(rng.integers(lo, min(j, lo + 32768)))
        if i in used or j in used or i == j:
            continue
        used.update((i, j))
        pairs.add((i, j))
    noise = synth.corpus(npairs, d, seed=73)
    for (i, j), u in zip(sorted(pairs), noise):
        u = u - (u @ x[i]) * x[i]
        x[j] = 0.95 * x[i] + np.sqrt(1.0 - 0.95 ** 2) * u / np.linalg.norm(u)
    assert {i % 256 < 128 for i, _ in pairs} == {True, False}  # both query blocks of a wave
    x16 = x.astype(np.float16)
    p = be.pack(x16, F16)
    be.timing_enable(True)
    q, j, sc = be.range_join(p, be.slice_rows(p, 0, 65536), 0.9, IP, q_row0=0)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    assert t["kernel"] == "lvs_rj_kernel" and t["launches"] >= 2, t
    got = set(zip(q.cpu().numpy().tolist(), j.cpu().numpy().tolist()))
    assert len(got) == int(q.numel())  # no pair twice
    oi, oj, osc = range_self_join(x16.astype(np.float32), 0.9)
    want = {(a, b) for a, b in zip(oi.tolist(), oj.tolist()) if a < b}
    print(f"threshold join: {len(got)} pairs, oracle {len(want)}, planted {len(pairs)}")
    assert want == pairs  # (nothing but the planted pairs is near the threshold: the comparison below is exact)
    assert got == want, (sorted(want - got)[:5], sorted(got - want)[:5])
    ref = {(a, b): s for a, b, s in zip(oi.tolist(), oj.tolist(), osc.tolist())}
    dev = np.array([ref[pr] for pr in zip(q.cpu().numpy().tolist(), j.cpu().numpy().tolist())], np.float32)
    assert np.abs(sc.cpu().numpy() - dev).max() <= 1e-5
