"""GPU parity of `lvs_rj_kernel`'s staging cursor at the shortest corpus ranges it can meet.

The cursor (the unit whose 1 KiB staging loads go out next) runs RING - 1 units ahead of the unit being computed.  Its k-half is
a compile-time constant of every call site, and the source advance is a select between a byte step and 0 that stops at the
range's last unit: past it the last unit is loaded again into a free slot.  What can go wrong is therefore decided by the
range's length in units (blocks x U) against RING - 1, and by which k-half the clamp falls on:

    d     NJ   U   RING (k <= 10 / k = 16)   prologue runs into the clamp for ranges of ...
    256   16   1   6 / 6                     1 .. 4 blocks
    384   24   1   4 / 4                     1 .. 2 blocks
    512   32   2   7 / 6                     1 .. 2 blocks
    768   48   2   5 / 4                     1 block

Geometry comes from the compiled planner (`lvs_grouped_geometry` through tests/plan_native.py) and is asserted per case, so a
planner change cannot silently move a case to longer ranges:

  * 200 queries (one group, up to 256 corpus ranges) x 1 024 blocks: EVERY range is 4 blocks long;
  * 200 queries x 1 026 / 1 027 / 1 028 blocks: 205 ranges of 5 blocks and a last one of 1 / 2 / 3;
  * 300 queries (two sibling groups) x 2 058 / 2 059 / 2 060 blocks: 121 ranges of 17 blocks and a last one of 1 / 2 / 3;
  * 12 288 queries x 1 030 blocks, one call that goes out as chunks of 8 192 and 4 096 queries (a single call of 4 096 needs
    524 288 rows for this kernel): the 4 096-query launch has 16 groups x 16 ranges, 15 of 65 blocks and one of 55 - the shared
    form with every CU's workgroup on another group;
  * 65 536 queries x 32 768 + 64 rows: ONE range of 1 026 blocks - the form without threshold sharing;
  * a threshold self-join of 33 000 rows: one RANGE launch of 32 768 query rows over 1 031 blocks in two ranges (516 + 515);
  * a threshold join of 4 296 query rows whose last 200 go out as one group over 206 / 256 ranges: the RANGE form at a last
    range of 1 or 2 blocks and at ranges of 4.

Every top-k case but the 65 536-query one (one (k, metric) per width) is run for d = 256 / 384 / 512 / 768, k = 10 / 16 (the
two list depths = ring depths) and both metrics, and checked twice: the keys are equal BIT FOR BIT to those of the same search
made with an id table (`row_ids` = the positions: such a call never runs lvs_rj_kernel, and a key is (score, id)), and a sample of queries - the planted ones among them - passes
`check_topk_exact` against the float64 scores of the stored values.  Queries planted ON rows sit where a cursor fault shows: the
first and last row of the last range, the last row of the range before it, row 0."""
import numpy as np
import pytest
import torch

import plan_native
import synth
from lotus_amd import _capi
from width_cases import check_topk_exact, scores_from_products

pytestmark = pytest.mark.gpu
F16 = _capi.PACK_F16
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
NB_MAX = 2060 * 32
WIDTHS = [256, 384, 512, 768]
FORMS = [(10, IP), (16, L2), (16, IP), (10, L2)]

_CORPUS = {}


def _corpus(be, d):
    """(fp16 rows, device image) of the longest corpus of this file at width d; the cases search its first rows."""
    if d not in _CORPUS:
        _CORPUS.clear()  # one resident corpus at a time
        xb = synth.corpus(NB_MAX, d, seed=300 + d).astype(np.float16)
        _CORPUS[d] = (xb, be.pack(xb, F16))
    return _CORPUS[d]


def _geometry(nq, nblocks):
    """(groups, ranges, blocks per range, blocks of the last range) of a launch, from the compiled planner."""
    groups, nparts, bpw, _grid = plan_native.ask([f"grouped {nq} {nblocks}"])[0]
    return groups, nparts, bpw, nblocks - (nparts - 1) * bpw


def _search(be, cb, cq, k, metric, **kw):
    be.timing_enable(True)
    keys = be.search_keys(cb, cq, k, metric, **kw)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    return keys, t


def _topk_case(be, nq, nblocks, d, geometry, forms=FORMS, tail=0, sample=48, launch_nq=None):
    """launch_nq: the queries of the launch whose geometry is asserted (a chunk of the call); default: the call is one launch."""
    assert _geometry(launch_nq or nq, nblocks) == geometry, _geometry(launch_nq or nq, nblocks)
    groups, nparts, bpw, last = geometry
    nb = nblocks * 32 + tail
    xb_all, cb_all = _corpus(be, d)
    xb, cb = xb_all[:nb], be.slice_rows(cb_all, 0, nb)
    xq, _ = synth.queries(xb.astype(np.float32), nq, seed=nblocks + d)
    xq = xq.astype(np.float16)
    r_last0 = (nparts - 1) * bpw * 32  # first row of the last range
    plants = {0: 0, 1: nblocks * 32 - 1, 2: r_last0, 3: max(r_last0 - 1, 0), nq - 1: nblocks * 32 - 32, nq // 2 + 1: r_last0 + 31}
    for q, row in plants.items():
        xq[q] = xb[row]
    cq = be.pack(xq, F16)
    ids = be.to_device((np.arange(nb, dtype=np.uint32) + np.uint32(11)).view(np.int32))
    rng = np.random.default_rng(nblocks * 7 + d)
    rows = np.unique(np.concatenate([list(plants), rng.integers(0, nq, sample)]))
    dev = be.to_device(rows.astype(np.int64))
    xb64, xq64 = xb.astype(np.float64), xq[rows].astype(np.float64)
    qb, qn, bn = xq64 @ xb64.T, (xq64 * xq64).sum(1), (xb64 * xb64).sum(1)  # float64, of the stored fp16 values
    del xb64
    for k, metric in forms:
        keys, t = _search(be, cb, cq, k, metric, id_offset=11)
        assert t["kernel"] == "lvs_rj_kernel", t
        ref, tr = _search(be, cb, cq, k, metric, row_ids=ids)
        assert tr["kernel"] != "lvs_rj_kernel", tr
        diff = int((keys != ref).any(dim=1).sum())
        print(f"nq {nq} blocks {nblocks} d {d} k {k} metric {metric}: {t['kernel']} vs {tr['kernel']}, {diff} queries differ")
        assert torch.equal(keys, ref), f"{diff} queries differ from the id-table search (k {k}, metric {metric})"
        D, I = be.keys_to_result(keys[dev], metric)
        Dg, Ig = D.cpu().numpy().astype(np.float64), I.cpu().numpy() - 11
        err = check_topk_exact(scores_from_products(qb, qn, bn, metric), Dg if metric == IP else -Dg, Ig, k)
        print(f"    check_topk_exact on {rows.size} queries: largest score error {err:.2e}")
        at = {int(r): i for i, r in enumerate(rows)}
        for q, row in plants.items():
            assert Ig[at[q], 0] == row, (q, row, Ig[at[q], :3], Dg[at[q], :3])


@pytest.mark.parametrize("d", WIDTHS)
def test_every_range_four_blocks_long(hip_backend, d):
    """200 queries x 32 768 rows: 256 ranges of 4 blocks - at d = 256 the prologue alone issues more units than a range has."""
    _topk_case(hip_backend, 200, 1024, d, (1, 256, 4, 4))


@pytest.mark.parametrize("last", [1, 2, 3])
@pytest.mark.parametrize("d", WIDTHS)
def test_one_group_last_range_of_one_two_three_blocks(hip_backend, d, last):
    """200 queries: 205 ranges of 5 blocks next to a last one of 1, 2 or 3; the last case with 7 tail rows behind it."""
    _topk_case(hip_backend, 200, 1025 + last, d, (1, 206, 5, last), tail=7 if last == 3 else 0)


@pytest.mark.parametrize("last", [1, 2, 3])
@pytest.mark.parametrize("d", WIDTHS)
def test_sibling_groups_last_range_of_one_two_three_blocks(hip_backend, d, last):
    """300 queries (two groups, the second ragged): 121 ranges of 17 blocks next to a last one of 1, 2 or 3."""
    _topk_case(hip_backend, 300, 2057 + last, d, (2, 122, 17, last))


@pytest.mark.parametrize("d", WIDTHS)
def test_shared_form_at_4096_queries(hip_backend, d):
    """The 4 096-query launch (16 groups x 16 ranges: 15 ranges of 65 blocks and one of 55) as the last chunk of a 12 288-query call."""
    assert plan_native.ask(["chunks 12288 65536", "chunks 12288 32768"]) == [[8192, 4096], [8192, 4096]]
    _topk_case(hip_backend, 12288, 1030, d, (16, 16, 65, 55), launch_nq=4096)


@pytest.mark.parametrize("d,k,metric", [(256, 10, IP), (768, 10, L2), (512, 16, L2), (384, 16, IP)])
def test_single_range_form_65536_queries(hip_backend, d, k, metric):
    """65 536 queries x 32 768 + 64 rows: one range of 1 026 blocks, no threshold sharing.  d = 256, k = 10, inner product; then
    the form's other paths: U = 2 (d = 768, 512), and under squared L2 its one side-word DMA per block (the rows' |y|^2)."""
    _topk_case(hip_backend, 65536, 1026, d, (256, 1, 1026, 1026), forms=[(k, metric)], sample=64)


@pytest.mark.parametrize("d,nblocks,geometry", [(768, 1026, (1, 206, 5, 1)), (256, 1024, (1, 256, 4, 4)), (512, 1027, (1, 206, 5, 2))])
def test_range_join_over_ranges_shorter_than_the_ring(hip_backend, d, nblocks, geometry):
    """The RANGE instantiations where the prologue runs into the clamp: a threshold join of 4 296 query rows against nblocks x 32
    corpus rows goes out as chunks of 4 096 and 200 query rows, and the 200-row launch is one group over up to 256 ranges - a
    last range of 1 block (d = 768) or 2 (d = 512), or every range 4 blocks long (d = 256).  Queries at cosine 0.97 of corpus
    rows in the last range's first and last row, the last row of the range before it, row 0 and a middle range's last block, in
    both chunks; near misses (0.93) beside them.  The exact pair set."""
    be = hip_backend
    nq, nb, tau = 4296, nblocks * 32, 0.95
    assert plan_native.ask(["range_chunks 4296"]) == [[4096, 200]]
    assert _geometry(200, nblocks) == geometry, _geometry(200, nblocks)
    _groups, nparts, bpw, _last = geometry
    xb_all, cb_all = _corpus(be, d)
    xb, cb = xb_all[:nb].astype(np.float32), be.slice_rows(cb_all, 0, nb)
    xq = synth.corpus(nq, d, seed=500 + d)
    r_last0 = (nparts - 1) * bpw * 32  # first row of the 200-row launch's last range
    rows = [r_last0, nb - 1, r_last0 - 1, 0, (nparts // 2) * bpw * 32 - 1, nb - 32]
    hit = {4096 + 7 * i: r for i, r in enumerate(rows)}           # in the 200-row chunk (every wave: queries 0 .. 35 of it)
    hit.update({4096 + 190 + i: r for i, r in enumerate(rows)})   # ... and its last wave's second query block
    hit.update({600 * i + 5: r for i, r in enumerate(rows)})      # in the 4 096-row chunk
    miss = {4096 + 100: nb - 1, 4096 + 101: r_last0, 77: nb - 1}
    noise = synth.corpus(len(hit) + len(miss), d, seed=501 + d)
    for (qi, r), u in zip(sorted({**hit, **miss}.items()), noise):
        c = 0.97 if qi in hit else 0.93
        u = u - (u @ xb[r]) * xb[r]
        xq[qi] = c * xb[r] / np.linalg.norm(xb[r]) + np.sqrt(1.0 - c * c) * u / np.linalg.norm(u)
    xq16 = xq.astype(np.float16)
    be.timing_enable(True)
    q, j, sc = be.range_join(cb, be.pack(xq16, F16), tau, IP)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    print(t)
    assert (t["launches"], t["calls"], t["kernel"]) == (2, 1, "lvs_rj_kernel"), t  # whole blocks: both chunks, nothing else
    got = set(zip(q.cpu().numpy().tolist(), j.cpu().numpy().tolist()))
    assert len(got) == int(q.numel())  # no pair twice
    touched = sorted({**hit, **miss})
    s = xq16[touched].astype(np.float32) @ xb.T
    want = {(qi, int(b)) for qi, row in zip(touched, s) for b in np.nonzero(row > tau)[0]}
    assert np.abs(s[(s > 0.9) & (s < 0.999)] - tau).min() > 5e-3  # nothing near the threshold: the comparison is exact
    assert want == set(hit.items()), (sorted(want - set(hit.items()))[:5], sorted(set(hit.items()) - want)[:5])
    assert got == want, (sorted(want - got)[:5], sorted(got - want)[:5])
    qi, ji = q.cpu().numpy(), j.cpu().numpy()
    assert np.allclose(sc.cpu().numpy(), np.einsum("ij,ij->i", xq16[qi].astype(np.float32), xb[ji]), atol=1e-5)


def test_range_self_join_pair_in_the_last_block_of_the_shorter_last_range(hip_backend):
    """Threshold self-join of 33 000 rows, d = 512 (U = 2): the first 32 768 query rows go out as ONE RANGE launch over the 1 031
    whole blocks in two ranges of 516 and 515 blocks; the last 8 rows and the last 232 query rows go through the list kernel.
    Pairs (cosine 0.97) are planted with their later row in the last block of the shorter last range, in the last block of
    the first range and in both ranges' first blocks; near misses (0.93) beside them.  The exact pair set."""
    be = hip_backend
    n, d, tau = 33_000, 512, 0.95
    assert _geometry(32768, n // 32) == (128, 2, 516, 515)
    x = synth.corpus(n, d, seed=17)
    later = [1030 * 32, 1030 * 32 + 31, 515 * 32 + 5, 516 * 32, 516 * 32 + 31, 40, 32999, 1029 * 32 + 9]
    later_near = [1030 * 32 + 7, 515 * 32 + 30, 516 * 32 + 1]
    rng = np.random.default_rng(18)
    pairs, near, used = set(), set(), set(later) | set(later_near)
    for j in later + later_near:
        i = int(rng.integers(0, j))
        while i in used:
            i = int(rng.integers(0, j))
        used.add(i)
        (pairs if j in later else near).add((i, j))
    noise = synth.corpus(len(pairs | near), d, seed=19)
    for (i, j), u in zip(sorted(pairs | near), noise):
        c = 0.97 if (i, j) in pairs else 0.93
        u = u - (u @ x[i]) * x[i]
        x[j] = c * x[i] + np.sqrt(1.0 - c * c) * u / np.linalg.norm(u)
    x16 = x.astype(np.float16)
    p = be.pack(x16, F16)
    be.timing_enable(True)
    q, j, sc = be.range_join(p, p, tau, IP, q_row0=0)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    print(t)
    # one call: the RANGE launch of lvs_rj_kernel, the list kernel for the corpus' last 8 rows and for the last 232 query rows
    assert (t["launches"], t["calls"], t["kernel"]) == (3, 1, "lvs_tile_kernel"), t
    got = set(zip(q.cpu().numpy().tolist(), j.cpu().numpy().tolist()))
    assert len(got) == int(q.numel())  # no pair twice
    xf = x16.astype(np.float32)
    touched = sorted({r for pr in pairs | near for r in pr})
    s = xf[touched] @ xf.T
    want = set()
    for a, row in zip(touched, s):
        for b in np.nonzero(row > tau)[0].tolist():
            if a != b:
                want.add((min(a, b), max(a, b)))
    assert np.abs(s[(s > 0.9) & (s < 0.999)] - tau).min() > 5e-3  # nothing near the threshold: the comparison is exact
    assert want == pairs, (sorted(want - pairs)[:5], sorted(pairs - want)[:5])
    assert got == want, (sorted(want - got)[:5], sorted(got - want)[:5])
    qi, ji = q.cpu().numpy(), j.cpu().numpy()
    assert np.allclose(sc.cpu().numpy(), np.einsum("ij,ij->i", xf[qi], xf[ji]), atol=1e-5)
