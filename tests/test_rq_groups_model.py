"""CPU model of the launch arithmetic of the grouped ``lvs_rq_kernel`` (``lvs_rq_ranges_for``, ``lvs_rq_fits`` and
``lvs_grouped_geometry`` in lotus_amd/csrc/lvs_plan.h, as ``lvs_rq_launch`` uses them, and the kernel's blockIdx -> (corpus
range, query group) map), for the calls the literal ``sem_search`` loop and small joins make with 257 .. 4 096 queries
(lotus/sem_ops/sem_search.py:120-138, sem_sim_join.py:132-134).  The GPU parity rows of ``test_seeded_list_kernel`` run the
code itself; this pins the rules the comments state: one workgroup per (range, group), the siblings of a range on ONE XCD,
never more workgroups than CUs.

`test_the_models_are_the_compiled_rules` compares every model below with the compiled
code (tests/native/plan_check.cpp) on the parameters the tests use."""
import itertools

import pytest

import plan_native

GROUPQ, MAXQ, CUS, XCDS = 256, 4096, 256, 8


def max_ranges(groups):
    return 256 if groups <= 1 else 8 * (32 // groups)


def fits(nq, nb):
    groups = -(-nq // GROUPQ)
    if not (96 < nq <= MAXQ and nb >= 32768):
        return False
    if groups == 1:
        return True
    return groups * max_ranges(groups) >= 224 and nb >= 32768 * groups


def launch(nq, nb):
    """-> (groups, ranges, blocks_per_wg, grid) as lvs_rq_launch computes them."""
    nblocks = -(-nb // 32)
    groups = max(1, -(-nq // GROUPQ))
    ranges = min(max_ranges(groups), (nblocks + 3) // 4)
    ranges = max(ranges, 1)
    bpw = -(-nblocks // ranges)
    ranges = -(-nblocks // bpw)
    grid = ranges if groups == 1 else 8 * groups * -(-ranges // 8)
    return groups, ranges, bpw, grid


def block_map(b, groups, ranges):
    """The kernel's prologue: workgroup b -> (range, group) or None (grid padding)."""
    if groups == 1:
        return b, 0
    s = b >> 3
    rng = (s // groups) * 8 + (b & 7)
    return (rng, s % groups) if rng < ranges else None


def test_group_counts_taken_are_the_ones_that_fill_the_chip():
    taken = [g for g in range(1, 17) if fits(g * GROUPQ, 32768 * 16)]
    assert taken == [1, 2, 3, 4, 5, 6, 7, 8, 10, 14, 15, 16]  # 9 and 11 - 13 groups would idle 40 - 80 CUs
    for g in taken[1:]:
        assert 224 <= g * max_ranges(g) <= CUS and max_ranges(g) % 8 == 0
    assert not fits(96, 10 ** 6) and fits(97, 10 ** 6) and fits(4096, 10 ** 6) and not fits(4097, 10 ** 6)
    assert not fits(512, 60_000) and fits(512, 65_536)  # every group's workgroups need a few blocks each


@pytest.mark.parametrize("nq,nb", [(300, 70_001), (512, 66_000), (700, 100_000), (1300, 200_000), (2560, 1_000_000),
                                   (4000, 530_000), (4096, 1_000_000), (3500, 500_000), (3840, 600_001), (257, 32768 * 2), (200, 40_000), (128, 33_000)])
def test_every_range_and_group_has_exactly_one_workgroup_and_siblings_share_an_xcd(nq, nb):
    assert fits(nq, nb)
    groups, ranges, bpw, grid = launch(nq, nb)
    assert grid <= CUS and ranges * bpw * 32 >= nb and (ranges - 1) * bpw * 32 < nb  # no empty range, whole corpus covered
    seen = {}
    for b in range(grid):
        m = block_map(b, groups, ranges)
        if m is not None:
            assert m not in seen
            seen[m] = b
    assert set(seen) == set(itertools.product(range(ranges), range(groups)))
    per_xcd = [0] * XCDS
    for (rng, _grp), b in seen.items():
        per_xcd[b % XCDS] += 1
        assert b % XCDS == seen[(rng, 0)] % XCDS          # a range's siblings: one XCD (one L2)
    assert max(per_xcd) <= CUS // XCDS                    # and never more workgroups on an XCD than it has CUs
    if groups > 1:
        for rng in range(ranges):                         # consecutive dispatch slots of that XCD
            slots = sorted(seen[(rng, g)] >> 3 for g in range(groups))
            assert slots == list(range(slots[0], slots[0] + groups))
    # the last group may be ragged; its queries are the call's last ones
    assert (groups - 1) * GROUPQ < nq <= groups * GROUPQ


# ---- round 6: chunked calls (lvs_rq_item / lvs_rq_ranges_for / lvs_rq_grid and the chunk policy in lvs_plan.h) -----
def ranges_for(groups):
    return 256 if groups <= 1 else (8 * (32 // groups) if groups <= 32 else 256 // groups)


def item(b, groups, nparts):
    """lvs_rq_item: workgroup b -> (range, group) or None."""
    if groups <= 1:
        return b, 0
    if groups <= 32:
        s = b >> 3
        rng = (s // groups) * 8 + (b & 7)
        return (rng, s % groups) if rng < nparts else None
    it = (b & 7) * 32 + (b >> 3)
    rng, grp = divmod(it, groups)
    return (rng, grp) if rng < nparts else None


def chunks(nq, chunk=32768):
    """The chunk policy: `chunk` queries while that many are left, then 8 192s, one 4 096, the rest."""
    out, left = [], nq
    while left > 0:
        cn = chunk if left >= chunk else (8192 if left >= 8192 else (4096 if left > 4096 else left))
        out.append(cn)
        left -= cn
    return out


@pytest.mark.parametrize("groups", [32, 64, 128, 256])
def test_beyond_32_groups_an_xcd_runs_32_items_of_one_range(groups):
    ranges = ranges_for(groups)
    assert groups * ranges == CUS  # one workgroup per CU, every CU busy
    seen = {}
    for b in range(CUS if groups > 32 else 8 * groups * -(-ranges // 8)):
        m = item(b, groups, ranges)
        assert m is not None and m not in seen
        seen[m] = b
    assert set(seen) == set(itertools.product(range(ranges), range(groups)))
    for x in range(XCDS):
        mine = [m for m, b in seen.items() if b % XCDS == x]
        assert len(mine) == 32
        if groups >= 32:
            assert len({rng for rng, _ in mine}) == 1  # the XCD's 32 workgroups stream ONE range through its L2
    # the earlier rule is unchanged up to 32 groups
    for g in range(2, 33):
        for b in range(8 * g * -(-ranges_for(g) // 8)):
            assert item(b, g, ranges_for(g)) == block_map(b, g, ranges_for(g))


@pytest.mark.parametrize("nq", [4097, 5000, 9000, 10_000, 20_000, 33_000, 40_000, 65_536, 100_000, 1_000_000])
def test_chunk_policy_covers_the_queries_with_launchable_group_counts(nq):
    cs = chunks(nq)
    assert sum(cs) == nq and all(c > 0 for c in cs)
    for c in cs[:-1]:
        assert c in (32768, 8192, 4096)
    for c in cs:
        groups = -(-c // GROUPQ)
        assert groups <= 32 or groups % 32 == 0  # what lvs_rq_launch / lvs_rj_launch accept
    assert cs == sorted(cs, reverse=True)
    assert chunks(100_000) == [32768, 32768, 32768, 1696]


LAUNCHES = [(300, 70_001), (512, 66_000), (700, 100_000), (1300, 200_000), (2560, 1_000_000), (4000, 530_000), (4096, 1_000_000),
            (3500, 500_000), (3840, 600_001), (257, 32768 * 2), (200, 40_000), (128, 33_000)]


def test_the_models_are_the_compiled_rules():
    ask = plan_native.ask
    shapes = [(g * GROUPQ, 32768 * 16) for g in range(1, 17)] + LAUNCHES
    shapes += [(96, 10 ** 6), (97, 10 ** 6), (4096, 10 ** 6), (4097, 10 ** 6), (512, 60_000), (512, 65_536)]
    assert ask([f"rq_fits {nq} {nb} 768 10" for nq, nb in shapes]) == [[int(fits(nq, nb))] for nq, nb in shapes]
    # lvs_rq_launch: the corpus in rounded-up 32-row blocks
    assert ask([f"grouped {nq} {-(-nb // 32)}" for nq, nb in LAUNCHES]) == [list(launch(nq, nb)) for nq, nb in LAUNCHES]
    groups = list(range(1, 33)) + [64, 128, 256]
    assert ask([f"ranges_for {g}" for g in groups]) == [[ranges_for(g)] for g in groups]
    assert all(ranges_for(g) == max_ranges(g) for g in range(1, 33))
    for g in (1, 2, 7, 16, 32, 64, 128, 256):
        grid = ranges_for(g) if g == 1 else (CUS if g > 32 else 8 * g * -(-ranges_for(g) // 8))
        got = ask([f"item {b} {g} {ranges_for(g)}" for b in range(grid)])
        assert got == [None if item(b, g, ranges_for(g)) is None else list(item(b, g, ranges_for(g))) for b in range(grid)]
    # chunks() at its default records the threshold join's cut (range_chunk_len)
    nqs = [1, 4096, 4097, 5000, 9000, 10_000, 20_000, 33_000, 40_000, 65_536, 100_000, 1_000_000]
    assert ask([f"range_chunks {nq}" for nq in nqs]) == [chunks(nq) for nq in nqs]


@pytest.mark.parametrize("n", [2047, 2048, 4296, 40_000, 70_001])
def test_self_join_launches_offer_every_pair_above_the_diagonal_once(n):
    """The threshold join's plan (``lvs_range_rj_ok``, ``range_chunk_len``, ``lvs_range_chunk_plan`` through the ``range_plan``
    question) for a self-join of n fp16 rows under the inner product: query i is row i and the join reports every pair
    (i, j > i).  A launch is a rectangle of queries x rows in which the kernel keeps j > i; the rectangles are disjoint, and
    for every query the rows above it that the rectangles hold are all n - 1 - i of them - so each pair is offered exactly
    once.  ``lvs_rj_kernel`` gets whole 32-row blocks, at least 32 768 rows and a group count it deals; the last n % 32 rows go
    to the list kernel, once per chunk that still has rows."""
    import numpy as np

    flat = plan_native.ask([f"range_plan {n} {n} 0 0 768 0 0 1"])[0]
    launches = [tuple(flat[i:i + 5]) for i in range(0, len(flat), 5)]  # kernel (1: lvs_rj_kernel, 0: list kernel), c0, cn, r0, rn
    if n < 2048:
        assert launches == [(0, 0, n, 0, n)]
    else:
        cuts = np.cumsum([0] + chunks(n))
        assert sorted({(c0, cn) for _, c0, cn, _, _ in launches} | {(int(cuts[-2]), int(cuts[-1] - cuts[-2]))}) == \
            [(int(a), int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])]  # (the last chunk may have no row left above it)
    offered = np.zeros(n, np.int64)
    for a, (kernel, c0, cn, r0, rn) in enumerate(launches):
        assert cn > 0 and rn > 0 and 0 <= r0 and r0 + rn <= n and c0 + cn <= n
        for _, c0b, cnb, r0b, rnb in launches[a + 1:]:
            assert c0 + cn <= c0b or c0b + cnb <= c0 or r0 + rn <= r0b or r0b + rnb <= r0, "rectangles overlap"
        i = np.arange(c0, c0 + cn)
        offered[c0:c0 + cn] += np.maximum(0, r0 + rn - np.maximum(r0, i + 1))
        if kernel == 1:
            groups = -(-cn // GROUPQ)
            assert r0 % 32 == 0 and rn % 32 == 0 and rn >= 32768 and cn > 128 and (groups <= 32 or groups % 32 == 0)
            assert r0 + rn == n // 32 * 32
            tails = [l for l in launches if l[0] == 0 and l[1:3] == (c0, cn)]
            assert tails == ([(0, c0, cn, n // 32 * 32, n % 32)] if n % 32 else [])
        else:
            assert r0 + rn == n  # the list kernel takes a chunk's rows to the end, ragged block included
    assert np.array_equal(offered, n - 1 - np.arange(n))
