"""CPU model of the greedy chunk plan of a chunked ``lvs_rq_kernel`` / ``lvs_rj_kernel`` call (``rq_chunk_size`` /
``rq_chunk_len`` in lotus_amd/csrc/lvs_plan.h): every chunk is the largest of 65 536, 32 768, 16 384, 8 192 that is <= the
queries left and <= the configured maximum, then one of 4 096 while more than 4 096 are left, then the rest.

``chunks()`` in ``test_rq_groups_model.py`` describes the rule BEFORE this one (the maximum while that many are left, then
8 192s, one 4 096, the rest) and stays there as a record; the threshold join (``lvs_range_join``) still cuts its rows that
way.

The model keeps its assertions; `test_the_model_is_the_compiled_rule` compares it with the compiled ``rq_chunk_size`` /
``rq_chunk_len`` (lotus_amd/csrc/lvs_plan.h through tests/native/plan_check.cpp) on every parameter used here."""
import pytest

import plan_native

GROUPQ, MAXQ, CHUNK_MAX = 256, 4096, 65536


def chunk_size(want):
    """rq_chunk_size: the largest launchable chunk (4 096 x 2^i, up to 65 536) that is <= `want`."""
    c = MAXQ
    while 2 * c <= want and 2 * c <= CHUNK_MAX:
        c *= 2
    return c


def plan(nq, maximum):
    """The chunks of a call of nq queries, as search_rq_chunks cuts them."""
    out, left, top = [], nq, chunk_size(maximum)
    while left > 0:
        cn, c = None, top
        while c >= 8192 and cn is None:
            if left >= c:
                cn = c
            c //= 2
        if cn is None:
            cn = MAXQ if left > MAXQ else left
        out.append(cn)
        left -= cn
    return out


@pytest.mark.parametrize("maximum", [32768, 65536])
@pytest.mark.parametrize("nq", [4097, 9000, 20_000, 33_000, 40_000, 50_000, 65_536, 100_000, 1_000_000])
def test_plan_covers_the_queries_with_launchable_chunks_in_descending_order(nq, maximum):
    cs = plan(nq, maximum)
    assert sum(cs) == nq and all(0 < c <= maximum for c in cs)
    for c in cs:
        groups = -(-c // GROUPQ)
        assert groups <= 32 or (groups % 32 == 0 and 256 % groups == 0)  # what lvs_rq_launch / lvs_rj_launch accept
    assert cs == sorted(cs, reverse=True)
    for c in cs[:-1]:
        assert c in (65536, 32768, 16384, 8192, 4096)
    assert cs[:-1].count(4096) <= 1  # one 4 096 at the most, and only the rest behind it
    if 4096 in cs[:-1]:
        assert cs[:-1].index(4096) == len(cs) - 2


def test_the_literal_plans():
    assert plan(100_000, 65536) == [65536, 32768, 1696]
    assert plan(50_000, 65536) == [32768, 16384, 848]
    assert plan(50_000, 32768) == [32768, 16384, 848]
    assert plan(100_000, 32768) == [32768, 32768, 32768, 1696]  # the headline at the earlier maximum: as before
    assert plan(40_000, 32768) == [32768, 4096, 3136]           # ... and calls a little above one chunk
    assert plan(33_000, 32768) == [32768, 232]
    assert plan(65_536, 65536) == [65536] and plan(65_536, 32768) == [32768, 32768]
    assert plan(4097, 65536) == [4096, 1] and plan(9000, 65536) == [8192, 808]
    assert plan(20_000, 32768) == [16384, 3616]  # (8 192 + 8 192 + 3 616 under the earlier rule)
    assert plan(1_000_000, 65536) == [65536] * 15 + [16384, 576]
    assert plan(25_000, 65536) == [16384, 8192, 424]
    # a maximum that is not a launchable size is rounded down to one
    assert plan(100_000, 40_000) == plan(100_000, 32768)


def test_the_model_is_the_compiled_rule():
    wants = [4096, 8191, 8192, 32768, 40_000, 65535, 65536, 100_000, 1 << 20]
    assert plan_native.ask([f"chunk_size {w}" for w in wants]) == [[chunk_size(w)] for w in wants]
    cases = [(nq, m) for m in (32768, 65536) for nq in (4097, 9000, 20_000, 33_000, 40_000, 50_000, 65_536, 100_000, 1_000_000)]
    cases += [(25_000, 65536), (100_000, 40_000), (1, 65536), (4096, 65536), (8192, 4096)]
    assert plan_native.ask([f"chunks {nq} {m}" for nq, m in cases]) == [plan(nq, m) for nq, m in cases]
