"""The guarded allocator of the extent tests (tests/ws_guard.py) on CPU tensors: the detector detects, and reports where."""
import pytest
import torch

import ws_guard
from ws_guard import ALIGN, GUARD, GUARD_BYTE, GuardedPool, guarded

NBYTES = 1000  # not a multiple of 256: 24 bytes of slack up to 1024


def _poke(pool, view, offset, ordinal=-1):
    """One byte written at ``offset`` relative to the payload start of ``view``, through the pool's own allocation."""
    whole, lead, _ = pool._bufs[ordinal]
    assert whole.data_ptr() + lead == view.data_ptr()
    whole[lead + offset] = (GUARD_BYTE ^ 0xFF)


@pytest.mark.parametrize("offset,side", [
    (-1, "before"),
    (-GUARD, "before"),                                 # a whole guard before the payload
    (NBYTES, "slack"),
    (1023, "slack"),
    (1024, "after"),                                    # the rounded end
    (1024 + GUARD - 1, "after"),                        # the last byte of a whole guard behind it
])
def test_one_byte_is_reported_with_side_and_offset(offset, side):
    pool = GuardedPool("cpu")
    pool.alloc(64, 0)  # an undamaged neighbour: the ordinal counts buffers, not damage
    v = pool.alloc(NBYTES, 0x00)
    assert pool.violations() == []
    _poke(pool, v, offset)
    got = pool.violations()
    assert len(got) == 1
    assert (got[0].ordinal, got[0].nbytes, got[0].side, got[0].first, got[0].last, got[0].count) == \
        (1, NBYTES, side, offset, offset, 1)
    with pytest.raises(AssertionError, match=f"buffer #1 .{NBYTES} bytes.*{side} the payload, offsets {offset} .. {offset}"):
        pool.assert_clean()


def test_the_allocations_first_and_last_bytes_are_guard_bytes():
    pool = GuardedPool("cpu")
    v = pool.alloc(NBYTES, 0x00)
    whole, lead, _ = pool._bufs[0]
    first, last = -lead, int(whole.numel()) - lead - 1
    assert first <= -GUARD and last >= 1024 + GUARD - 1
    _poke(pool, v, first)
    _poke(pool, v, last)
    got = {x.side: (x.first, x.last, x.count) for x in pool.violations()}
    assert got == {"before": (first, first, 1), "after": (last, last, 1)}


def test_last_payload_byte_is_the_callers():
    pool = GuardedPool("cpu")
    v = pool.alloc(NBYTES, 0x00)
    v[NBYTES - 1] = 0x5A
    v[0] = 0x5A
    _poke(pool, v, NBYTES - 1)
    assert pool.violations() == []
    pool.assert_clean()


def test_a_range_is_reported_once_with_its_ends():
    pool = GuardedPool("cpu")
    v = pool.alloc(NBYTES, 0xFF)
    for off in (1030, 1040, 5000):
        _poke(pool, v, off)
    _poke(pool, v, -7)
    got = {x.side: (x.first, x.last, x.count) for x in pool.violations()}
    assert got == {"before": (-7, -7, 1), "after": (1030, 5000, 3)}


@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 257, NBYTES, 1 << 16])
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x3C])
def test_view_size_alignment_fill_and_layout(nbytes, fill):
    pool = GuardedPool("cpu")
    v = pool.alloc(nbytes, fill)
    assert v.dtype == torch.uint8 and v.numel() == nbytes
    assert nbytes == 0 or v.data_ptr() % ALIGN == 0
    assert bool((v == fill).all())
    whole, lead, n = pool._bufs[0]
    rounded = -(-nbytes // ALIGN) * ALIGN
    assert n == nbytes and lead >= GUARD and whole.numel() - (lead + rounded) >= GUARD
    assert bool((whole[:lead] == GUARD_BYTE).all()) and bool((whole[lead + nbytes:] == GUARD_BYTE).all())
    assert pool.sizes() == [nbytes]
    pool.assert_clean()


def test_guarded_gives_a_typed_view_inside_the_guards():
    pool = GuardedPool("cpu")
    t = guarded(pool, (7, 5), torch.int64, 0xEE)
    assert t.shape == (7, 5) and t.dtype == torch.int64 and t.is_contiguous()
    assert bool((t.view(torch.uint8) == 0xEE).all())
    assert pool.sizes() == [7 * 5 * 8]
    t.fill_(-1)  # the whole payload, and nothing else
    pool.assert_clean()
    f = guarded(pool, 3, torch.float32, 0x00)
    assert f.shape == (3,) and f.data_ptr() % ALIGN == 0


class _FakeBackend:
    """What ``exact_workspace`` touches of a HipBackend."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._obj_ws = "kept"

    def _workspace(self, n):
        return "ordinary"

    def kmeans_objective(self, *a):
        return "ordinary"

    def _c(self, name, *args):
        return ("called", name, args)


def test_exact_workspace_replaces_and_restores():
    be = _FakeBackend()
    with ws_guard.exact_workspace(be, 0xFF) as pool:
        a, b = be._workspace(300), be._workspace(300)
        assert a.numel() == b.numel() == 300 and a.data_ptr() != b.data_ptr()  # a fresh buffer per request
        assert bool((a == 0xFF).all())
        assert be._obj_ws is None and be.kmeans_objective.__name__ == "objective"
        assert pool.sizes() == [300, 300]
        assert be._c("lvs_x", 1, 2) == ("called", "lvs_x", (1, 2)) and pool.entries == {"lvs_x"}  # calls pass through, recorded
    assert be._c("lvs_y") == ("called", "lvs_y", ()) and pool.entries == {"lvs_x"} and "_c" not in be.__dict__
    assert be._workspace(1) == "ordinary" and be.kmeans_objective() == "ordinary" and be._obj_ws == "kept"
    assert "_workspace" not in be.__dict__ and "kmeans_objective" not in be.__dict__


def test_every_flat_search_route_has_a_case_on_the_path_it_names():
    """The shapes the GPU extent tests run (extent_cases.FLAT) against the host planner."""
    import extent_cases

    extent_cases.check_routes()
