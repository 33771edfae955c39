"""A guarded allocator for the extent tests: every buffer handed to the library sits between two 1 MiB guards filled with a
known byte, so a write before it, into the rounding slack behind it or past its end is harmless (it lands in memory this
module owns) and visible (``GuardedPool.violations``).  Works on any torch device, CPU included - the detector's own logic
is tested without a GPU (test_ws_guard_host.py).

Layout of one allocation:  [GUARD | payload: nbytes, rounded up to 256 | GUARD]; the guards and the slack between
``nbytes`` and the rounded end hold ``GUARD_BYTE``, the payload holds the caller's fill."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import torch

# A condition, not a measurement: one query's row of LVS_MAX_K keys is 16 KiB, so a stray list of a whole query block still
# lands inside the guard and not in foreign memory.
GUARD = 1 << 20
ALIGN = 256
GUARD_BYTE = 0xA5


@dataclass
class Violation:
    ordinal: int   # the buffer's number in the pool, in the order handed out
    nbytes: int    # its requested size
    side: str      # "before" (the leading guard), "slack" (nbytes .. rounded end) or "after" (the far guard)
    first: int     # first and last damaged byte, relative to the payload start (negative: before it)
    last: int
    count: int     # damaged bytes in [first, last]

    def __str__(self) -> str:
        return (f"buffer #{self.ordinal} ({self.nbytes} bytes): {self.count} byte(s) damaged {self.side} the payload, "
                f"offsets {self.first} .. {self.last}")


class GuardedPool:
    """Buffers with guards on ``device``; everything handed out stays alive until the pool goes."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._bufs = []  # (whole allocation, payload start inside it, nbytes)

    def alloc(self, nbytes: int, fill: int = 0):
        """-> uint8 view of exactly ``nbytes`` elements, 256-byte aligned, holding ``fill``."""
        nbytes = int(nbytes)
        assert nbytes >= 0
        rounded = -(-nbytes // ALIGN) * ALIGN
        # torch's allocators align to at least 64 (CPU) / 512 (device) bytes; ALIGN spare bytes let the payload start on a
        # multiple of 256 whatever the base is.  The spare bytes belong to the leading guard.
        whole = torch.empty(GUARD + ALIGN + rounded + GUARD, dtype=torch.uint8, device=self.device)
        lead = GUARD + (-(whole.data_ptr() + GUARD)) % ALIGN
        whole.fill_(GUARD_BYTE)
        view = whole[lead:lead + nbytes]
        view.fill_(int(fill) & 0xFF)
        assert view.numel() == nbytes and (nbytes == 0 or view.data_ptr() % ALIGN == 0)
        self._bufs.append((whole, lead, nbytes))
        return view

    def violations(self) -> list:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = []
        for ordinal, (whole, lead, nbytes) in enumerate(self._bufs):
            rounded = -(-nbytes // ALIGN) * ALIGN
            for side, a, b in (("before", 0, lead), ("slack", lead + nbytes, lead + rounded),
                               ("after", lead + rounded, int(whole.numel()))):
                if b <= a:
                    continue
                bad = torch.nonzero(whole[a:b] != GUARD_BYTE).reshape(-1)
                if bad.numel():
                    out.append(Violation(ordinal, nbytes, side, int(bad[0]) + a - lead, int(bad[-1]) + a - lead,
                                         int(bad.numel())))
        return out

    def assert_clean(self) -> None:
        v = self.violations()
        assert not v, "writes outside the declared extent:\n" + "\n".join(str(x) for x in v)

    def sizes(self) -> list:
        """The requested sizes, in the order handed out."""
        return [n for _, _, n in self._bufs]


def guarded(pool: GuardedPool, shape, dtype, fill: int = 0):
    """An output tensor of ``shape`` / ``dtype`` for a raw call: the pool's layout, every BYTE set to ``fill``."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = 1
    for s in shape:
        n *= s
    itemsize = torch.empty((), dtype=dtype).element_size()
    return pool.alloc(n * itemsize, fill).view(dtype).reshape(shape)


@contextlib.contextmanager
def exact_workspace(be, fill: int):
    """Inside, every ``be._workspace(n)`` is a FRESH guarded buffer of exactly ``n`` bytes holding ``fill`` - the backend
    passes ``ws.numel()`` as ``workspace_bytes``, so every entry runs with exactly its declared need.  ``kmeans_objective``
    keeps a scratch of its own (``_obj_ws``, a plain ``torch.empty``): inside, that entry is called raw with a guarded buffer
    of exactly ``lvs_kmeans_objective_workspace_bytes``.  Yields the pool; all buffers stay alive until it goes
    (``_nearest3_begin`` holds its scratch across begin and finish).  ``pool.entries``: the names of the C entry points the
    backend called inside (everything that goes through ``be._c``), so a case can assert that the entry it is here for ran."""
    pool = GuardedPool(be.device)
    pool.entries = set()
    plain_c = be._c

    def recording_c(name, *args):
        pool.entries.add(name)
        return plain_c(name, *args)

    def objective(centroids, sums, counts, x2, out):
        k, d = int(centroids.shape[0]), int(centroids.shape[1])
        ws = pool.alloc(int(be.lib.lvs_kmeans_objective_workspace_bytes(k)), fill)
        be._c("lvs_kmeans_objective", centroids.data_ptr(), sums.data_ptr(), counts.data_ptr(), k, d, x2.data_ptr(),
              out.data_ptr(), ws.data_ptr(), int(ws.numel()), be._stream())

    patched = ("_workspace", "kmeans_objective", "_obj_ws", "_c")
    saved = {name: be.__dict__.get(name) for name in patched if name in be.__dict__}
    be._workspace = lambda n: pool.alloc(n, fill)
    be._c = recording_c
    be.kmeans_objective = objective
    be._obj_ws = None
    try:
        yield pool
    finally:
        for name in patched:
            be.__dict__.pop(name, None)
        be.__dict__.update(saved)
