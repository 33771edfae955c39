"""Ranks as threads of the test process: what the library's multi-GPU entry points (``lvs_search_sharded``,
``lvs_kmeans_iteration``) need from a transport, with one GPU and one process.  Every rank is a thread with its own
``torch.cuda.Stream`` on the one device; what crosses the ranks goes through a shared device pool between two waits at a
``threading.Barrier``.  A helper, not a test: tests/test_gpu_dist.py and tests/test_gpu_sharded_abi.py run on it.

``run_ranks(W, fn, device, pool_bytes)`` starts ``fn(rank)`` on W threads and returns the W results; ``rank`` carries the rank
number, its stream and the two callbacks the library calls back into:

* ``rank.all_gather``: ``lvs_all_gather_fn`` - copy ``nbytes`` into ``pool[r]``, wait, copy ``pool[0 .. W)`` out, wait;
* ``rank.all_reduce``: ``lvs_all_reduce_fn`` - copy ``count`` float32 (dtype 0) or float64 (dtype 1) elements into ``pool[r]``,
  wait, sum ``pool[0 .. W)`` IN RANK ORDER into the rank's own buffer, wait.  The fixed order makes every rank's result the
  same bits.

Both assert that the stream they are handed is the rank's stream, and count their calls.  Any exception on a rank aborts the
barrier, so a failing rank never leaves the others waiting (the waits themselves give up after 120 s)."""
from __future__ import annotations

import ctypes
import threading

BARRIER_TIMEOUT = 120  # seconds: a wait that no peer joins
JOIN_TIMEOUT = 300


class DevBytes:
    """A raw device pointer as something torch.as_tensor understands."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


class _Callback:
    """One rank's side of a collective: a ctypes callback (``ptr``) around ``exchange``, its call count, the status protocol."""

    typedef = None

    def __init__(self, rank):
        from lotus_amd import _capi

        self.rank, self.calls = rank, 0
        self._fn = _capi.CALLBACKS[self.typedef](self._entry)  # kept alive with the object
        self.ptr = ctypes.cast(self._fn, ctypes.c_void_p)

    def _entry(self, ctx, *args):
        from lotus_amd import _capi

        try:
            assert int(args[-1] or 0) == int(self.rank.stream.cuda_stream), "the callback got another stream than the rank's"
            self.calls += 1
            self.exchange(*args[:-1])
            return 0
        except Exception as e:  # noqa: BLE001 - reported through the status
            self.rank.world.errs.append(f"rank {self.rank.r}: {e!r}")
            self.rank.world.barrier.abort()
            return _capi.EDEVICE

    def _view(self, ptr, nbytes):
        import torch

        return torch.as_tensor(DevBytes(ptr, nbytes), device=self.rank.world.device)

    def _staged(self, send, nbytes, finish):
        """``send`` -> pool[r]; wait; ``finish(pool[:, :nbytes])``; wait."""
        import torch

        rank, world = self.rank, self.rank.world
        assert nbytes <= world.pool.shape[1], f"{nbytes} bytes exchanged, the pool holds {world.pool.shape[1]} per rank"
        with torch.cuda.stream(rank.stream):
            world.pool[rank.r, :nbytes].copy_(self._view(send, nbytes))
        rank.stream.synchronize()
        world.barrier.wait(timeout=BARRIER_TIMEOUT)
        with torch.cuda.stream(rank.stream):
            finish(world.pool[:, :nbytes])
        rank.stream.synchronize()
        world.barrier.wait(timeout=BARRIER_TIMEOUT)


class ThreadAllGather(_Callback):
    typedef = "lvs_all_gather_fn"

    def exchange(self, send, recv, nbytes):
        self._staged(send, nbytes, lambda pool: self._view(recv, self.rank.world.W * nbytes).copy_(pool.reshape(-1)))


class ThreadAllReduce(_Callback):
    typedef = "lvs_all_reduce_fn"

    def exchange(self, buf, count, dtype):
        import torch

        assert dtype in (0, 1), dtype
        dt, size = (torch.float32, 4) if dtype == 0 else (torch.float64, 8)

        def finish(pool):
            out = self._view(buf, count * size).view(dt)
            out.copy_(pool[0].view(dt))
            for r in range(1, self.rank.world.W):  # rank order, one addition at a time: the same bits on every rank
                out.add_(pool[r].view(dt))

        self._staged(buf, count * size, finish)


class _World:
    def __init__(self, W, device, pool_bytes):
        import torch

        self.W, self.device = int(W), torch.device(device)
        # (rows of a multiple of 256 bytes: every rank's slot is aligned for its float64 view)
        self.pool = torch.empty((self.W, -(-max(int(pool_bytes), 1) // 256) * 256), dtype=torch.uint8, device=self.device)
        self.barrier = threading.Barrier(self.W)
        self.errs = []


class Rank:
    def __init__(self, world, r):
        import torch

        self.world, self.r, self.W = world, r, world.W
        self.stream = torch.cuda.Stream(device=world.device)
        self.all_gather = ThreadAllGather(self)
        self.all_reduce = ThreadAllReduce(self)

    def on_stream(self):
        import torch

        return torch.cuda.stream(self.stream)


def run_ranks(W, fn, device, pool_bytes=0):
    """``fn(rank)`` on W threads -> [fn's result per rank]; raises AssertionError with every rank's error if one failed.
    ``pool_bytes``: the largest message of one rank (the pool is [W, pool_bytes])."""
    world = _World(W, device, pool_bytes)
    outs = [None] * world.W

    def body(r):
        try:
            rank = Rank(world, r)
            outs[r] = fn(rank)
            rank.stream.synchronize()
        except Exception as e:  # noqa: BLE001
            world.errs.append(f"rank {r}: {e!r}")
            world.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world.W)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_TIMEOUT)
    assert not any(t.is_alive() for t in threads), "a rank did not finish"
    assert not world.errs, world.errs
    return outs
