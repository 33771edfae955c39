"""Capture a sequence of C-ABI calls once, replay it on other data in the same buffers.

include/lotus_hip.h promises that an entry point only ENQUEUES work on ``stream``: no allocation, no synchronisation, no
pointer kept.  Stream capture checks that without a race: while a stream is captured nothing executes and a synchronisation
or an allocation is an error (``capture_error_mode="global"``: on any thread); a replay runs exactly what was enqueued on the
capture stream.  So a call captured once and replayed on different inputs in the same buffers gives the right result only if

  1. every launch, memset and copy of the call went to ``stream``,
  2. every data-dependent decision was taken on the device,
  3. the call itself re-initialises whatever scratch state it needs.

What it does not show: anything about two LIVE streams racing, or about the device guards of a multi-GPU process."""
import numpy as np
import torch

SENT = 0xC3     # every output before the capture (tests/test_gpu_output_extents.py's byte)
WS_SENT = 0x5A  # every workspace


def fill_bytes(tensors, byte):
    for t in tensors:
        t.view(torch.uint8).fill_(byte)


def holds(t, byte):
    return bool((t.contiguous().view(torch.uint8) == byte).all())


def host(be, tensors):
    be.synchronize()
    return tuple(np.ascontiguousarray(t.cpu().numpy()) for t in tensors)


def eager(be, enqueue, outputs, load, which, scratch=()):
    """The same calls made directly on the current (default) stream with input set ``which``, from the same sentinel-filled
    outputs and workspaces as a replay starts from -> host copies of the outputs."""
    fill_bytes(outputs, SENT)
    fill_bytes(scratch, WS_SENT)
    load(which)  # (after the sentinel: an in-out buffer is an output AND holds an input)
    enqueue()
    return host(be, outputs)


def replayed(be, enqueue, outputs, load, scratch=(), order=("B", "A")):
    """``enqueue()``: the raw calls under test, each taking ``be._stream()`` when it is made, together with the ``zero_()`` of
    every counter the header has the caller zero.  ``outputs`` / ``scratch``: the device tensors the calls write / use as
    workspace.  ``load(which)``: writes input set "A" or "B" into the input buffers with ``copy_`` (same buffers, same shapes).

    Warm-up with A (arms the kernels' attributes, as before any capture); sentinel into every output and workspace; capture on
    a fresh side stream; every output must still hold the sentinel (nothing ran eagerly, on any stream); then for each set in
    ``order``: load it, replay, synchronise -> list of the outputs' host copies.  The second replay starts from the scratch
    the first one left."""
    be.lib.lvs_timing_enable(0)  # (its event pairs are not part of the contract)
    load("A")
    enqueue()
    be.synchronize()
    fill_bytes(outputs, SENT)
    fill_bytes(scratch, WS_SENT)
    be.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        enqueue()
    be.synchronize()
    for i, t in enumerate(outputs):
        assert holds(t, SENT), f"output {i} was written while the call was being captured: something ran outside the capture"
    for i, t in enumerate(scratch):
        assert holds(t, WS_SENT), f"workspace {i} was written while the call was being captured"
    got = []
    for which in order:
        load(which)
        g.replay()
        got.append(host(be, outputs))
    return got
