"""The dynamic-LDS launch helper (lvs_launch_lds, lvs_common.h): hipFuncSetAttribute(MaxDynamicSharedMemorySize) is latched
per (kernel instantiation, device) and must be set again when a later call of the same instantiation needs more LDS.  Each
test runs a small-LDS call, a call beyond the 64 KB default and the small one again on ONE instantiation; a latch that does
not grow fails the second call with an invalid-value launch error.  Every result is checked as in its kernel's own tests."""
import numpy as np
import pytest

import oracle
import synth
import test_gpu_ivf as flat
import test_gpu_ivf_sq8 as sq8
from ivf_sq8_oracle_backend import sq8_decode, sq8_reference
from lotus_amd import _capi
from test_gpu_parity import _run, _stored

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
NB, NLIST, NQ, K = 2000, 8, 40, 10  # nprobe = nlist: the exact search over all rows


def _dpad(d):
    return (d + 63) // 64 * 64


def test_ivf_flat_u4_grows_its_lds(hip_backend):
    """lvs_ivf_scan_kernel<4>: fp16 d = 64 (4 fragments, ~8 KB), hi|lo d = 960 (120 fragments, ~124 KB), d = 64 again."""
    be = hip_backend
    shapes = {64: (F16, IP), 960: (SPLIT, L2)}
    for d in shapes:
        assert (_dpad(d) // 16) % 4 == 0 and (_dpad(d) // 16) % 8 != 0  # fragments per K segment: batches of 4, not 8
    assert 2 * (_dpad(960) // 16) * 1024 > 64 * 1024 and be.ivf_fits(960, K, SPLIT)
    case = {}
    for d, (mode, metric) in shapes.items():
        xb, xb_s, xq, xq_s = flat._data(NB, NQ, d, mode, seed=d)
        c = flat._centroids(xb_s, NLIST, metric, seed=d + 1)
        case[d] = (xb, xb_s, xq, xq_s, c, mode, metric, oracle.flat_search(xb_s, xq_s, K, metric))
    for d in (64, 960, 64):
        xb, xb_s, xq, xq_s, c, mode, metric, (D_ref, I_ref) = case[d]
        D, I, probe, off, rows, _ = flat._search(be, xb, xq, c, K, mode, metric, NLIST)
        flat._check(D_ref, I_ref, D, I, rescore=(xb_s, xq_s, metric, off, rows, probe))


def test_ivf_sq8_u1_grows_its_lds(hip_backend):
    """lvs_ivf_sq8_scan_kernel<1>: d = 64 (one 64-dimension block, ~4 KB), d = 1 472 (23 blocks, ~94 KB), d = 64 again."""
    be = hip_backend
    shapes = {64: (F16, IP), 1472: (SPLIT, L2)}
    for d in shapes:
        assert _dpad(d) == d and (d // 64) % 2 == 1  # an odd count of 64-dimension blocks: batches of 1
    assert (1472 // 32) * 2 * 1024 > 64 * 1024 and be.ivf_sq8_fits(1472, K, SPLIT)
    case = {}
    for d, (mode, metric) in shapes.items():
        xb, xb_s, xq, xq_s = sq8._data(NB, NQ, d, mode, seed=d + 2)
        c = sq8._centroids(xb_s, NLIST, metric, seed=d + 3)
        packed, lists, sq, h = sq8._build(be, xb, c, mode, metric, np.arange(NB))
        xhat = sq8_decode(h["c"], h["where"], h["vmin"], h["vdiff"], h["codes"])
        case[d] = (packed, lists, sq, h, xq, xq_s, xhat, mode, metric)
    ref = {}
    for d in (64, 1472, 64):
        packed, lists, sq, h, xq, xq_s, xhat, mode, metric = case[d]
        D, I, probe = sq8._search(be, packed, lists, sq, xq, mode, K, metric, NLIST)
        if d not in ref:
            ref[d] = sq8_reference(xhat, xq_s, K, metric, h["off"], h["rows"], probe)
        sq8._check(*ref[d], D, I, rescore=(xhat, xq_s, metric, h["off"], h["rows"], probe))


def test_stream_kernel_grows_its_lds(hip_backend):
    """lvs_stream_kernel<16, 1, 4, false> twice.  One fp16 query at d = 64: one query block per workgroup, 4 fragments per K
    segment divide by none of 16 / 24 / 8 - the general loop with UNROLL 16 (~20 KB).  64 hi|lo queries at d = 768: 96 query
    fragments, two query blocks do not fit 160 KB, so lvs_stream_plan deals them to two sibling workgroups of one block each;
    48 fragments per K segment - UNROLL 16 (~112 KB).  4 096 rows: the stream kernel's shortest corpus, too short for a sample,
    so neither call runs the SEED instantiation."""
    be = hip_backend
    nb = 4096
    for nq, d, mode in ((1, 64, F16), (64, 768, SPLIT)):
        xb = synth.corpus(nb, d, seed=d)
        xq, _ = synth.queries(xb, nq, seed=3)
        be.timing_enable(True)
        D, I, _ = _run(be, xb, xq, K, mode, IP, one_pass=False)
        kernel = be.timing_read_full()["kernel"]
        be.timing_enable(False)
        assert kernel == "lvs_stream_kernel", kernel
        Dr, Ir = oracle.flat_search(_stored(xb, mode), _stored(xq, mode), K, IP)
        err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=1e-5)
        assert (I >= 0).sum() == (Ir >= 0).sum()
        assert err <= 1e-5 and hard == 0 and recall >= 0.9999, (err, hard, recall)
