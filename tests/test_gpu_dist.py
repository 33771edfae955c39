"""The N>1 path on the REAL HIP backend: two processes share cuda:0, rendezvous over gloo, and
run every sharded operator - row-sharded search with id offsets, device-side merge of the gathered candidate lists
(short and long lists), sharded K = N ranking / score rows, k-means on a row-sharded index (device sums all-reduced,
per-shard final assignment), tile-dealt dedup - against the single-process CPU oracle.  On an 8-GPU node the only
difference is the transport inside ``lotus_amd/_dist.py`` (RCCL on device tensors instead of host staging)."""
import pytest

import dist_cases

pytestmark = pytest.mark.gpu


def test_sharded_operators_on_hip_backend_two_ranks_one_gpu(tmp_path):
    res = dist_cases.run(tmp_path, "hip")
    dist_cases.check(res, exact=False)


def test_2d_split_on_the_hip_backend(tmp_path):
    """HipVS(shard=(2, 2)): four processes (2 query groups x 2 corpus shards) on cuda:0 - merge inside a corpus group,
    concatenation across the query groups, k-means and score rows through the corpus sub-group."""
    res = dist_cases.run_2d(tmp_path, "hip")
    dist_cases.check_2d(res, exact=False)


def test_shard_scale_agreement_and_query_validation_on_the_hip_backend(tmp_path):
    """fp32 rows with per-shard magnitudes: one agreed pack exponent (re-agreed after an outlier row), and the validation
    verdict of one rank's query slice taken by both ranks - on the real packers / flag words."""
    res = dist_cases.run_scale(tmp_path, "hip")
    dist_cases.check_scale(res, exact=False)


def _rccl_worker(port, out_q):
    import os

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from lotus_amd import _dist

        dev = torch.device("cuda", 0)
        keys = torch.arange(12, dtype=torch.int64, device=dev).reshape(4, 3) * (1 << 40)
        g = _dist.all_gather_rows(keys)  # device tensor straight into RCCL (no host staging under nccl)
        sums = torch.ones((5, 7), dtype=torch.float32, device=dev)
        counts = torch.full((5,), 2.0, dtype=torch.float32, device=dev)
        obj = torch.tensor([3.5], dtype=torch.float64, device=dev)
        _dist.all_reduce_sum_([sums, counts, obj])
        _dist.barrier()
        staged = _dist._staging_device(keys, None)
        out_q.put((tuple(g.shape), bool(torch.equal(g[0], keys)), g.is_cuda, float(sums.sum()), float(counts.sum()), float(obj.item()),
                   staged is None))
    finally:
        dist.destroy_process_group()


def test_rccl_transport_branch_runs_on_device_tensors():
    """The `nccl` (= RCCL) branch of lotus_amd/_dist.py - device tensors handed to the collectives as they are - executed on
    the one GPU of this box (world size 1: RCCL has no second device here; the 8-GPU run is the driver's).  Covers the API
    shapes the path uses: all_gather_into_tensor of int64 keys, all-reduce of float32 sums / counts and the float64 objective."""
    import os

    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(30500 + os.getpid() % 2000, q))
    p.start()
    shape, same, on_gpu, s, c, o, direct = q.get(timeout=300)
    p.join(60)
    assert p.exitcode == 0
    assert shape == (1, 4, 3) and same and on_gpu and direct
    assert s == 35.0 and c == 10.0 and o == 3.5


# (at most four ranks: with the test process itself no more than five processes have the one GPU open at a time)
@pytest.mark.parametrize("gpus,split,queries,corpus", [(2, "rows", 4096, 262144), (4, "rows", 20480, 300_003), (4, "queries", 10240, 262144)])
def test_bench_self_launches_its_ranks_and_prints_one_line(gpus, split, queries, corpus):
    """`python bench.py --gpus 2 ...` with no launcher around it (the form of the driver's N = 1 command): bench.py starts its
    own two ranks under torch.distributed.run, rank 0 prints the one JSON line.  Rehearsal mode (both ranks on cuda:0 over
    gloo) because this box has one GPU - the code path is the N > 1 path of the real run: shared inputs through /dev/shm,
    pooled sample thresholds, seeded shard search, key all-gather, merge, max-over-ranks timing, oracle check on rank 0."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LOTUS_BENCH_REHEARSAL="1")
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(var, None)
    # (the per-rank shapes of the driver's N = 8 command on a one-GPU box, with four ranks: row split with 75 001-row shards
    # through the chunked register-resident path and pooled thresholds, and the query split with 2 560 queries per rank; RCCL
    # itself cannot run here - two ranks on one device are refused - so the transport under rehearsal is gloo)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus), "--steps", "2", "--warmup", "1",
                        "--queries", str(queries), "--corpus", str(corpus), "--check-sample", "128", "--split", split, "--full"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["steps"] == 2 and out["unit"] == "queries/s" and out["config"]["split"] == split
    assert out["roofline"]["bound"] == "mfma" and out["roofline"]["frac"] > 0
    assert out["recall_at_k"] == 1.0 and out["id_mismatches_outside_near_ties"] == 0
    assert out["planted_neighbour_at_rank1"] > 0.99
    assert "REHEARSAL" in out["data"]
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("lotus_bench_")]


# ---- the row-sharded search with its exchange steps inside the library (lvs_search_sharded / _rccl) --------------------------
def _sharded_inputs(hip_backend, n, nq, d, seed):
    import numpy as np

    import synth
    from lotus_amd import _capi

    xb = synth.corpus(n, d, seed=seed).astype(np.float16)
    xq = synth.corpus(nq, d, seed=seed + 1).astype(np.float16)
    xb[n // 2 + 7] = xb[5]  # an exact duplicate across shards: equal scores, ids decide
    return xb, xq, hip_backend.pack(xb, _capi.PACK_F16), hip_backend.pack(xq, _capi.PACK_F16)


@pytest.mark.parametrize("sizes", [(90_000, 70_000, 40_000), (120_000, 80_000, 0), (200_000,),
                                   # the node's shape: EIGHT shards (one of them empty, one a single ragged block) - r6
                                   (40_000, 30_000, 25_001, 0, 45_000, 31, 35_000, 24_968)])
def test_sharded_search_inside_the_library_with_a_thread_all_gather(hip_backend, sizes):
    """lvs_search_sharded on `len(sizes)` ranks = threads of this process, each with its own stream on cuda:0; the all-gather the
    library calls back into is a device copy through a shared pool + a thread barrier.  Uneven shards, an EMPTY shard, pooled
    sample thresholds on: every rank's merged keys equal the single-launch search of the whole corpus bit for bit (and the
    oracle's ids)."""
    import numpy as np
    import torch

    import oracle
    import thread_ranks
    from lotus_amd import _capi
    from lotus_amd.backend import _ptr

    be, lib = hip_backend, hip_backend.lib
    n, nq, d, k = sum(sizes), 4096, 128, 10
    xb, xq, corpus, queries = _sharded_inputs(be, n, nq, d, seed=31)
    want = be.search_keys(corpus, queries, k, _capi.METRIC_IP)
    be.synchronize()
    W = len(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tiles = int(lib.lvs_flat_search_seed_tiles(nq, max(sizes), k))
    assert W == 1 or tiles > 0

    def rank(rk):
        r, s = rk.r, rk.stream
        shard = be.slice_rows(corpus, int(offs[r]), int(offs[r + 1]))
        need = int(lib.lvs_search_sharded_workspace_bytes(W, nq, shard.n, d, k, shard.mode, queries.mode, tiles))
        assert need > 0
        with rk.on_stream():
            ws = torch.empty(need, dtype=torch.uint8, device=be.device)
            keys = torch.zeros((nq, k), dtype=torch.int64, device=be.device)
            st = lib.lvs_search_sharded(rk.all_gather.ptr, None, W, _ptr(shard.rows) if shard.n else None,
                                        shard.mode, shard.n, _ptr(queries.rows), queries.mode, nq, d, _capi.METRIC_IP, k,
                                        _ptr(shard.norms) if shard.n else None, _ptr(queries.norms), int(offs[r]), tiles,
                                        _ptr(keys), _ptr(ws), need, int(s.cuda_stream))
        s.synchronize()
        assert st == 0, lib.lvs_last_error()
        return keys, rk.all_gather.calls

    res = thread_ranks.run_ranks(W, rank, be.device, pool_bytes=max(tiles * nq * 4, nq * k * 8))
    outs = [keys for keys, _ in res]
    assert [c for _, c in res] == [0 if W == 1 else 2] * W  # sample scores + key lists
    for r in range(W):
        assert torch.equal(outs[r], want), r
    _, I = be.keys_to_result(outs[0], _capi.METRIC_IP)
    Dr, Ir = oracle.flat_search(xb.astype(np.float32), xq[:256].astype(np.float32), k, 0)
    got = I[:256].cpu().numpy()
    assert np.mean([len(set(a) & set(b)) / k for a, b in zip(got.tolist(), Ir.tolist())]) == 1.0
    assert got[0, 0] >= 0


def _rccl_sharded_worker(out_q):
    import ctypes
    import os

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
    import torch

    import synth
    from lotus_amd import _capi
    from lotus_amd.backend import HipBackend, _ptr

    be = HipBackend("cuda:0")
    lib = be.lib
    rccl = ctypes.CDLL("librccl.so.1")

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    # the communicator belongs to THIS copy of RCCL (torch bundles another): name its entry points explicitly
    addr = lambda f: ctypes.cast(f, ctypes.c_void_p)
    assert lib.lvs_rccl_bind(addr(rccl.ncclAllGather), addr(rccl.ncclCommCount), addr(rccl.ncclGetErrorString)) == 0
    assert lib.lvs_rccl_available() == 1
    n, nq, d, k = 150_000, 2048, 128, 10
    xb = synth.corpus(n, d, seed=41).astype(np.float16)
    xq = synth.corpus(nq, d, seed=42).astype(np.float16)
    corpus, queries = be.pack(xb, _capi.PACK_F16), be.pack(xq, _capi.PACK_F16)
    want = be.search_keys(corpus, queries, k, _capi.METRIC_IP, id_offset=1000)
    tiles = int(lib.lvs_flat_search_seed_tiles(nq, n, k))
    need = int(lib.lvs_search_sharded_workspace_bytes(1, nq, n, d, k, 0, 0, tiles))
    ws = torch.empty(need, dtype=torch.uint8, device=be.device)
    keys = torch.zeros((nq, k), dtype=torch.int64, device=be.device)
    s = torch.cuda.current_stream(be.device)
    st = lib.lvs_search_sharded_rccl(comm, _ptr(corpus.rows), 0, n, _ptr(queries.rows), 0, nq, d, _capi.METRIC_IP, k,
                                     _ptr(corpus.norms), _ptr(queries.norms), 1000, tiles, _ptr(keys), _ptr(ws), need,
                                     int(s.cuda_stream))
    be.synchronize()
    # and the transport itself through the library's own wrapper: a one-rank all-gather of the key lists = a copy
    gathered = torch.zeros_like(keys)
    rc = rccl.ncclAllGather(ctypes.c_void_p(_ptr(keys)), ctypes.c_void_p(_ptr(gathered)), ctypes.c_size_t(keys.numel() * 8), 0,
                            comm, ctypes.c_void_p(int(s.cuda_stream)))
    be.synchronize()
    out_q.put((int(st), bool(torch.equal(keys, want)), int(rc), bool(torch.equal(gathered, keys))))
    rccl.ncclCommDestroy(comm)


def test_sharded_search_over_rccl_on_a_one_rank_communicator():
    """lvs_search_sharded_rccl with a real ncclComm_t (one rank: this box has one GPU and RCCL refuses two ranks on a device):
    communicator size read through ncclCommCount, the library's RCCL resolution / lvs_rccl_bind, same keys as the plain search.
    The two ncclAllGather calls of the N > 1 path are exercised by the thread test above with a stand-in transport and by the
    driver's multi-GPU run with RCCL itself."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_sharded_worker, args=(q,))
    p.start()
    st, same, rc, copied = q.get(timeout=300)
    p.join(60)
    assert st == 0 and same and rc == 0 and copied
