#!/usr/bin/env python
"""bench.py - sem_sim_join hot path on N MI355X GPUs of one node.

One "step" = one full pass of the hot path over one batch: every one of Q left rows (queries, d=768 fp16) is
searched against the N-row right index (corpus, d=768 fp16), k=10, exactly what `sem_sim_join` hands to
`VS.__call__` (lotus/sem_ops/sem_sim_join.py:134).  The corpus is row-sharded over the ranks, queries are replicated,
each rank runs the tiled MFMA distance + fused top-k kernel on its shard, then ONE RCCL all-gather of the per-shard
candidate keys (8 B each) and a merge + decode give every rank the final (D, I).  Inputs are resident in HBM before
the timed region; total work is fixed as N grows ("strong" scaling).

Inputs are SURVEY.md 8(d)'s recipe (benchdata.py): numpy streams SeedSequence([20260923, config, block]) in 1 M-row
blocks, generated on the host - anyone can rebuild the inputs of a BENCH line.

Prints ONE JSON line on rank 0 (see the contract in the task statement): value = Q * steps / time in queries/s.
A plain run does only what that figure needs: inputs, warm-up, the timed steps, `--dump-outputs`, the line.  Its extra
figures come from the last timed step and the timed steps' own events - `planted_neighbour_at_rank1` and:
  "roofline"      dominant kernel vs the dense fp16 MFMA peak, timed with HIP events on the launch stream;
                  `traffic` = HBM-side bytes per launch from the committed rocprofv3 PMC passes, reported only when the
                  kernel sources are byte-identical to the ones the counters were collected on (else null).
`--full` adds everything else, after the timed steps:
  "cpu_baseline"  (N=1) the CPU comparators (C + OpenMP twin and torch-MKL, both timed, the faster reported) on a bounded
                  sample of the same workload;
  "recall_at_k" / "id_mismatches_outside_near_ties" / "max_abs_score_err": the GPU result of the LAST timed step checked
                  against the CPU oracle (oracle/flat.py) on a query sample - at every N, rank 0;
  "legs"          (N=1) the other BASELINE configs and regimes in the same process, each with its own in-run check:
                  configs[1] (10k x 1M), the HBM-bound small-batch calls (1 .. 256 queries), the per-GPU shapes of every
                  8-GPU split of the join (`node_plan_8gpu`), a one-GPU rehearsal of the 8-shard run with real id offsets
                  and the 8-way merge (`world8_rehearsal`), configs[3] (threshold self-join with planted duplicates),
                  configs[4] (k-means, full-data iteration and faiss-parity mode), fp32 embeddings, and T_call
                  (`HipVS.__call__` host ndarray -> host (D, I)).
All GPU work of `--full` runs first and back to back; the CPU-side checks and the CPU baseline follow.

The stdout line is kept below 6 KB (floats at 5 significant digits, one short object per leg, the figures that matter once
more in a flat `legs_summary` printed LAST) so that a tail of the line still holds every leg; the verbose form of the same
objects (notes, per-iteration lists) goes to stderr as `BENCH_DETAILS {...}`.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP16_MFMA_TFLOPS = 2500.0  # dense, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def sig(x, digits=5):
    """Floats rounded to `digits` significant digits, recursively (the line stays short; nothing is measured to more)."""
    if isinstance(x, float):
        return float(f"{x:.{digits}g}") if x == x and abs(x) != float("inf") else x
    if isinstance(x, dict):
        return {k: sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [sig(v, digits) for v in x]
    return x


DETAIL_KEYS = ("note", "objective", "iteration_ms", "searched_row_fraction_per_iteration", "comparators_timed", "algorithmic_flops",
               "algorithmic_flops_per_iteration", "mfma_frac_secondary")


LEG_DETAIL_KEYS = ("rows", "k", "niter", "train_rows", "threshold", "kernel_launches", "expected_in_band", "unplanted_pairs",
                   "shards", "shard_rows", "ids_from_every_shard", "short_lists_slots", "objective_first_last", "blob_purity",
                   "oracle_iterations", "bound", "seconds_10_iterations_incl_setup", "oracle_seconds",
                   "mfma_floor_node_qps", "best_node_qps", "fp16_same_shape_ms")


def compact(x, in_legs=False):
    """The stdout form of the line: verbose keys dropped (they go to stderr); inside `legs` also the keys that restate a leg's
    configuration (its name says it) and a call's wall time where the kernel time is given."""
    if isinstance(x, dict):
        out = {}
        for k, v in x.items():
            if k in DETAIL_KEYS or (in_legs and (k in LEG_DETAIL_KEYS or (k == "ms_per_call" and "kernel_ms" in x))):
                continue
            out[k] = compact(v, in_legs or k == "legs")
        return out
    return x


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--corpus", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the oracle check, the CPU baseline and the secondary legs "
                         "(--cpu-sample ... --kmeans-k shape them; a plain run ignores those options)")
    ap.add_argument("--cpu-sample", type=int, default=8192, help="queries timed on the CPU comparator (N=1 only)")
    ap.add_argument("--check-sample", type=int, default=512, help="queries re-checked against the CPU oracle (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-legs", action="store_true", help="skip the secondary legs (N=1)")
    ap.add_argument("--dedup-rows", type=int, default=5_000_000, help="configs[3] leg: rows of the threshold self-join (0 = skip)")
    ap.add_argument("--kmeans-rows", type=int, default=10_000_000, help="configs[4] legs: rows (0 = skip)")
    ap.add_argument("--kmeans-k", type=int, default=1024)
    ap.add_argument("--split", choices=("rows", "queries", "auto"), default="rows",
                    help="N > 1: 'rows' = BASELINE's configuration (corpus row-sharded, RCCL all-gather + top-k merge); 'queries' = "
                         "every GPU holds the corpus and answers Q / N queries (one all-gather, no merge); 'auto' = whichever "
                         "lotus_amd.plan.pick_split projects ahead for this shape")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one returned - distances.npy (float32) and indices.npy "
                         "(float64), [Q, k] - to DIR (rank 0); above 64 MB a fixed, seeded row sample, its row numbers in rows.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(np, out_dir, D, I):
    """The (D, I) a caller of the timed path receives, as .npy files: D float32, I float64 (ids < 2^53 are exact).  Results of
    more than DUMP_MAX_BYTES are cut to a fixed sample of rows (seeded, sorted), whose row numbers go to rows.npy."""
    os.makedirs(out_dir, exist_ok=True)
    nq, k = int(D.shape[0]), int(D.shape[1])
    max_rows = max(1, DUMP_MAX_BYTES // (k * (4 + 8) + 8))  # + 8: the row number in rows.npy
    if nq > max_rows:
        rows = np.sort(np.random.default_rng(20260923).choice(nq, max_rows, replace=False))
        sel = D.new_tensor(rows, dtype=I.dtype)
        D, I = D[sel], I[sel]
        np.save(os.path.join(out_dir, "rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "distances.npy"), D.cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "indices.npy"), I.cpu().numpy().astype(np.float64))


def csrc_hash() -> str:
    """sha256 over the kernel sources + the C-ABI header: ties committed counter data to the binary that ran."""
    h = hashlib.sha256()
    base = os.path.join(ROOT, "lotus_amd", "csrc")
    names = sorted(f for f in os.listdir(base) if f.endswith((".hip", ".h")))
    for p in [os.path.join(base, f) for f in names] + [os.path.join(ROOT, "include", "lotus_hip.h")]:
        with open(p, "rb") as f:
            h.update(os.path.basename(p).encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def self_launch(args) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks ourselves - the same
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`
    command the torchrun form of the contract spells out, on a free port - and hand its exit code back.  Rank r runs on
    cuda:r over RCCL; rank 0 prints the one JSON line to the inherited stdout."""
    import socket
    import subprocess

    rehearsal = os.environ.get("LOTUS_BENCH_REHEARSAL") == "1"
    if not rehearsal:
        import torch

        have = torch.cuda.device_count()
        if have < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but this host shows {have} GPU(s); nothing was measured "
                  "(LOTUS_BENCH_REHEARSAL=1 runs the N-rank code path on one GPU over gloo - a rehearsal, not a number)",
                  file=sys.stderr)
            return 1
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # torchrun pins OMP_NUM_THREADS=1 per rank when it is unset; rank 0 runs the CPU oracle check - give every rank its share
    env.setdefault("OMP_NUM_THREADS", str(max(1, min(32, (os.cpu_count() or 1) // args.gpus))))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver; before any HIP call
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    import numpy as np
    import torch
    import torch.distributed as dist

    import benchdata

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        args.gpus = world  # started under torch.distributed.run: the launcher's world size is the truth
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU")
    # LOTUS_BENCH_REHEARSAL=1 (development only, never a reported number): the ranks share cuda:0 and talk over gloo, so that
    # the N > 1 code path of this file can be exercised on a one-GPU box (RCCL refuses two ranks on one device)
    rehearsal = world > 1 and os.environ.get("LOTUS_BENCH_REHEARSAL") == "1"
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)  # RCCL

    from lotus_amd import _capi, _dist
    from lotus_amd.backend import HipBackend

    be = HipBackend(device)
    n, d, nq, k = args.corpus, args.dim, args.queries, args.k
    legs_on = args.full and world == 1 and not args.no_legs

    # ---- inputs (host, numpy streams).  The other configs' rows are drawn by background threads while the GPU works on
    # the headline (numpy releases the GIL), so the GPU legs below run back to back ----
    pool = ThreadPoolExecutor(2)
    fut_dedup = fut_km = None
    t_gen0 = time.perf_counter()
    if legs_on and args.dedup_rows > 0:
        fut_dedup = pool.submit(benchdata.dedup_rows, benchdata.CFG_DEDUP, args.dedup_rows, d)
    if legs_on and args.kmeans_rows > 0:
        fut_km = pool.submit(benchdata.blobs, benchdata.CFG_KMEANS, args.kmeans_rows, d, args.kmeans_k)
    xb_h, xq_h, planted_h, shm_dir = shared_inputs(np, dist, benchdata, world, rank, n, d, nq)
    gen_s = time.perf_counter() - t_gen0
    # the split of the join over the ranks: BASELINE configs[2] names the ROW split (corpus sharded, RCCL top-k merge) - the
    # default; --split queries / auto runs the query split (the planner's choice when the corpus fits every GPU)
    split = args.split
    if split == "auto":
        from lotus_amd import plan as _plan

        gq_, gc_ = _plan.pick_split(world, nq=nq, nb=n, d=d) if world > 1 else (1, 1)
        split = "queries" if gq_ == world and world > 1 else "rows"
    if world == 1:
        split = "rows"
    per = -(-n // world) if split == "rows" else n
    lo, hi = (min(n, rank * per), min(n, (rank + 1) * per)) if split == "rows" else (0, n)
    qper = -(-nq // world) if split == "queries" else nq
    q_lo, q_hi = (min(nq, rank * qper), min(nq, (rank + 1) * qper)) if split == "queries" else (0, nq)
    corpus = be.pack(xb_h[lo:hi], _capi.PACK_F16)  # this rank's shard (row split) or the whole corpus (query split), resident
    queries = be.pack(xq_h, _capi.PACK_F16)  # replicated
    my_queries = be.slice_rows(queries, q_lo, q_hi) if split == "queries" else queries
    planted = torch.from_numpy(planted_h).to(device)

    # row-sharded join: every shard's starting thresholds come from ALL shards' samples (one small all-gather before the
    # search, lvs_flat_search_seed_scores / lvs_flat_search_keys_seeded - what HipVS(shard=True).__call__ does)
    seed_tiles = be.seed_tiles(nq, per, k, _capi.PACK_F16, _capi.PACK_F16) if (world > 1 and split == "rows") else 0

    def step():
        if split == "queries":  # every rank answers its own queries against the whole corpus; one all-gather concatenates
            keys = be.search_keys(corpus, my_queries, k, _capi.METRIC_IP)
            if keys.shape[0] < qper:  # (the last rank's slice may be short: equal blocks for the all-gather)
                keys = torch.cat([keys, torch.zeros((qper - keys.shape[0], k), dtype=keys.dtype, device=keys.device)])
            keys = _dist.all_gather_rows(keys).reshape(world * qper, k)[:nq].contiguous()
            return keys, be.keys_to_result(keys, _capi.METRIC_IP)
        seeds = None
        if seed_tiles:
            seeds = _dist.all_gather_rows(be.seed_scores(corpus, queries, _capi.METRIC_IP, seed_tiles)).reshape(world * seed_tiles, nq)
        keys = be.search_keys(corpus, queries, k, _capi.METRIC_IP, id_offset=lo, seed_scores=seeds)
        if world > 1:
            keys = be.merge_keys(_dist.all_gather_rows(keys))  # one RCCL all-gather of [Q,k] uint64 keys + merge
        return keys, be.keys_to_result(keys, _capi.METRIC_IP)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        keys, (D, I) = step()
    barrier()
    be.timing_enable(True)
    from powermon import PowerMonitor  # board power / engine clock sampled in a background thread during the timed steps

    with PowerMonitor(index=dev_index, skip=0.15) as pmon:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            keys, (D, I) = step()
        barrier()
        dt = time.perf_counter() - t0
    power = pmon.summary()
    ktime = be.timing_read_full()
    ktot_ms, klaunches, kcalls = ktime["total_ms"], ktime["launches"], ktime["calls"]
    be.timing_enable(False)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if rehearsal else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    if rank == 0 and args.dump_outputs:
        dump_outputs(np, args.dump_outputs, D, I)

    # ---- sanity on the result (outside the timed region) ----
    planted_at_1 = float((I[:, 0] == planted).float().mean().item())

    if rank == 0:
        # 2*Q*N*d per step, N = rows of this rank's shard.  A step is ONE launch of the list kernel or - the
        # register-resident-queries kernels beyond 4 096 queries - one launch per chunk of up to 32 768 queries: the roofline
        # figure is (algorithmic flops of the launches) / (their summed durations) = flops per launch / average launch duration
        # with both averaged over the same launches; `kernel_ms` is the dominant kernel's time per STEP, `launches` per step
        flops_per_step = 2.0 * (q_hi - q_lo) * (hi - lo) * d
        kernel_ms = ktot_ms / max(1, kcalls)
        launches_per_step = klaunches / max(1, kcalls)
        flops_per_launch = flops_per_step / max(1.0, launches_per_step)
        achieved = flops_per_step / (kernel_ms * 1e-3) / 1e12
        alg_bytes = (hi - lo) * d * 2 + nq * d * 2 + nq * k * 12  # 8(d): every input once + outputs once
        traffic, traffic_src = pmc_traffic(n, nq, world)
        out = {
            "metric": "sem_sim_join queries/sec (d=768, k=10, exact top-k, recall vs CPU oracle)",
            "value": nq * args.steps / dt,
            "unit": "queries/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f16",
            "data": "synthetic" if not rehearsal else "synthetic; REHEARSAL: all ranks on one GPU over gloo - not a measurement",
            "config": {"workload": (f"sem_sim_join {nq} x {n} rows, d={d} fp16, k={k}, IP; corpus row-sharded over {world} "
                                    f"GPU(s) ({hi - lo} rows each), pooled sample thresholds + RCCL all-gather top-k merge; "
                                    "device-resident in/out") if split == "rows" else
                                   (f"sem_sim_join {nq} x {n} rows, d={d} fp16, k={k}, IP; QUERY split over {world} GPUs ({qper} queries "
                                    f"each against the whole corpus), one RCCL all-gather of the key lists; device-resident in/out"),
                       "split": split,
                       "inputs": f"benchdata.py SeedSequence([{benchdata.SEED},{benchdata.CFG_JOIN},block])"},
            "planted_neighbour_at_rank1": planted_at_1,
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP16_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP16_MFMA_TFLOPS, "traffic": traffic, "traffic_source": traffic_src,
                         "kernel": ktime["kernel"], "kernel_ms": kernel_ms, "kernel_ms_per_launch": ktot_ms / max(1, klaunches),
                         "launches": klaunches, "launches_per_step": launches_per_step,
                         "algorithmic_flops_per_launch": flops_per_launch, "algorithmic_bytes_per_launch": alg_bytes / max(1.0, launches_per_step),
                         "sclk_mhz": power.get("sclk_mhz"), "power_w": power.get("power_w"), "power_samples": power.get("samples"),
                         "power_source": power.get("source") or power.get("error"),
                         "gflop_per_joule": (flops_per_step * world / (dt / args.steps) / power["power_w"] / 1e9 / world
                                             if power.get("power_w") else None),
                         "csrc_sha": csrc_hash()},
        }
        details = {"gen_s": gen_s, "hbm_frac_secondary": alg_bytes / (kernel_ms * 1e-3) / 1e9 / PEAK_HBM_GBS}
        if args.full:  # checks, CPU baseline and legs: after the timed steps, never in a plain run
            n_chk = max(args.check_sample, args.cpu_sample if (world == 1 and not args.no_cpu_baseline) else 0, 1)
            D_h, I_h = D[:n_chk].cpu().numpy(), I[:n_chk].cpu().numpy()
            chk_rows = check_rows(np, nq, args.check_sample)
            chk_dev = torch.from_numpy(chk_rows).to(device)
            D_chk, I_chk = D[chk_dev].cpu().numpy(), I[chk_dev].cpu().numpy()
            checks = []  # CPU-side work deferred until every GPU leg has run
            legs = {}
            if legs_on:
                ctx = dict(np=np, torch=torch, be=be, _capi=_capi, xb_h=xb_h, xq_h=xq_h, corpus=corpus, queries=queries, k=k,
                           d=d, keys=keys, args=args)
                search_legs(ctx, legs)
                node_plan_legs(ctx, legs)
                world8_rehearsal(ctx, legs, checks)
                for fut in (fut_dedup, fut_km):  # the legs below have the HOST in their timed region (T_call stages host memory
                    if fut is not None:          # with a few threads; the certified fp32 search reads one count back per call): let
                        fut.result()             # the generators of the other configs' rows (up to 64 threads on a 16-CPU quota)
                fp32_leg(ctx, legs)              # finish first - with them running the fp32 10 k x 1 M call measured 18.4 instead
                t_call_leg(ctx, legs)            # of 16.1 ms, two runs on the same box
                t_op_leg(ctx, legs)
                if fut_dedup is not None:
                    dedup_leg(ctx, legs, checks, fut_dedup)
                if fut_km is not None:
                    kmeans_legs(ctx, legs, checks, fut_km)
            be.synchronize()
            # ---- CPU side ----
            if args.check_sample > 0:
                out.update(oracle_check(np, xb_h, xq_h, D_chk, I_chk, chk_rows, k))
            for fn in checks:
                fn()
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(np, xb_h, xq_h, args.cpu_sample, k, D_h, I_h)
            if legs.get("t_call_host_to_host"):
                # SURVEY.md 8(d) calls T_call - VS.__call__(host ndarray) -> host (D, I), corpus resident - "the queries/sec figure"; the
                # bench contract wants `value` device-resident.  Both are on the line's top level
                out["value_t_call"] = legs["t_call_host_to_host"]["queries_per_s"]
                out["value_t_call_note"] = "host ndarray in -> host (D, I) out through HipVS.__call__ (PCIe + packing included), median of 5"
            if legs:
                out["legs"] = legs
                out["legs_summary"] = legs_summary(out, legs)  # printed LAST: the tail of the line holds the figures that matter
        details["line"] = out
        print("BENCH_DETAILS " + json.dumps(sig(details, 7)), file=sys.stderr, flush=True)
        print(json.dumps(sig(compact(out))), flush=True)
    pool.shutdown(wait=False, cancel_futures=True)
    if world > 1:
        dist.barrier()
        if rank == 0 and shm_dir:
            import shutil

            shutil.rmtree(shm_dir, ignore_errors=True)
        dist.destroy_process_group()


def shared_inputs(np, dist, benchdata, world, rank, n, d, nq):
    """-> (corpus [n, d], queries [nq, d], planted [nq], shm dir or None), all host arrays.  The queries are planted on rows
    of every shard and a block's numpy stream cannot be entered in the middle, so SOMEBODY has to draw the whole corpus: at
    N > 1 rank 0 draws it once into /dev/shm and the other ranks map it (each touches only its own shard's pages and the
    queries) instead of N ranks repeating the same host work side by side.  Falls back to every rank drawing when /dev/shm
    cannot hold it."""
    def draw():
        xb = benchdata.corpus(benchdata.CFG_JOIN, n, d)
        xq, planted = benchdata.queries(benchdata.CFG_JOIN, xb, nq)
        return xb, xq, planted

    if world == 1:
        return (*draw(), None)
    shm = os.path.join("/dev/shm", f"lotus_bench_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}")
    flag = [0]
    got = None
    if rank == 0:
        try:
            os.makedirs(shm, exist_ok=True)
            if os.statvfs(shm).f_bavail * os.statvfs(shm).f_frsize < (n + nq) * d * 2 * 1.1:
                raise OSError("no room in /dev/shm")
            got = draw()
            for name, a in zip(("xb", "xq", "planted"), got):
                np.save(os.path.join(shm, name + ".npy"), a)
            flag[0] = 1
        except Exception:  # whatever went wrong on rank 0, the others must not wait for a file that will not come
            flag[0] = 0
    dist.broadcast_object_list(flag, src=0)  # also the barrier the readers wait at
    if not flag[0]:
        return (*(got if got is not None else draw()), None)
    if rank != 0:
        got = tuple(np.load(os.path.join(shm, name + ".npy"), mmap_mode="r") for name in ("xb", "xq", "planted"))
        got = (got[0], np.array(got[1]), np.array(got[2]))  # the corpus stays mapped (a rank touches its shard only); queries copied
    return (*got, shm)


def legs_summary(out, legs):
    """The numbers a reader looks for first, flat: fraction of the binding roof per BASELINE config / regime."""
    g = lambda name, key="frac": (legs.get(name) or {}).get(key)
    plan = (legs.get("node_plan_8gpu") or {}).get("splits", {})
    w8 = legs.get("world8_rehearsal") or {}
    km = legs.get("kmeans_parity_mode") or {}
    return {
        "cfg3_join_100k_x_1M_mfma_frac": out["roofline"]["frac"],
        "cfg2_10k_x_1M_mfma_frac": g("cfg2_10k_x_1M"),
        "q1_hbm_frac": g("q1"), "q64_hbm_frac": g("q64"), "q128_hbm_frac": g("q128"), "q256_hbm_frac": g("q256"),
        "q512_mfma_frac": g("q512"), "q1024_mfma_frac": g("q1024"), "q4096_mfma_frac": g("q4096"),
        "shard_100k_x_125k_mfma_frac": (plan.get("1x8") or {}).get("frac"),
        "split_8x1_12500_x_1M_mfma_frac": (plan.get("8x1") or {}).get("frac"),
        "world8_pooled_seeds_ms_per_shard": w8.get("kernel_ms_per_shard"),
        "world8_projected_node_qps": w8.get("projected_node_qps"),
        "t_call_ms": g("t_call_host_to_host", "ms_per_call"), "t_call_qps": g("t_call_host_to_host", "queries_per_s"),
        "t_op_ms": g("t_op_sem_sim_join_100k_x_1M", "ms_per_call"), "t_op_qps": g("t_op_sem_sim_join_100k_x_1M", "queries_per_s"),
        "cfg4_dedup_5M_mfma_frac": g("range_selfjoin_cfg4"),
        "cfg5_kmeans_iter_ms": g("kmeans_full_iter_10M_x_1024", "ms_per_iteration"),
        "cfg5_kmeans_iter_mfma_frac": g("kmeans_full_iter_10M_x_1024"),
        "kmeans_first_divergence_iteration": km.get("first_divergence_iteration"),
        "kmeans_all_flips_are_near_ties": km.get("all_flips_are_near_ties"),
        "fp32_10k_x_1M_ms": (legs.get("fp32_10k_x_1M") or {}).get("one_pass_ms"),
        "fp32_join_100k_x_1M_ms": g("fp32_join_100k_x_1M", "ms_per_call"),
    }


def pmc_traffic(n, nq, world):
    """HBM-side bytes per launch of the tile kernel from the committed rocprofv3 PMC passes of this same command
    (profiles/latest_pmc.json: FETCH_SIZE x 2 x 1024 per the gfx950 correction of MI355X_MICROARCH.md, + WRITE_SIZE x
    1024; separate --pmc runs, tools/pmc_summary.py).  Counters cannot be read from inside the timed process, so the
    figure is a committed measurement - and it is only reported when (i) the configuration is the one it was
    collected on (1 GPU, default sizes) and (ii) the kernel sources hash to the value stamped at collection time.
    -> (bytes or None, provenance string)."""
    try:
        with open(os.path.join(ROOT, "profiles", "latest_pmc.json")) as f:
            pmc = json.load(f)
    except Exception:
        return None, "no committed PMC summary"
    if not (world == 1 and n == 1_000_000 and nq == 100_000):
        return None, "PMC passes exist for the 1-GPU default configuration only"
    have, want = pmc.get("csrc_sha"), csrc_hash()
    if have != want:
        return None, f"profiles/latest_pmc.json was collected on csrc {have}, this build is {want}: stale, not reported"
    return pmc.get("traffic_bytes_per_launch"), f"profiles/latest_pmc.json ({pmc.get('tag', '?')}, csrc {have})"


def _near_tie_mismatches(np, Dr, Ir, Ig, k):
    """ids must match wherever the oracle's neighbouring scores are > 2e-5 apart (near-ties may swap)."""
    hard = 0
    for q, r in zip(*np.nonzero(Ir != Ig)):
        gaps = [abs(float(Dr[q, r]) - float(Dr[q, r - 1]))] if r > 0 else []
        gaps.append(abs(float(Dr[q, r]) - float(Dr[q, r + 1])) if r + 1 < k else 0.0)
        hard += min(gaps) > 2e-5
    return int(hard)


def _topk_vs_oracle(np, xb_h, xq_h, Dg, Ig, k, metric=0):
    import oracle

    Dr, Ir = oracle.flat_search(xb_h.astype(np.float32), xq_h.astype(np.float32), k, metric)
    inter = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(Ir, Ig))
    return {"recall_at_k": inter / float(Ir.size), "max_abs_score_err": float(np.abs(Dr - Dg).max()),
            "id_mismatches_outside_near_ties": _near_tie_mismatches(np, Dr, Ir, Ig, k)}


def oracle_check(np, xb_h, xq_h, Dg, Ig, rows, k):
    """The GPU result of the last timed step against the CPU oracle (oracle/flat.py: 4096 x 1024 sgemm blocks + k-best
    collector with faiss's tie rule) on the queries `rows` x the WHOLE corpus (the same fp16 values, upcast - SURVEY.md 8(c)).
    `rows`: the first queries of the batch AND one query of every 256-query tile of the launch, at a position that walks
    through the tile (tile t: row 256 t + 37 t mod 256) - every workgroup row of the launch, every wave and lane position is
    sampled, not just the head of the batch.  Dg / Ig hold the GPU rows in that order.  Runs at every N on rank 0."""
    res = _topk_vs_oracle(np, xb_h, xq_h[rows], Dg, Ig, k)
    res["oracle_check_queries"] = int(len(rows))
    res["oracle_check_rows"] = "first rows + one per 256-query tile (row 256 t + 37 t mod 256)"
    return res


def check_rows(np, nq, head):
    """Query rows of the oracle check: the first `head` rows, then one per 256-query tile (stratified, see oracle_check)."""
    t = np.arange(-(-nq // 256))
    strat = np.minimum(256 * t + (37 * t) % 256, nq - 1)
    return np.unique(np.concatenate([np.arange(min(head, nq)), strat]))


def _cpu_quota():
    """CPUs this process may use according to its cgroup (cpu.max), or None when unlimited / unknown."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if quota == "max" else float(quota) / float(period)
    except Exception:
        return None


def cpu_baseline(np, xb_h, xq_h, sample, k, Dg=None, Ig=None):
    """Time the CPU comparators on a bounded sample of the same workload - the first `sample` queries against the WHOLE
    corpus, all host cores: (a) faiss's BLAS search path (blocked sgemm + k-best collector) as one fused C + OpenMP loop
    nest with an AVX-512 micro-kernel (oracle/c/lvs_blas_twin.c) and (b) the same on torch-CPU (MKL sgemm + topk).  The
    FASTER one is the stated baseline.  kind = "port": real faiss-cpu is not installable here."""
    from oracle import blas_twin

    sample = min(sample, xq_h.shape[0])
    xb32 = xb_h.astype(np.float32)
    xq32 = xq_h[:sample].astype(np.float32)
    impls = []
    # If a faiss wheel is importable the reference's CPU path itself is timed - `faiss.IndexFlatIP` + `add` + `search`, exactly
    # what FaissVS does (lotus/vector_store/faiss_vs.py:14 METRIC_INNER_PRODUCT, :23-24 index_factory + add, :75 search) - and it IS
    # the stated baseline (kind "reference"), whatever the twins below measure.  No wheel exists in this image.
    faiss_impl = None
    try:
        import faiss  # noqa: F401

        def _faiss_search(xb, xq, kk):
            index = faiss.index_factory(int(xb.shape[1]), "Flat", faiss.METRIC_INNER_PRODUCT)
            index.add(np.ascontiguousarray(xb, dtype=np.float32))
            Df, If = index.search(np.ascontiguousarray(xq, dtype=np.float32), int(kk))
            return Df, If, int(faiss.omp_get_max_threads())

        faiss_impl = ("faiss-cpu index_factory('Flat', METRIC_INNER_PRODUCT).search - the reference's own CPU path (faiss_vs.py:23-24,75)",
                      _faiss_search)
        impls.append(faiss_impl)
    except ImportError:
        pass
    if blas_twin.c_available():
        impls.append(("oracle/c/lvs_blas_twin.c (C + OpenMP, AVX-512 sgemm micro-kernel fused with the k-best collector)",
                      blas_twin.flat_search_c))
    impls.append((f"oracle/blas_twin.py (torch-CPU: {blas_twin.QUERY_BLOCK} x {blas_twin.DB_BLOCK} MKL sgemm blocks + topk)",
                  blas_twin.flat_search_blas))
    # the C twin's best thread count is not the host's CPU count (GPU boxes of the pool, 2 x EPYC 9575F, 256 CPUs visible: 32
    # threads 3.3, 64 2.7, 128 1.75, 256 1.3 TFLOP/s - the rate FALLS with the thread count, as under a CPU quota or with the
    # packed blocks of SMT siblings sharing an L2): calibrate the thread count on a short sample and time the best one
    twin_threads = os.cpu_count() or 1
    if blas_twin.c_available():
        blas_twin.flat_search_c(xb32[:65536], xq32[:256], k)
        best_rate = 0.0
        cands = {max(1, (os.cpu_count() or 1) // dv) for dv in (1, 2, 4, 8, 16)}
        if _cpu_quota():  # a container may be allowed fewer CPUs than it can see: more threads than that only get throttled
            cands.add(max(1, int(_cpu_quota())))
        for th in sorted(cands):
            t0 = time.perf_counter()
            blas_twin.flat_search_c(xb32[:262144], xq32[:1024], k, threads=th)
            rate = 1.0 / (time.perf_counter() - t0)
            if rate > best_rate:
                best_rate, twin_threads = rate, th
    runs = []
    for impl, fn in impls:
        if fn is blas_twin.flat_search_c:
            fn = (lambda f, th: (lambda a, b, kk: f(a, b, kk, threads=th)))(fn, twin_threads)
        fn(xb32[:65536], xq32[:256], k)  # thread pool / page warm-up, not timed
        # a slower comparator gets a smaller sample (its rate is what is compared): keep the leg within ~30 s
        ns = sample if not runs else max(256, sample // 8)
        t0 = time.perf_counter()
        Dc, Ic, threads = fn(xb32, xq32[:ns], k)
        dt = time.perf_counter() - t0
        runs.append({"impl": impl, "queries": ns, "seconds": dt, "queries_per_s": ns / dt,
                     "gflops": 2.0 * ns * xb32.shape[0] * xb32.shape[1] / dt / 1e9, "threads": int(threads)})
        # the timed run's OUTPUT is a second, wider parity sample for free: the comparator restates the same faiss search
        # path as the oracle (tests/test_oracle.py holds it to the oracle), so the GPU result of the last timed step is
        # compared with it on every query it answered (8 192 by default, against the 512 of the numpy oracle's check)
        if Dg is not None and len(Dg) >= ns:
            Dc, Ic = np.asarray(Dc, np.float32), np.asarray(Ic, np.int64)
            inter = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(Ic, Ig[:ns]))
            runs[-1]["gpu_parity"] = {"queries": ns, "recall_at_k": inter / float(Ic.size),
                                      "max_abs_score_err": float(np.abs(Dc - Dg[:ns]).max()),
                                      "id_mismatches_outside_near_ties": _near_tie_mismatches(np, Dc, Ic, Ig[:ns], k)}
            # (recall counts a swap across the k-th boundary inside a near-tie - scores < 2e-5 apart, different summation
            # order - as a miss; such swaps are not id mismatches)
    best = max(runs, key=lambda r: r["queries_per_s"])
    if faiss_impl is not None:
        best = next(r for r in runs if r["impl"] == faiss_impl[0])
    quota = _cpu_quota()
    # cores = CPUs the timed comparator could actually occupy: its threads, capped by the container's cgroup quota
    cores = int(min(best["threads"], quota)) if quota else int(best["threads"])
    cores_note = (f"{best['threads']} threads under a cgroup quota of {quota:g} CPUs ({os.cpu_count()} visible)" if quota else
                  f"{best['threads']} threads, {os.cpu_count()} CPUs visible, no cgroup quota")
    short = ("faiss-cpu IndexFlatIP (the reference's dependency)" if faiss_impl is not None else
             "C+OpenMP AVX-512 sgemm+k-best twin" if "lvs_blas_twin.c" in best["impl"] else "torch-CPU MKL sgemm+topk")
    out = {"value": best["queries_per_s"], "unit": "queries/s", "cores": cores, "cores_note": cores_note,
           "kind": "reference" if faiss_impl is not None else "port",
           "sample": f"first {best['queries']} queries x full {xb32.shape[0]}-row corpus, {short}, {best['seconds']:.1f} s",
           "gflops": best["gflops"], "threads": best["threads"], "host_cpus": os.cpu_count(), "host_cpu_quota": quota,
           "comparators_timed": runs}
    if "gpu_parity" in best:
        out["gpu_parity_on_the_timed_sample"] = best["gpu_parity"]
    return out


# ======================================================================================================================
# secondary legs (N = 1): same process, same resident data
# ======================================================================================================================
def _kernel_leg(ctx, cb, cq, reps, kk=None, id_offset=0):
    """-> (kernel ms from the library's HIP events, wall ms per call, last keys)."""
    be, _capi = ctx["be"], ctx["_capi"]
    kk = ctx["k"] if kk is None else kk
    for _ in range(2):
        be.search_keys(cb, cq, kk, _capi.METRIC_IP, id_offset=id_offset)
    be.synchronize()
    be.timing_enable(True)
    wall = 1e9
    for _ in range(3 if reps >= 10 else 1):  # sub-millisecond calls: the fastest of three loops (the host also generates the
        t0 = time.perf_counter()             # other configs' rows in background threads while these legs run)
        for _ in range(reps):
            keys = be.search_keys(cb, cq, kk, _capi.METRIC_IP, id_offset=id_offset)
            be.keys_to_result(keys, _capi.METRIC_IP)
        be.synchronize()
        wall = min(wall, (time.perf_counter() - t0) / reps)
    tot, cnt = be.timing_read()
    be.timing_enable(False)
    return tot / max(cnt, 1), wall * 1e3, keys


def _mfma_leg(ctx, cb, cq, reps, **extra):
    kms, wms, _ = _kernel_leg(ctx, cb, cq, reps)
    fl = 2.0 * cq.n * cb.n * ctx["d"]
    leg = {"kernel_ms": kms, "ms_per_call": wms, "bound": "mfma", "frac": fl / (kms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS}
    leg.update(extra)
    return leg


def search_legs(ctx, legs):
    be, corpus, queries = ctx["be"], ctx["corpus"], ctx["queries"]
    # BASELINE configs[1]: 10k queries x 1M rows, MFMA-bound
    q10k = be.slice_rows(queries, 0, min(10_000, queries.n))
    leg = _mfma_leg(ctx, corpus, q10k, 5)
    leg["queries_per_s"] = q10k.n / (leg["ms_per_call"] * 1e-3)
    legs["cfg2_10k_x_1M"] = leg
    # the HBM-bound regime: the literal sem_search issues ONE query per call (sem_search.py:121-122); small sim-joins and the
    # K-doubling loop send a few dozen to a few hundred.  Every corpus byte exactly once = the algorithmic bytes (1.536 GB).
    by = corpus.n * int(corpus.rows.shape[1]) * 2.0
    for nq_small in (1, 32, 64, 96, 128, 192, 256):
        if nq_small > queries.n:
            continue
        qs = be.slice_rows(queries, 0, nq_small)
        kms, wms, _ = _kernel_leg(ctx, corpus, qs, 20)
        legs[f"q{nq_small}"] = {"kernel_ms": kms, "ms_per_call": wms, "bound": "hbm", "frac": by / (kms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                "mfma_frac_secondary": 2.0 * nq_small * corpus.n * ctx["d"] / (kms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS}
    # between the two regimes: a few query tiles x many corpus slabs - the list kernel with thresholds seeded from a sample
    for nq_mid in (512, 1024, 4096):
        if nq_mid <= queries.n:
            legs[f"q{nq_mid}"] = _mfma_leg(ctx, corpus, be.slice_rows(queries, 0, nq_mid), 10)


def node_plan_legs(ctx, legs):
    """What ONE of 8 GPUs does under every (query groups x corpus shards) split of the same 100k x 1M join, measured here
    on one GPU with the shard's OWN sample thresholds: gq x gc = 1 x 8 (BASELINE's row split), 2 x 4, 4 x 2, 8 x 1 (the query
    split).  The node's kernel-side ceiling is Q / (per-GPU kernel time); `HipVS(shard=(gq, gc))` runs any of them,
    `lotus_amd.plan.pick_split` chooses.  (world8_rehearsal runs the row split with the POOLED thresholds of all shards.)"""
    be, corpus, queries, d = ctx["be"], ctx["corpus"], ctx["queries"], ctx["d"]
    plan = {}
    for gq, gc in ((1, 8), (2, 4), (4, 2), (8, 1)):
        rows, qn = -(-corpus.n // gc), -(-queries.n // gq)
        leg = _mfma_leg(ctx, be.slice_rows(corpus, 0, rows), be.slice_rows(queries, 0, qn), 3 if rows * qn > 2e10 else 5)
        leg["shape"] = f"{qn}x{rows}"
        leg["node_qps_if_8_gpus"] = queries.n / (leg["kernel_ms"] * 1e-3)
        del leg["bound"]
        plan[f"{gq}x{gc}"] = leg
    best = max(plan, key=lambda s: plan[s]["node_qps_if_8_gpus"])
    legs["node_plan_8gpu"] = {"splits": plan, "best_split": best, "best_node_qps": plan[best]["node_qps_if_8_gpus"],
                              "mfma_floor_node_qps": 8 * PEAK_FP16_MFMA_TFLOPS * 1e12 / (2.0 * corpus.n * d),
                              "note": "kernel side only: the all-gathers and the merge come on top (world8_rehearsal)"}
    # the N = 2 / 4 shapes of the row split the driver's scaling run uses
    for rows, ng in ((500_000, 2), (250_000, 4)):
        if rows <= corpus.n:
            leg = _mfma_leg(ctx, be.slice_rows(corpus, 0, rows), queries, 3)
            leg[f"node_qps_if_{ng}_gpus"] = queries.n / (leg["kernel_ms"] * 1e-3)
            legs[f"shard_100k_x_{rows // 1000}k"] = leg


def world8_rehearsal(ctx, legs, checks):
    """The device-side half of the 8-GPU run at full size, on one GPU, exactly as bench.py's N = 8 step / HipVS(shard=True)
    run it: every shard scores its sample tiles (lvs_flat_search_seed_scores), the eight blocks are laid side by side as the
    all-gather would, all eight shards are searched in turn with those POOLED starting thresholds and their REAL id offsets,
    and the eight [Q, k] key lists are merged with lvs_merge_keys.  The merged result is compared with the single-launch
    result (bit for bit: keys are a total order) and with the CPU oracle.  The same eight searches with each shard's own
    sample thresholds are timed beside it."""
    np, torch, be, _capi = ctx["np"], ctx["torch"], ctx["be"], ctx["_capi"]
    corpus, queries, k = ctx["corpus"], ctx["queries"], ctx["k"]
    W = 8
    per = -(-corpus.n // W)
    bounds = [(min(corpus.n, r * per), min(corpus.n, (r + 1) * per)) for r in range(W)]
    shards = [be.slice_rows(corpus, lo, hi) for lo, hi in bounds]
    tiles = be.seed_tiles(queries.n, per, k, corpus.mode, queries.mode)

    def pooled():
        return torch.cat([be.seed_scores(sh, queries, _capi.METRIC_IP, tiles) for sh in shards]) if tiles else None

    def run(seeds):
        return torch.stack([be.search_keys(sh, queries, k, _capi.METRIC_IP, id_offset=lo, seed_scores=seeds)
                            for sh, (lo, _) in zip(shards, bounds)])

    res = {}
    for tag in ("own", "pooled"):
        run(pooled() if tag == "pooled" else None)
        be.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        seeds = pooled() if tag == "pooled" else None
        e1.record()
        be.timing_enable(True)
        parts = run(seeds)
        be.synchronize()
        ktot, kcnt = be.timing_read()
        be.timing_enable(False)
        res[tag] = (ktot / max(kcnt, 1), e0.elapsed_time(e1) / W, parts)
    shard_ms, seed_ms, parts = res["pooled"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    be.merge_keys(parts)
    e0.record()
    for _ in range(5):
        merged = be.merge_keys(parts)
    e1.record()
    be.synchronize()
    merge_ms = e0.elapsed_time(e1) / 5
    same = bool(torch.equal(merged, ctx["keys"]))
    same_own = bool(torch.equal(be.merge_keys(res["own"][2]), ctx["keys"]))
    D, I = be.keys_to_result(merged, _capi.METRIC_IP)
    sample = min(ctx["args"].check_sample, queries.n)
    D_h, I_h = D[:sample].cpu().numpy(), I[:sample].cpu().numpy()
    fl = 2.0 * queries.n * per * ctx["d"]
    leg = {"shards": W, "shard_rows": per, "seed_tiles_per_shard": tiles, "kernel_ms_per_shard": shard_ms,
           "frac": fl / (shard_ms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS, "seed_pass_ms_per_shard": seed_ms,
           "kernel_ms_per_shard_own_seeds": res["own"][0], "merge_ms": merge_ms,
           "merged_equals_single_gpu_keys": same, "own_seeds_merged_equals_single_gpu_keys": same_own,
           "short_lists_slots": int((parts == 0).sum().item()),
           "ids_from_every_shard": int(torch.unique(I // per).numel()),
           "projected_node_qps": queries.n / ((shard_ms + seed_ms + merge_ms) * 1e-3),
           "note": "projection = Q / (sample pass + per-shard kernel + 8-way merge); the two all-gathers over xGMI (4 MB of "
                   "sample scores and 8 MB of keys per rank) are not in it"}
    legs["world8_rehearsal"] = leg
    if sample > 0:
        checks.append(lambda: leg.update({"oracle_" + a: b for a, b in
                                          _topk_vs_oracle(np, ctx["xb_h"], ctx["xq_h"][:sample], D_h, I_h, k).items()}))


def fp32_leg(ctx, legs):
    """LOTUS's default storage: fp32 embeddings (fp16 hi|lo pairs on the device).  10k queries x the same 1M rows, plain
    search (three K segments) vs the certified one-pass search (same exact result)."""
    np, torch, be, _capi, d, k = ctx["np"], ctx["torch"], ctx["be"], ctx["_capi"], ctx["d"], ctx["k"]
    dev = ctx["corpus"].rows.device
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    xb = torch.from_numpy(ctx["xb_h"]).to(dev).float()
    xb += 1e-4 * torch.randn(xb.shape, generator=g, device=dev)  # values that are NOT fp16-representable
    c32 = be.pack(torch.nn.functional.normalize(xb, dim=1), _capi.PACK_SPLIT)
    del xb
    xq = torch.from_numpy(ctx["xq_h"][:10_000]).to(dev).float()
    xq += 1e-4 * torch.randn(xq.shape, generator=g, device=dev)
    q32 = be.pack(torch.nn.functional.normalize(xq, dim=1), _capi.PACK_SPLIT)
    res32, got = {}, {}
    for tag, one_pass in (("plain_3seg", False), ("one_pass", True)):
        stats = {}
        for _ in range(2):
            be.search_keys(c32, q32, k, _capi.METRIC_IP, one_pass=one_pass)
        be.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            got[tag] = be.search_keys(c32, q32, k, _capi.METRIC_IP, one_pass=one_pass, stats=stats)
        be.synchronize()
        res32[tag + "_ms"] = (time.perf_counter() - t0) / 3 * 1e3
        if one_pass:
            res32["uncertified_fraction"] = stats["uncertified"] / max(1, stats["queries"])
            res32["plain_search_fraction"] = stats.get("plain", 0) / max(1, stats["queries"])  # still open after the 56-deep round
    _, Ia = be.keys_to_result(got["plain_3seg"], _capi.METRIC_IP)
    _, Ib = be.keys_to_result(got["one_pass"], _capi.METRIC_IP)
    res32["one_pass_ids_equal_plain"] = float((Ia == Ib).float().mean().item())
    res32["fp16_same_shape_ms"] = (legs.get("cfg2_10k_x_1M") or {}).get("ms_per_call")
    legs["fp32_10k_x_1M"] = res32
    # the headline join with LOTUS's default storage on both sides (faiss_vs.py:24): 100 k fp32 queries x 1 M fp32 rows
    xq = torch.from_numpy(ctx["xq_h"]).to(dev).float()
    xq += 1e-4 * torch.randn(xq.shape, generator=g, device=dev)
    q32 = be.pack(torch.nn.functional.normalize(xq, dim=1), _capi.PACK_SPLIT)
    del xq
    stats = {}
    be.search_keys(c32, q32, k, _capi.METRIC_IP)
    be.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        be.search_keys(c32, q32, k, _capi.METRIC_IP, stats=stats)
    be.synchronize()
    ms = (time.perf_counter() - t0) / 2 * 1e3
    legs["fp32_join_100k_x_1M"] = {"ms_per_call": ms, "queries_per_s": q32.n / (ms * 1e-3), "bound": "mfma",
                                   "frac": 2.0 * q32.n * c32.n * d / (ms * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS,
                                   "uncertified_fraction": stats["uncertified"] / max(1, stats["queries"]),
                                   "plain_search_fraction": stats.get("plain", 0) / max(1, stats["queries"]),
                                   "note": "fp32 embeddings as fp16 hi|lo rows, exact (fp32-accurate) top-k through the certified "
                                           "one-pass search; frac counts 2 Q N d once, as for fp16 storage"}


def t_call_leg(ctx, legs):
    """T_call: VS.__call__(host ndarray) -> host (D, I), corpus resident; includes packing the queries,
    the H2D copy of 154 MB and the D2H copy of the results.  Reported beside `value`, never as `value`: the bench contract
    times device-resident inputs."""
    from lotus_amd.vs import HipVS, _Resident

    be, corpus, xq_h, k, d = ctx["be"], ctx["corpus"], ctx["xq_h"], ctx["k"], ctx["d"]
    vs = HipVS(backend=be, storage="fp16")
    vs._resident["bench"] = _Resident(vecs=None, packed=corpus, n=corpus.n, d=d, lo=0, hi=corpus.n)
    vs.index_dir = "bench"
    vs(xq_h[:1000], k)
    vs(xq_h, k)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = vs(xq_h, k)
        ts.append(time.perf_counter() - t0)
    tcall = sorted(ts)[len(ts) // 2]
    assert out.indices.shape == (xq_h.shape[0], k)
    same = bool((ctx["torch"].from_numpy(out.indices[:4096]).to(ctx["keys"].device) ==
                 be.keys_to_result(ctx["keys"][:4096], ctx["_capi"].METRIC_IP)[1]).all().item())
    legs["t_call_host_to_host"] = {"ms_per_call": tcall * 1e3, "queries_per_s": xq_h.shape[0] / tcall,
                                   "same_ids_as_the_timed_step": same,
                                   "note": "HipVS.__call__(numpy fp16 [Q,d]) -> numpy (D, I); PCIe and packing included; "
                                           "median of 5"}


def t_op_leg(ctx, legs):
    """T_op (the third timing boundary): the whole operator, frames in, frame out -
    `lotus_amd.ops.sem_sim_join(left, right, ...)` = what `df1.sem_sim_join(df2, ...)` (sem_sim_join.py:84-166) does around the
    search: query vectors from the retriever model, VS.__call__ with the right frame's index labels as ids, the post-filter and
    the joined frame with its `_scores` column (1 M result rows).  The retriever model hands the precomputed embeddings over
    (the embedding model itself is outside the path)."""
    import pandas as pd

    from lotus_amd import ops
    from lotus_amd.vs import HipVS, _Resident

    np, be, corpus, xq_h, k, d = ctx["np"], ctx["be"], ctx["corpus"], ctx["xq_h"], ctx["k"], ctx["d"]

    class PassRM:  # RM.convert_query_to_query_vector (models/rm.py:77-78) passes ndarrays through; so does this stand-in
        def convert_query_to_query_vector(self, q):
            return xq_h

    vs = HipVS(backend=be, storage="fp16")
    vs._resident["bench"] = _Resident(vecs=None, packed=corpus, n=corpus.n, d=d, lo=0, hi=corpus.n)
    vs.index_dir = "bench"
    right = pd.DataFrame({"R": np.arange(corpus.n)})
    right.attrs["index_dirs"] = {"R": "bench"}
    left = pd.DataFrame({"L": np.arange(xq_h.shape[0])})
    run = lambda: ops.sem_sim_join(left, right, "L", "R", k, rm=PassRM(), vs=vs)
    out = run()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = run()
        ts.append(time.perf_counter() - t0)
    t_op = sorted(ts)[1]
    want_I = be.keys_to_result(ctx["keys"][:4096], ctx["_capi"].METRIC_IP)[1].cpu().numpy()
    got_I = out["R"].to_numpy()[:4096 * k].reshape(4096, k)
    legs["t_op_sem_sim_join_100k_x_1M"] = {
        "ms_per_call": t_op * 1e3, "queries_per_s": xq_h.shape[0] / t_op, "result_rows": int(len(out)),
        "columns": list(out.columns), "same_ids_as_the_timed_step": bool(np.array_equal(want_I, got_I)),
        "note": "lotus_amd.ops.sem_sim_join(left frame, right frame) -> joined frame, host in / host out; median of 3"}


def dedup_leg(ctx, legs, checks, fut):
    """BASELINE configs[3]: threshold self-join (sem_dedup.py:45-46 without the N^2 result), tau = 0.95 strict, on rows with
    planted near-duplicates, chains and hard negatives.  In-run checks: the pair SET against the planted structure (float32
    cosines of the stored values on the host; pairs within 2e-5 of tau may go either way) and, for a sample of query rows,
    against a brute-force float32 scan of ALL rows."""
    np, be, _capi, d = ctx["np"], ctx["be"], ctx["_capi"], ctx["d"]
    import benchdata
    from lotus_amd.dedup import threshold_pairs

    x_h, plants = fut.result()
    n = x_h.shape[0]
    tau = 0.95
    pk = be.pack(x_h, _capi.PACK_F16)
    be.synchronize()
    be.timing_enable(True)
    t0 = time.perf_counter()
    i, j, s = threshold_pairs(be, pk, tau)
    be.synchronize()
    dt = time.perf_counter() - t0
    ktot, kcnt = be.timing_read()
    be.timing_enable(False)
    del pk
    leg = {"rows": n, "threshold": tau, "seconds": dt, "kernel_seconds": ktot * 1e-3, "kernel_launches": kcnt,
           "pairs": int(len(i)), "bound": "mfma", "algorithmic_flops": 1.0 * n * n * d,
           "frac": n * n * d / (ktot * 1e-3) / 1e12 / PEAK_FP16_MFMA_TFLOPS,
           "note": "algorithmic flops = N^2 d (each unordered pair once; only the upper triangle is computed); "
                   "kernel_seconds = sum of the tile kernel's launches (HIP events)"}
    legs["range_selfjoin_cfg4"] = leg

    def check():
        sure, maybe = benchdata.dedup_expected_pairs(x_h, plants, tau)
        got = set(zip(i.tolist(), j.tolist()))
        missing = sure - got
        extra = got - sure - maybe
        # an "extra" pair is only wrong if its float32 cosine is not above the band either (e.g. two unrelated rows)
        bad_extra = 0
        for a, b in list(extra)[:10000]:
            c = float(np.dot(x_h[a].astype(np.float32), x_h[b].astype(np.float32)))
            bad_extra += not (c > tau - 2e-5)
        leg.update({"expected_pairs": len(sure), "expected_in_band": len(maybe), "missing_pairs": len(missing),
                    "unplanted_pairs": len(extra), "wrong_pairs": int(bad_extra)})
        # brute-force band check on a sample of query rows x ALL rows
        rng = np.random.default_rng(5)
        rows = np.unique(np.concatenate([rng.integers(0, n, 192), plants["src"][:32], plants["row"][-32:]]))
        xs = x_h[rows].astype(np.float32)
        by_row = {}
        for a, b in zip(i.tolist(), j.tolist()):
            by_row.setdefault(a, set()).add(b)
            by_row.setdefault(b, set()).add(a)
        wrong = 0
        for c0 in range(0, n, 262144):
            sc = xs @ x_h[c0:c0 + 262144].astype(np.float32).T
            r, c = np.nonzero(sc > tau - 2e-5)
            for rr, cc in zip(r.tolist(), c.tolist()):
                a, b = int(rows[rr]), c0 + cc
                if a == b:
                    continue
                have = b in by_row.get(a, ())
                if sc[rr, cc] > tau + 2e-5 and not have:
                    wrong += 1
            # pairs the GPU reported for these rows must be above the band's lower edge
            for rr, a in enumerate(rows.tolist()):
                for b in by_row.get(a, ()):
                    if c0 <= b < c0 + 262144 and not sc[rr, b - c0] > tau - 2e-5:
                        wrong += 1
        leg.update({"brute_force_sample_rows": int(len(rows)), "brute_force_sample_mismatches": int(wrong)})

    checks.append(check)


def kmeans_legs(ctx, legs, checks, fut):
    """BASELINE configs[4]: k-means K = 1024 on 10 M rows, d = 768 (fp16 points, fp32-accurate centroids).
    (i) full-data mode: every row every iteration (what BASELINE's wording implies) - per-iteration time from the slope
    between runs of different lengths; (ii) faiss-parity mode: what the reference does (utils.py:61-65): faiss subsamples
    K * 256 = 262 144 training rows, 20 iterations, then assigns all rows.  In-run checks: train ids and the trajectory of
    (ii) against oracle.kmeans_faiss on the same rows, iteration by iteration (identical assignments and bit-identical
    centroids up to the first differing iteration, whose differing rows must all be near-ties), and the final assignment of
    a row sample against a brute-force float32 nearest-centroid search."""
    np, be, _capi, d, args = ctx["np"], ctx["be"], ctx["_capi"], ctx["d"], ctx["args"]
    from lotus_amd.cluster import kmeans

    x_h, labels = fut.result()
    n, K = x_h.shape[0], args.kmeans_k
    pk = be.pack(x_h, _capi.PACK_F16)
    kmeans(None, K, niter=1, backend=be, packed=pk)  # first use of the k-means kernels: code-object load, allocator growth
    be.synchronize()
    # (ii) parity mode
    t0 = time.perf_counter()
    r = kmeans(None, K, niter=20, backend=be, packed=pk)
    be.synchronize()
    t_par = time.perf_counter() - t0
    par = {"rows": n, "k": K, "train_rows": int(len(r.train_ids)), "niter": 20, "seconds": t_par,
           "objective_first_last": [float(r.obj[0]), float(r.obj[-1])], "empty_clusters_reseeded": int(r.nsplit.sum()),
           "blob_purity": _purity(np, r.assign, labels, K)}
    legs["kmeans_parity_mode"] = par
    # the first iterations once more with every iteration's centroids and assignment kept (same run: the loop is deterministic)
    NIT_CMP = 6
    tr = []
    rt = kmeans(None, K, niter=NIT_CMP, backend=be, packed=pk, final_assign=False, trace=tr)
    tr_host = [{"centroids": t["centroids"].cpu().numpy(),
                "assign": be.keys_to_result(t["keys"], _capi.METRIC_L2)[1].reshape(-1).cpu().numpy()} for t in tr]
    del tr
    # (i) full-data mode, exhaustive: every row searched every iteration.  Slope between niter = 2 and niter = 6 (set-up -
    # the init permutation, centroid unpack - cancels)
    kw = dict(backend=be, packed=pk, max_points_per_centroid=None, final_assign=False)
    ts = {}
    stats = {}
    # every iteration timed on its own (events on the launch stream, incl. the one host round trip an iteration has); three
    # runs of 10 iterations, per iteration the fastest of the three, `ms_per_iteration` = their mean.  (Round 3 took the slope
    # between a 2- and a 6-iteration run: a 2-iteration run's set-up varies by tens of ms between runs, and so did the slope.)
    its = None
    for _ in range(3):
        st_run = {"time_iterations": True}
        be.synchronize()
        t0 = time.perf_counter()
        rf = kmeans(None, K, niter=10, stats=st_run, bounds=False, **kw)
        be.synchronize()
        ts[10] = min(ts.get(10, 1e9), time.perf_counter() - t0)
        its = st_run["iteration_ms"] if its is None else [min(a, b) for a, b in zip(its, st_run["iteration_ms"])]
        stats = st_run
    per_iter = sum(its) / len(its) * 1e-3
    fl = 2.0 * n * K * d
    legs["kmeans_full_iter_10M_x_1024"] = {
        "rows": n, "k": K, "ms_per_iteration": per_iter * 1e3, "bound": "mfma", "algorithmic_flops_per_iteration": fl,
        "frac": fl / per_iter / 1e12 / PEAK_FP16_MFMA_TFLOPS,
        "uncertified_fraction": stats.get("uncertified", 0) / max(1, stats.get("queries", 0)),
        "objective_decreasing": bool(np.all(np.diff(rf.obj) <= 1e-6 * np.abs(rf.obj[:-1]))),
        "pair_fraction": stats.get("pairs", 0) / max(1, stats.get("queries", 0)),
        "iteration_ms": [round(v, 2) for v in its], "seconds_10_iterations_incl_setup": ts[10],
        "objective": [float(v) for v in rf.obj],
        "note": "EXHAUSTIVE: all rows searched every iteration (bounds off): certified one-pass assignment (fp16 points x "
                "fp32-accurate centroids, lvs_nearest3) + two exact dot products for the rows only two centroids can win + exact "
                "re-search of the rest + in-row-order centroid sums + update; mean of ten iterations, each timed by device events"}
    # (i') the same 20 iterations with exact distance bounds (Hamerly): rows whose nearest centroid provably did not change
    # are not searched again - identical objectives (checked against the exhaustive run above), far less work once the
    # centroids settle.  NOT comparable with a roofline (work is skipped): reported as wall time and searched rows
    st2 = {}
    be.synchronize()
    t0 = time.perf_counter()
    rb = kmeans(None, K, niter=20, stats=st2, bounds=True, **kw)
    be.synchronize()
    t_b = time.perf_counter() - t0
    legs["kmeans_bounds_20_iters"] = {
        "rows": n, "k": K, "seconds": t_b, "ms_per_iteration_mean": t_b / 20 * 1e3,
        "searched_row_fraction_per_iteration": [round(v / n, 4) for v in st2.get("searched_rows", [])],
        "searched_row_fraction_mean": float(np.mean(st2.get("searched_rows", [n]))) / n,
        "first_objectives_equal_exhaustive": bool(np.array_equal(rb.obj[:10], rf.obj[:10])),
        "objective_last": float(rb.obj[-1]), "empty_clusters_reseeded": int(rb.nsplit.sum()),
        "note": "Hamerly distance bounds (lvs_kmeans_bounds_step): same assignments, sums, centroids and objectives as the "
                "exhaustive iteration; the sums still read every row every iteration"}
    del pk

    def check():
        import oracle

        # (a) the final assignment of the 10 M rows is exact against the run's OWN centroids (brute-force float32 scan of a
        # row sample) - whatever path the training took
        t0 = time.perf_counter()
        rng = np.random.default_rng(11)
        rows = rng.integers(0, n, 65536)
        _, Ir = oracle.flat_search(r.centroids, x_h[rows].astype(np.float32), 1, 1)
        par["final_assign_agreement_sample"] = float((Ir[:, 0] == r.assign[rows]).mean())
        # (b) the training trajectory against oracle.kmeans_faiss on the same 262 144 rows, iteration by iteration.  Lloyd's
        # iteration at K = 1024 is chaotic (one row flipping on a float32 near-tie moves two centroids, and on blob data can
        # shift faiss's split_clusters RNG walk), so what is required is: identical assignments, bit-identical centroids,
        # equal split counts and objectives up to the first iteration in which any row differs - and THERE every differing
        # row must be a near-tie (its two candidate distances within 2e-5 relative in the oracle's arithmetic)
        want_ids = oracle.rand_perm(n, 1234)[:K * 256] if n > K * 256 else np.arange(n)
        par["train_ids_equal_oracle"] = bool(np.array_equal(r.train_ids, want_ids))
        try:
            from threadpoolctl import threadpool_limits
            lim = threadpool_limits(limits=min(64, os.cpu_count() or 1))
        except Exception:
            lim = None
        trace = []
        xt32 = x_h[r.train_ids].astype(np.float32)
        ref = oracle.kmeans_faiss(xt32, K, niter=NIT_CMP, final_assign=False, trace=trace, max_points_per_centroid=1 << 30)
        if lim is not None:
            lim.restore_original_limits()
        par["oracle_iterations"] = NIT_CMP
        par["split_counts"] = [int(v) for v in rt.nsplit[:NIT_CMP]]
        par["oracle_split_counts"] = [int(v) for v in ref.nsplit]
        first, flips, near, gap, same_c, obj_err = None, 0, True, 0.0, True, 0.0
        for it in range(NIT_CMP):
            same_c &= bool(np.array_equal(tr_host[it]["centroids"], trace[it]["centroids"]))
            obj_err = max(obj_err, abs(float(rt.obj[it]) / float(ref.obj[it]) - 1))
            fl_ = oracle.flipped_rows(xt32, trace[it]["centroids"], tr_host[it]["assign"], trace[it]["assign"])
            if len(fl_["rows"]):
                first, flips, near, gap = it, int(len(fl_["rows"])), bool(fl_["all_near_ties"]), float(fl_["gaps"].max())
                break
        par.update({"first_divergence_iteration": first, "flipped_rows": flips, "all_flips_are_near_ties": near,
                    "max_flip_rel_gap": gap, "centroids_bit_identical_until_divergence": same_c,
                    "objective_max_rel_err_until_divergence": obj_err, "oracle_seconds": time.perf_counter() - t0})

    checks.append(check)


def _purity(np, assign, labels, K):
    """Fraction of rows whose cluster's majority blob is their own blob."""
    m = np.zeros((K, int(labels.max()) + 1), np.int64)
    np.add.at(m, (assign, labels), 1)
    return float(m.max(axis=1).sum() / len(assign))


if __name__ == "__main__":
    main()
