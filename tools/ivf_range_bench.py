"""The threshold self-join through the lists (dedup.threshold_pairs_ivf, lvs_ivf_range_kernel) against the exact join
(dedup.threshold_pairs, the path of sem_dedup()) on one MI355X: --n rows x --d, fp16, planted as benchdata's dedup config
plants them, store "IVF<--nlist>,Flat", threshold --tau.

Every path - exact, then nprobe in --nprobe - is warmed once; then --reps rounds run in one process, each round timing one
call of every path in turn, so that the paths alternate and drift of the box falls on all of them alike:
  * call_ms: host clock around the whole call - it ends with the sorted pair arrays on the host - median of the rounds, with
    the fastest and slowest round beside it (call_ms_min / call_ms_max);
  * kernel_ms: the library's HIP events around the dominant kernel's launches (lvs_timing_read_calls), summed over one call;
    median, fastest and slowest round likewise; the coarse step, the pair grouping and the host's canonicalisation are in
    call_ms only;
  * pairs: pairs returned; recall: share of the exact join's pairs among them (every returned pair is a pair of the exact
    join up to the 2e-5 band around the threshold; `extra` counts those that are not);
  * pairs_scored: (query, row) scores computed - the rows of every row's probed lists - and its share of the exact join's
    n (n - 1) / 2;
  * mfma_share: 2 d flop per scored pair over the fp16 MFMA peak, over kernel time;
  * hbm_share_requested: the bytes the kernel asks for - every work item (a list x a tile of 32 probing rows, cut per
    in-call chunk of 16 384 queries) reads its whole list, plus each query row once per probe - over the HBM peak, over
    kernel time.  Lists re-read by neighbouring tiles are served by L2 / MALL where they still are, so this is requested,
    not measured, traffic.
Prints one JSON document (and writes it to --out); `python tools/ivf_range_bench.py > profiles/ivf_range_bench.log`."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS, PEAK_BPS = 2.5e15, 8e12
IN_CALL_CHUNK = 16384  # IVF_CHUNK_MAX (lotus_amd/csrc/lvs_ivf_plan.h): queries per chunk inside lvs_ivf_range_search (the tiles are cut per chunk)


def timed_rounds(be, paths, reps):
    """paths: {name: callable} -> ({name: last result}, {name: timings}); one call of every path per round."""
    out = {name: fn() for name, fn in paths.items()}  # warm-up: code objects, the workspace, the pair buffers
    walls, kerns, info = {n: [] for n in paths}, {n: [] for n in paths}, {}
    for _ in range(reps):
        for name, fn in paths.items():
            be.synchronize()
            be.timing_enable(True)  # resets the totals: one call per reading
            t0 = time.perf_counter()
            out[name] = fn()
            walls[name].append((time.perf_counter() - t0) * 1e3)
            t = be.timing_read_full()
            be.timing_enable(False)
            kerns[name].append(t["total_ms"])
            info[name] = {"launches_per_call": t["launches"], "kernel": t["kernel"]}
    res = {}
    for name in paths:
        w, k = np.asarray(walls[name]), np.asarray(kerns[name])
        res[name] = {"call_ms": float(np.median(w)), "call_ms_min": float(w.min()), "call_ms_max": float(w.max()),
                     "kernel_ms": float(np.median(k)), "kernel_ms_min": float(k.min()), "kernel_ms_max": float(k.max()), **info[name]}
    return out, res


def scan_work(probe, sizes, d):
    """(scores computed, bytes asked for) of a self-join whose row i probes the lists probe[i]."""
    scored = int(sizes[probe].sum())
    nbytes = probe.size * d * 2  # every pair's query row into LDS
    for c0 in range(0, probe.shape[0], IN_CALL_CHUNK):
        cnt = np.bincount(probe[c0:c0 + IN_CALL_CHUNK].reshape(-1), minlength=len(sizes))
        nbytes += int((-(-cnt // 32) * sizes).sum()) * d * 2
    return scored, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--tau", type=float, default=0.95)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import benchdata
    from lotus_amd import HipVS, dedup

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    res = {"n": a.n, "d": a.d, "nlist": a.nlist, "tau": a.tau, "storage": "fp16", "device": torch.cuda.get_device_name(0)}
    t0 = time.perf_counter()
    x, _ = benchdata.dedup_rows(benchdata.CFG_DEDUP, a.n, a.d, dtype=np.float16)
    res["gen_s"] = time.perf_counter() - t0
    vs = HipVS(storage="fp16", device="cuda:0", factory_string=f"IVF{a.nlist},Flat")
    t0 = time.perf_counter()
    vs.index(None, x, "range-bench", persist=False)
    torch.cuda.synchronize()
    res["build_s"] = time.perf_counter() - t0
    be = vs.backend
    packed = vs.packed_rows()

    paths = {"exact": lambda: dedup.threshold_pairs(be, packed, a.tau)}
    for p in a.nprobe:
        paths[f"nprobe{p}"] = lambda p=p: dedup.threshold_pairs_ivf(vs, a.tau, nprobe=p)
    outs, times = timed_rounds(be, paths, a.reps)
    res["reps"] = a.reps
    ref = outs["exact"]
    res["exact"] = times["exact"]
    res["exact"]["pairs"] = int(len(ref[0]))
    res["exact"]["pairs_scored"] = a.n * (a.n - 1) // 2
    res["exact"]["mfma_share"] = 2.0 * a.d * res["exact"]["pairs_scored"] / PEAK_FLOPS / (res["exact"]["kernel_ms"] * 1e-3)
    ref_codes = ref[0] * a.n + ref[1]

    _, off, _ = vs.ivf_lists()
    sizes = np.diff(off)
    res["list_rows"] = {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max())}
    probe = vs.ivf_probe(x, max(a.nprobe))  # best first: the first p columns are the probes at nprobe = p
    for p in a.nprobe:
        got, r = outs[f"nprobe{p}"], times[f"nprobe{p}"]
        codes = got[0] * a.n + got[1]
        r["pairs"] = int(len(codes))
        r["recall"] = float(np.isin(ref_codes, codes).mean()) if len(ref_codes) else 1.0
        r["extra"] = int((~np.isin(codes, ref_codes)).sum())
        scored, nbytes = scan_work(probe[:, :p], sizes, a.d)
        r["pairs_scored"] = scored
        r["pairs_scored_share"] = scored / res["exact"]["pairs_scored"]
        r["mfma_share"] = 2.0 * a.d * scored / PEAK_FLOPS / (r["kernel_ms"] * 1e-3)
        r["hbm_share_requested"] = nbytes / PEAK_BPS / (r["kernel_ms"] * 1e-3)
        r["speedup_call"] = res["exact"]["call_ms"] / r["call_ms"]
        r["speedup_kernel"] = res["exact"]["kernel_ms"] / r["kernel_ms"]
        res[f"nprobe{p}"] = r
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
