"""IVF-Flat against the exact path on one MI355X: 1 M x 768 fp16 rows, nlist 4 096, nprobe in {8, 32, 128}.

Per nprobe and for 1 and 10 000 queries (k = 10):
  * wall ms per call: host clock around a call that ends with the results on the host (so it includes the copies and the
    launch gaps), median of the timed calls;
  * kernel ms per call: lvs_timing_read_calls (HIP events around the dominant kernel: lvs_ivf_scan_kernel for IVF, the
    flat path's search kernel for exact);
  * the scan kernel's HBM share (1 query: bytes of the probed lists' rows over 8 TB/s, over kernel time) and MFMA share
    (10 000 queries: 2 x sum over (query, probed row) x d over 2.5 PFLOP/s, over kernel time);
  * recall@10 against the exact search on benchdata's configs[2] rows (uniform: the worst case for IVF) and on a seeded
    clustered set (benchdata.blobs).
Prints one JSON document (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8e12
MFMA_FLOPS = 2.5e15


def timed(vs, q, k, reps, warmup, **kw):
    be = vs.backend
    for _ in range(warmup):
        vs(q, k, **kw)
    be.synchronize()
    be.timing_enable(True)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        vs(q, k, **kw)
        walls.append((time.perf_counter() - t0) * 1e3)
    t = be.timing_read_full()
    be.timing_enable(False)
    return {"wall_ms": float(np.median(walls)), "kernel_ms": t["total_ms"] / max(1, t["calls"]), "kernel": t["kernel"]}


def probed_rows(vs, q, nprobe):
    """(sum over queries of the rows of their probed lists, rows of the union over all queries)."""
    _, off, _ = vs.ivf_lists()
    sizes = np.diff(off)
    probe = vs.ivf_probe(q, nprobe)
    return int(sizes[probe].sum()), int(sizes[np.unique(probe)].sum())


def recall(ivf, exact, q, k, nprobe):
    a = ivf(q, k, nprobe=nprobe).indices
    b = exact(q, k).indices
    return float(np.mean([len(set(x) & set(y)) / k for x, y in zip(a, b)]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--big", type=int, default=10_000)
    ap.add_argument("--reps1", type=int, default=50)
    ap.add_argument("--repsbig", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--skip-clustered", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import benchdata
    from lotus_amd import HipVS

    if not torch.cuda.is_available():
        raise SystemExit("ivf_bench needs a GPU")
    k = 10
    res = {"n": a.n, "d": a.d, "nlist": a.nlist, "k": k, "storage": "fp16", "device": torch.cuda.get_device_name(0)}
    xb = benchdata.corpus(benchdata.CFG_SEARCH, a.n, a.d)
    xq, _ = benchdata.queries(benchdata.CFG_SEARCH, xb, a.big)
    exact = HipVS(storage="fp16", device="cuda:0")
    exact.index(None, xb, "bench-exact", persist=False)
    ivf = HipVS(storage="fp16", device="cuda:0", factory_string=f"IVF{a.nlist},Flat")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ivf.index(None, xb, "bench-ivf", persist=False)
    torch.cuda.synchronize()
    res["build_s"] = time.perf_counter() - t0
    _, off, _ = ivf.ivf_lists()
    sizes = np.diff(off)
    res["list_rows"] = {"min": int(sizes.min()), "median": float(np.median(sizes)), "max": int(sizes.max()),
                        "empty": int((sizes == 0).sum())}
    q1, qb = xq[:1], xq[:a.big]
    res["exact"] = {"q1": timed(exact, q1, k, a.reps1, 5), f"q{a.big}": timed(exact, qb, k, a.repsbig, 1)}
    row_bytes = a.d * 2
    res["ivf"] = {}
    for nprobe in a.nprobe:
        r = {"q1": timed(ivf, q1, k, a.reps1, 5, nprobe=nprobe), f"q{a.big}": timed(ivf, qb, k, a.repsbig, 1, nprobe=nprobe)}
        rows1, _ = probed_rows(ivf, q1, nprobe)
        pairs, union = probed_rows(ivf, qb, nprobe)
        r["q1"]["probed_rows"] = rows1
        r["q1"]["hbm_share"] = rows1 * row_bytes / HBM_BPS / (r["q1"]["kernel_ms"] * 1e-3)
        r[f"q{a.big}"]["query_row_pairs"] = pairs
        r[f"q{a.big}"]["union_rows"] = union
        r[f"q{a.big}"]["mfma_share"] = 2.0 * pairs * a.d / MFMA_FLOPS / (r[f"q{a.big}"]["kernel_ms"] * 1e-3)
        r["recall10_uniform"] = recall(ivf, exact, xq[:a.recall_queries], k, nprobe)
        r["speedup_q1_kernel"] = res["exact"]["q1"]["kernel_ms"] / r["q1"]["kernel_ms"]
        r[f"speedup_q{a.big}_kernel"] = res["exact"][f"q{a.big}"]["kernel_ms"] / r[f"q{a.big}"]["kernel_ms"]
        res["ivf"][str(nprobe)] = r
    del exact, ivf
    torch.cuda.empty_cache()
    if not a.skip_clustered:
        xc, _ = benchdata.blobs(benchdata.CFG_KMEANS, a.n, a.d, a.nlist)
        qc, _ = benchdata.queries(benchdata.CFG_KMEANS, xc, a.recall_queries)
        exact = HipVS(storage="fp16", device="cuda:0")
        exact.index(None, xc, "bench-exact-c", persist=False)
        ivf = HipVS(storage="fp16", device="cuda:0", factory_string=f"IVF{a.nlist},Flat")
        ivf.index(None, xc, "bench-ivf-c", persist=False)
        for nprobe in a.nprobe:
            res["ivf"][str(nprobe)]["recall10_clustered"] = recall(ivf, exact, qc, k, nprobe)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
