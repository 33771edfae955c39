"""The IVF modes (--modes flat sq8 pq sq8r pqr) against the exact path on one MI355X: 1 M rows, nlist 4 096, nprobe in {8, 32, 128},
k = 10, per --workloads d:storage pair (default: d = 768 and d = 3072, text-embedding-3-large's width, stored as hi|lo).

Per workload, column (exact, then every chosen mode whose list scan takes the width) and nprobe, for 1 and 10 000 queries:
  * wall ms per call: host clock around a call that ends with the results on the host, median of the timed calls;
  * kernel ms per call: lvs_timing_read_calls (HIP events around the dominant kernel: for IVF-PQ the table kernel and
    lvs_ivf_pq_scan_kernel together, for the others their list scan or the flat path's search kernel; the split between the
    two PQ kernels comes from a rocprofv3 --kernel-trace --stats run of this tool);
  * hbm_share: bytes of the probed rows as the scan reads them (PQ: M code bytes per row; SQ8: d; IVF-Flat: 2 or 4 bytes
    per dimension) over 8 TB/s, over kernel time - 1 query: every probed row once; 10 000 queries: the union of the probed
    lists once (a lower bound);
  * recall@10 against the exact search (HipVS.recall: the store's own comparison of its keys with the exact ones, on the
    device) on benchdata's configs[2] rows (uniform: the worst case for IVF) and on a seeded clustered set (benchdata.blobs).
The refined modes (sq8r, pqr: "...,Refine(Flat)" at --k-factor) run two timed kernels per call, the codes' scan at kc =
refine_candidates(k) and lvs_refine_kernel; their kernel ms per call is the sum of both.  Beside it stands the plain store's
search at K = kc (first_stage_kernel_ms: the same code and shape as the refined store's first stage), the difference
(refine_kernel_ms) and the re-ranking's rate: queries x kc x bytes of a stored row over that difference (refine_tbps).
Prints one JSON document (and writes it to --out).

--select FRACTION [FRACTION ...] measures the ids subsets instead: per workload, chosen mode, nprobe and fraction a random
ascending subset of that share of the rows goes in as ``ids`` to the same store, once with ``ids_probe=False`` (the rows are
gathered and searched exactly: gather_exact), once with ``ids_probe=True`` (the mode's list scan with the row selector:
probe), beside the unselected scan (plain); wall ms per call as above for 1 and --big queries, the dominant kernel of each
path, and whether HipVS's own rows-scored rule (len(ids) * nlist > n * nprobe) would send the call through the lists.

The committed profiles are records of these runs (the first two of earlier generations of this tool, whose JSON named some
keys differently):
  profiles/ivf_bench.json      python tools/ivf_bench.py --modes flat --workloads 768:fp16 --reps1 50
  profiles/ivf_sq8_bench.json  python tools/ivf_bench.py --modes flat sq8 --workloads 768:fp16 768:fp32 1536:fp32
  profiles/ivf_pq_bench.json   python tools/ivf_bench.py
  profiles/ivf_refine_bench.json  python tools/ivf_bench.py --modes sq8 pq sq8r pqr --k-factor 5
  profiles/ivf_select_bench.json  python tools/ivf_bench.py --workloads 768:fp16 --nprobe 32 --select 0.5 0.1 0.01 --big 1000"""
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
MODES = ("flat", "sq8", "pq", "sq8r", "pqr")
REFINED = {"sq8r": "sq8", "pqr": "pq"}  # a refined column -> the plain column whose scan is its first stage


def timed(vs, q, k, reps, warmup, per_call=1, **kw):
    """per_call: timed entry points per search (2 for a refined store: the scan and the re-ranking are added up)."""
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
    return {"wall_ms": float(np.median(walls)), "kernel_ms": t["total_ms"] / max(1, t["calls"] // per_call), "kernel": t["kernel"]}


def probed_rows(vs, q, nprobe):
    """(sum over queries of the rows of their probed lists, rows of the union over all queries)."""
    _, off, _ = vs.ivf_lists()
    sizes = np.diff(off)
    probe = vs.ivf_probe(q, nprobe)
    return int(sizes[probe].sum()), int(sizes[np.unique(probe)].sum())


def columns(a, be, d, k, mode):
    """{the column's key in the JSON: the second half of its factory string} of the chosen modes whose list scan takes the shape."""
    cols = {}
    if "flat" in a.modes and be.ivf_fits(d, k, mode):
        cols["ivf_flat"] = "Flat"
    if "sq8" in a.modes and be.ivf_sq8_fits(d, k, mode):
        cols["sq8"] = "SQ8"
    if "pq" in a.modes and be.ivf_pq_fits(d, a.M, k, mode):
        cols["pq"] = f"PQ{a.M}"
    kc = min(56, max(k, int(np.ceil(k * a.k_factor))))  # the refined stores' first stage runs at kc
    if "sq8r" in a.modes and be.ivf_sq8_fits(d, kc, mode):
        cols["sq8r"] = "SQ8,Refine(Flat)"
    if "pqr" in a.modes and be.ivf_pq_fits(d, a.M, kc, mode):
        cols["pqr"] = f"PQ{a.M},Refine(Flat)"
    return cols


def run_workload(d, storage, a, HipVS, benchdata, torch):  # noqa: C901
    from lotus_amd import _capi

    k = 10
    mode = _capi.PACK_F16 if storage == "fp16" else _capi.PACK_SPLIT
    dtype = np.float16 if storage == "fp16" else np.float32
    res = {"n": a.n, "d": d, "storage": storage, "nlist": a.nlist, "k": k}
    xb = benchdata.corpus(benchdata.CFG_SEARCH, a.n, d, dtype=dtype)
    xq, _ = benchdata.queries(benchdata.CFG_SEARCH, xb, a.big, dtype=dtype)
    exact = HipVS(storage=storage, device="cuda:0")
    exact.index(None, xb, "bench-exact", persist=False)
    kinds = columns(a, exact.backend, d, k, mode)
    if "pq" in kinds or "pqr" in kinds:
        res["M"] = a.M
    if set(kinds) & set(REFINED):
        res["k_factor"] = a.k_factor
    stores = {}
    for name, kind in kinds.items():
        vs = HipVS(storage=storage, device="cuda:0", factory_string=f"IVF{a.nlist},{kind}", k_factor=a.k_factor)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vs.index(None, xb, f"bench-{name}", persist=False)
        torch.cuda.synchronize()
        res[f"{name}_build_s"] = time.perf_counter() - t0
        stores[name] = vs
    q1, qb = xq[:1], xq[:a.big]
    res["exact"] = {"q1": timed(exact, q1, k, a.reps1, 5), f"q{a.big}": timed(exact, qb, k, a.repsbig, 1)}
    stored_row_bytes = d * (2 if storage == "fp16" else 4)
    row_bytes = {"pq": a.M, "sq8": d, "ivf_flat": stored_row_bytes, "pqr": a.M, "sq8r": d}
    for name, vs in stores.items():
        col = {}
        per_call = 2 if name in REFINED else 1
        measured = vs.recall(xq[:a.recall_queries], k, nprobe=a.nprobe).intersection
        for at, nprobe in enumerate(a.nprobe):
            r = {"q1": timed(vs, q1, k, a.reps1, 5, per_call, nprobe=nprobe),
                 f"q{a.big}": timed(vs, qb, k, a.repsbig, 1, per_call, nprobe=nprobe)}
            if name in REFINED:  # the plain store at K = kc is the refined store's first stage: the rest is the re-ranking
                kc = vs.refine_candidates(k)
                r["kc"] = kc
                plain = stores.get(REFINED[name])
                for key, qs, reps, warm in (("q1", q1, a.reps1, 5), (f"q{a.big}", qb, a.repsbig, 1)):
                    if plain is None:
                        continue
                    first = timed(plain, qs, kc, reps, warm, nprobe=nprobe)
                    r[key]["first_stage_kernel_ms"] = first["kernel_ms"]
                    r[key]["first_stage_wall_ms"] = first["wall_ms"]
                    r[key]["refine_kernel_ms"] = r[key]["kernel_ms"] - first["kernel_ms"]
                    r[key]["refine_bytes"] = len(qs) * kc * stored_row_bytes
                    r[key]["refine_tbps"] = r[key]["refine_bytes"] / max(1e-9, r[key]["refine_kernel_ms"] * 1e-3) / 1e12
            rows1, _ = probed_rows(vs, q1, nprobe)
            pairs, union = probed_rows(vs, qb, nprobe)
            r["q1"]["probed_rows"] = rows1
            r["q1"]["hbm_share"] = rows1 * row_bytes[name] / HBM_BPS / (r["q1"]["kernel_ms"] * 1e-3)
            r[f"q{a.big}"]["query_row_pairs"] = pairs
            r[f"q{a.big}"]["union_rows"] = union
            r[f"q{a.big}"]["hbm_share"] = union * row_bytes[name] / HBM_BPS / (r[f"q{a.big}"]["kernel_ms"] * 1e-3)
            r["recall10_uniform"] = float(measured[at])
            r["speedup_q1_kernel_vs_exact"] = res["exact"]["q1"]["kernel_ms"] / r["q1"]["kernel_ms"]
            r[f"speedup_q{a.big}_kernel_vs_exact"] = res["exact"][f"q{a.big}"]["kernel_ms"] / r[f"q{a.big}"]["kernel_ms"]
            col[str(nprobe)] = r
        res[name] = col
    del exact, stores
    torch.cuda.empty_cache()
    if not a.skip_clustered:
        xc, _ = benchdata.blobs(benchdata.CFG_KMEANS, a.n, d, a.nlist, dtype=dtype)
        qc, _ = benchdata.queries(benchdata.CFG_KMEANS, xc, a.recall_queries, dtype=dtype)
        for name, kind in kinds.items():
            vs = HipVS(storage=storage, device="cuda:0", factory_string=f"IVF{a.nlist},{kind}", k_factor=a.k_factor)
            vs.index(None, xc, f"bench-{name}-c", persist=False)
            measured = vs.recall(qc, k, nprobe=a.nprobe).intersection
            for at, nprobe in enumerate(a.nprobe):
                res[name][str(nprobe)]["recall10_clustered"] = float(measured[at])
            del vs
        torch.cuda.empty_cache()
    return res


def run_select(d, storage, a, HipVS, benchdata, torch):
    """The --select table of one workload: {mode: {nprobe: {fraction: {plain, gather_exact, probe}}}}."""
    k = 10
    dtype = np.float16 if storage == "fp16" else np.float32
    res = {"n": a.n, "d": d, "storage": storage, "nlist": a.nlist, "k": k, "select": list(a.select)}
    xb = benchdata.corpus(benchdata.CFG_SEARCH, a.n, d, dtype=dtype)
    xq, _ = benchdata.queries(benchdata.CFG_SEARCH, xb, a.big, dtype=dtype)
    from lotus_amd import _capi

    mode = _capi.PACK_F16 if storage == "fp16" else _capi.PACK_SPLIT
    rng = np.random.default_rng(20261018)
    subsets = {f: np.sort(rng.choice(a.n, max(k + 1, int(round(f * a.n))), replace=False)) for f in a.select}
    probe_be = HipVS(storage=storage, device="cuda:0").backend
    for name, kind in columns(a, probe_be, d, k, mode).items():
        vs = HipVS(storage=storage, device="cuda:0", factory_string=f"IVF{a.nlist},{kind}", k_factor=a.k_factor)
        vs.index(None, xb, f"bench-sel-{name}", persist=False)
        nlist = len(vs.ivf_lists()[1]) - 1
        col = {}
        for nprobe in a.nprobe:
            per = {}
            for key, qs, reps, warm in (("q1", xq[:1], a.reps1, 5), (f"q{a.big}", xq[:a.big], a.repsbig, 2)):
                plain = timed(vs, qs, k, reps, warm, nprobe=nprobe)
                for f, ids in subsets.items():
                    r = per.setdefault(str(f), {"ids": int(ids.size), "rule_takes_the_lists": bool(ids.size * nlist > a.n * nprobe)})
                    # ids_probe=True goes through HipVS's own rule: where it keeps the call exact, "probe" times the exact
                    # path again and its "kernel" says so
                    exact = timed(vs, qs, k, reps, warm, nprobe=nprobe, ids=ids, ids_probe=False)
                    probe = timed(vs, qs, k, reps, warm, nprobe=nprobe, ids=ids, ids_probe=True)
                    r[key] = {"plain": plain, "gather_exact": exact, "probe": probe,
                              "probe_speedup_wall": exact["wall_ms"] / probe["wall_ms"]}
            col[str(nprobe)] = per
        res[name] = col
        del vs
        torch.cuda.empty_cache()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[8, 32, 128])
    ap.add_argument("--modes", nargs="+", choices=MODES, default=["flat", "sq8", "pq"],
                    help="the columns beside the exact one; a mode whose list scan refuses a workload's width is skipped there")
    ap.add_argument("--M", type=int, default=64, help="subspaces of the pq and pqr modes")
    ap.add_argument("--k-factor", type=float, default=5.0, help="k_factor of the refined modes (sq8r, pqr)")
    ap.add_argument("--workloads", nargs="+", default=["768:fp32", "3072:fp32"],
                    help="d:storage pairs (storage fp16 or fp32 = hi|lo)")
    ap.add_argument("--big", type=int, default=10_000)
    ap.add_argument("--reps1", type=int, default=30)
    ap.add_argument("--repsbig", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--skip-clustered", action="store_true")
    ap.add_argument("--select", type=float, nargs="+", default=None,
                    help="fractions of the rows passed as ids: time the gathered exact path against ids_probe=True instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import benchdata
    from lotus_amd import HipVS

    if not torch.cuda.is_available():
        raise SystemExit("ivf_bench needs a GPU")
    out = {"device": torch.cuda.get_device_name(0), "workloads": []}
    for wl in a.workloads:
        d, storage = wl.split(":")
        run = run_select if a.select else run_workload
        out["workloads"].append(run(int(d), storage, a, HipVS, benchdata, torch))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
