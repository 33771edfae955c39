"""bench.py's plain run (no --full) on one GPU: the headline line and --dump-outputs, nothing else - and the dumped result of
the last timed step holds against the CPU oracle (the in-run check of that result is a --full figure)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import bench
    import benchdata
    import oracle

    nq, n, d, k = 2048, 131072, 768, 10
    env = dict(os.environ)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "LOTUS_BENCH_REHEARSAL"):
        env.pop(var, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--queries", str(nq), "--corpus", str(n), "--dump-outputs", str(tmp_path / "out")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "queries/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] * 1e-3 / nq - 1) < 1e-3
    assert out["roofline"]["bound"] == "mfma" and out["roofline"]["frac"] > 0
    assert out["planted_neighbour_at_rank1"] > 0.99
    assert not {"recall_at_k", "cpu_baseline", "legs", "legs_summary", "value_t_call"} & set(out)

    D = np.load(tmp_path / "out" / "distances.npy")
    I = np.load(tmp_path / "out" / "indices.npy")
    assert D.shape == (nq, k) and I.shape == (nq, k) and not os.path.exists(tmp_path / "out" / "rows.npy")
    xb = benchdata.corpus(benchdata.CFG_JOIN, n, d)
    xq, _ = benchdata.queries(benchdata.CFG_JOIN, xb, nq)
    rows = bench.check_rows(np, nq, 64)
    Dr, Ir = oracle.flat_search(xb.astype(np.float32), xq[rows].astype(np.float32), k, 0)
    assert np.abs(Dr - D[rows]).max() <= 1e-5
    assert bench._near_tie_mismatches(np, Dr, Ir, I[rows].astype(np.int64), k) == 0
