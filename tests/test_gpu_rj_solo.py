"""GPU parity of `lvs_rj_kernel` launched with ONE corpus range (256 groups of 256 queries: a chunk of 65 536 queries), where
the kernel runs without threshold sharing (no side-word DMA of thresholds, no side-word read in a block's last unit, no
atomicMax) and - when the corpus has no nb % 32 tail rows - writes its lists straight into the caller's [nq][k] keys, with no
merge launch.

Two references:
  * the same queries searched as two calls of 32 768 (128 groups x 2 ranges: the shared kernel form and the merge).  Keys are a
    total order and every chunk is a complete exact search, so the keys must be equal BIT FOR BIT;
  * the CPU oracle on a stratified sample of query rows - the first 256, then row 256 t + 37 t mod 256 of every 256-query group t
    (bench.py's `check_rows`) - with the bars of `test_gpu_rj.py`: scores within 1e-5, no id mismatch outside 2e-5 near-ties.
    The planted rows are sample rows.

A planted query is an exact copy of a unit row rounded to fp16: its score with itself is within 2^-10 of 1 (squared L2: 0).

Case (b) was specified with 65 536 - 300 queries (a ragged last group) and is kept that way; under the greedy chunk plan such a call goes out as
32 768 + 16 384 + 8 192 + 4 096 + 3 796 - a single-range launch always has 256 FULL groups - so the same case is also run with
65 536 queries, which is the one that reaches the unshared squared-L2 form (with a one-row tail: two lists, merge kept)."""
import os
import re

import numpy as np
import pytest
import torch

import oracle
import synth
from lotus_amd import _capi

pytestmark = pytest.mark.gpu
F16 = _capi.PACK_F16
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _default_max():
    """LVS_RQ_CHUNK_DEFAULT as the library was built (lvs_plan.h)."""
    text = open(os.path.join(ROOT, "lotus_amd", "csrc", "lvs_plan.h")).read()
    return int(re.search(r"^#define LVS_RQ_CHUNK_DEFAULT (\d+)", text, re.M).group(1))


def _plan(nq, maximum):
    """The greedy cut of a call (rq_chunk_len; modelled and pinned in test_rq_chunk_plan.py)."""
    out, left = [], nq
    while left > 0:
        cn = next((c for c in (65536, 32768, 16384, 8192) if c <= maximum and c <= left), min(left, 4096))
        out.append(cn)
        left -= cn
    return out


def _sample_rows(nq):
    t = np.arange(-(-nq // 256))
    strat = np.minimum(256 * t + (37 * t) % 256, nq - 1)
    return np.unique(np.concatenate([np.arange(min(256, nq)), strat]))


def _strat(t):
    return 256 * t + (37 * t) % 256


def _make(be, nq, nb, d, seed, plants=(), equal=None):
    """Corpus, queries (fp16) and their device images.  plants: (query, row) copies; equal: (query, first row, count) - `count`
    identical rows from `first row` on, equal to that query."""
    xb = synth.corpus(nb, d, seed=seed).astype(np.float16)
    if equal:
        xb[equal[1]:equal[1] + equal[2]] = xb[equal[1]]
    xq, planted = synth.queries(xb.astype(np.float32), nq, seed=seed + 1)
    xq = xq.astype(np.float16)
    for q, row in plants:
        xq[q] = xb[row]
    if equal:
        xq[equal[0]] = xb[equal[1]]
    return xb, xq, planted, be.pack(xb, F16), be.pack(xq, F16)


def _search(be, cb, cq, k, metric, id_offset=0, kernel="lvs_rj_kernel"):
    be.timing_enable(True)
    keys = be.search_keys(cb, cq, k, metric, id_offset=id_offset)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    assert t["kernel"] == kernel, t  # (the kernel of the call's LAST timed launch)
    return keys, t


def _in_pieces(be, cb, cq, k, metric, sizes, id_offset=0):
    out, c0 = [], 0
    for cn in sizes:
        out.append(be.search_keys(cb, be.slice_rows(cq, c0, c0 + cn), k, metric, id_offset=id_offset))
        c0 += cn
    assert c0 == cq.n
    return torch.cat(out)


def _oracle_parity(be, keys, xb, xq, k, metric, id_offset=0):
    rows = _sample_rows(xq.shape[0])
    D, I = be.keys_to_result(keys[torch.from_numpy(rows).to(keys.device)], metric)
    Dg, Ig = D.cpu().numpy(), I.cpu().numpy() - id_offset
    Dr, Ir = oracle.flat_search(xb.astype(np.float32), xq[rows].astype(np.float32), k, metric)
    err, hard, recall = synth.compare_topk(Dr, Ir, Dg, Ig, atol=1e-5)
    print(f"oracle sample of {rows.size} queries: score error {err:.2e}, hard id mismatches {hard}, recall {recall:.6f}")
    assert err <= 1e-5, f"score error {err}"
    assert hard == 0, f"{hard} id mismatches outside near-ties"
    assert recall >= 0.9999, recall
    return rows, Dg, Ig, Ir


def test_a_whole_blocks_direct_write_equals_two_shared_half_calls_bit_for_bit(hip_backend):
    """(a) 65 536 queries x 32 768 + 64 rows (whole blocks: no tail list, the kernel writes the result itself), d 256, k 10, IP."""
    be = hip_backend
    nq, nb, d, k = 65536, 32768 + 64, 256, 10
    q_eq, eq0, eqn = 5, 32 * 700 + 23, 40            # 40 equal rows straddling two block seams, equal to query 5
    q_last = _strat(255)                             # the last group's sample row sits on the last corpus row
    q_first = _strat(128)
    xb, xq, planted, cb, cq = _make(be, nq, nb, d, 81, plants=[(q_last, nb - 1), (q_first, 0)], equal=(q_eq, eq0, eqn))
    keys, t = _search(be, cb, cq, k, IP, id_offset=11)
    print(t)
    if _default_max() >= 65536:
        assert t["launches"] == 1 and t["calls"] == 1, t
    halves = _in_pieces(be, cb, cq, k, IP, [32768, 32768], id_offset=11)
    assert keys.shape == halves.shape == (nq, k)
    assert torch.equal(keys, halves), f"{int((keys != halves).any(dim=1).sum())} queries differ from the two-range calls"
    rows, Dg, Ig, Ir = _oracle_parity(be, keys, xb, xq, k, IP, id_offset=11)
    at = {int(r): i for i, r in enumerate(rows)}
    assert {q_eq, q_last, q_first} <= set(at)
    assert np.array_equal(Ig[at[q_eq]], np.arange(eq0, eq0 + k)), Ig[at[q_eq]]  # ties come back in id order
    assert np.array_equal(Ig[at[q_eq]], Ir[at[q_eq]])
    for q, row in ((q_last, nb - 1), (q_first, 0)):
        assert Ig[at[q], 0] == row and abs(float(Dg[at[q], 0]) - 1.0) <= 2.0 ** -10, (q, Ig[at[q], :3], Dg[at[q], 0])


@pytest.mark.parametrize("nq", [65536 - 300, 65536])
def test_b_one_row_tail_two_lists_merge_kept_squared_l2_k16(hip_backend, nq):
    """(b) 32 768 + 96 + 1 rows (a one-row tail through lvs_rq_kernel: two lists per query, the merge stays), d 384, k 16, squared L2;
    65 536 - 300 queries as specified (see the module docstring) and 65 536 (the single-range launch)."""
    be = hip_backend
    nb, d, k = 32768 + 96 + 1, 384, 16
    q_tail = _strat(200)                             # a sample row planted on the tail row
    q_blk = _strat(-(-nq // 256) - 1)                # the last group's sample row on the last whole-block row
    assert q_blk < nq
    xb, xq, planted, cb, cq = _make(be, nq, nb, d, 83, plants=[(q_tail, nb - 1), (q_blk, nb - 2), (9, 31)])
    keys, t = _search(be, cb, cq, k, L2)
    print(t)
    halves = _in_pieces(be, cb, cq, k, L2, [32768, nq - 32768])
    assert torch.equal(keys, halves), f"{int((keys != halves).any(dim=1).sum())} queries differ from the half-calls"
    rows, Dg, Ig, Ir = _oracle_parity(be, keys, xb, xq, k, L2)
    at = {int(r): i for i, r in enumerate(rows)}
    for q, row in ((q_tail, nb - 1), (q_blk, nb - 2), (9, 31)):
        assert Ig[at[q], 0] == row and abs(float(Dg[at[q], 0])) <= 2.0 ** -10, (q, Ig[at[q], :3], Dg[at[q], 0])


def test_c_plan_of_a_100k_call_and_keys_equal_the_per_chunk_calls(hip_backend):
    """(c) 100 000 queries x 65 536 + 224 rows, d 256, k 10, IP: one call, the launches of the greedy plan at the built default
    maximum (65 536: 65 536 + 32 768 + 1 696 = 3 launches; 32 768: 3 x 32 768 + 1 696 = 4), keys = the per-chunk calls'."""
    be = hip_backend
    nq, nb, d, k = 100_000, 65536 + 224, 256, 10
    xb, xq, planted, cb, cq = _make(be, nq, nb, d, 85, plants=[(_strat(390), nb - 1), (_strat(255), 0), (_strat(256), 32)])
    # (the last chunk, 1 696 queries against a corpus this short, is one lvs_rq_kernel takes: it is the call's last timed launch)
    keys, t = _search(be, cb, cq, k, IP, kernel="lvs_rq_kernel")
    print(t)
    plan = _plan(nq, _default_max())
    assert plan == ([65536, 32768, 1696] if _default_max() == 65536 else [32768, 32768, 32768, 1696])
    assert t["launches"] == len(plan) and t["calls"] == 1, (t, plan)
    assert torch.equal(keys, _in_pieces(be, cb, cq, k, IP, plan))
    assert torch.equal(keys, _in_pieces(be, cb, cq, k, IP, [32768, 32768, 32768, 1696]))  # ... and the two-range launches'
    rows, Dg, Ig, Ir = _oracle_parity(be, keys, xb, xq, k, IP)
    at = {int(r): i for i, r in enumerate(rows)}
    for q, row in ((_strat(390), nb - 1), (_strat(255), 0), (_strat(256), 32)):
        assert Ig[at[q], 0] == row, (q, Ig[at[q], :3])


def test_d_the_headline_instantiation_d768_k10_ip(hip_backend):
    """(d) 65 536 queries x 32 768 + 32 rows, d 768, k 10, IP: oracle parity on the sample, every sampled query's planted
    neighbour at rank 1 (bench.py's `planted_neighbour_at_rank1` == 1.0), keys = the two shared half-calls'."""
    be = hip_backend
    nq, nb, d, k = 65536, 32768 + 32, 768, 10
    xb, xq, planted, cb, cq = _make(be, nq, nb, d, 87)
    keys, t = _search(be, cb, cq, k, IP)
    print(t)
    rows, Dg, Ig, Ir = _oracle_parity(be, keys, xb, xq, k, IP)
    at_rank1 = float((Ig[:, 0] == planted[rows]).mean())
    print(f"planted at rank 1: {at_rank1}")
    assert at_rank1 == 1.0
    assert torch.equal(keys, _in_pieces(be, cb, cq, k, IP, [32768, 32768]))


@pytest.mark.parametrize("d,k,metric,tail", [(512, 16, IP, 0), (768, 10, L2, 0), (384, 10, IP, 5), (256, 16, L2, 0), (512, 10, L2, 31)])
def test_other_instantiations_equal_the_shared_half_calls(hip_backend, d, k, metric, tail):
    """The remaining widths / list depths / metrics of the unshared form, with and without tail rows: bit-identical keys."""
    be = hip_backend
    nq, nb = 65536, 32768 + 64 + tail
    xb, xq, planted, cb, cq = _make(be, nq, nb, d, 89 + d // 128, plants=[(3, nb - 1), (65535, 0)])
    keys, t = _search(be, cb, cq, k, metric)
    assert torch.equal(keys, _in_pieces(be, cb, cq, k, metric, [32768, 32768]))
    D, I = be.keys_to_result(keys[[3, 65535]], metric)
    assert I.cpu().numpy()[:, 0].tolist() == [nb - 1, 0]


def test_e_threshold_self_join_unchanged(hip_backend):
    """(e) `lvs_range_join` keeps its own 32 768-row chunks and remainder rule: a self-join of 70 000 unit rows, d 256, threshold
    0.95, pairs planted at cosine 0.97 and near misses at 0.93 (random rows: cosine 0 +- 1/16).  The exact pair set against
    brute force over the planted rows, and the launch count of the parent of this change, read from a run of this test on the
    parent's library: {'launches': 6, 'calls': 2, 'kernel': 'lvs_tile_kernel'} - two C calls (65 536 + 4 464 query rows); the first
    makes two RANGE launches of lvs_rj_kernel (32 768 rows each) and two of the list kernel for the corpus' last 16 rows, the second
    two of the list kernel (chunks of 4 096 and 368 rows with fewer than 32 768 rows left to pair with)."""
    be = hip_backend
    n, d, tau = 70_000, 256, 0.95
    x = synth.corpus(n, d, seed=91)
    rng = np.random.default_rng(92)
    # the later row of a pair: around the chunk boundaries (32 768, 65 536, 69 632), in the corpus' last 16 (tail) rows, anywhere
    later = [32767, 32768, 32799, 65535, 65536, 65567, 69631, 69632, 69983, 69984, 69999, 31, 32, 40_000, 68_000]
    later_near = [100, 32770, 65540, 69700, 69990, 50_000]  # ... of a near miss
    pairs, near = set(), set()
    used = set(later) | set(later_near)
    for j in later + later_near:
        i = int(rng.integers(0, j))
        while i in used:
            i = int(rng.integers(0, j))
        used.add(i)
        (pairs if j in later else near).add((i, j))
    noise = synth.corpus(len(later) + len(later_near), d, seed=93)
    for (i, j), u in zip(sorted(pairs | near), noise):
        c = 0.97 if (i, j) in pairs else 0.93
        u = u - (u @ x[i]) * x[i]
        x[j] = c * x[i] + np.sqrt(1.0 - c * c) * u / np.linalg.norm(u)
    x16 = x.astype(np.float16)
    p = be.pack(x16, F16)
    be.timing_enable(True)
    q, j, sc = be.range_join(p, p, tau, IP, q_row0=0)
    be.synchronize()
    t = be.timing_read_full()
    be.timing_enable(False)
    print(t)
    got = set(zip(q.cpu().numpy().tolist(), j.cpu().numpy().tolist()))
    assert len(got) == int(q.numel())  # no pair twice
    # brute force over the planted rows (every row that takes part in a pair or a near miss) against all rows
    xf = x16.astype(np.float32)
    touched = sorted({r for pr in pairs | near for r in pr})
    s = xf[touched] @ xf.T
    want = set()
    for a, row in zip(touched, s):
        for b in np.nonzero(row > tau)[0].tolist():
            if a != b:
                want.add((min(a, b), max(a, b)))
    assert np.abs(s[(s > 0.9) & (s < 0.999)] - tau).min() > 5e-3  # nothing near the threshold: the comparison is exact
    assert want == pairs, (sorted(want - pairs)[:5], sorted(pairs - want)[:5])
    assert got == want, (sorted(want - got)[:5], sorted(got - want)[:5])
    assert (t["launches"], t["calls"], t["kernel"]) == (6, 2, "lvs_tile_kernel"), t
