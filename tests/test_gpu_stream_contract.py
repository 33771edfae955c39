"""The enqueue-only contract of include/lotus_hip.h: "the library allocates nothing, keeps no pointer after a call returns and
never synchronises: work is only enqueued on `stream`".

Every device-side entry point is captured once into a graph on a side stream (tests/graph_replay.py) with input set A in its
buffers and replayed on set B, then on A again, in the SAME buffers.  Each replay must equal, bit for bit, the same calls made
eagerly on the default stream with those inputs - where the header leaves an order open, after the canonical ordering the
extent tests use - and the searches must also meet the CPU oracle at the bars of their home test files.  B is chosen to take
the other device-side branch of the entry (an overflow, a fallback, an empty list, an uncertified query ...), and every case
asserts that it does wherever the header makes that observable.  A replay runs what was enqueued on the capture stream and
nothing else: a launch, memset or copy that went to another stream, a decision taken on the host from device data, or scratch
state the call does not set up itself makes one of the replays differ (or the capture fail).

tests/stream_contract_cases.py is the case table; tests/test_stream_contract_host.py holds it against the header."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import oracle
import synth
from extent_cases import F16, FLAT_BY_NAME, IP, L2, LIST, SPLIT, Flat
from graph_replay import SENT, eager, replayed
from ivf_oracle_backend import ivf_reference
from ivf_pq_oracle_backend import pq_decode, pq_reference
from ivf_sq8_oracle_backend import list_of_rows, sq8_decode, sq8_reference
from lotus_amd import _capi
from stream_contract_cases import CASES, FLAT_ROUTES, IVF_KINDS
from test_gpu_output_extents import ivf  # noqa: F401 - the fixture: one small IVF index
from test_gpu_output_extents import (P, _accumulate_inputs, call, np_, raw_accumulate, raw_build_lists, raw_flat,
                                     raw_iteration, raw_ivf, raw_ivf_range, raw_nearest3, raw_nearest_hi, raw_objective,
                                     raw_sharded, raw_sort_rows)
from test_gpu_parity import _stored
from test_gpu_workspace_extents import _assert_same_bits, _check_flat, _check_ivf, _flat_data, _pack2, _sel_reference
from ws_guard import GuardedPool, guarded

pytestmark = pytest.mark.gpu


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    """``enqueue()``: the raw calls (and the zeroing the header leaves to the caller), ``outputs`` / ``scratch``: what they write
    and their workspaces, ``load(which)``: input set "A" / "B" into the input buffers, ``canon(arrays)``: a canonical order
    where the header leaves one open, ``check(which, arrays)``: that B takes its branch and A does not, and the oracle."""
    enqueue: object
    outputs: list
    load: object
    scratch: list = dataclasses.field(default_factory=list)
    canon: object = None
    check: object = None
    keep: list = dataclasses.field(default_factory=list)


class Sets:
    """Input buffers that hold set A or set B: ``tensor`` / ``packed`` -> the buffer the calls read (a clone of A's)."""

    def __init__(self):
        self.pairs = []

    def tensor(self, a, b):
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous(), (a.shape, b.shape)
        dst = a.clone()
        self.pairs.append((dst, a, b))
        return dst

    def packed(self, a, b):
        assert (a.n, a.d, a.mode, a.exp) == (b.n, b.d, b.mode, b.exp)
        return dataclasses.replace(a, rows=self.tensor(a.rows, b.rows), norms=self.tensor(a.norms, b.norms))

    def inout(self, dst, a, b):
        """``dst`` is written by the calls as well: restored from a / b before every run."""
        self.pairs.append((dst, a, b))
        return dst

    def load(self, which):
        for dst, a, b in self.pairs:
            dst.copy_(a if which == "A" else b)


def ok(be, name, *args):
    rc = call(be, name, *args)
    assert rc == _capi.OK, (name, rc, be.lib.lvs_last_error())


def run_raw(be, raw, ws):
    rc = raw.run(ws, raw.need)
    assert rc == _capi.OK, (raw.entry, rc, be.lib.lvs_last_error())


def dev(be, a, dtype=None):
    return be.to_device(np.ascontiguousarray(a, dtype=dtype))


def keys_dev(be, keys):
    return be.to_device(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))


def listed(idx, count, cap=None):
    """An index list whose order the header leaves open: its first ``count`` entries, sorted.  (What stands behind them is the
    sentinel in an eager run and the longer list of the replay before in a replay: not the call's output.)"""
    n = int(count) if cap is None else min(int(count), cap)
    return np.sort(idx[:n])


def result(be, keys, metric):
    D, I = be.keys_to_result(torch.from_numpy(np.ascontiguousarray(keys)).to(be.device), metric)
    return np_(D), np_(I)


# ---- the flat search ---------------------------------------------------------------------------------------------------------
def _flat_sets(c):
    """A: the extent tests' data.  B: a corpus from another seed whose queries are aimed at the row AFTER the one A's query was
    drawn from (``synth.queries``: 0.7 row + 0.7 noise), so every query's winner moves."""
    xbA, xqA = _flat_data(c)
    _, drawn = synth.queries(xbA, c.nq, seed=3)  # (the rows A's queries were drawn from: _flat_data's own call)
    xbB = synth.corpus(c.nb, c.d, seed=c.nb % 97 + 1)
    rng = np.random.default_rng(c.nq)
    u = rng.standard_normal((c.nq, c.d)).astype(np.float32)
    xqB = 0.7 * xbB[(drawn + 1) % c.nb] + 0.7 * u / np.linalg.norm(u, axis=1, keepdims=True)
    xqB /= np.linalg.norm(xqB, axis=1, keepdims=True)
    if c.metric == L2:
        xbB = xbB * 1.5
    return (xbA, xqA), (xbB, xqB.astype(np.float32))


def case_flat(be, c, entry="lvs_flat_search_keys", oracle_check=True):
    data = dict(zip("AB", _flat_sets(c)))
    pk = {w: _pack2(be, *data[w], c.mode) for w in "AB"}
    s, pool = Sets(), GuardedPool(be.device)
    cb, cq = s.packed(pk["A"][0], pk["B"][0]), s.packed(pk["A"][1], pk["B"][1])
    raw = raw_flat(be, pool, c, cb, cq, entry)
    ws = pool.alloc(raw.need, 0)
    outputs, seen = list(raw.outs), {}
    if entry == "lvs_flat_search_keys_seeded":  # the seeds come from the captured sequence too (raw.keep: [tiles][nq])
        tiles = int(raw.keep.shape[0])
        outputs.append(raw.keep)

        def enqueue():
            ok(be, "lvs_flat_search_seed_scores", P(cb.rows), cb.mode, cb.n, P(cq.rows), cq.mode, cq.n, c.d, c.metric, P(cb.norms),
               P(cq.norms), tiles, P(raw.keep), be._stream())
            run_raw(be, raw, ws)
    else:
        def enqueue():
            run_raw(be, raw, ws)

    def check(which, arrays):
        keys = arrays[0]
        if oracle_check and entry in ("lvs_flat_search_keys", "lvs_flat_search_keys_seeded"):
            _check_flat(be, c, *data[which], keys)
        seen[which] = result(be, keys[:4096], c.metric)[1][:, 0]
        if which == "B":
            assert (seen["A"] != seen["B"]).all(), "B's winners are A's"

    return Case(enqueue, outputs, s.load, [ws], check=check, keep=[pool, raw])


def case_fallback(be):
    """The predicated fallback of the large-k search: the capture sees 32 000 tie-free rows (A), the replay the mass ties of
    test_large_k_with_mass_ties_falls_back_to_selection_passes (B: 4 rows x 3 000 copies + 20 000 rows, 30 queries, k = 200),
    whose candidate buckets overflow, and must still be exact.  The shipped build does not report that the fallback ran: the
    case asserts the cause (whole result lists of one tied score in B, none in A) and the exact result, not the path."""
    c = Flat("fallback", 30, 32000, 64, 200, F16, IP, LIST)
    base = synth.corpus(40, 64, seed=3)
    xbB = np.concatenate([np.repeat(base[:4], 3000, axis=0), synth.corpus(20000, 64, seed=4)])
    xqB, _ = synth.queries(base, 30, seed=5)
    xbA = synth.corpus(32000, 64, seed=6)
    xqA, _ = synth.queries(xbA, 30, seed=5)
    data = {"A": (xbA, xqA), "B": (xbB, xqB)}
    pk = {w: _pack2(be, *data[w], c.mode) for w in "AB"}
    s, pool = Sets(), GuardedPool(be.device)
    cb, cq = s.packed(pk["A"][0], pk["B"][0]), s.packed(pk["A"][1], pk["B"][1])
    raw = raw_flat(be, pool, c, cb, cq)
    ws = pool.alloc(raw.need, 0)

    def check(which, arrays):
        D, I = result(be, arrays[0], IP)
        Dr, Ir = oracle.flat_search(_stored(data[which][0], F16), _stored(data[which][1], F16), c.k, IP)
        assert np.abs(D - Dr).max() <= 1e-5 and (I == Ir).mean() > 0.99  # (the bars of the parity test)
        tied = D[:, 0] == D[:, -1]
        assert tied.any() if which == "B" else not tied.any()

    return Case(lambda: run_raw(be, raw, ws), raw.outs, s.load, [ws], check=check, keep=[pool, raw])


def case_certified(be):
    """_hi_banded -> rescore -> sort -> certify (banded, and the plain rule on the same lists) as ONE graph.  A: fp16-valued rows,
    every query certifies.  B: test_one_pass_certificate_refuses_rows_that_differ_below_fp16_resolution's twins (same hi part,
    lo parts growing with the copy number) around rank k."""
    d, nb, nq, k1, k = 96, 20_000, 64, 15, 10
    c = Flat("certified", nq, nb, d, k1, SPLIT, IP, LIST)
    h16 = (synth.corpus(nb, d, seed=5) * 1.1).astype(np.float16)
    xbA = h16.astype(np.float32)
    xq = xbA[:64].copy()
    xbB = xbA.copy()
    for qi in range(64):
        rows = 1000 + qi * 30 + np.arange(30)
        xbB[rows] = xbB[qi]
        xbB[rows, :8] += (np.arange(30)[:, None] / 100.0) * np.spacing(np.abs(h16[qi, :8])).astype(np.float32)
    pA, pB, cq = be.pack(xbA, SPLIT), be.pack(xbB, SPLIT), be.pack(xq, SPLIT)
    scale, slack = (max(v) for v in zip(be._cert_bound(pA, cq, IP), be._cert_bound(pB, cq, IP)))
    s, pool = Sets(), GuardedPool(be.device)
    cb = s.packed(pA, pB)
    raw = raw_flat(be, pool, c, cb, cq, "lvs_flat_search_keys_hi_banded")  # (its band: 1e-3 |q| + 1e-3 below the k-th slot)
    assert 2.02 * (scale * 1.2 + slack) < 1e-3  # ... which the certificate's band must not exceed
    ws = pool.alloc(raw.need, 0)
    approx = raw.outs[0]
    exact = guarded(pool, (nq, k1), torch.int64, SENT)
    idx, cnt = guarded(pool, (nq,), torch.int64, SENT), guarded(pool, (1,), torch.int64, SENT)
    idx0, cnt0 = guarded(pool, (nq,), torch.int64, SENT), guarded(pool, (1,), torch.int64, SENT)

    def enqueue():
        run_raw(be, raw, ws)
        exact.copy_(approx)
        ok(be, "lvs_rescore_keys", P(cb.rows), cb.mode, P(cq.rows), cq.mode, nq, d, IP, P(cb.norms), P(cq.norms), 0, k1, P(exact),
           be._stream())
        ok(be, "lvs_sort_keys_desc", P(exact), nq, k1, be._stream())
        cnt.zero_()
        ok(be, "lvs_certify_topk_banded", P(approx), P(exact), P(cq.norms), nq, k1, k, scale, slack, 2.02, P(idx), P(cnt), be._stream())
        cnt0.zero_()
        ok(be, "lvs_certify_topk", P(approx), P(exact), P(cq.norms), nq, k1, k, scale, slack, P(idx0), P(cnt0), be._stream())

    def canon(a):
        return a[0], a[1], listed(a[2], a[3][0]), a[3], listed(a[4], a[5][0]), a[5]

    def check(which, a):
        assert (int(a[3][0]) > 0) if which == "B" else (int(a[3][0]) == 0), (which, a[3], a[5])
        if which == "A":  # every query certified: the exact top k of the candidates is the exact top k
            D, I = result(be, a[1][:, :k], IP)
            Dr, Ir = oracle.flat_search(xbA, xq, k, IP)
            err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=1e-5)
            assert err <= 1e-5 and hard == 0 and recall >= 0.9999, (err, hard, recall)

    return Case(enqueue, [approx, exact, idx, cnt, idx0, cnt0], s.load, [ws], canon, check, keep=[pool, raw])


def _corpus_stats(be, cb):
    dpad = int(cb.rows.shape[1]) // 2
    return torch.stack([cb.norms.max(), cb.rows[:, dpad:].float().square().sum(dim=1).max()]).to(torch.float32).contiguous()


def _near_duplicates(be, nb):
    """-> (corpus A, corpus B, queries): hi|lo rows, fp16 queries.  A: well-separated rows.  B: row 1 repeats row 0 and rows
    11, 12 repeat row 10 up to a relative 2^-13 (below fp16's resolution: equal hi parts), and ten queries sit on rows 0 and 10 -
    a query on row 0 has two possible winners, one on row 10 three."""
    xb = synth.corpus(nb, 100, seed=5) * 1.2
    xq = synth.queries(xb, 300, seed=8)[0].astype(np.float16)
    xq[:5], xq[5:10] = xb[0].astype(np.float16), xb[10].astype(np.float16)
    xbB = xb.copy()
    xbB[1] = xb[0] * np.float32(1 + 2.0 ** -13)
    xbB[11], xbB[12] = xb[10] * np.float32(1 + 2.0 ** -13), xb[10] * np.float32(1 - 2.0 ** -13)
    return be.pack(xb, SPLIT), be.pack(xbB, SPLIT), be.pack(xq, F16), xb, xbB, xq


def _winners_are_exact(be, keys, xb, xq, metric=L2):
    """test_nearest_hi_and_nearest3_outputs' bar: the exact search's winner ids outside near-ties of the hi-only scores."""
    Dw, Iw = oracle.flat_search(xb, xq.astype(np.float32), 2, metric)
    _, Ig = result(be, keys.reshape(-1, 1), metric)
    other = Ig[:, 0] != Iw[:, 0]
    assert np.all(np.abs(Dw[other, 0] - Dw[other, 1]) <= 3e-3) and other.mean() < 0.05


def case_nearest3(be):
    """lvs_nearest3 -> lvs_nearest3_select -> lvs_resolve_pairs (which reads its pair count from the device) as ONE graph."""
    pA, pB, cq, xbA, xbB, xq = _near_duplicates(be, 3 * 256 - 1)
    s, pool = Sets(), GuardedPool(be.device)
    cb = s.packed(pA, pB)
    cstats = s.tensor(_corpus_stats(be, pA), _corpus_stats(be, pB))
    coef5 = (ctypes.c_float * 5)(*be._nearest_coef(pA, cq, L2)[0])
    raw = raw_nearest3(be, pool, cb, cq)
    ws = pool.alloc(raw.need, 0)
    keys, keys2, sec, third = raw.outs
    nq = cq.n
    pair, opn, counts = (guarded(pool, (nq,), torch.int64, SENT), guarded(pool, (nq,), torch.int64, SENT),
                         guarded(pool, (2,), torch.int64, SENT))

    def enqueue():
        run_raw(be, raw, ws)
        counts.zero_()
        ok(be, "lvs_nearest3_select", P(keys), P(keys2), P(sec), P(third), P(cq.norms), nq, P(cstats), ctypes.addressof(coef5),
           P(pair), P(opn), P(counts), be._stream())
        ok(be, "lvs_resolve_pairs", P(cb.rows), cb.mode, P(cq.rows), cq.mode, cb.d, L2, P(cb.norms), P(cq.norms), 0, P(pair),
           P(counts), nq, P(keys), P(keys2), be._stream())

    def canon(a):
        return a[:4] + (listed(a[4], a[6][0]), listed(a[5], a[6][1]), a[6])

    def check(which, a):
        n_pair, n_open = (int(v) for v in a[6])
        assert (n_pair > 0 and n_open > 0) if which == "B" else (n_pair == 0 and n_open == 0), (which, n_pair, n_open)
        _winners_are_exact(be, a[0], xbA if which == "A" else xbB, xq)

    return Case(enqueue, [keys, keys2, sec, third, pair, opn, counts], s.load, [ws], canon, check, keep=[pool, raw, coef5])


def case_nearest_hi(be):
    """lvs_nearest_hi over thirteen slabs (its merge kernel writes the outputs) with both margin selections behind it."""
    pA, pB, cq, xbA, xbB, xq = _near_duplicates(be, 16385)
    s, pool = Sets(), GuardedPool(be.device)
    cb = s.packed(pA, pB)
    cstats = s.tensor(_corpus_stats(be, pA), _corpus_stats(be, pB))
    coef = be._nearest_coef(pA, cq, L2)[0]
    coef5 = (ctypes.c_float * 5)(*coef)
    R, E = max(be.row_norm_max(pA), be.row_norm_max(pB)), max(be.lo_norm_max(pA), be.lo_norm_max(pB))
    scale, slack = coef[0] * E + coef[1] * R, coef[2] + coef[3] * R + coef[4] * R * R
    raw = raw_nearest_hi(be, pool, cb, cq)
    ws = pool.alloc(raw.need, 0)
    keys, sec = raw.outs
    nq = cq.n
    idx, cnt = guarded(pool, (nq,), torch.int64, SENT), guarded(pool, (1,), torch.int64, SENT)
    idx2, cnt2 = guarded(pool, (nq,), torch.int64, SENT), guarded(pool, (1,), torch.int64, SENT)

    def enqueue():
        run_raw(be, raw, ws)
        cnt.zero_()
        ok(be, "lvs_margin_select", P(keys), P(sec), P(cq.norms), nq, scale, slack, P(idx), P(cnt), be._stream())
        cnt2.zero_()
        ok(be, "lvs_margin_select_stats", P(keys), P(sec), P(cq.norms), nq, P(cstats), ctypes.addressof(coef5), P(idx2), P(cnt2),
           be._stream())

    def canon(a):
        return a[0], a[1], listed(a[2], a[3][0]), a[3], listed(a[4], a[5][0]), a[5]

    def check(which, a):
        n, n2 = int(a[3][0]), int(a[5][0])
        assert (n >= 10 and n2 >= 10) if which == "B" else (n == 0 and n2 == 0), (which, n, n2)
        _winners_are_exact(be, a[0], xbA if which == "A" else xbB, xq)

    return Case(enqueue, [keys, sec, idx, cnt, idx2, cnt2], s.load, [ws], canon, check, keep=[pool, raw, coef5])


# ---- other flat-side entries ---------------------------------------------------------------------------------------------------
def case_merge_keys(be, nparts, nq, k):
    def parts_of(seed):
        rng = np.random.default_rng(seed)
        sc = rng.standard_normal((nparts, nq, k)).astype(np.float32)
        ids = rng.permutation(nparts * nq * k).reshape(nparts, nq, k).astype(np.int64)
        parts = np.ascontiguousarray(np.sort(oracle.pack_keys(sc, ids), axis=2)[:, :, ::-1])
        parts[-1, :, k - 2 - seed % 2:] = 0  # empty slots at a list's end
        return parts

    host = {"A": parts_of(nparts * 1000 + k), "B": parts_of(nparts * 1000 + k + 1)}
    s, pool = Sets(), GuardedPool(be.device)
    p_dev = s.tensor(keys_dev(be, host["A"]), keys_dev(be, host["B"]))
    out = guarded(pool, (nq, k), torch.int64, SENT)

    def check(which, a):
        want = np.sort(host[which].transpose(1, 0, 2).reshape(nq, nparts * k), axis=1)[:, ::-1][:, :k]
        assert np.array_equal(a[0].view(np.uint64), want)

    return Case(lambda: ok(be, "lvs_merge_keys", P(p_dev), nparts, nq, k, P(out), be._stream()), [out], s.load, check=check,
                keep=[pool])


def case_sort_rows(be):
    nq, nb = 300, 2049
    host = {w: np.random.default_rng(seed).standard_normal((nq, nb)).astype(np.float32) for w, seed in (("A", 1), ("B", 2))}
    host["B"][:, 5] = host["B"][:, nb - 1]  # a tie with the last column: ids decide
    s, pool = Sets(), GuardedPool(be.device)
    sc = s.tensor(dev(be, host["A"]), dev(be, host["B"]))
    raw = raw_sort_rows(be, pool, sc, nb)
    ws = pool.alloc(raw.need, 0)

    def check(which, a):
        ids = np.broadcast_to(np.arange(nb, dtype=np.int64) + 9, (nq, nb))
        assert np.array_equal(a[0].view(np.uint64), np.sort(oracle.pack_keys(host[which], ids), axis=1)[:, ::-1])

    return Case(lambda: run_raw(be, raw, ws), raw.outs, s.load, [ws], check=check, keep=[pool, raw])


def case_keys_to_result(be):
    nq, k = 33, 7

    def keys_of(seed):
        rng = np.random.default_rng(seed)
        keys = oracle.pack_keys(rng.standard_normal((nq, k)).astype(np.float32), rng.integers(0, 50, (nq, k)))
        keys[:, k - 1 - seed % 2:] = 0
        return keys

    host = {"A": keys_of(4), "B": keys_of(5)}
    s, pool = Sets(), GuardedPool(be.device)
    k_dev = s.tensor(keys_dev(be, host["A"]), keys_dev(be, host["B"]))
    id_map = s.tensor(dev(be, np.arange(50, dtype=np.int64) * 3 + 1), dev(be, np.arange(50, dtype=np.int64)[::-1] * 5))
    D, I = guarded(pool, (nq, k), torch.float32, SENT), guarded(pool, (nq, k), torch.int64, SENT)

    def check(which, a):
        better, ids, empty = oracle.unpack_keys(host[which])
        assert np.array_equal(a[1], np.where(empty, -1, ids * 3 + 1 if which == "A" else (49 - ids) * 5))
        assert np.array_equal(a[0][~empty], (-better[~empty] * np.float32(0.25)))

    return Case(lambda: ok(be, "lvs_keys_to_result", P(k_dev), nq, k, L2, P(id_map), 2, P(D), P(I), be._stream()), [D, I], s.load,
                check=check, keep=[pool])


def case_scores(be):
    nq, nb, d, ld = 130, 1001, 100, 1001 + 3
    host = {}
    for w, seed in (("A", 2), ("B", 12)):
        xb = synth.corpus(nb, d, seed=seed)
        host[w] = (xb.astype(np.float16), synth.queries(xb, nq, seed=seed + 1)[0].astype(np.float16))
    pk = {w: (be.pack(host[w][0], F16), be.pack(host[w][1], F16)) for w in "AB"}
    s, pool = Sets(), GuardedPool(be.device)
    cb, cq = s.packed(pk["A"][0], pk["B"][0]), s.packed(pk["A"][1], pk["B"][1])
    out = guarded(pool, (nq, ld), torch.float32, SENT)

    def check(which, a):
        xb, xq = host[which]
        assert np.abs(a[0][:, :nb] - xq.astype(np.float32) @ xb.astype(np.float32).T).max() <= 1e-5
        assert (a[0][:, nb:].view(np.uint8) == SENT).all()

    return Case(lambda: ok(be, "lvs_scores", P(cb.rows), cb.mode, nb, P(cq.rows), cq.mode, nq, d, IP, P(cb.norms), P(cq.norms), 0,
                           P(out), ld, be._stream()), [out], s.load, check=check, keep=[pool])


def _pairs_canon(cap, nb):
    """(out_q, out_j, out_s, count, ...): up to the capacity the triples sorted by (q, j); over it WHICH pairs are stored is
    left to the atomics - the count, and the buffers from ``cap`` on, are what two runs share."""
    def canon(a):
        q, j, sc, cnt = a[:4]
        n = int(cnt[0])
        if n > cap:
            return cnt, q[cap:], j[cap:], sc[cap:]
        order = np.lexsort((j[:n], q[:n]))
        return cnt, q[:n][order], j[:n][order], sc[:n][order], q[cap:], j[cap:], sc[cap:]
    return canon


def _stored_pairs_are_hits(a, cap, S, thr, self_join=False):
    """Every stored triple is a (query, row) above the threshold, once, with its score."""
    q, j, sc, cnt = a[:4]
    n = min(int(cnt[0]), cap)
    q, j, sc = q[:n], j[:n], sc[:n]
    assert np.unique(q * S.shape[1] + j).size == n and (sc > thr).all() and np.abs(S[q, j] - sc).max() <= 1e-5
    if self_join:
        assert (j > q).all()


def case_range_join(be, self_join):
    """A: fewer hits than the capacity.  B: rows that share a common direction, far more hits than the capacity - counted, not
    stored, and nothing written at or past ``capacity`` (the buffers are 64 entries longer)."""
    n, nq, d, thr, cap = 3000, 3000 if self_join else 700, 100, 0.25, 60_000
    xA = synth.corpus(n, d, seed=6).astype(np.float16)
    common = synth.corpus(1, d, seed=7)
    xB = (0.6 * common + 0.8 * synth.corpus(n, d, seed=8)).astype(np.float16)
    host = {"A": xA, "B": xB}
    s, pool = Sets(), GuardedPool(be.device)
    cb = s.packed(be.pack(xA, F16), be.pack(xB, F16))
    cq = cb if self_join else s.packed(be.pack(xA[:nq], F16), be.pack(xB[:nq], F16))
    q0 = 0 if self_join else -1
    oq, oj = guarded(pool, (cap + 64,), torch.int64, SENT), guarded(pool, (cap + 64,), torch.int64, SENT)
    os_, cnt = guarded(pool, (cap + 64,), torch.float32, SENT), guarded(pool, (1,), torch.int64, SENT)

    def enqueue():
        cnt.zero_()
        ok(be, "lvs_range_join", P(cb.rows), cb.mode, n, P(cq.rows), cq.mode, nq, d, IP, P(cb.norms), P(cq.norms), thr, 0, q0, 0,
           1, 0, cap, P(oq), P(oj), P(os_), P(cnt), be._stream())

    def check(which, a):
        x = host[which].astype(np.float32)
        S = x[:nq] @ x.T
        hits = S > thr
        if self_join:
            hits &= np.arange(n)[None, :] > np.arange(nq)[:, None]
        true = int(a[3][0])
        assert abs(true - int(hits.sum())) <= int((np.abs(S - thr) < 1e-5).sum())
        assert (0 < true < cap) if which == "A" else (true > 2 * cap), (which, true)
        assert all((t[cap:].view(np.uint8) == SENT).all() for t in a[:3])
        _stored_pairs_are_hits(a, cap, S, thr, self_join)

    return Case(enqueue, [oq, oj, os_, cnt], s.load, canon=_pairs_canon(cap, n), check=check, keep=[pool])


def case_pack(be, d, mode):
    """The packing family at n = 257 (d = 100: the scalar kernel, 200: the vector one).  B carries one inf and one value
    beyond fp16's range, so lvs_pack_rows_checked's flag word and lvs_absmax's maximum change."""
    n = 257
    rng = np.random.default_rng(d)
    xA, xB = (rng.standard_normal((n, d)).astype(np.float32) for _ in range(2))
    xB[7, 3], xB[200, d - 1] = np.inf, 1e6
    ids = {w: rng.integers(0, n, 2 * n + 3).astype(np.int64) for w in "AB"}
    m = 2 * n + 3
    ld = int(be.lib.lvs_packed_ld(d, mode))
    s, pool = Sets(), GuardedPool(be.device)
    x, ids_dev = s.tensor(dev(be, xA), dev(be, xB)), s.tensor(dev(be, ids["A"]), dev(be, ids["B"]))
    rows, norms = guarded(pool, (n, ld), torch.float16, SENT), guarded(pool, (n,), torch.float32, SENT)
    rows3, norms3 = guarded(pool, (n, ld), torch.float16, SENT), guarded(pool, (n,), torch.float32, SENT)
    flags, bits = guarded(pool, (1,), torch.int32, SENT), guarded(pool, (1,), torch.int32, SENT)
    g_rows, g_norms = guarded(pool, (m, ld), torch.float16, SENT), guarded(pool, (m,), torch.float32, SENT)
    vals = guarded(pool, (m, d), torch.float32, SENT)
    F32 = _capi.DTYPE_F32

    def enqueue():
        st = be._stream()
        ok(be, "lvs_pack_rows", P(x), F32, n, d, mode, 0, P(rows), P(norms), st)
        flags.zero_()
        ok(be, "lvs_pack_rows_checked", P(x), F32, n, d, mode, 0, 0, P(rows3), P(norms3), P(flags), st)
        bits.zero_()
        ok(be, "lvs_absmax", P(x), F32, n, d, P(bits), st)
        ok(be, "lvs_gather_rows", P(rows), ld, P(ids_dev), m, P(g_rows), st)
        ok(be, "lvs_gather_f32", P(norms), P(ids_dev), m, P(g_norms), st)
        ok(be, "lvs_unpack_rows", P(rows), d, mode, P(ids_dev), m, 0, P(vals), st)

    def check(which, a):
        r, nr, r3, nr3, fl, bt, gr, gn, v = a
        xs = xA if which == "A" else xB
        assert int(fl[0]) == (0 if which == "A" else _capi.PACK_FLAG_NONFINITE | _capi.PACK_FLAG_RANGE)
        assert bt.view(np.float32)[0] == np.abs(xs).max()
        assert r.tobytes() == r3.tobytes() and nr.tobytes() == nr3.tobytes()
        assert gr.tobytes() == r[ids[which]].tobytes() and gn.tobytes() == nr[ids[which]].tobytes()
        if which == "A":
            stored = xs.astype(np.float16).astype(np.float32) if mode == F16 else xs
            assert np.abs(v - stored[ids[which]]).max() <= (0 if mode == F16 else 2.0 ** -20 * np.abs(xs).max())

    return Case(enqueue, [rows, norms, rows3, norms3, flags, bits, g_rows, g_norms, vals], s.load, check=check, keep=[pool])


# ---- IVF, on the fixture's small index -----------------------------------------------------------------------------------------
def case_build_lists(be):
    """B assigns every row but a few to ONE list, and those few to none (-1)."""
    n, nlist = 8192 * 2 + 77, 37
    rng = np.random.default_rng(3)
    host = {"A": rng.integers(0, nlist, n).astype(np.int64), "B": np.full(n, 5, np.int64)}
    host["A"][rng.choice(n, 100, replace=False)] = nlist + 3
    host["B"][rng.choice(n, 100, replace=False)] = -1
    s, pool = Sets(), GuardedPool(be.device)
    a_dev = s.tensor(dev(be, host["A"]), dev(be, host["B"]))
    raw = raw_build_lists(be, pool, a_dev, n, nlist)
    ws = pool.alloc(raw.need, 0)

    def canon(a):  # (what stands past offsets[nlist] is unspecified)
        return a[0], a[1][:int(a[0][-1])]

    def check(which, a):
        assign = host[which]
        keep = (assign >= 0) & (assign < nlist)
        off, rows = a[0], a[1].view(np.uint32)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(assign[keep], minlength=nlist))]))
        assert np.array_equal(rows[:n - 100], np.flatnonzero(keep)[np.argsort(assign[keep], kind="stable")].astype(np.uint32))
        assert (np.diff(off) > 0).sum() == (1 if which == "B" else nlist)

    return Case(lambda: run_raw(be, raw, ws), raw.outs, s.load, [ws], canon, check, keep=[pool, raw])


_TRUTH = {}


def _ivf_truth(be, ivf):
    """Host copies of what the fixture's index holds, and the decoded rows of its two code modes (made once)."""
    if id(ivf) not in _TRUTH:
        nb, d = ivf["nb"], ivf["d"]
        lists, sq, pq = ivf["lists"], ivf["sq"], ivf["pq"]
        off, rows = np_(lists.offsets), np_(lists.rows).view(np.uint32)
        c, where = np_(be.unpack(lists.centroids)), list_of_rows(off, rows, nb)
        codes = np.empty((nb, d), np.uint8)
        codes[rows.astype(np.int64)] = np_(sq.codes[:, :d])
        pcodes = np.empty((nb, pq.M), np.uint8)
        pcodes[rows.astype(np.int64)] = np_(pq.codes[:, :pq.M])
        _TRUTH[id(ivf)] = dict(off=off, rows=rows, c=c, xb=np_(be.unpack(ivf["packed"])),
                               sq=sq8_decode(c, where, np_(sq.vmin), np_(sq.vdiff), codes),
                               pq=pq_decode(c, where, np_(pq.codebooks), pcodes), keep=ivf)
    return _TRUTH[id(ivf)]


def _ivf_query_sets(be, ivf, s):
    """A: the fixture's queries.  B: every query a copy of centroid 3 - all of them probe the same lists."""
    t = _ivf_truth(be, ivf)
    qB = be.pack(np.repeat(t["c"][3:4], ivf["nq"], axis=0).astype(np.float16), F16)
    host = {"A": np_(be.unpack(ivf["qp"])), "B": np_(be.unpack(qB))}
    return s.packed(ivf["qp"], qB), host


def _selectors(be, nb, s):
    """A: every third row.  B: every other block of 32 rows has no selected row."""
    masks = {"A": np.arange(nb) % 3 == 0, "B": (np.arange(nb) // 32) % 2 == 0}
    return s.tensor(*(be.row_bitmap(np.flatnonzero(masks[w]), nb)[0] for w in "AB")), masks


def case_ivf_search(be, ivf, kind, nprobe):
    """The plain entry and its ``_sel`` form, one call each in the captured sequence."""
    k, t = 10, _ivf_truth(be, ivf)
    s, pool = Sets(), GuardedPool(be.device)
    qp, xq = _ivf_query_sets(be, ivf, s)
    sel, masks = _selectors(be, ivf["nb"], s)
    mine = dict(ivf, qp=qp)
    plain, withsel = raw_ivf(be, pool, mine, kind, k, nprobe), raw_ivf(be, pool, mine, kind, k, nprobe, sel)
    assert (plain.entry, withsel.entry) == CASES[f"ivf/{kind}/nprobe{nprobe}"]
    ws = [pool.alloc(plain.need, 0), pool.alloc(withsel.need, 0)]
    ref, scored = {"lvs_ivf_search": (lambda x, q, k_, m, o, r, p: ivf_reference(x, q, k_, m, None, o, r, p), t["xb"]),
                   "lvs_ivf_sq8_search": (sq8_reference, t["sq"]), "lvs_ivf_pq_search": (pq_reference, t["pq"])}[kind]

    def enqueue():
        run_raw(be, plain, ws[0])
        run_raw(be, withsel, ws[1])

    def check(which, a):
        keys, probe, keys_sel, probe_sel = a
        assert np.array_equal(probe, probe_sel)  # (the probes do not depend on the selector)
        assert (probe == probe[0]).all() if which == "B" else not (probe == probe[0]).all()
        for got, mask in ((keys, None), (keys_sel, masks[which])):
            _check_ivf(*_sel_reference(ref, scored, xq[which], k, IP, t["off"], t["rows"], probe, mask), *result(be, got, IP))

    return Case(enqueue, plain.outs + withsel.outs, s.load, ws, check=check, keep=[pool, plain, withsel])


def case_ivf_encode(be, ivf):
    """B: another image under the same lists - other residuals, other codes."""
    lists, sq, pq = ivf["lists"], ivf["sq"], ivf["pq"]
    n, d = ivf["nb"], ivf["d"]
    other = be.pack(synth.corpus(n, d, seed=77).astype(np.float16), F16)
    s, pool = Sets(), GuardedPool(be.device)
    packed = s.packed(ivf["packed"], other)
    codes, rn = guarded(pool, (n, 128), torch.uint8, SENT), guarded(pool, (n,), torch.float32, SENT)
    pcodes, beta = guarded(pool, (n, 16), torch.uint8, SENT), guarded(pool, (n,), torch.float32, SENT)
    seen = {}

    def enqueue():
        ok(be, "lvs_ivf_sq8_encode", P(packed.rows), packed.mode, n, d, P(lists.offsets), P(lists.rows), lists.nlist,
           P(sq.centroids), P(sq.vmin), P(sq.vdiff), P(codes), P(rn), be._stream())
        ok(be, "lvs_ivf_pq_encode", P(packed.rows), packed.mode, n, d, P(lists.offsets), P(lists.rows), lists.nlist,
           P(pq.centroids), pq.M, pq.ksub, P(pq.codebooks), P(pcodes), P(beta), be._stream())

    def check(which, a):
        seen[which] = a
        if which == "A":  # the fixture's own codes
            assert all(x.tobytes() == np_(y).tobytes() for x, y in zip(a, (sq.codes, sq.rnorm, pq.codes, pq.beta)))
        else:
            assert (seen["A"][0] != a[0]).mean() > 0.2 and (seen["A"][2][:, :pq.M] != a[2][:, :pq.M]).mean() > 0.2

    return Case(enqueue, [codes, rn, pcodes, beta], s.load, check=check, keep=[pool])


def case_ivf_range(be, ivf):
    """B: every query three times centroid 3 - all of them probe the same lists and clear the threshold on most of their rows:
    more hits than the capacity."""
    t, nprobe, thr, cap = _ivf_truth(be, ivf), 5, 0.3, 8192
    s, pool = Sets(), GuardedPool(be.device)
    qB = be.pack(np.repeat(3 * t["c"][3:4], ivf["nq"], axis=0).astype(np.float16), F16)
    xq = {"A": np_(be.unpack(ivf["qp"])), "B": np_(be.unpack(qB))}
    probes = {w: np_(be.ivf_search(ivf["packed"], ivf["lists"], q, 1, IP, nprobe, want_probe=True)[1])
              for w, q in (("A", ivf["qp"]), ("B", qB))}
    qp = s.packed(ivf["qp"], qB)
    raw = raw_ivf_range(be, pool, dict(ivf, qp=qp), nprobe, thr, cap)
    ws = pool.alloc(raw.need, 0)
    cnt = raw.outs[3]

    def enqueue():
        cnt.zero_()
        run_raw(be, raw, ws)

    def check(which, a):
        from ivf_range_oracle_backend import check_pairs, ivf_range_reference

        want, near = ivf_range_reference(t["xb"], xq[which], thr, IP, t["off"], t["rows"], probes[which])
        true = int(a[3][0])
        assert len(want) <= true <= len(want) + len(near)
        assert (0 < true < cap) if which == "A" else (true > cap), (which, true)
        S = xq[which].astype(np.float64) @ t["xb"].astype(np.float64).T
        _stored_pairs_are_hits(a, cap, S, thr)
        if which == "A":
            check_pairs(np.stack([a[0][:true], a[1][:true]], axis=1), want, near, ivf["nb"])

    return Case(enqueue, raw.outs, s.load, [ws], _pairs_canon(cap, ivf["nb"]), check, keep=[pool, raw])


def case_refine(be, ivf):
    """B: candidate lists with empty slots (key 0, and rows past the image) scattered through them."""
    packed, t = ivf["packed"], _ivf_truth(be, ivf)
    kc, k, nq = 40, 7, ivf["nq"]
    s, pool = Sets(), GuardedPool(be.device)
    qp, xq = _ivf_query_sets(be, ivf, s)
    candA = be.ivf_pq_search(packed, ivf["lists"], ivf["pq"], ivf["qp"], kc, IP, 4).contiguous()
    hB = np_(be.ivf_pq_search(packed, ivf["lists"], ivf["pq"], qp_of_B(be, ivf), kc, IP, 4)).copy()
    rng = np.random.default_rng(9)
    hB[rng.random(hB.shape) < 0.3] = 0
    hB[:, 5] = np.int64((0x7F000000 << 32) | (0xFFFFFFFF - (ivf["nb"] + 7)))  # a row past the image: an empty slot too
    cand = s.tensor(candA, dev(be, hB))
    host = {"A": np_(candA), "B": hB}
    out = guarded(pool, (nq, k), torch.int64, SENT)

    def enqueue():
        ok(be, "lvs_refine_keys", P(packed.rows), packed.mode, packed.n, P(packed.norms), P(qp.rows), qp.mode, nq, P(qp.norms),
           ivf["d"], IP, P(cand), kc, k, P(out), be._stream())

    def check(which, a):
        keys = host[which].view(np.uint64)
        rows = (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
        empty = (keys == 0) | (rows >= ivf["nb"])
        assert empty.any() == (which == "B")
        Dr = np.full((nq, k), -np.finfo(np.float32).max, np.float32)
        Ir = np.full((nq, k), -1, np.int64)
        for q in range(nq):
            live = np.unique(rows[q][~empty[q]])
            sc = xq[which][q].astype(np.float64) @ t["xb"][live].astype(np.float64).T
            order = np.lexsort((live, -sc))[:k]
            Dr[q, :len(order)], Ir[q, :len(order)] = sc[order], live[order]
        _check_ivf(Dr, Ir, *result(be, a[0], IP))

    return Case(enqueue, [out], s.load, check=check, keep=[pool])


def qp_of_B(be, ivf):
    t = _ivf_truth(be, ivf)
    return be.pack(np.repeat(t["c"][3:4], ivf["nq"], axis=0).astype(np.float16), F16)


def case_recall(be, ivf):
    """lvs_keys_overlap, lvs_ivf_row_lists, lvs_ivf_probe_ranks on the keys and probes of two query sets; B also has empty
    truth slots and lists of another assignment."""
    packed, lists, nq, nb, nlist = ivf["packed"], ivf["lists"], ivf["nq"], ivf["nb"], ivf["nlist"]
    kt, kg, Pn = 10, 10, 4
    host = {}
    for w, q in (("A", ivf["qp"]), ("B", qp_of_B(be, ivf))):
        truth = np_(be.search_keys(packed, q, kt, IP, one_pass=False)).copy()
        got, probe = be.ivf_search(packed, lists, q, kg, IP, Pn, want_probe=True)
        host[w] = [truth, np_(got).copy(), np_(probe).copy()]
    host["B"][0][:, kt - 3:] = 0
    rng = np.random.default_rng(2)
    assign = rng.integers(0, nlist, nb)
    order = np.argsort(assign, kind="stable")
    offB = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int64)
    s, pool = Sets(), GuardedPool(be.device)
    truth, got, probe = (s.tensor(dev(be, host["A"][i]), dev(be, host["B"][i])) for i in range(3))
    off = s.tensor(lists.offsets.contiguous(), dev(be, offB))
    rows = s.tensor(lists.rows.contiguous(), dev(be, order.astype(np.uint32).view(np.int32)))
    hits, first = guarded(pool, (nq,), torch.int32, SENT), guarded(pool, (nq,), torch.int32, SENT)
    row_list = guarded(pool, (nb,), torch.int32, SENT)
    rank, hist = guarded(pool, (nq, kt), torch.int32, SENT), guarded(pool, (Pn + 1,), torch.int64, SENT)

    def enqueue():
        st = be._stream()
        ok(be, "lvs_keys_overlap", P(truth), kt, P(got), kg, nq, P(hits), P(first), st)
        row_list.fill_(-1)
        ok(be, "lvs_ivf_row_lists", P(off), P(rows), nb, nlist, P(row_list), st)
        hist.zero_()
        ok(be, "lvs_ivf_probe_ranks", P(truth), kt, P(row_list), nb, P(probe), Pn, nq, P(rank), P(hist), st)

    def check(which, a):
        tr, gt, pr = host[which]
        row = lambda keys: np.where(keys == 0, -1, 0xFFFFFFFF - (keys.view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64))  # noqa: E731
        want = np.array([np.isin(t_[t_ >= 0], g_[g_ >= 0]).sum() for t_, g_ in zip(row(tr), row(gt))])
        assert np.array_equal(a[0], want) and int(a[4].sum()) == int((tr != 0).sum())
        where = np.empty(nb, np.int64)
        where[(np_(lists.rows).view(np.uint32) if which == "A" else order).astype(np.int64)] = np.repeat(
            np.arange(nlist), np.diff(np_(lists.offsets) if which == "A" else offB))
        assert np.array_equal(a[2], where)
        assert ((a[3] == -1) == (tr == 0)).all() and ((tr == 0).any() == (which == "B"))

    return Case(enqueue, [hits, first, row_list, rank, hist], s.load, check=check, keep=[pool])


# ---- k-means pieces --------------------------------------------------------------------------------------------------------------
def case_accumulate(be):
    """n = 16 385, k = 37, from assignments and from keys.  B sends every row to one centroid; sums and counts are zeroed in the
    captured sequence - B's sums continue from A's replay if that zeroing was not captured."""
    k = 37
    x, assign, p, _ = _accumulate_inputs(be, k=k)
    host = {"A": assign, "B": np.full_like(assign, 5)}
    to_keys = lambda a: np.where(a >= 0, oracle.pack_keys(np.zeros(p.n, np.float32), np.maximum(a, 0)), np.uint64(0))  # noqa: E731
    s, pool = Sets(), GuardedPool(be.device)
    a_dev = s.tensor(dev(be, host["A"]), dev(be, host["B"]))
    keys = s.tensor(keys_dev(be, to_keys(host["A"])), keys_dev(be, to_keys(host["B"])))
    by_assign, by_keys = raw_accumulate(be, pool, p, a_dev, k), raw_accumulate(be, pool, p, a_dev, k, keys)
    ws = [pool.alloc(by_assign.need, 0), pool.alloc(by_keys.need, 0)]
    outputs = by_assign.outs + by_keys.outs

    def enqueue():
        for t in outputs:
            t.zero_()
        run_raw(be, by_assign, ws[0])
        run_raw(be, by_keys, ws[1])

    def check(which, a):
        keep = host[which] >= 0
        ref = np.zeros((k, p.d), np.float32)
        np.add.at(ref, host[which][keep], x.astype(np.float32)[keep])
        counts = np.bincount(host[which][keep], minlength=k).astype(np.float32)
        assert np.array_equal(a[0], ref) and np.array_equal(a[1], counts) and np.array_equal(a[2], ref) and np.array_equal(a[3], counts)
        assert (counts > 0).sum() == (1 if which == "B" else k)

    return Case(enqueue, outputs, s.load, ws, check=check, keep=[pool, by_assign, by_keys, p])


def _sums_sets(be, k=37):
    """(x, packed x, {A, B: (sums, counts) on the device}): A from random assignments, B with clusters 3, 4 and 30 empty."""
    x, assign, p, a_dev = _accumulate_inputs(be, k=k)
    b = assign.copy()
    b[np.isin(b, (3, 4, 30))] = 7
    return x, p, {"A": be.kmeans_accumulate(p, a_dev, k), "B": be.kmeans_accumulate(p, dev(be, b), k)}


def case_objective(be):
    k = 37
    x, p, sums = _sums_sets(be, k)
    cents = {"A": x[:k].astype(np.float32), "B": x[100:100 + k].astype(np.float32) * 1.5}
    s, pool = Sets(), GuardedPool(be.device)
    cent = s.tensor(dev(be, cents["A"]), dev(be, cents["B"]))
    sm, cn = s.tensor(sums["A"][0], sums["B"][0]), s.tensor(sums["A"][1], sums["B"][1])
    x2h = {"A": float(p.norms.double().sum()), "B": 123.5}
    x2 = s.tensor(dev(be, np.float64([x2h["A"]])), dev(be, np.float64([x2h["B"]])))
    raw = raw_objective(be, pool, cent, sm, cn, x2)
    ws = pool.alloc(raw.need, 0)
    ld = int(be.lib.lvs_packed_ld(p.d, SPLIT))
    rows, norms, cstats = (guarded(pool, (k, ld), torch.float16, SENT), guarded(pool, (k,), torch.float32, SENT),
                           guarded(pool, (2,), torch.float32, SENT))

    def enqueue():
        run_raw(be, raw, ws)
        ok(be, "lvs_kmeans_pack_centroids", P(cent), k, p.d, SPLIT, P(rows), P(norms), P(cstats), be._stream())

    def check(which, a):
        c, S, n = cents[which].astype(np.float64), np_(sums[which][0]).astype(np.float64), np_(sums[which][1]).astype(np.float64)
        want = x2h[which] - 2.0 * (c * S).sum() + (n * (c * c).sum(axis=1)).sum()
        assert abs(float(a[0][0]) - want) <= 1e-5 * abs(want)  # (test_kmeans_objective's bar)
        pk, st = be.kmeans_pack_centroids(dev(be, cents[which]), SPLIT)
        assert a[1].tobytes() == np_(pk.rows).tobytes() and a[2].tobytes() == np_(pk.norms).tobytes() and a[3].tobytes() == np_(st).tobytes()

    return Case(enqueue, raw.outs + [rows, norms, cstats], s.load, [ws], check=check, keep=[pool, raw])


def case_update_centroids(be):
    """n_train > 0.  B has empty clusters, so faiss's split runs on the device (*out_nsplit > 0) - and equals the host helper."""
    k = 37
    x, p, sums = _sums_sets(be, k)
    d, ld = p.d, int(be.lib.lvs_packed_ld(p.d, SPLIT))
    start = x[:k].astype(np.float32)
    s, pool = Sets(), GuardedPool(be.device)
    sm = s.tensor(sums["A"][0], sums["B"][0])
    counts = s.inout(guarded(pool, (k,), torch.float32, SENT), sums["A"][1], sums["B"][1])
    cent = s.inout(guarded(pool, (k, d), torch.float32, SENT), dev(be, start), dev(be, start * 2))
    rows, norms = guarded(pool, (k, ld), torch.float16, SENT), guarded(pool, (k,), torch.float32, SENT)
    cstats, nsplit = guarded(pool, (2,), torch.float32, SENT), guarded(pool, (1,), torch.int32, SENT)

    def enqueue():
        ok(be, "lvs_kmeans_update_centroids", P(sm), P(counts), k, d, p.n, P(cent), P(nsplit), SPLIT, P(rows), P(norms), P(cstats),
           be._stream())

    def check(which, a):
        S, n = np_(sums[which][0]), np_(sums[which][1]).copy()
        c = np.ascontiguousarray(np.where(n[:, None] > 0, S * (np.float32(1.0) / np.where(n > 0, n, 1))[:, None],
                                          start * (1 if which == "A" else 2)).astype(np.float32))
        ns = be.split_clusters(p.n, n, c)
        assert int(a[1][0]) == ns and ((ns > 0) == (which == "B"))
        assert np.array_equal(a[0], c) and np.array_equal(a[5], n)

    return Case(enqueue, [cent, nsplit, rows, norms, cstats, counts], s.load, check=check, keep=[pool])


def case_bounds(be):
    """centroid_shift -> bounds_set -> bounds_fix -> bounds_step on synthetic keys (test_gpu_kmeans_bounds.py holds the rules to
    their float64 restatement; here: the same bits from a replay).  B moves the centroids a hundred times further, so the step
    lists far more rows."""
    N, m2, k, d = 1000, 300, 37, 100
    stats, coef5 = np.float32([4.0, 0.25]), (ctypes.c_float * 5)(1e-3, 1e-3, 1e-4, 0.0, 0.0)  # (a search error of about 3e-3)
    exact2 = (ctypes.c_float * 2)(8e-6, 4e-6)
    host = {}
    for w, seed, move in (("A", 1, 1e-3), ("B", 2, 1e-1)):
        rng = np.random.default_rng(seed)
        d1 = (10.0 ** rng.uniform(-1, 1, N)).astype(np.float32)
        d2 = (d1 * rng.uniform(1.0, 40.0, N)).astype(np.float32)
        ids = rng.integers(0, k, N)
        sel = rng.permutation(N)[:m2]
        c_old = rng.standard_normal((k, d)).astype(np.float32)
        host[w] = dict(keys=oracle.pack_keys(-d1, ids), second=-d2, qn=rng.uniform(0.5, 2.0, N).astype(np.float32),
                       pos=sel.astype(np.int64), approx=oracle.pack_keys(-d1, ids)[sel],
                       exact=oracle.pack_keys(-(d1[sel] * np.float32(0.9)), np.where(rng.random(m2) < 0.5, ids[sel], (ids[sel] + 1) % k)),
                       qn_sel=None, c_old=c_old, c_new=c_old + np.float32(move) * rng.standard_normal((k, d)).astype(np.float32))
        host[w]["qn_sel"] = host[w]["qn"][sel]
    s, pool = Sets(), GuardedPool(be.device)
    t = {name: s.tensor(*((keys_dev if host["A"][name].dtype == np.uint64 else dev)(be, host[w][name]) for w in "AB"))
         for name in host["A"]}
    st = dev(be, stats)
    assign = guarded(pool, (N,), torch.int32, SENT)
    ub, lb = guarded(pool, (N,), torch.float32, SENT), guarded(pool, (N,), torch.float32, SENT)
    delta, top2 = guarded(pool, (k,), torch.float32, SENT), guarded(pool, (3,), torch.float32, SENT)
    idx, cnt = guarded(pool, (N,), torch.int64, SENT), guarded(pool, (1,), torch.int64, SENT)
    seen = {}

    def enqueue():
        sm = be._stream()
        ok(be, "lvs_kmeans_centroid_shift", P(t["c_old"]), P(t["c_new"]), k, d, P(delta), P(top2), sm)
        ok(be, "lvs_kmeans_bounds_set", P(t["keys"]), 1, P(t["second"]), P(t["qn"]), None, N, P(st), ctypes.addressof(coef5), 0,
           P(assign), P(ub), P(lb), sm)
        ok(be, "lvs_kmeans_bounds_fix", P(t["approx"]), P(t["exact"]), P(t["qn_sel"]), P(t["pos"]), m2, P(st),
           ctypes.addressof(coef5), ctypes.addressof(exact2), 0, P(assign), P(ub), P(lb), sm)
        cnt.zero_()
        ok(be, "lvs_kmeans_bounds_step", P(assign), P(ub), P(lb), P(delta), P(top2), N, P(idx), P(cnt), sm)

    def canon(a):
        return a[:5] + (listed(a[5], a[6][0]), a[6])

    def check(which, a):
        h = host[which]
        assert np.abs(a[3] - np.linalg.norm(h["c_new"].astype(np.float64) - h["c_old"], axis=1)).max() <= 1e-5 * a[3].max()
        assert ((a[0] >= 0) & (a[0] < k)).all() and (a[1] > 0).all()
        seen[which] = int(a[6][0])
        if which == "B":
            assert seen["B"] > 2 * seen["A"] + 50, seen

    return Case(enqueue, [assign, ub, lb, delta, top2, idx, cnt], s.load, canon=canon, check=check, keep=[pool, coef5, exact2, st])


def case_sharded(be):
    """A world of one: the library's two exchanges are the callback's torch copy on the current stream, which is captured like
    the library's own launches."""
    c = FLAT_BY_NAME["list-k15"]
    data = dict(zip("AB", _flat_sets(c)))
    pk = {w: _pack2(be, *data[w], c.mode) for w in "AB"}
    s, pool, keep = Sets(), GuardedPool(be.device), []
    cb, cq = s.packed(pk["A"][0], pk["B"][0]), s.packed(pk["A"][1], pk["B"][1])
    raw = raw_sharded(be, pool, cb, cq, c.k, keep)
    ws = pool.alloc(raw.need, 0)
    return Case(lambda: run_raw(be, raw, ws), raw.outs, s.load, [ws], check=lambda which, a: _check_flat(be, c, *data[which], a[0]),
                keep=[pool, raw, keep])


BUILDERS = {
    **{f"flat/{name}": (lambda be, ivf, name=name: case_flat(be, FLAT_BY_NAME[name])) for name in FLAT_ROUTES},
    "flat/seeded": lambda be, ivf: case_flat(be, FLAT_BY_NAME["list-seeded"], "lvs_flat_search_keys_seeded"),
    "flat/hi": lambda be, ivf: case_flat(be, FLAT_BY_NAME["list-split"], "lvs_flat_search_keys_hi"),
    "flat/hi_banded": lambda be, ivf: case_flat(be, FLAT_BY_NAME["list-split"], "lvs_flat_search_keys_hi_banded"),
    "flat/fallback": lambda be, ivf: case_fallback(be),
    "chain/certified": lambda be, ivf: case_certified(be),
    "chain/nearest3": lambda be, ivf: case_nearest3(be),
    "chain/nearest_hi": lambda be, ivf: case_nearest_hi(be),
    "merge_keys/7x33x10": lambda be, ivf: case_merge_keys(be, 7, 33, 10),
    "merge_keys/20x3x300": lambda be, ivf: case_merge_keys(be, 20, 3, 300),
    "sort_rows_desc": lambda be, ivf: case_sort_rows(be),
    "keys_to_result": lambda be, ivf: case_keys_to_result(be),
    "scores": lambda be, ivf: case_scores(be),
    "range_join/plain": lambda be, ivf: case_range_join(be, False),
    "range_join/self": lambda be, ivf: case_range_join(be, True),
    "pack/d100": lambda be, ivf: case_pack(be, 100, F16),
    "pack/d200": lambda be, ivf: case_pack(be, 200, SPLIT),
    "ivf/build_lists": lambda be, ivf: case_build_lists(be),
    **{f"ivf/{kind}/nprobe{nprobe}": (lambda be, ivf, kind=kind, nprobe=nprobe: case_ivf_search(be, ivf, kind, nprobe))
       for kind in IVF_KINDS for nprobe in (1, 16)},
    "ivf/encode": lambda be, ivf: case_ivf_encode(be, ivf),
    "ivf/range_search": lambda be, ivf: case_ivf_range(be, ivf),
    "ivf/refine_keys": lambda be, ivf: case_refine(be, ivf),
    "ivf/recall": lambda be, ivf: case_recall(be, ivf),
    "kmeans/accumulate": lambda be, ivf: case_accumulate(be),
    "kmeans/objective": lambda be, ivf: case_objective(be),
    "kmeans/update_centroids": lambda be, ivf: case_update_centroids(be),
    "kmeans/bounds": lambda be, ivf: case_bounds(be),
    "search_sharded": lambda be, ivf: case_sharded(be),
}


def test_every_case_of_the_table_has_a_builder():
    assert set(BUILDERS) == set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_captured_once_replayed_on_other_data(hip_backend, ivf, name):  # noqa: F811 - the imported fixture
    """Sentinel after the capture; replay on B, then on A, bit for bit the eager default-stream runs; B takes its branch; the
    searches meet the oracle."""
    be = hip_backend
    case = BUILDERS[name](be, ivf)
    canon = case.canon or (lambda arrays: arrays)
    want = {which: eager(be, case.enqueue, case.outputs, case.load, which, case.scratch) for which in "AB"}
    assert any(a.tobytes() != b.tobytes() for a, b in zip(canon(want["A"]), canon(want["B"]))), "B gives A's result"
    for which in "AB":
        if case.check is not None:
            case.check(which, want[which])
    got = replayed(be, case.enqueue, case.outputs, case.load, case.scratch, order=("B", "A"))
    for which, arrays in zip(("B", "A"), got):
        for i, (a, b) in enumerate(zip(canon(want[which]), canon(arrays))):
            _assert_same_bits(f"{name}: replay on set {which}", i, a, b)
        if case.check is not None:
            case.check(which, arrays)
    for obj in case.keep:
        if isinstance(obj, GuardedPool):
            obj.assert_clean()


# ---- the one entry point that synchronises -----------------------------------------------------------------------------------
def test_kmeans_iteration_orders_its_launches_on_a_side_stream(hip_backend):
    """lvs_kmeans_iteration synchronises `stream` by contract, so it cannot be captured.  Instead: on a non-blocking side
    stream its input buffers hold zeros until an on-stream copy from staging tensors, queued behind a device-side delay on that
    same stream immediately before the call.  Every launch of the call that is ordered on `stream` sees the real inputs; one
    on another stream would run during the delay, on zeros.  The result must equal the eager default-stream result bit for
    bit.  This can MISS a stray launch (one that happens to start late, or whose result does not depend on its inputs); it
    cannot fail falsely; it is not a substitute for the capture the other entries get."""
    be = hip_backend
    pool = GuardedPool(be.device)
    raw = raw_iteration(be, pool)
    e = raw.extra
    ws = pool.alloc(raw.need, 0)
    outputs = raw.outs + [e["cent"]]
    e["reset"]()
    be.synchronize()
    inputs = [e["p"].rows, e["p"].norms, e["x2"], e["cent"], e["rows"], e["norms"], e["cstats"]]
    staged = [t.clone() for t in inputs]
    for t in raw.outs:
        t.view(torch.uint8).fill_(SENT)
    run_raw(be, raw, ws)
    be.synchronize()
    want = [np_(t).copy() for t in outputs]
    assert int(want[2][0]) >= 0 and np.isfinite(want[1][0])
    for t in inputs:
        t.zero_()
    for t in raw.outs:
        t.view(torch.uint8).fill_(SENT)
    ws.fill_(0x5A)
    be.synchronize()
    side = torch.cuda.Stream(device=be.device)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)  # (device time in front of everything below: thousands of launch latencies)
        for t, src in zip(inputs, staged):
            t.copy_(src)
        run_raw(be, raw, ws)
    side.synchronize()
    be.synchronize()
    for i, (t, w) in enumerate(zip(outputs, want)):
        _assert_same_bits("lvs_kmeans_iteration on a side stream", i, w, np_(t))


# ---- the backend's per-stream scratch ----------------------------------------------------------------------------------------
def test_the_backend_keeps_one_scratch_buffer_per_stream(hip_backend):
    """HipBackend._workspace: another buffer under another current stream, the same one when asked again, and the default
    stream's buffer survives the eviction at MAX_STREAM_WORKSPACES.  No kernel runs."""
    from lotus_amd.backend import HipBackend

    be = HipBackend(hip_backend.device)  # (a backend of its own: the shared one keeps its buffers)
    main = be._workspace(1000)
    assert be._stream() == 0 and be._workspace(1000) is main and be._workspace(int(main.numel())) is main
    streams = [torch.cuda.Stream(device=be.device) for _ in range(be.MAX_STREAM_WORKSPACES + 2)]
    seen, kept = {int(main.data_ptr())}, []
    for st in streams:
        with torch.cuda.stream(st):
            ws = be._workspace(1000)
            assert be._workspace(1000) is ws and int(ws.data_ptr()) not in seen
            seen.add(int(ws.data_ptr()))
            kept.append(ws)  # (stays referenced, so no address comes back)
        assert len(be._ws) <= be.MAX_STREAM_WORKSPACES and be._ws[0] is main
    assert be._workspace(1000) is main
    with torch.cuda.stream(streams[-1]):
        assert be._workspace(1000) is kept[-1]  # the latest side stream still has its own
