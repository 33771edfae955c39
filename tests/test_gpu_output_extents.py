"""Outputs and nothing past them; and the refusal of a workspace one byte short.

Raw ctypes calls through ``be.lib``: the inputs are made with the backend, every output (and every workspace) is a tensor
between two guards (tests/ws_guard.py) prefilled with a sentinel byte.  First half: the guards stay clean, the values equal the
same call made through the backend, and elements the header leaves alone keep the sentinel.  Second half: every entry with a
``*_workspace_bytes`` returns LVS_ENOMEM for ``need - 1`` bytes, having written nothing, and succeeds with ``need``.

The library is never told a size larger than the buffer it gets, and never pointed at memory without both guards."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

import oracle
import synth
from extent_cases import F16, FLAT, FLAT_BY_NAME, IP, L2, SPLIT
from lotus_amd import _capi
from test_gpu_workspace_extents import NEEDS_A_COMMUNICATOR, _flat_data, _ivf_index, _pack2, workspace_entries
from ws_guard import GuardedPool, guarded

pytestmark = pytest.mark.gpu

SENT = 0xC3   # outputs
WS_SENT = 0x5A  # workspaces of the refusal half


def P(t):
    return None if t is None else int(t.data_ptr())


def call(be, name, *args):
    with torch.cuda.device(be.device):
        return int(getattr(be.lib, name)(*args))


def ok(be, name, *args):
    rc = call(be, name, *args)
    assert rc == _capi.OK, (name, rc, be.lib.lvs_last_error())


def untouched(t):
    """Does every byte of the (part of a) guarded tensor still hold the output sentinel?"""
    return bool((t.contiguous().view(torch.uint8) == SENT).all())


def np_(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(np_(a)), np.ascontiguousarray(np_(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@dataclass
class Raw:
    """One raw entry point, ready to run: ``run(ws, ws_bytes) -> status``; ``outs``: its guarded outputs; ``entry``: its name."""
    need: int
    run: object
    outs: list = field(default_factory=list)
    entry: str = ""


def _ws(be, pool, raw, fill=0x00):
    return pool.alloc(raw.need, fill)


# ---- builders: every entry that takes a workspace (used by both halves) ------------------------------------------------------
def raw_flat(be, pool, c, cb, cq, name="lvs_flat_search_keys"):
    """``name``: lvs_flat_search_keys or one of its siblings - _seeded (the shard's own sample tiles as seeds), _hi, _hi_banded
    (kc = k - 5 slots inside a narrow band) - which share its size function and its check."""
    keys = guarded(pool, (c.nq, c.k), torch.int64, SENT)
    need = int(be.lib.lvs_flat_search_workspace_bytes(c.nq, c.nb, c.d, c.k, c.mode, c.mode))
    band, seeds, scores = (), (), None
    if name == "lvs_flat_search_keys_hi_banded":
        band = (c.k - 5, 1e-3, 1e-3)
    if name == "lvs_flat_search_keys_seeded":
        tiles = int(be.lib.lvs_flat_search_seed_tiles(c.nq, c.nb, c.k))
        assert tiles > 0
        scores = be.seed_scores(cb, cq, c.metric, tiles)
        seeds = (P(scores), tiles)
    run = lambda ws, n: call(be, name, P(cb.rows), cb.mode, cb.n, P(cq.rows), cq.mode, cq.n, c.d, c.metric, c.k, *band,  # noqa: E731
                             P(cb.norms), P(cq.norms), 0, None, *seeds, P(keys), P(ws), n, be._stream())
    raw = Raw(need, run, [keys], name)
    raw.keep = scores  # (alive as long as the case)
    return raw


def _nearest_inputs(be, nb, nq=300, d=100):
    xb = synth.corpus(nb, d, seed=5) * 1.2
    xq = synth.queries(xb, nq, seed=8)[0].astype(np.float16)
    return be.pack(xb, SPLIT), be.pack(xq, F16)


def raw_nearest_hi(be, pool, cb, cq, metric=L2):
    keys, sec = guarded(pool, (cq.n, 1), torch.int64, SENT), guarded(pool, (cq.n,), torch.float32, SENT)
    need = int(be.lib.lvs_nearest_hi_workspace_bytes(cq.n, cb.n, cb.d))
    run = lambda ws, n: call(be, "lvs_nearest_hi", P(cb.rows), cb.mode, cb.n, P(cq.rows), cq.mode, cq.n, cb.d, metric,  # noqa: E731
                             P(cb.norms), P(cq.norms), 0, P(keys), P(sec), P(ws), n, be._stream())
    return Raw(need, run, [keys, sec], "lvs_nearest_hi")


def raw_nearest3(be, pool, cb, cq, metric=L2):
    keys, keys2 = guarded(pool, (cq.n, 1), torch.int64, SENT), guarded(pool, (cq.n,), torch.int64, SENT)
    sec, third = guarded(pool, (cq.n,), torch.float32, SENT), guarded(pool, (cq.n,), torch.float32, SENT)
    need = int(be.lib.lvs_nearest3_workspace_bytes(cq.n, cb.n, cb.d))
    run = lambda ws, n: call(be, "lvs_nearest3", P(cb.rows), cb.mode, cb.n, P(cq.rows), cq.mode, cq.n, cb.d, metric,  # noqa: E731
                             P(cb.norms), P(cq.norms), 0, P(keys), P(keys2), P(sec), P(third), P(ws), n, be._stream())
    return Raw(need, run, [keys, keys2, sec, third], "lvs_nearest3")


def raw_sort_rows(be, pool, sc, nb, id_offset=9):
    nq, ld = int(sc.shape[0]), int(sc.stride(0))
    keys = guarded(pool, (nq, nb), torch.int64, SENT)
    need = int(be.lib.lvs_sort_rows_workspace_bytes(nq, nb))
    run = lambda ws, n: call(be, "lvs_sort_rows_desc", P(sc), nq, nb, ld, id_offset, P(keys), P(ws), n, be._stream())  # noqa: E731
    return Raw(need, run, [keys], "lvs_sort_rows_desc")


def _accumulate_inputs(be, n=8192 * 2 + 1, d=100, k=37):
    rng = np.random.default_rng(k)
    x = rng.standard_normal((n, d)).astype(np.float16)
    assign = rng.integers(0, k, n).astype(np.int64)
    assign[rng.integers(0, n, 30)] = -1
    return x, assign, be.pack(x, F16), be.to_device(assign)


def raw_accumulate(be, pool, p, a_dev, k, keys=None):
    """``keys`` None: lvs_kmeans_accumulate over ``a_dev``; else lvs_kmeans_accumulate_keys.  sums / counts are in-out: zeros."""
    sums, counts = guarded(pool, (k, p.d), torch.float32, 0x00), guarded(pool, (k,), torch.float32, 0x00)
    need = int(be.lib.lvs_kmeans_accumulate_workspace_bytes(p.n, k))
    if keys is None:
        run = lambda ws, n: call(be, "lvs_kmeans_accumulate", P(p.rows), p.n, p.d, p.mode, P(a_dev), k, P(sums), P(counts),  # noqa: E731
                                 P(ws), n, be._stream())
    else:
        run = lambda ws, n: call(be, "lvs_kmeans_accumulate_keys", P(p.rows), p.n, p.d, p.mode, P(keys), 0, k, P(sums),  # noqa: E731
                                 P(counts), P(ws), n, be._stream())
    return Raw(need, run, [sums, counts], "lvs_kmeans_accumulate" if keys is None else "lvs_kmeans_accumulate_keys")


def raw_objective(be, pool, cent, sums, counts, x2):
    k, d = int(cent.shape[0]), int(cent.shape[1])
    out = guarded(pool, (1,), torch.float64, SENT)
    need = int(be.lib.lvs_kmeans_objective_workspace_bytes(k))
    run = lambda ws, n: call(be, "lvs_kmeans_objective", P(cent), P(sums), P(counts), k, d, P(x2), P(out), P(ws), n,  # noqa: E731
                             be._stream())
    return Raw(need, run, [out], "lvs_kmeans_objective")


def raw_build_lists(be, pool, a_dev, n, nlist):
    off, rows = guarded(pool, (nlist + 1,), torch.int64, SENT), guarded(pool, (n,), torch.int32, SENT)
    need = int(be.lib.lvs_ivf_build_workspace_bytes(n, nlist))
    run = lambda ws, nbytes: call(be, "lvs_ivf_build_lists", P(a_dev), n, nlist, P(off), P(rows), P(ws), nbytes, be._stream())  # noqa: E731
    return Raw(need, run, [off, rows], "lvs_ivf_build_lists")


@pytest.fixture(scope="module")
def ivf(hip_backend):
    """One small IVF index, d = 100 (code rows padded to 128 / 16 bytes), fp16 rows, shared by the IVF cases."""
    be = hip_backend
    nb, d, nq, nlist = 3000, 100, 130, 16
    xb_s, xq_s, packed, lists, qp, off, rows = _ivf_index(be, nb, d, nq, F16, F16, IP, nlist, seed=5)
    vmin, vdiff = be.ivf_sq8_train(packed, lists, np.arange(0, nb, 2))
    sq = be.ivf_sq8_encode(packed, lists, vmin, vdiff)
    M, ksub = 10, 64
    c = np_(be.unpack(lists.centroids))
    where = np.empty(nb, np.int64)
    where[rows.astype(np.int64)] = np.repeat(np.arange(nlist), np.diff(off))
    r = np_(be.unpack(packed)) - c[where]
    rng = np.random.default_rng(1)
    books = np.stack([r[rng.choice(nb, ksub, replace=False), m * (d // M):(m + 1) * (d // M)] for m in range(M)]).astype(np.float32)
    pq = be.ivf_pq_encode(packed, lists, books)
    be.synchronize()
    return dict(nb=nb, d=d, nq=nq, nlist=nlist, packed=packed, lists=lists, qp=qp, sq=sq, pq=pq, books=pq.codebooks)


def _ivf_head(kind, ivf, sel):
    packed, lists, sq, pq = ivf["packed"], ivf["lists"], ivf["sq"], ivf["pq"]
    cpk = lists.centroids
    s = () if sel is None else (P(sel),)
    if kind == "lvs_ivf_search":
        return (P(packed.rows), packed.mode, packed.n, P(packed.norms), P(lists.offsets), P(lists.rows), *s, lists.nlist,
                P(cpk.rows), cpk.mode, P(cpk.norms)), ()
    if kind == "lvs_ivf_sq8_search":
        return (P(sq.codes), P(sq.rnorm), P(sq.vmin), P(sq.vdiff), P(lists.offsets), P(lists.rows), *s, packed.n, lists.nlist,
                P(cpk.rows), cpk.mode, P(cpk.norms), P(sq.centroids)), ()
    return (P(pq.codes), P(pq.beta), P(pq.codebooks), pq.M, pq.ksub, P(lists.offsets), P(lists.rows), *s, packed.n, lists.nlist,
            P(cpk.rows), cpk.mode, P(cpk.norms), P(pq.centroids)), (pq.M,)


def raw_ivf(be, pool, ivf, kind, k, nprobe, sel=None, metric=IP):
    qp = ivf["qp"]
    keys, probe = guarded(pool, (qp.n, k), torch.int64, SENT), guarded(pool, (qp.n, nprobe), torch.int32, SENT)
    head, extra = _ivf_head(kind, ivf, sel)
    need = int(getattr(be.lib, kind + "_workspace_bytes")(qp.n, ivf["nlist"], nprobe, ivf["d"], *extra, k, qp.mode))
    name = kind + "_keys" + ("_sel" if sel is not None else "")
    run = lambda ws, n: call(be, name, *head, P(qp.rows), qp.mode, qp.n, P(qp.norms), ivf["d"], metric, nprobe, k, P(keys),  # noqa: E731
                             P(probe), P(ws), n, be._stream())
    return Raw(need, run, [keys, probe], name)


def raw_ivf_range(be, pool, ivf, nprobe, thr, cap):
    packed, lists, qp = ivf["packed"], ivf["lists"], ivf["qp"]
    cpk = lists.centroids
    oq, oj = guarded(pool, (cap,), torch.int64, SENT), guarded(pool, (cap,), torch.int64, SENT)
    os_ = guarded(pool, (cap,), torch.float32, SENT)
    cnt = guarded(pool, (1,), torch.int64, 0x00)
    need = int(be.lib.lvs_ivf_range_workspace_bytes(qp.n, lists.nlist, nprobe, ivf["d"], qp.mode))
    run = lambda ws, n: call(be, "lvs_ivf_range_search", P(packed.rows), packed.mode, packed.n, P(packed.norms),  # noqa: E731
                             P(lists.offsets), P(lists.rows), None, lists.nlist, P(cpk.rows), cpk.mode, P(cpk.norms), P(qp.rows),
                             qp.mode, qp.n, P(qp.norms), None, ivf["d"], IP, nprobe, thr, 0, cap, P(oq), P(oj), P(os_), P(cnt),
                             P(ws), n, be._stream())
    return Raw(need, run, [oq, oj, os_, cnt], "lvs_ivf_range_search")


def raw_sharded(be, pool, corpus, queries, k, keep):
    """World of one rank; the all-gather callback copies ``send`` to ``recv`` (kept alive in ``keep``)."""
    FN = _capi.CALLBACKS["lvs_all_gather_fn"]

    def gather(ctx, send, recv, nbytes, stream):
        try:
            return _copy(be, send, recv, nbytes)
        except Exception:  # noqa: BLE001 - reported through the status
            return _capi.EDEVICE

    cb = FN(gather)
    keep.append(cb)
    keys = guarded(pool, (queries.n, k), torch.int64, SENT)
    tiles = be.seed_tiles(queries.n, corpus.n, k, F16, F16)
    need = int(be.lib.lvs_search_sharded_workspace_bytes(1, queries.n, corpus.n, corpus.d, k, corpus.mode, queries.mode, tiles))
    run = lambda ws, n: call(be, "lvs_search_sharded", ctypes.cast(cb, ctypes.c_void_p), None, 1, P(corpus.rows), corpus.mode,  # noqa: E731
                             corpus.n, P(queries.rows), queries.mode, queries.n, corpus.d, IP, k, P(corpus.norms), P(queries.norms),
                             0, tiles, P(keys), P(ws), n, be._stream())
    return Raw(need, run, [keys], "lvs_search_sharded")


def _copy(be, send, recv, nbytes):
    from lotus_amd.backend import _DevBytes

    torch.as_tensor(_DevBytes(recv, nbytes), device=be.device).copy_(torch.as_tensor(_DevBytes(send, nbytes), device=be.device))
    return 0


def raw_iteration(be, pool, n=20_001, d=64, K=12):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((n, d)).astype(np.float16)
    p = be.pack(x, F16)
    cent_h = x[:K].astype(np.float32)
    cent = guarded(pool, (K, d), torch.float32, 0x00)
    cent.copy_(be.to_device(cent_h))
    src, _ = be.kmeans_pack_centroids(cent, SPLIT)
    ld = int(src.rows.shape[1])
    rows, norms = guarded(pool, (K, ld), torch.float16, 0x00), guarded(pool, (K,), torch.float32, 0x00)
    cstats = guarded(pool, (2,), torch.float32, 0x00)
    keys, obj = guarded(pool, (n,), torch.int64, SENT), guarded(pool, (1,), torch.float64, SENT)
    nsplit = guarded(pool, (1,), torch.int32, SENT)
    x2 = p.norms.double().sum().reshape(1)
    host_counts = (ctypes.c_int64 * 2)()
    need = int(be.lib.lvs_kmeans_iteration_workspace_bytes(n, d, K, p.mode, SPLIT))

    def reset():
        cent.copy_(be.to_device(cent_h))
        be._c("lvs_kmeans_pack_centroids", P(cent), K, d, SPLIT, P(rows), P(norms), P(cstats), be._stream())

    reset()
    run = lambda ws, nbytes: call(be, "lvs_kmeans_iteration", None, None, P(p.rows), p.mode, n, d, P(p.norms), P(x2), 0, K, n,  # noqa: E731
                                  P(cent), SPLIT, P(rows), P(norms), P(cstats), P(keys), P(obj), P(nsplit),
                                  ctypes.addressof(host_counts), P(ws), nbytes, be._stream())
    raw = Raw(need, run, [keys, obj, nsplit], "lvs_kmeans_iteration")
    raw.extra = dict(p=p, x=x, cent_h=cent_h, cent=cent, reset=reset, K=K, x2=x2, rows=rows, norms=norms, cstats=cstats)
    return raw


# ---- first half: outputs ---------------------------------------------------------------------------------------------------------
OUT_FLAT = ["stream-2blocks", "stream-seeded", "stream-siblings", "rq-1group", "join-ragged-tail", "join-solo", "list-k15",
            "list-k16", "list-seeded", "passes-57", "two-phase-k100", "k-beyond-nb"]


@pytest.mark.parametrize("name", OUT_FLAT)
def test_flat_search_keys_writes_its_keys_only(hip_backend, name):
    """One shape per route; ``join-solo`` is written by the kernel itself, ``k-beyond-nb`` pads with key 0."""
    be, c = hip_backend, FLAT_BY_NAME[name]
    assert {FLAT_BY_NAME[n].route for n in OUT_FLAT} == {x.route for x in FLAT}
    xb, xq = _flat_data(c)
    cb, cq = _pack2(be, xb, xq, c.mode)
    pool = GuardedPool(be.device)
    raw = raw_flat(be, pool, c, cb, cq)
    assert raw.run(_ws(be, pool, raw, 0xFF), raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    assert same(raw.outs[0], be.search_keys(cb, cq, c.k, c.metric, one_pass=False))
    if name == "k-beyond-nb":
        assert bool((raw.outs[0][:, c.nb:] == 0).all()) and bool((raw.outs[0][:, :c.nb] != 0).all())


def _nearest_hi_slabs(be, nq, nb, d):
    """The slab count of lvs_nearest_hi's launch, from its declared size: 256 bytes, then [nslab][nq] keys and [nslab][nq] second
    scores, each rounded up to 256 (lvs_nearest_hi_workspace_bytes)."""
    need = int(be.lib.lvs_nearest_hi_workspace_bytes(nq, nb, d))
    r256 = lambda n: -(-n // 256) * 256  # noqa: E731
    fits = [s for s in range(1, 4097) if 256 + r256(s * nq * 8) + r256(s * nq * 4) == need]
    assert len(fits) == 1, (need, fits)
    return fits[0]


@pytest.mark.parametrize("metric", [IP, L2])
def test_nearest_hi_and_nearest3_outputs(hip_backend, metric):
    """lvs_nearest_hi at ONE slab (300 x 200: the tile kernel itself writes ``out_keys`` / ``out_second``) and at thirteen
    (300 x 16 385: the kernel writes the workspace lists, merge_top2_kernel the outputs); lvs_nearest3: all four outputs."""
    be = hip_backend
    pool = GuardedPool(be.device)
    cb1, cq1 = _nearest_inputs(be, 200)
    assert _nearest_hi_slabs(be, cq1.n, cb1.n, cb1.d) == 1
    hi1 = raw_nearest_hi(be, pool, cb1, cq1, metric)
    assert hi1.run(_ws(be, pool, hi1, 0xFF), hi1.need) == _capi.OK, be.lib.lvs_last_error()
    cb, cq = _nearest_inputs(be, 16385)
    assert _nearest_hi_slabs(be, cq.n, cb.n, cb.d) == 13
    hi = raw_nearest_hi(be, pool, cb, cq, metric)
    assert hi.run(_ws(be, pool, hi, 0xFF), hi.need) == _capi.OK, be.lib.lvs_last_error()
    cb3, cq3 = _nearest_inputs(be, 3 * 256 - 1)
    n3 = raw_nearest3(be, pool, cb3, cq3, metric)
    assert n3.run(_ws(be, pool, n3, 0xFF), n3.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    # the same calls on plain tensors with the backend's scratch
    for raw, (b, q), entry in ((hi1, (cb1, cq1), raw_nearest_hi), (hi, (cb, cq), raw_nearest_hi), (n3, (cb3, cq3), raw_nearest3)):
        plain = GuardedPool(be.device)
        ref = entry(be, plain, b, q, metric)
        ws = be._workspace(ref.need)
        assert ref.run(ws, int(ws.numel())) == _capi.OK
        for a, r in zip(raw.outs, ref.outs):
            assert same(a, r)
    # winner ids: the exact search's, outside near-ties of the hi-only scores
    for raw, (b, q) in ((hi1, (cb1, cq1)), (hi, (cb, cq)), (n3, (cb3, cq3))):
        want = be.search_keys(b, q, 2, metric, one_pass=False)
        Dw, Iw = (np_(t) for t in be.keys_to_result(want, metric))
        _, Ig = (np_(t) for t in be.keys_to_result(raw.outs[0], metric))
        other = Ig[:, 0] != Iw[:, 0]
        # (a hi-only score is off by at most c |q| |lo_row| <= c 2^-11 x 1.2, c = 1 / 2 for IP / L2: 1.2e-3 per score, two scores)
        assert np.all(np.abs(Dw[other, 0] - Dw[other, 1]) <= 3e-3) and other.mean() < 0.05


def test_seed_scores_fill_the_tiles_past_the_shard(hip_backend):
    """[tiles][nq] with nb / 256 < tiles: whole tiles are scored, the rest is -inf, nothing past the block."""
    be = hip_backend
    nq, nb, d, tiles = 129, 256 * 3 + 100, 100, 5
    xb = synth.corpus(nb, d, seed=2)
    xq, _ = synth.queries(xb, nq, seed=3)
    cb, cq = _pack2(be, xb, xq, F16)
    pool = GuardedPool(be.device)
    out = guarded(pool, (tiles, nq), torch.float32, SENT)
    ok(be, "lvs_flat_search_seed_scores", P(cb.rows), cb.mode, nb, P(cq.rows), cq.mode, nq, d, IP, P(cb.norms), P(cq.norms), tiles,
       P(out), be._stream())
    pool.assert_clean()
    assert same(out, be.seed_scores(cb, cq, IP, tiles))
    got = np_(out)
    assert np.all(np.isneginf(got[3:])) and np.all(np.isfinite(got[:3]))
    S = xq.astype(np.float16).astype(np.float32) @ xb.astype(np.float16).astype(np.float32).T
    assert np.abs(got[:3] - np.stack([S[:, 256 * t:256 * t + 256].max(axis=1) for t in range(3)])).max() <= 1e-5


@pytest.mark.parametrize("nparts,nq,k", [(1, 33, 10), (7, 33, 10), (16, 33, 10), (40, 5, 10), (3, 9, 100), (20, 3, 300)])
def test_merge_keys(hip_backend, nparts, nq, k):
    """The three merge kernels: one part, fewer than 16, 16 and more, and k > 64 (folded in rounds)."""
    be = hip_backend
    rng = np.random.default_rng(nparts * 1000 + k)
    sc = rng.standard_normal((nparts, nq, k)).astype(np.float32)
    ids = rng.permutation(nparts * nq * k).reshape(nparts, nq, k).astype(np.int64)
    parts = np.ascontiguousarray(np.sort(oracle.pack_keys(sc, ids), axis=2)[:, :, ::-1])  # every list best first
    parts[-1, :, k - 2:] = 0  # empty slots at a list's end
    want = np.sort(parts.transpose(1, 0, 2).reshape(nq, nparts * k), axis=1)[:, ::-1][:, :k]
    p_dev = be.to_device(parts.view(np.int64))
    pool = GuardedPool(be.device)
    out = guarded(pool, (nq, k), torch.int64, SENT)
    ok(be, "lvs_merge_keys", P(p_dev), nparts, nq, k, P(out), be._stream())
    pool.assert_clean()
    assert np.array_equal(np_(out).view(np.uint64), want)
    assert same(out, be.merge_keys(p_dev))


def test_sort_rows_desc_with_a_wider_leading_dimension(hip_backend):
    be = hip_backend
    nq, nb, ld = 5, 2049, 2049 + 37
    rng = np.random.default_rng(1)
    full = rng.standard_normal((nq, ld)).astype(np.float32)
    full[:, nb:] = 1e9  # columns past nb would win every rank if they were read
    sc = be.to_device(full)[:, :nb]
    pool = GuardedPool(be.device)
    raw = raw_sort_rows(be, pool, sc, nb)
    assert raw.run(_ws(be, pool, raw, 0xFF), raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    ids = np.broadcast_to(np.arange(nb, dtype=np.int64) + 9, (nq, nb))
    assert np.array_equal(np_(raw.outs[0]).view(np.uint64), np.sort(oracle.pack_keys(full[:, :nb], ids), axis=1)[:, ::-1])
    assert same(raw.outs[0], be.rank_scores(sc, id_offset=9))


def test_keys_to_result(hip_backend):
    be = hip_backend
    nq, k = 33, 7
    rng = np.random.default_rng(4)
    keys = oracle.pack_keys(rng.standard_normal((nq, k)).astype(np.float32), rng.integers(0, 50, (nq, k)))
    keys[:, k - 1] = 0
    k_dev = be.to_device(np.ascontiguousarray(keys).view(np.int64))
    id_map = be.to_device(np.arange(50, dtype=np.int64) * 3 + 1)
    pool = GuardedPool(be.device)
    D, I = guarded(pool, (nq, k), torch.float32, SENT), guarded(pool, (nq, k), torch.int64, SENT)
    ok(be, "lvs_keys_to_result", P(k_dev), nq, k, L2, P(id_map), 2, P(D), P(I), be._stream())
    pool.assert_clean()
    Db, Ib = be.keys_to_result(k_dev, L2, id_map, score_exp=2)
    assert same(D, Db) and same(I, Ib)
    better, ids, empty = oracle.unpack_keys(keys)
    assert np.array_equal(np_(I), np.where(empty, -1, ids * 3 + 1))
    assert np.array_equal(np_(D)[~empty], (-better[~empty] * np.float32(0.25)))


@pytest.mark.parametrize("d", [100, 200])      # the scalar and the vector kernel
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("mode", [F16, SPLIT])
def test_pack_rows_and_their_inverse(hip_backend, d, n, mode):
    """lvs_pack_rows / _checked with norms requested and NULL, then lvs_unpack_rows, lvs_gather_rows, lvs_gather_f32."""
    be = hip_backend
    rng = np.random.default_rng(d + n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x_dev = be.to_device(x)
    ld = int(be.lib.lvs_packed_ld(d, mode))
    pool = GuardedPool(be.device)
    rows, norms = guarded(pool, (n, ld), torch.float16, SENT), guarded(pool, (n,), torch.float32, SENT)
    rows2 = guarded(pool, (n, ld), torch.float16, SENT)
    rows3, norms3, flags = guarded(pool, (n, ld), torch.float16, SENT), guarded(pool, (n,), torch.float32, SENT), guarded(pool, (1,), torch.int32, 0)
    ok(be, "lvs_pack_rows", P(x_dev), _capi.DTYPE_F32, n, d, mode, 0, P(rows), P(norms), be._stream())
    ok(be, "lvs_pack_rows", P(x_dev), _capi.DTYPE_F32, n, d, mode, 0, P(rows2), None, be._stream())
    ok(be, "lvs_pack_rows_checked", P(x_dev), _capi.DTYPE_F32, n, d, mode, 0, 0, P(rows3), P(norms3), P(flags), be._stream())
    pool.assert_clean()
    ref = be.pack(x_dev, mode)
    assert same(rows, ref.rows) and same(rows2, ref.rows) and same(rows3, ref.rows)
    assert same(norms, ref.norms) and same(norms3, ref.norms) and int(flags.item()) == 0
    ids = be.to_device(rng.integers(0, n, 2 * n + 3).astype(np.int64))
    m = int(ids.numel())
    vals, g_rows, g_norms = (guarded(pool, (m, d), torch.float32, SENT), guarded(pool, (m, ld), torch.float16, SENT),
                             guarded(pool, (m,), torch.float32, SENT))
    all_vals = guarded(pool, (n, d), torch.float32, SENT)
    ok(be, "lvs_unpack_rows", P(rows), d, mode, P(ids), m, 0, P(vals), be._stream())
    ok(be, "lvs_unpack_rows", P(rows), d, mode, None, n, 0, P(all_vals), be._stream())
    ok(be, "lvs_gather_rows", P(rows), ld, P(ids), m, P(g_rows), be._stream())
    ok(be, "lvs_gather_f32", P(norms), P(ids), m, P(g_norms), be._stream())
    pool.assert_clean()
    assert same(vals, be.unpack(ref, ids)) and same(all_vals, be.unpack(ref))
    g = be.gather(ref, ids)
    assert same(g_rows, g.rows) and same(g_norms, g.norms)
    stored = x.astype(np.float16).astype(np.float32) if mode == F16 else x
    assert np.abs(np_(all_vals) - stored).max() <= (0 if mode == F16 else 2.0 ** -20 * np.abs(x).max())


@pytest.mark.parametrize("self_join", [False, True])
def test_range_join_capacity_is_a_wall(hip_backend, self_join):
    """``capacity`` below the hit count: nothing at or past it in out_q / out_j / out_s, and the count is the true count."""
    be = hip_backend
    n, d, thr = 3000, 100, 0.25
    xb = synth.corpus(n, d, seed=6)
    xb[1::2] = 0.8 * xb[::2] + 0.6 * synth.corpus(n // 2, d, seed=7)
    x16 = xb.astype(np.float16)
    cb = be.pack(x16, F16)
    cq = cb if self_join else be.pack(x16[:700], F16)
    q0 = 0 if self_join else -1
    fq, fj, fs = be.range_join(cb, cq, thr, IP, q_row0=q0)
    true = int(fq.numel())
    S = x16[:cq.n].astype(np.float32) @ x16.astype(np.float32).T
    hits = S > thr
    if self_join:
        hits &= np.arange(n)[None, :] > np.arange(cq.n)[:, None]
    assert abs(true - int(hits.sum())) <= int((np.abs(S - thr) < 1e-5).sum()) and true > 3000
    cap = true // 3
    pool = GuardedPool(be.device)
    oq, oj = guarded(pool, (cap + 64,), torch.int64, SENT), guarded(pool, (cap + 64,), torch.int64, SENT)
    os_, cnt = guarded(pool, (cap + 64,), torch.float32, SENT), guarded(pool, (1,), torch.int64, 0)
    ok(be, "lvs_range_join", P(cb.rows), cb.mode, cb.n, P(cq.rows), cq.mode, cq.n, d, IP, P(cb.norms), P(cq.norms), thr, 0, q0, 0,
       1, 0, cap, P(oq), P(oj), P(os_), P(cnt), be._stream())
    pool.assert_clean()
    assert int(cnt.item()) == true
    assert untouched(oq[cap:]) and untouched(oj[cap:]) and untouched(os_[cap:])
    code = lambda q, j: np_(q) * n + np_(j)  # noqa: E731
    got, full = code(oq[:cap], oj[:cap]), code(fq, fj)
    assert np.unique(got).size == cap and np.isin(got, full).all()  # every stored triple is a pair of the full result, once
    order = np.argsort(full)
    at = order[np.searchsorted(full[order], got)]
    assert np.array_equal(np_(os_[:cap]), np_(fs)[at])


@pytest.mark.parametrize("kind", ["lvs_ivf_search", "lvs_ivf_sq8_search", "lvs_ivf_pq_search"])
@pytest.mark.parametrize("nprobe,use_sel", [(1, False), (16, True)])
def test_ivf_search_keys_and_probes(hip_backend, ivf, kind, nprobe, use_sel):
    be = hip_backend
    k = 10
    sel = be.row_bitmap(np.arange(0, ivf["nb"], 3), ivf["nb"])[0] if use_sel else None
    pool = GuardedPool(be.device)
    raw = raw_ivf(be, pool, ivf, kind, k, nprobe, sel)
    assert raw.run(_ws(be, pool, raw, 0xFF), raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    extra = {"lvs_ivf_search": (), "lvs_ivf_sq8_search": (ivf["sq"],), "lvs_ivf_pq_search": (ivf["pq"],)}[kind]
    keys, probe = getattr(be, kind[4:])(ivf["packed"], ivf["lists"], *extra, ivf["qp"], k, IP, nprobe, want_probe=True, sel=sel)
    assert same(raw.outs[0], keys) and same(raw.outs[1], probe)


def test_ivf_encoders_pad_their_code_rows(hip_backend, ivf):
    """codes [n][ldc] at d = 100: SQ8 rows of 128 bytes, PQ (M = 10) rows of 16; bytes past d / M are 0; the norms."""
    be = hip_backend
    packed, lists, sq, pq = ivf["packed"], ivf["lists"], ivf["sq"], ivf["pq"]
    n, d = packed.n, ivf["d"]
    pool = GuardedPool(be.device)
    codes, rn = guarded(pool, (n, 128), torch.uint8, SENT), guarded(pool, (n,), torch.float32, SENT)
    ok(be, "lvs_ivf_sq8_encode", P(packed.rows), packed.mode, n, d, P(lists.offsets), P(lists.rows), lists.nlist, P(sq.centroids),
       P(sq.vmin), P(sq.vdiff), P(codes), P(rn), be._stream())
    pcodes, beta = guarded(pool, (n, 16), torch.uint8, SENT), guarded(pool, (n,), torch.float32, SENT)
    ok(be, "lvs_ivf_pq_encode", P(packed.rows), packed.mode, n, d, P(lists.offsets), P(lists.rows), lists.nlist, P(pq.centroids),
       pq.M, pq.ksub, P(pq.codebooks), P(pcodes), P(beta), be._stream())
    pool.assert_clean()
    assert tuple(sq.codes.shape) == (n, 128) and tuple(pq.codes.shape) == (n, 16)
    assert same(codes, sq.codes) and same(rn, sq.rnorm) and same(pcodes, pq.codes) and same(beta, pq.beta)
    assert bool((codes[:, d:] == 0).all()) and bool((pcodes[:, pq.M:] == 0).all())


def test_ivf_build_lists(hip_backend):
    """offsets [nlist + 1], rows [n] (what stands past offsets[nlist] - assignments out of range - is unspecified)."""
    be = hip_backend
    n, nlist = 8192 * 2 + 77, 37
    rng = np.random.default_rng(3)
    assign = rng.integers(0, nlist, n).astype(np.int64)
    assign[rng.choice(n, 100, replace=False)] = nlist + 3
    a_dev = be.to_device(assign)
    pool = GuardedPool(be.device)
    raw = raw_build_lists(be, pool, a_dev, n, nlist)
    assert raw.run(_ws(be, pool, raw, 0xFF), raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    off, rows = np_(raw.outs[0]), np_(raw.outs[1]).view(np.uint32)
    keep = assign < nlist
    order = np.argsort(assign[keep], kind="stable")
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(assign[keep], minlength=nlist))]))
    assert off[-1] == n - 100 and np.array_equal(rows[:n - 100], np.flatnonzero(keep)[order].astype(np.uint32))


def test_refine_keys(hip_backend, ivf):
    be = hip_backend
    packed, qp = ivf["packed"], ivf["qp"]
    kc, k = 40, 7
    cand = be.ivf_pq_search(packed, ivf["lists"], ivf["pq"], qp, kc, IP, 4)
    pool = GuardedPool(be.device)
    out = guarded(pool, (qp.n, k), torch.int64, SENT)
    ok(be, "lvs_refine_keys", P(packed.rows), packed.mode, packed.n, P(packed.norms), P(qp.rows), qp.mode, qp.n, P(qp.norms),
       ivf["d"], IP, P(cand), kc, k, P(out), be._stream())
    pool.assert_clean()
    assert same(out, be.refine_keys(packed, qp, cand, k, IP))


def test_kmeans_accumulate_and_update_centroids(hip_backend):
    """sums [k][d] at d = 100 (one wave per centroid and 128 columns: the last 28 lanes idle); then the division with a repack."""
    be = hip_backend
    k = 37
    x, assign, p, a_dev = _accumulate_inputs(be, k=k)
    pool = GuardedPool(be.device)
    raw = raw_accumulate(be, pool, p, a_dev, k)
    assert raw.run(_ws(be, pool, raw, 0xFF), raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    sums, counts = raw.outs
    keep = assign >= 0
    ref = np.zeros((k, p.d), np.float32)
    np.add.at(ref, assign[keep], x.astype(np.float32)[keep])
    assert np.array_equal(np_(sums), ref) and np.array_equal(np_(counts), np.bincount(assign[keep], minlength=k).astype(np.float32))
    bs, bc = be.kmeans_accumulate(p, a_dev, k)
    assert same(sums, bs) and same(counts, bc)
    # lvs_kmeans_update_centroids with a repack: centroids in place, the hi|lo image, its norms and statistics
    ld = int(be.lib.lvs_packed_ld(p.d, SPLIT))
    cent = guarded(pool, (k, p.d), torch.float32, 0x00)
    rows, norms = guarded(pool, (k, ld), torch.float16, SENT), guarded(pool, (k,), torch.float32, SENT)
    cstats, nsplit = guarded(pool, (2,), torch.float32, SENT), guarded(pool, (1,), torch.int32, SENT)
    c2 = counts.clone()
    ok(be, "lvs_kmeans_update_centroids", P(sums), P(c2), k, p.d, p.n, P(cent), P(nsplit), SPLIT, P(rows), P(norms), P(cstats),
       be._stream())
    pool.assert_clean()
    cent_b = torch.zeros((k, p.d), dtype=torch.float32, device=be.device)
    ns_b = torch.zeros(1, dtype=torch.int32, device=be.device)
    pk, st = be.kmeans_finish(bs, bc.clone(), cent_b, p.n, SPLIT, ns_b)
    assert same(cent, cent_b) and same(rows, pk.rows) and same(norms, pk.norms) and same(cstats, st) and same(nsplit, ns_b)
    assert np.array_equal(np_(cent), ref * (np.float32(1.0) / np_(counts))[:, None])


# ---- second half: one byte short is refused, and nothing was written -------------------------------------------------------
def _refusal_case(be, pool, name, ivf, keep):
    if name == "lvs_flat_search_workspace_bytes":
        c = FLAT_BY_NAME["two-phase-k2048"]  # the two-phase plan is the larger layout here (its buckets: 32 KiB per query)
        from extent_cases import planner_says

        says = planner_says(c)
        assert says["tp_bytes"] == says["bytes"]
        cb, cq = _pack2(be, *_flat_data(c), c.mode)
        return raw_flat(be, pool, c, cb, cq)
    if name.startswith("lvs_flat_search_workspace_bytes/"):
        c = FLAT_BY_NAME["list-seeded" if name.endswith("/seeded") else "list-k15"]
        cb, cq = _pack2(be, *_flat_data(c), c.mode)
        return raw_flat(be, pool, c, cb, cq, REFUSALS[name])
    if name == "lvs_search_sharded_workspace_bytes":
        c = FLAT_BY_NAME["list-k15"]
        cb, cq = _pack2(be, *_flat_data(c), c.mode)
        return raw_sharded(be, pool, cb, cq, c.k, keep)
    if name == "lvs_sort_rows_workspace_bytes":
        return raw_sort_rows(be, pool, be.to_device(np.random.default_rng(0).standard_normal((3, 4097)).astype(np.float32)), 4097)
    if name == "lvs_nearest_hi_workspace_bytes":
        return raw_nearest_hi(be, pool, *_nearest_inputs(be, 16385))
    if name == "lvs_nearest_hi_workspace_bytes/one-slab":
        return raw_nearest_hi(be, pool, *_nearest_inputs(be, 200))
    if name == "lvs_nearest3_workspace_bytes":
        return raw_nearest3(be, pool, *_nearest_inputs(be, 3 * 256 - 1))
    if name.startswith("lvs_kmeans_accumulate_workspace_bytes"):
        x, assign, p, a_dev = _accumulate_inputs(be)
        keys = be.to_device(np.ascontiguousarray(oracle.pack_keys(np.zeros(p.n, np.float32), np.maximum(assign, 0))).view(np.int64))
        return raw_accumulate(be, pool, p, a_dev, 37, keys if name.endswith("/keys") else None)
    if name == "lvs_kmeans_objective_workspace_bytes":
        x, assign, p, a_dev = _accumulate_inputs(be)
        sums, counts = be.kmeans_accumulate(p, a_dev, 37)
        return raw_objective(be, pool, be.to_device(x[:37].astype(np.float32)), sums, counts, p.norms.double().sum().reshape(1))
    if name == "lvs_kmeans_iteration_workspace_bytes":
        return raw_iteration(be, pool)
    if name == "lvs_ivf_build_workspace_bytes":
        n, nlist = 8192 * 2 + 77, 37
        return raw_build_lists(be, pool, be.to_device(np.random.default_rng(3).integers(0, nlist, n).astype(np.int64)), n, nlist)
    if name == "lvs_ivf_range_workspace_bytes":
        return raw_ivf_range(be, pool, ivf, 5, 0.3, 1 << 16)
    kind = name.split("/")[0][:-len("_workspace_bytes")]
    sel = be.row_bitmap(np.arange(0, ivf["nb"], 3), ivf["nb"])[0] if name.endswith("/sel") else None
    return raw_ivf(be, pool, ivf, kind, 10, 5, sel)


# case -> the entry point it calls (a size function may serve several entries: every one of them has a case)
REFUSALS = {
    "lvs_flat_search_workspace_bytes": "lvs_flat_search_keys",
    "lvs_flat_search_workspace_bytes/one-pass": "lvs_flat_search_keys",
    "lvs_flat_search_workspace_bytes/seeded": "lvs_flat_search_keys_seeded",
    "lvs_flat_search_workspace_bytes/hi": "lvs_flat_search_keys_hi",
    "lvs_flat_search_workspace_bytes/hi_banded": "lvs_flat_search_keys_hi_banded",
    "lvs_search_sharded_workspace_bytes": "lvs_search_sharded",
    "lvs_sort_rows_workspace_bytes": "lvs_sort_rows_desc",
    "lvs_nearest_hi_workspace_bytes": "lvs_nearest_hi",
    "lvs_nearest_hi_workspace_bytes/one-slab": "lvs_nearest_hi",
    "lvs_nearest3_workspace_bytes": "lvs_nearest3",
    "lvs_kmeans_accumulate_workspace_bytes": "lvs_kmeans_accumulate",
    "lvs_kmeans_accumulate_workspace_bytes/keys": "lvs_kmeans_accumulate_keys",
    "lvs_kmeans_objective_workspace_bytes": "lvs_kmeans_objective",
    "lvs_kmeans_iteration_workspace_bytes": "lvs_kmeans_iteration",
    "lvs_ivf_build_workspace_bytes": "lvs_ivf_build_lists",
    "lvs_ivf_search_workspace_bytes": "lvs_ivf_search_keys",
    "lvs_ivf_search_workspace_bytes/sel": "lvs_ivf_search_keys_sel",
    "lvs_ivf_sq8_search_workspace_bytes": "lvs_ivf_sq8_search_keys",
    "lvs_ivf_sq8_search_workspace_bytes/sel": "lvs_ivf_sq8_search_keys_sel",
    "lvs_ivf_pq_search_workspace_bytes": "lvs_ivf_pq_search_keys",
    "lvs_ivf_pq_search_workspace_bytes/sel": "lvs_ivf_pq_search_keys_sel",
    "lvs_ivf_range_workspace_bytes": "lvs_ivf_range_search",
}


@pytest.mark.parametrize("name", REFUSALS)
def test_one_byte_short_is_refused_and_nothing_is_written(hip_backend, ivf, name):
    be = hip_backend
    pool, keep = GuardedPool(be.device), []
    raw = _refusal_case(be, pool, name, ivf, keep)
    assert raw.need > 1 and raw.entry == REFUSALS[name]
    before = [np_(t).tobytes() for t in raw.outs]
    ws = pool.alloc(raw.need, WS_SENT)
    rc = raw.run(ws, raw.need - 1)  # (the buffer itself has `need` bytes: the library is never told more than it gets)
    be.synchronize()
    assert rc == _capi.ENOMEM, (rc, be.lib.lvs_last_error())
    assert bool((ws == WS_SENT).all()), "the refused call wrote to its workspace"
    for t, b in zip(raw.outs, before):
        assert np_(t).tobytes() == b, "the refused call wrote to an output"
    pool.assert_clean()
    assert raw.run(ws, raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()
    if name == "lvs_kmeans_iteration_workspace_bytes":  # ... and the accepted call is the launch-by-launch iteration
        e = raw.extra
        got = np_(e["cent"]).copy()
        c_dev = be.to_device(e["cent_h"])
        cpk, cstats = be.kmeans_pack_centroids(c_dev, SPLIT)
        keys = be.nearest(cpk, e["p"], L2, exact_scores=False, corpus_stats=cstats)
        sums, counts = be.kmeans_accumulate_keys(e["p"], keys, e["K"])
        be.kmeans_finish(sums, counts, c_dev, e["p"].n, SPLIT)
        assert np.array_equal(got, np_(c_dev))


@pytest.mark.parametrize("name", REFUSALS)  # every entry that takes a workspace has the check
def test_a_misaligned_workspace_is_refused(hip_backend, ivf, name):
    """Every layout rounds its regions to 256 bytes from the base (include/lotus_hip.h): a base 8 bytes off is LVS_EINVAL, and
    nothing is written."""
    be = hip_backend
    pool, keep = GuardedPool(be.device), []
    raw = _refusal_case(be, pool, name, ivf, keep)
    assert raw.entry == REFUSALS[name]
    before = [np_(t).tobytes() for t in raw.outs]
    ws = pool.alloc(raw.need + 256, WS_SENT)
    assert raw.run(ws[8:], raw.need) == _capi.EINVAL, be.lib.lvs_last_error()
    be.synchronize()
    assert bool((ws == WS_SENT).all()) and all(np_(t).tobytes() == b for t, b in zip(raw.outs, before))
    pool.assert_clean()
    assert raw.run(ws[256:], raw.need) == _capi.OK, be.lib.lvs_last_error()
    pool.assert_clean()


def test_every_size_function_and_entry_has_a_refusal_case():
    """... and so has every entry point of the header with a ``workspace_bytes`` argument (the two behind an RCCL communicator
    apart: they are lvs_search_sharded and lvs_kmeans_iteration with another reduction)."""
    have = {name for name in _capi.SIGNATURES if name.endswith("_workspace_bytes")}
    assert have == {name.split("/")[0] for name in REFUSALS}, have ^ {name.split("/")[0] for name in REFUSALS}
    assert set(REFUSALS.values()) == workspace_entries() - NEEDS_A_COMMUNICATOR
