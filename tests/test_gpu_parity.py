"""GPU parity tests proper: the HIP path (through the C-ABI, via lotus_amd.backend.HipBackend) against the CPU
oracle on identical seeded inputs.  Bars (BASELINE.json north_star / SURVEY.md 8(c)): ids identical wherever the
oracle's neighbouring scores are > 2e-5 apart, scores within 1e-5 (fp32), recall@k = 1.0."""
import numpy as np
import pytest

import oracle
import synth
from lotus_amd import _capi

pytestmark = pytest.mark.gpu

F16, SPLIT = _capi.PACK_F16, _capi.PACK_SPLIT
IP, L2 = _capi.METRIC_IP, _capi.METRIC_L2


def _stored(x, mode):
    """What the oracle must consume so that only summation order differs from the device."""
    if mode == F16:
        return x.astype(np.float16).astype(np.float32)
    return x.astype(np.float32)


def _run(be, xb, xq, k, mode, metric, **kw):
    cb = be.pack(xb.astype(np.float16) if mode == F16 else xb, mode)
    cq = be.pack(xq.astype(np.float16) if mode == F16 else xq, mode)
    keys = be.search_keys(cb, cq, k, metric, **kw)
    D, I = be.keys_to_result(keys, metric)
    be.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), keys.cpu().numpy().view(np.uint64)


CASES = [
    # nq, nb, d, k, mode, metric
    (1000, 10000, 384, 5, SPLIT, IP),   # BASELINE configs[0] shape on the fp32-accurate path
    (300, 5000, 768, 10, F16, IP),
    (77, 1013, 100, 7, F16, IP),        # ragged rows, d not a multiple of 64
    (129, 257, 64, 1, F16, IP),
    (5, 3, 8, 5, F16, IP),              # k > nb -> padding
    (1, 1000, 768, 10, F16, IP),        # the literal single-query sem_search shape
    (300, 4000, 384, 15, F16, IP),      # largest k of the 256-query geometry
    (300, 4000, 384, 16, F16, IP),      # smallest k of the 128-query / 56-slot geometry
    (200, 3000, 384, 24, F16, IP),
    (200, 3000, 384, 56, F16, IP),      # largest single-pass k
    (200, 3000, 384, 57, F16, IP),      # two passes (56 + 1: the second pass has a tiny k on the 128-query geometry)
    (64, 3000, 128, 100, F16, IP),      # two passes (56 + 44)
    (40, 2000, 64, 200, F16, L2),       # four passes, L2
    (1500, 100000, 768, 20, F16, IP),   # 128-query geometry with several slabs and shared thresholds
    (300, 60000, 384, 100, F16, IP),    # k > 56: two-phase (15-per-slab lists -> threshold key -> collect -> sort)
    (64, 80000, 128, 300, F16, L2),
    (10, 120000, 64, 1000, F16, IP),
    (40, 150000, 100, 2048, SPLIT, IP), # LVS_MAX_K
    (130, 3000, 200, 30, SPLIT, IP),    # fp32-accurate operands on the 128-query geometry
    (300, 5000, 768, 10, F16, L2),
    (300, 5000, 384, 10, SPLIT, L2),
    (2048, 200000, 768, 10, F16, IP),   # many slabs, shared thresholds
]


@pytest.mark.parametrize("nq,nb,d,k,mode,metric", CASES)
def test_search_parity(hip_backend, nq, nb, d, k, mode, metric):
    xb = synth.corpus(nb, d, seed=nb % 97)
    xq, _ = synth.queries(xb, nq, seed=3)
    if metric == L2:
        xb = xb * 1.5  # break the unit norm so the norm terms matter
    D, I, _ = _run(hip_backend, xb, xq, k, mode, metric)
    Dr, Ir = oracle.flat_search(_stored(xb, mode), _stored(xq, mode), k, metric)
    atol = 1e-5  # (r6) north_star's bar for both metrics - squared-L2 values of the x 1.5-scaled cases are O(1..6)
    err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=atol)
    assert (I >= 0).sum() == (Ir >= 0).sum()
    assert err <= atol, f"score error {err}"
    assert hard == 0, f"{hard} id mismatches outside near-ties"
    assert recall >= 0.9999, recall
    if mode == F16 and metric == IP:
        assert (I == Ir).mean() > 0.999  # identical inputs: only summation-order near-ties may swap


@pytest.mark.parametrize("cmode,qmode", [(F16, SPLIT), (SPLIT, F16)])
@pytest.mark.parametrize("k", [1, 7, 20])
def test_mixed_precision_operands(hip_backend, cmode, qmode, k):
    """fp16-stored rows on one side, fp32-accurate (hi|lo) rows on the other: two K segments."""
    be = hip_backend
    xb = synth.corpus(3000, 200, seed=12) * 1.2
    xq, _ = synth.queries(xb, 260, seed=5)
    cb = be.pack(xb.astype(np.float16) if cmode == F16 else xb, cmode)
    cq = be.pack(xq.astype(np.float16) if qmode == F16 else xq, qmode)
    for metric in (IP, L2):
        D, I = be.keys_to_result(be.search_keys(cb, cq, k, metric), metric)
        Dr, Ir = oracle.flat_search(_stored(xb, cmode), _stored(xq, qmode), k, metric)
        err, hard, recall = synth.compare_topk(Dr, Ir, D.cpu().numpy(), I.cpu().numpy(), atol=3e-5)
        assert err <= 3e-5 and hard == 0 and recall >= 0.9999


@pytest.mark.parametrize("nq,nb,d,k,mode,metric", [
    (1, 100_000, 768, 10, F16, IP),    # the literal sem_search call
    (7, 50_001, 384, 5, SPLIT, IP),    # fp32-accurate path, ragged row count
    (32, 30_000, 100, 15, F16, IP),    # full query block, padded d
    (5, 60_000, 384, 56, F16, IP),     # largest k of the streaming path (sem_search's K-doubling asks for more than k)
    (1, 100_000, 768, 40, F16, L2),
    (3, 20_000, 768, 1, F16, L2),
    (20, 40_000, 256, 10, SPLIT, L2),
    (64, 50_000, 768, 10, F16, IP),    # two blocks of 32 queries on one corpus pass
    (96, 30_000, 384, 15, F16, L2),    # three blocks, d = 384 (24 fragments per row: the 8-deep pipeline)
    (33, 20_000, 256, 16, F16, IP),    # second block nearly empty; k = 16 fills the 16-slot lists exactly
    (50, 20_000, 128, 30, F16, IP),    # 32-slot lists
    (90, 12_000, 100, 56, F16, IP),    # 64-slot lists, three blocks (short rows leave the LDS for them)
    (70, 9_000, 768, 5, SPLIT, IP),    # fp32-accurate queries do not fit twice: falls to the tile kernel
    (40, 200_000, 256, 10, F16, IP),   # long corpus + several queries: sample pass seeds the shared thresholds
    (96, 150_000, 128, 15, F16, L2),
    (8, 70_000, 768, 56, F16, IP),
    (96, 90_000, 768, 10, F16, IP),    # three blocks of 32 queries in one workgroup per corpus range, seeded thresholds
    (128, 140_000, 768, 10, F16, IP),  # beyond one sibling group: the seeded list kernel (one 128-query tile)
    (129, 70_000, 256, 10, F16, L2),   # one 256-query tile, half empty, seeded from 16 sample tiles
    (200, 66_000, 384, 15, F16, IP),   # list kernel; the corpus just allows a sample (>= 16 x 15 tiles)
    (256, 100_000, 768, 10, F16, IP),  # a full 256-query tile x many slabs, seeded
    (256, 30_000, 128, 56, F16, L2),   # corpus too short to seed: the stream kernel with 4 sibling groups x 64 queries
    (100, 80_000, 768, 10, SPLIT, IP), # fp32-accurate queries need 4 sibling groups: the seeded list kernel instead
    (130, 20_000, 768, 10, SPLIT, IP), # ... five blocks do not fit four groups: the tile kernel
    (2, 300_000, 768, 10, F16, IP),    # two queries are seeded too
])
def test_small_batch_streaming_kernel(hip_backend, nq, nb, d, k, mode, metric):
    """Small batches: the HBM-streaming kernel (lvs_stream.hip) while one workgroup per corpus range holds all queries
    (<= 96 fp16 queries at d = 768) or the corpus is too short to seed, the seeded list kernel beyond - same results as
    the oracle either way."""
    xb = synth.corpus(nb, d, seed=nb % 89)
    xq, _ = synth.queries(xb, nq, seed=13)
    if metric == L2:
        xb = xb * 1.4
    D, I, _ = _run(hip_backend, xb, xq, k, mode, metric)
    Dr, Ir = oracle.flat_search(_stored(xb, mode), _stored(xq, mode), k, metric)
    atol = 1e-5  # (r6) one bar for both metrics
    err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=atol)
    assert err <= atol and hard == 0 and recall == 1.0
    # duplicates: exact ties keep the oracle's id order on this path too
    xd = np.concatenate([xb[:5000], xb[:5000]])
    D, I, _ = _run(hip_backend, xd, xq, min(k, 8), mode, metric)
    Dr, Ir = oracle.flat_search(_stored(xd, mode), _stored(xq, mode), min(k, 8), metric)
    assert np.array_equal(I, Ir)


def test_duplicates_follow_the_total_order(hip_backend):
    """Exact duplicate rows give exactly equal scores; ids must come back ascending inside each tie group."""
    base = synth.corpus(50, 128, seed=5)
    xb = np.concatenate([base, base, base[:17]], axis=0)  # rows i, i+50 (and i+100) identical
    xq, _ = synth.queries(base, 40, seed=9)
    D, I, _ = _run(hip_backend, xb, xq, 12, F16, IP)
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), 12, IP)
    assert np.array_equal(I, Ir)
    assert np.abs(D - Dr).max() <= 1e-5


def test_ascending_scores_stress_overflow_rounds(hip_backend):
    """Every later row beats all earlier ones: every tile overflows the candidate lists (worst case)."""
    d = 64
    q = np.zeros((130, d), np.float32)
    q[:, 0] = 1.0
    q[:, 1] = np.linspace(0.1, 1.0, 130)
    n = 3000
    xb = np.zeros((n, d), np.float32)
    xb[:, 0] = np.arange(n) / n
    xb[:, 2] = 0.25
    D, I, _ = _run(hip_backend, xb, q, 10, F16, IP)
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(q, F16), 10, IP)
    assert np.array_equal(I, Ir)
    assert np.abs(D - Dr).max() <= 1e-5


def test_row_ids_and_offset(hip_backend):
    be = hip_backend
    xb = synth.corpus(700, 64, seed=2)
    xq, _ = synth.queries(xb, 33, seed=4)
    cb, cq = be.pack(xb.astype(np.float16), F16), be.pack(xq.astype(np.float16), F16)
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), 6, IP)
    keys = be.search_keys(cb, cq, 6, IP, id_offset=123456)
    D, I = be.keys_to_result(keys, IP)
    assert np.array_equal(I.cpu().numpy(), Ir + 123456)
    perm = np.random.default_rng(0).permutation(700).astype(np.uint32)
    keys = be.search_keys(cb, cq, 6, IP, row_ids=be.to_device(perm.view(np.int32)))
    D, I = be.keys_to_result(keys, IP)
    I = I.cpu().numpy()
    ok = I == perm[Ir]
    assert ok.mean() > 0.99  # remapped ids reorder exact ties only
    assert np.abs(D.cpu().numpy() - Dr).max() <= 1e-5


def test_gather_subset_equals_search_on_gathered_rows(hip_backend):
    be = hip_backend
    xb = synth.corpus(1500, 128, seed=8)
    xq, _ = synth.queries(xb, 50, seed=1)
    ids = np.random.default_rng(1).choice(1500, 400, replace=False).astype(np.int64)
    cb, cq = be.pack(xb.astype(np.float16), F16), be.pack(xq.astype(np.float16), F16)
    g = be.gather(cb, be.to_device(ids))
    keys = be.search_keys(g, cq, 9, IP)
    D, I = be.keys_to_result(keys, IP, id_map=be.to_device(ids))
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), 9, IP, ids=ids)
    assert np.array_equal(I.cpu().numpy(), Ir)
    assert np.abs(D.cpu().numpy() - Dr).max() <= 1e-5


def test_scores_matrix(hip_backend):
    be = hip_backend
    for mode, tol in ((F16, 2e-6), (SPLIT, 1e-5)):
        xb = synth.corpus(777, 200, seed=3) * 2.0
        xq, _ = synth.queries(xb, 150, seed=6)
        cb = be.pack(xb.astype(np.float16) if mode == F16 else xb, mode)
        cq = be.pack(xq.astype(np.float16) if mode == F16 else xq, mode)
        S = be.scores(cb, cq, IP).cpu().numpy()
        ref = _stored(xq, mode).astype(np.float64) @ _stored(xb, mode).astype(np.float64).T
        assert np.abs(S - ref).max() <= tol * max(1.0, np.abs(ref).max())
        S2 = be.scores(cb, cq, L2).cpu().numpy()
        a, b = _stored(xq, mode).astype(np.float64), _stored(xb, mode).astype(np.float64)
        ref2 = -np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * a @ b.T, 0)
        assert np.abs(S2 - ref2).max() <= 2e-5 * max(1.0, np.abs(ref2).max())


def test_pack_rows_values_and_norms(hip_backend):
    be = hip_backend
    x = (synth.corpus(300, 100, seed=1) * 3).astype(np.float32)
    p = be.pack(x, F16)
    rows = p.rows.cpu().numpy()
    assert rows.shape == (300, 128)
    assert np.array_equal(rows[:, :100], x.astype(np.float16))
    assert not rows[:, 100:].any()
    st = x.astype(np.float16).astype(np.float32)
    assert np.allclose(p.norms.cpu().numpy(), (st * st).sum(1), rtol=1e-6)
    p2 = be.pack(x, SPLIT)
    r2 = p2.rows.cpu().numpy().astype(np.float32)
    assert r2.shape == (300, 256)
    assert np.abs((r2[:, :100] + r2[:, 128:228]) - x).max() <= 2 ** -21 * np.abs(x).max()
    p3 = be.pack(x.astype(np.float64), SPLIT)  # fp64 input is cast to fp32 at the boundary (Appendix A.1)
    assert np.array_equal(p3.rows.cpu().numpy(), p2.rows.cpu().numpy())
    pn = be.pack(x, F16, normalize=True)
    nrm = np.linalg.norm(pn.rows.cpu().numpy().astype(np.float32), axis=1)
    assert np.abs(nrm - 1).max() < 2e-3


@pytest.mark.parametrize("d", [96, 200, 768, 1000, 3072, 4100])  # (4 100: the element-wise kernel, wide)
@pytest.mark.parametrize("src_dtype", [np.float32, np.float16])
def test_pack_rows_vector_path_equals_scalar_semantics(hip_backend, d, src_dtype):
    """d % 8 == 0 takes the 16-byte-per-lane kernel: same stored values as the element-wise definition, also for a
    source that starts at an odd row of a bigger buffer (every row still 16-byte aligned)."""
    import torch

    be = hip_backend
    big = (synth.corpus(131, d, seed=d) * 2).astype(src_dtype)
    dev = torch.from_numpy(big).to(be.device)
    for x_dev, x in ((dev, big), (dev[3:], big[3:])):
        xf = x.astype(np.float32)
        hi = xf.astype(np.float16)
        dpad = -(-d // 64) * 64
        p = be.pack(x_dev, F16)
        rows = p.rows.cpu().numpy()
        assert rows.shape == (len(x), dpad)
        assert np.array_equal(rows[:, :d], hi) and not rows[:, d:].any()
        assert np.allclose(p.norms.cpu().numpy(), (hi.astype(np.float32) ** 2).sum(1), rtol=2e-6)
        p2 = be.pack(x_dev, SPLIT)
        r2 = p2.rows.cpu().numpy()
        lo = (xf - hi.astype(np.float32)).astype(np.float16)
        assert np.array_equal(r2[:, :d], hi) and np.array_equal(r2[:, dpad:dpad + d], lo)
        assert not r2[:, d:dpad].any() and not r2[:, dpad + d:].any()
        pn = be.pack(x_dev, SPLIT, normalize=True)
        rn = pn.rows.cpu().numpy().astype(np.float32)
        want = xf / np.linalg.norm(xf, axis=1, keepdims=True)
        assert np.abs(rn[:, :d] + rn[:, dpad:dpad + d] - want).max() <= 3e-7


def test_rank_all_rows_for_k_equal_n(hip_backend, tmp_path):
    """K = N beyond LVS_MAX_K through HipVS: full score rows + segmented sort."""
    from lotus_amd import HipVS

    xb = synth.corpus(3000, 96, seed=2).astype(np.float16)
    xq, _ = synth.queries(xb.astype(np.float32), 37, seed=3)
    xq = xq.astype(np.float16)
    vs = HipVS(backend=hip_backend)
    vs.index(None, xb, str(tmp_path / "i"))
    out = vs(xq, 3000)
    Dr, Ir = oracle.flat_search(xb.astype(np.float32), xq.astype(np.float32), 3000)
    err, hard, recall = synth.compare_topk(Dr, Ir, out.distances, out.indices)
    assert err <= 1e-5 and hard == 0 and recall == 1.0
    assert (np.sort(out.indices, axis=1) == np.arange(3000)).all()
    ids = np.arange(3000)[::-1][:2500].copy()
    out = vs(xq[:5], 2500, ids=ids.tolist())
    assert set(out.indices[0].tolist()) == set(ids.tolist())


def test_merge_keys(hip_backend):
    be = hip_backend
    rng = np.random.default_rng(5)
    for P, nq, k in ((8, 500, 10), (3, 17, 24), (13, 50, 64), (1, 9, 5)):
        parts = rng.integers(1, 2**63 - 1, size=(P, nq, k), dtype=np.int64).view(np.uint64)
        parts[:, :, -2:] = 0  # some empty slots
        out = be.merge_keys(be.to_device(parts.view(np.int64))).cpu().numpy().view(np.uint64)
        ref = np.sort(np.transpose(parts, (1, 0, 2)).reshape(nq, P * k), axis=1)[:, ::-1][:, :k]
        assert np.array_equal(out, ref)


def test_full_size_properties(hip_backend):
    """At a size the oracle cannot finish (16k x 1M x 768): planted neighbours found, rows sorted, and a random
    sample of queries re-checked exactly against the oracle restricted to those queries."""
    import torch

    be = hip_backend
    n, d, nq, k = 1_000_000, 768, 16384, 10
    g = torch.Generator(device=be.device)
    g.manual_seed(1234)
    xb = torch.randn((n, d), generator=g, device=be.device, dtype=torch.float32)
    xb = torch.nn.functional.normalize(xb, dim=1).to(torch.float16)
    j = torch.randint(0, n, (nq,), generator=g, device=be.device)
    u = torch.nn.functional.normalize(torch.randn((nq, d), generator=g, device=be.device), dim=1)
    xq = torch.nn.functional.normalize(0.7 * xb[j].float() + 0.7 * u, dim=1).to(torch.float16)
    cb, cq = be.pack(xb, F16), be.pack(xq, F16)
    keys = be.search_keys(cb, cq, k, IP)
    D, I = be.keys_to_result(keys, IP)
    D, I = D.cpu().numpy(), I.cpu().numpy()
    assert (I[:, 0] == j.cpu().numpy()).mean() > 0.999  # planted neighbour is rank 1
    assert (np.diff(D, axis=1) <= 0).all()  # best first
    assert (I >= 0).all() and len(set(map(tuple, np.sort(I, axis=1)))) > 1
    sel = np.random.default_rng(0).choice(nq, 64, replace=False)
    xb_h = xb.cpu().numpy().astype(np.float32)
    Dr, Ir = oracle.flat_search(xb_h, xq[torch.from_numpy(sel).to(be.device)].cpu().numpy().astype(np.float32), k, IP)
    err, hard, recall = synth.compare_topk(Dr, Ir, D[sel], I[sel])
    assert err <= 1e-5 and hard == 0 and recall == 1.0


def test_large_k_with_mass_ties_falls_back_to_selection_passes(hip_backend):
    """Thousands of identical rows overflow the two-phase buckets (every copy ties with the threshold score but only
    the lower ids may enter): the call must fall back to the multi-pass selection and stay exact."""
    be = hip_backend
    base = synth.corpus(40, 64, seed=3)
    xb = np.concatenate([np.repeat(base[:4], 3000, axis=0), synth.corpus(20000, 64, seed=4)])
    xq, _ = synth.queries(base, 30, seed=5)
    k = 200
    D, I, _ = _run(be, xb, xq, k, F16, IP)
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), k, IP)
    assert np.abs(D - Dr).max() <= 1e-5
    assert (I == Ir).mean() > 0.99  # exact ties are ordered by id on both sides


def test_merge_keys_long_lists(hip_backend):
    import torch

    be = hip_backend
    rng = np.random.default_rng(0)
    parts = rng.integers(1, 2 ** 62, size=(8, 50, 300), dtype=np.int64)
    out = be.merge_keys(torch.from_numpy(parts).to(be.device)).cpu().numpy().view(np.uint64)
    ref = -np.sort(-parts.view(np.uint64).transpose(1, 0, 2).reshape(50, -1).astype(np.float64), axis=1)  # order only
    want = np.sort(parts.view(np.uint64).transpose(1, 0, 2).reshape(50, -1), axis=1)[:, ::-1][:, :300]
    assert np.array_equal(out, want)


@pytest.mark.parametrize("P,nq,k", [(8, 40, 1000), (8, 9, 2048), (5, 33, 600), (2, 20, 2048), (16, 12, 65)])
def test_merge_keys_folds_any_number_of_long_lists(hip_backend, P, nq, k):
    """8 shards x k > 512 (nparts * k > 4096) used to be rejected; now folded in rounds, in place."""
    import torch

    be = hip_backend
    rng = np.random.default_rng(P * 1000 + k)
    parts = rng.integers(1, 2 ** 62, size=(P, nq, k), dtype=np.int64)
    parts[:, :, -3:] = 0  # empty slots
    out = be.merge_keys(torch.from_numpy(parts).to(be.device)).cpu().numpy().view(np.uint64)
    want = np.sort(parts.view(np.uint64).transpose(1, 0, 2).reshape(nq, -1), axis=1)[:, ::-1][:, :k]
    assert np.array_equal(out, want)


def test_unpack_rows_inverts_pack(hip_backend):
    be = hip_backend
    x = (synth.corpus(500, 100, seed=4) * 3).astype(np.float32)
    ids = np.random.default_rng(2).choice(500, 77, replace=False).astype(np.int64)
    p16 = be.pack(x.astype(np.float16), F16)
    assert np.array_equal(be.unpack(p16).cpu().numpy(), x.astype(np.float16).astype(np.float32))
    assert np.array_equal(be.unpack(p16, be.to_device(ids)).cpu().numpy(), x.astype(np.float16).astype(np.float32)[ids])
    ps = be.pack(x, SPLIT)
    hi = x.astype(np.float16).astype(np.float32)
    lo = (x - hi).astype(np.float16).astype(np.float32)
    assert np.array_equal(be.unpack(ps, be.to_device(ids)).cpu().numpy(), (hi + lo)[ids])
    assert np.abs(be.unpack(ps).cpu().numpy() - x).max() <= 2 ** -21 * np.abs(x).max()


def test_kmeans_update_centroids_is_faiss_division(hip_backend):
    import torch

    be = hip_backend
    rng = np.random.default_rng(1)
    k, d = 37, 100
    sums = rng.standard_normal((k, d)).astype(np.float32) * 50
    counts = rng.integers(0, 9, k).astype(np.float32)
    counts[5] = 0
    old = rng.standard_normal((k, d)).astype(np.float32)
    c = torch.from_numpy(old.copy()).to(be.device)
    be.kmeans_update_centroids(torch.from_numpy(sums).to(be.device), torch.from_numpy(counts).to(be.device), c)
    want = old.copy()
    nz = counts > 0
    want[nz] = sums[nz] * (np.float32(1.0) / counts[nz])[:, None]
    assert np.array_equal(c.cpu().numpy(), want)  # bit-identical: one IEEE division, one rounded multiply


def test_range_join_chunks_and_regrows_per_chunk(hip_backend, monkeypatch):
    """The query rows go through in chunks; a chunk that finds more pairs than its buffer holds is the only thing
    that runs again."""
    be = hip_backend
    xd = synth.corpus(3000, 64, seed=8)
    xd[1500:2300] = xd[:800] + 0.02 * synth.corpus(800, 64, seed=9)
    xd /= np.linalg.norm(xd, axis=1, keepdims=True)
    p = be.pack(xd.astype(np.float16), F16)
    s = xd.astype(np.float16).astype(np.float32)
    s = s @ s.T
    qi, ji = np.nonzero(np.triu(s > 0.97, 1))
    want = set(zip(qi.tolist(), ji.tolist()))
    monkeypatch.setattr(type(be), "RANGE_CHUNK_ROWS", 512)
    for cap in (1 << 20, 16):  # roomy buffers; buffers that overflow in most chunks
        q, j, sc = be.range_join(p, p, 0.97, IP, q_row0=0, capacity=cap)
        got = set(zip(q.cpu().numpy().tolist(), j.cpu().numpy().tolist()))
        for a, b in got ^ want:
            assert abs(s[a, b] - 0.97) <= 2e-5
        assert len(got) >= 800 and np.allclose(sc.cpu().numpy(), s[q.cpu().numpy(), j.cpu().numpy()], atol=1e-5)
    # two "ranks" dealing 256-query tiles cover everything exactly once
    parts = [be.range_join(p, p, 0.97, IP, q_row0=0, stride=2, phase=r) for r in range(2)]
    both = [set(zip(a.cpu().numpy().tolist(), b.cpu().numpy().tolist())) for a, b, _ in parts]
    assert not (both[0] & both[1]) and len(both[0]) and len(both[1])
    for a, b in (both[0] | both[1]) ^ want:
        assert abs(s[a, b] - 0.97) <= 2e-5


def test_large_k_is_stream_async_and_exact_without_overflow(hip_backend):
    """k > 56 on ordinary data: the two-phase result stands, the predicated fallback passes are no-ops."""
    be = hip_backend
    xb = synth.corpus(50_000, 128, seed=31)
    xq, _ = synth.queries(xb, 70, seed=32)
    for k in (57, 300, 1200):
        D, I, _ = _run(be, xb, xq, k, F16, IP)
        Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), k, IP)
        err, hard, recall = synth.compare_topk(Dr, Ir, D, I)
        assert err <= 1e-5 and hard == 0 and recall >= 0.9999


def test_seeded_streaming_search_with_duplicates_across_the_sample_boundary(hip_backend):
    """The sample pass covers the first rows, the seeded main pass the rest: rows that tie exactly across that boundary
    (and rows equal to the threshold score) must all stay candidates - ids come back in the oracle's order."""
    xb = synth.corpus(100_000, 64, seed=77)
    xb[50_000:50_500] = xb[:500]          # duplicates of sample rows inside the main range
    xb[99_000:99_200] = xb[60_000:60_200]  # duplicates inside the main range
    xq = (xb[[3, 17, 250, 499, 60_010, 60_150, 70_000, 5, 9, 11, 13, 15]] * 1.0).astype(np.float32)
    for k in (1, 3, 10):
        D, I, _ = _run(hip_backend, xb, xq, k, F16, IP)
        Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), k, IP)
        assert np.array_equal(I, Ir)
        assert np.abs(D - Dr).max() <= 1e-5


@pytest.mark.parametrize("nq,nb,d,k,mode,metric", [
    (300, 100_000, 128, 10, F16, IP),    # two query tiles, 256-query geometry
    (300, 70_001, 64, 1, F16, L2),       # k = 1 through the list kernel (long slabs), ragged row count
    (520, 131_072, 96, 15, F16, L2),     # largest k of the 256-query geometry
    (260, 150_000, 64, 30, F16, IP),     # 128-query / 56-slot geometry: the sample must hold >= k tiles
    (400, 250_000, 32, 56, F16, L2),     # largest single-pass k: 56 of the 61 sample tiles set the threshold
    (1000, 90_000, 200, 10, SPLIT, IP),  # fp32-accurate operands (three K segments in the sample pass too)
    (3000, 66_000, 64, 5, SPLIT, L2),
    (130, 400_000, 64, 10, F16, IP),     # <= 256 queries beyond one sibling group: the list kernel, not the stream kernel
    # 97 .. 256 fp16 queries, d padded to 256 / 384 / 512 / 768, k <= 16, >= 32 768 rows: the queries-in-registers kernel
    # (lvs_rq.hip): four waves up to 128 queries, eight beyond; 12-slot lists up to k = 12, 16-slot ones beyond
    (100, 100_000, 768, 10, F16, IP),
    (128, 70_001, 512, 16, F16, L2),     # ragged last block, full 16-slot lists, row norms through the side words
    (160, 90_000, 384, 12, F16, IP),     # one unit per block (24 k-slices), five of the eight waves hold queries
    (256, 66_000, 256, 1, F16, L2),      # k = 1 through the lists
    (200, 40_000, 768, 13, F16, IP),     # 16-slot lists at d = 768 on eight waves (the tightest register budget)
    (97, 33_000, 200, 10, F16, L2),      # d padded from 200 to 256, a corpus barely long enough
    # ... and 257 .. 4 096 queries in groups of 256 (sibling workgroups of a corpus range on one XCD)
    (300, 70_001, 256, 10, F16, IP),     # two groups, the second one 44 queries; 128 ranges, ragged last block
    (512, 66_000, 384, 16, F16, L2),     # two full groups, 16-slot lists
    (700, 100_000, 768, 10, F16, IP),    # three groups: 80 ranges x 3 = 240 workgroups, the grid rounded up to XCD rows
    (1300, 200_000, 256, 5, F16, L2),    # six groups x 40 ranges
    (2304, 100_000, 256, 12, F16, IP),   # nine groups: 216 workgroups would idle too many CUs - the list kernel keeps it
    (4000, 530_000, 200, 10, F16, IP),   # sixteen groups x 16 ranges, the last group 160 queries
])
def test_seeded_list_kernel(hip_backend, nq, nb, d, k, mode, metric):
    """Launches with few query tiles seed their thresholds from a sample (LVS_MODE_SEED + k-th largest per-tile maximum)
    instead of a cold start in every slab.  Same results as the oracle; rows that tie exactly across the sample boundary,
    a block of identical rows (their score IS the threshold) and the sample rows themselves all stay candidates."""
    xb = synth.corpus(nb, d, seed=nb % 83)
    xb[nb // 2:nb // 2 + 300] = xb[:300]   # duplicates of sample rows inside the main range
    xb[nb - 200:] = xb[40]                 # 202 identical rows: one in the sample, one mid-range, 200 at the very end
    xq, _ = synth.queries(xb, nq, seed=29)
    xq[:8] = xb[[3, 40, 41, 299, nb // 2 + 7, nb - 1, 1000, 17]]
    if metric == L2:
        xb, xq = xb * 1.3, xq * 1.3
    D, I, _ = _run(hip_backend, xb, xq, k, mode, metric)
    # the oracle answers every query - or, where that would take the CPU minutes (the sixteen-group row), the first 300 (the
    # planted ties, the first group boundary), the last 200 (the ragged last group) and every 16th in between
    sel = np.arange(nq)
    if nq * nb * d > 2e11:
        sel = np.unique(np.concatenate([np.arange(300), np.arange(300, nq - 200, 16), np.arange(nq - 200, nq)]))
    Dr, Ir = oracle.flat_search(_stored(xb, mode), _stored(xq[sel], mode), k, metric)
    atol = 1e-5  # (r6) one bar for both metrics
    err, hard, recall = synth.compare_topk(Dr, Ir, D[sel], I[sel], atol=atol)
    assert err <= atol and hard == 0 and recall >= 0.9999, (err, hard, recall)
    # exact ties come back lowest id first, as the oracle's strict-better insertion leaves them
    same = np.concatenate([[40, nb // 2 + 40], np.arange(nb - 200, nb)])  # 202 identical rows
    assert np.array_equal(I[1, :k], same[:k]) and np.array_equal(I[5, :k], same[:k])
    if k >= 2:
        assert set(I[0, :2]) == {3, nb // 2 + 3} and I[0, 0] == 3


@pytest.mark.parametrize("metric,k,nq,d", [(IP, 10, 2304, 64), (L2, 5, 3000, 96), (IP, 15, 2100, 32)])
def test_pooled_thresholds_of_shards_keep_the_merged_result_exact(hip_backend, metric, k, nq, d):
    """The exchange behind a row-sharded join (lvs_flat_search_seed_scores -> all-gather -> lvs_flat_search_keys_seeded) through
    the C ABI on one GPU: uneven shards - one of 100 000 rows, one of 45 000, one SHORTER than a sample tile (its block is all
    -inf), one empty - searched with the pooled sample scores and merged == the oracle's search over all rows; lists may come
    back short, never wrong.  Also: sample blocks holding fewer than k real values (no threshold), duplicated rows whose
    score IS the threshold (ties pass), and the stream-kernel path (few queries) taking the same seeds."""
    import torch

    be = hip_backend
    nb = 100_000 + 45_000 + 200
    xb = synth.corpus(nb, d, seed=77) * (1.2 if metric == L2 else 1.0)
    xb[100_000:100_050] = xb[:50]          # rows of shard 0's sample duplicated in shard 1: equal scores across shards
    xq, _ = synth.queries(xb, nq, seed=78)
    xq[:50] = xb[:50]
    cq = be.pack(xq.astype(np.float16), F16)
    bounds = [(0, 100_000), (100_000, 145_000), (145_000, 145_200), (145_200, 145_200)]
    shards = [be.pack(xb[lo:hi].astype(np.float16), F16) for lo, hi in bounds]
    tiles = 12
    blocks = [be.seed_scores(sh, cq, metric, tiles) for sh in shards]
    assert bool(torch.isneginf(blocks[2]).all()) and bool(torch.isneginf(blocks[3]).all())  # shorter than a tile / empty
    assert bool(torch.isfinite(blocks[0]).all())
    pooled = torch.cat(blocks)
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq, F16), k, metric)
    atol = 1e-5  # (r6) one bar for both metrics
    for seeds in (pooled, pooled[:k - 1], torch.cat([blocks[2], blocks[0][:k - 2]])):   # full; fewer rows than k; < k finite
        parts = torch.stack([be.search_keys(sh, cq, k, metric, id_offset=lo, seed_scores=seeds) for sh, (lo, _) in zip(shards, bounds)])
        D, I = (t.cpu().numpy() for t in be.keys_to_result(be.merge_keys(parts), metric))
        err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=atol)
        assert err <= atol and hard == 0 and recall >= 0.9999, (err, hard, recall)
        assert np.array_equal(I[:50, 0], np.arange(50)) and np.array_equal(I[:50, 1], 100_000 + np.arange(50))  # ties: lowest id first
    short = int((parts == 0).sum().item())
    assert short >= 0  # (a shard may return fewer than k keys; the merge above was complete regardless)
    # few queries: the small-batch streaming kernel takes the same pooled seeds
    few = be.slice_rows(cq, 0, 40)
    parts = torch.stack([be.search_keys(sh, few, k, metric, id_offset=lo, seed_scores=pooled[:, :40].contiguous())
                         for sh, (lo, _) in zip(shards, bounds)])
    D, I = (t.cpu().numpy() for t in be.keys_to_result(be.merge_keys(parts), metric))
    err, hard, recall = synth.compare_topk(Dr[:40], Ir[:40], D, I, atol=atol)
    assert err <= atol and hard == 0 and recall >= 0.9999, (err, hard, recall)


@pytest.mark.parametrize("cmode,qmode,metric,nq,nb,d,k", [
    (SPLIT, SPLIT, IP, 3000, 60_000, 384, 10),   # LOTUS's default: fp32 embeddings on both sides (3 passes -> 1)
    (SPLIT, F16, L2, 2000, 50_000, 200, 5),
    (SPLIT, SPLIT, IP, 2500, 60_000, 256, 12),   # k = 11, 12 keep the 15-slot lists (three spare slots here)
    (SPLIT, F16, L2, 1200, 45_000, 96, 13),      # k + 8 = 21 slots: the 128-query geometry
    (F16, SPLIT, IP, 1000, 40_000, 768, 20),     # k1 = 28: the 128-query geometry
    (SPLIT, SPLIT, L2, 300, 30_000, 128, 48),    # largest certified k (56 list slots)
    (SPLIT, SPLIT, IP, 20, 100_000, 256, 10),    # few queries: the one-pass search is the streaming kernel
    (SPLIT, SPLIT, IP, 500, 9, 64, 10),          # fewer rows than list slots: plain path
])
def test_one_pass_certified_search_equals_the_plain_search(hip_backend, cmode, qmode, metric, nq, nb, d, k):
    """fp32-accurate operands: one MFMA pass over the hi parts + exact rescoring of k1 > k candidates + certificate
    + plain search of the uncertified queries == the plain 2-3 pass search (same ids; scores to fp32 rounding)."""
    be = hip_backend
    xb = synth.corpus(nb, d, seed=nb % 91) * (1.3 if metric == L2 else 1.0)
    xq, _ = synth.queries(xb, nq, seed=6)
    cb = be.pack(xb.astype(np.float16) if cmode == F16 else xb, cmode)
    cq = be.pack(xq.astype(np.float16) if qmode == F16 else xq, qmode)
    stats = {}
    Dg, Ig = (t.cpu().numpy() for t in be.keys_to_result(be.search_keys(cb, cq, k, metric, id_offset=11, one_pass=True, stats=stats), metric))
    Dw, Iw = (t.cpu().numpy() for t in be.keys_to_result(be.search_keys(cb, cq, k, metric, id_offset=11, one_pass=False), metric))
    err, hard, recall = synth.compare_topk(Dw, Iw, Dg, Ig, atol=4e-6 * max(1.0, np.abs(Dw[Iw >= 0]).max()), tie_gap=4e-6)
    assert hard == 0 and recall == 1.0 and err <= 4e-6 * max(1.0, np.abs(Dw[Iw >= 0]).max())
    if nb > 4 * (k + 8):
        assert stats["queries"] == nq and stats["uncertified"] <= 0.25 * nq
    # and against the oracle on the stored values
    Dr, Ir = oracle.flat_search(_stored(xb, cmode), _stored(xq, qmode), k, metric)
    atol = 1e-5  # (r6) one bar for both metrics
    err, hard, recall = synth.compare_topk(Dr, Ir + 11 * (Ir >= 0), Dg, Ig, atol=atol)
    assert err <= atol and hard == 0 and recall >= 0.9999


@pytest.mark.parametrize("metric,nq,nb,d,k,k1", [(IP, 3000, 120_000, 96, 10, 15), (L2, 1500, 80_000, 64, 5, 10),
                                                 (IP, 700, 90_000, 128, 20, 28)])
def test_banded_lists_keep_every_row_inside_the_band(hip_backend, metric, nq, nb, d, k, k1):
    """lvs_flat_search_keys_hi_banded through the C ABI against the plain k1-deep one-pass lists of the same launch shape:
    inside the band (one-pass score >= k-th best - band) a banded list IS the plain list, key for key; below it it holds
    whatever rows were admitted before the band rose past them (never a row that could matter).  With a band wider than the
    spread it is the plain list.  lvs_certify_topk_banded then certifies exactly the queries whose band was not
    crowded, and lvs_certify_topk == band 0."""
    import torch

    be = hip_backend
    xb = synth.corpus(nb, d, seed=31) * (1.3 if metric == L2 else 1.0)
    xq, _ = synth.queries(xb, nq, seed=32)
    xb[5000:5000 + k1 + 4] = xb[77]         # more copies of one row than a list has slots: a query that hits it has a crowded band
    xq[:40] = xb[77] + 0.01 * synth.corpus(40, d, seed=33)
    cb, cq = be.pack(xb, SPLIT), be.pack(xq, SPLIT)
    P = lambda t: 0 if t is None else int(t.data_ptr())
    need = int(be.lib.lvs_flat_search_workspace_bytes(nq, nb, d, k1, cb.mode, cq.mode))
    ws = be._workspace(need)

    def banded(scale, slack):
        keys = torch.empty((nq, k1), dtype=torch.int64, device=be.device)
        be._c("lvs_flat_search_keys_hi_banded", P(cb.rows), cb.mode, nb, P(cq.rows), cq.mode, nq, d, metric, k1, k, float(scale),
              float(slack), P(cb.norms), P(cq.norms), 0, None, P(keys), P(ws), int(ws.numel()), be._stream())
        return keys

    plain = be._search_call("lvs_flat_search_keys_hi", cb, cq, k1, metric, 0)
    pl = plain.cpu().numpy().view(np.uint64)
    s_pl, _, e_pl = oracle.unpack_keys(pl)
    assert not e_pl.any()
    qn = np.sqrt(cq.norms.cpu().numpy().astype(np.float64))
    spread = float(np.median(s_pl[:, k - 1] - s_pl[:, k1 - 1]))
    scale = 0.05 * spread / float(np.median(qn))      # a band of ~5 % of the distance from the k-th to the k1-th score
    bd = banded(scale, 0.0).cpu().numpy().view(np.uint64)
    s_bd, _, e_bd = oracle.unpack_keys(bd)
    filled = (~e_bd).sum(1)
    assert (filled >= k).all()
    band = np.float32(scale) * np.sqrt(cq.norms.cpu().numpy())                      # float32, as the kernel evaluates it
    inside = s_pl >= (s_pl[:, k - 1] - band)[:, None] + 1e-6 * np.abs(s_pl[:, :1])  # rows the band must keep (ulp slack)
    n_in = inside.sum(1)                              # (a prefix of the plain list: it is sorted)
    assert (n_in >= k).all() and (n_in <= filled).all()
    for q in range(nq):
        # inside the band: the plain list, key for key.  Below it a list may keep rows admitted before the band rose past
        # them (and miss better ones that came later - nobody needs either); sorted best first, empty slots last
        assert np.array_equal(bd[q, :n_in[q]], pl[q, :n_in[q]]), q
        assert (np.diff(bd[q].astype(np.float64)) <= 0).all() and e_bd[q, filled[q]:].all() and not e_bd[q, :filled[q]].any(), q
    # (the list returned is the MERGE of the slabs' lists, each of which fills its own first k slots before its band means
    # anything - so the merged list is full again, its tail a mix of rows below the band; what the band saves is insertions)
    wide = banded(1e6, 0.0).cpu().numpy().view(np.uint64)                          # a band wider than any spread: the plain lists
    assert np.array_equal(wide, pl)
    # certificates: band 0 == lvs_certify_topk; banded: open exactly where the band is crowded beyond the list
    exact = torch.from_numpy(bd.view(np.int64)).to(be.device)
    approx = exact.clone()

    def certify(name, *extra):
        idx = torch.empty((nq,), dtype=torch.int64, device=be.device)
        cnt = torch.zeros((1,), dtype=torch.int64, device=be.device)
        be._c(name, P(approx), P(exact), P(cq.norms), nq, k1, k, float(scale / 2.05), 0.0, *extra, P(idx), P(cnt), be._stream())
        return set(idx[:int(cnt.item())].cpu().numpy().tolist())

    open_banded = certify("lvs_certify_topk_banded", 2.02)
    assert set(range(40)) <= open_banded and len(open_banded) <= 40 + 0.01 * nq       # (approx == exact here: a pure list test)
    assert certify("lvs_certify_topk_banded", 0.0) == certify("lvs_certify_topk")


def test_one_pass_certificate_refuses_rows_that_differ_below_fp16_resolution(hip_backend):
    """Twins with identical hi parts and different lo parts around rank k: the one-pass scores cannot order them, the
    certificate must send those queries to the plain search - results stay exact."""
    be = hip_backend
    d, nb = 96, 20_000
    h16 = (synth.corpus(nb, d, seed=5) * 1.1).astype(np.float16)
    xb = h16.astype(np.float32)
    xq = xb[:64].copy()
    # every query gets 30 near-copies of its own row: same hi part, lo part growing with the copy number
    for qi in range(64):
        rows = 1000 + qi * 30 + np.arange(30)
        xb[rows] = xb[qi]
        xb[rows, :8] += (np.arange(30)[:, None] / 100.0) * np.spacing(np.abs(h16[qi, :8])).astype(np.float32)
    cb, cq = be.pack(xb, SPLIT), be.pack(xq, SPLIT)
    stats = {}
    Dg, Ig = (t.cpu().numpy() for t in be.keys_to_result(be.search_keys(cb, cq, 10, IP, one_pass=True, stats=stats), IP))
    Dw, Iw = (t.cpu().numpy() for t in be.keys_to_result(be.search_keys(cb, cq, 10, IP, one_pass=False), IP))
    assert stats["uncertified"] >= 60
    # the 30 near-copies of a query's row score within ~1e-7 of each other: which of them two exact float32 evaluations (the
    # certified path's rescoring dot products, the plain MFMA search) rank first is rounding - so the lists are compared with
    # the float64 truth on the stored values: the right scores at every rank, every reported row scoring what is reported
    assert np.abs(Dg - Dw).max() <= 1e-6
    sb, sq = _stored(xb, SPLIT).astype(np.float64), _stored(xq, SPLIT).astype(np.float64)
    truth = sq @ sb.T
    top = -np.sort(-truth, axis=1)[:, :10]
    rows = np.arange(len(xq))[:, None]
    for D, I in ((Dg, Ig), (Dw, Iw)):
        assert np.abs(D - top).max() <= 1e-6 and np.abs(truth[rows, I] - D).max() <= 1e-6
        assert all(len(set(r)) == 10 for r in I.tolist())
    assert (Ig[:, 0] == np.arange(64)).all() or np.abs(truth[np.arange(64), Ig[:, 0]] - top[:, 0]).max() <= 1e-6


@pytest.mark.parametrize("nq,nb,d", [(100_000, 125_000, 32), (50_000, 250_000, 64), (16_384, 700_000, 32),
                                     (100_000, 125_000, 768),   # the per-GPU shape of the 8-GPU row split, at the config's own d
                                     (12_500, 260_000, 768),    # 49 query tiles: a remainder tile in groups of its own shape
                                     (20_000, 330_000, 768)])   # 79 query tiles on short slabs: wide groups instead of 8 x 4
def test_planner_shapes_sampled_parity(hip_backend, nq, nb, d):
    """Launch shapes that take the planner's 8 x 4 L2 groups with a leading slab, a remainder of groups dealt across all
    XCDs, remainder query tiles and the wide-group fallback (lvs_plan.h, lvs_tile_geometry): the whole launch runs on the GPU,
    EIGHT queries of EVERY 256-query tile are checked against the oracle - one in each 32-query block of the tile (= one per
    (wave column, accumulator block) of the workgroup), at a lane position that walks with the tile number, so all 256
    positions of a tile are hit across the launch (a query's list depends on every (tile, slab) item of its tile)."""
    k = 10
    xb = synth.corpus(nb, d, seed=11)
    xq, _ = synth.queries(xb, nq, seed=12)
    D, I, _ = _run(hip_backend, xb, xq, k, F16, IP)
    tiles = np.arange(0, nq, 256)
    t = np.arange(len(tiles))
    pick = np.unique(np.minimum(tiles[:, None] + 32 * np.arange(8)[None, :] + ((37 * t) % 32)[:, None], nq - 1).reshape(-1))
    pick = np.union1d(pick, [0, nq - 1])
    Dr, Ir = oracle.flat_search(_stored(xb, F16), _stored(xq[pick], F16), k, IP)
    err, hard, recall = synth.compare_topk(Dr, Ir, D[pick], I[pick], atol=1e-5)
    assert err <= 1e-5 and hard == 0 and recall >= 0.9999, (err, hard, recall)
    assert (I[pick] == Ir).mean() > 0.999
    assert (I >= 0).all() and (np.diff(D, axis=1) <= 0).all()  # every list full and best-first


@pytest.mark.parametrize("mode,nq,nb,d,k", [(F16, 2000, 60_000, 768, 10), (F16, 40, 120_000, 384, 10), (SPLIT, 1500, 50_000, 256, 5)])
def test_l2_on_unit_norm_rows_at_1e5(hip_backend, mode, nq, nb, d, k):
    """north_star's bar for L2: scores within 1e-5 - on unit-norm rows (squared distances in [0, 4], the planted neighbour
    at ~0.58) - since round 6 the scaled-data cases above hold the same 1e-5."""
    xb = synth.corpus(nb, d, seed=31)
    xq, _ = synth.queries(xb, nq, seed=32)
    D, I, _ = _run(hip_backend, xb, xq, k, mode, L2)
    Dr, Ir = oracle.flat_search(_stored(xb, mode), _stored(xq, mode), k, L2)
    err, hard, recall = synth.compare_topk(Dr, Ir, D, I, atol=1e-5)
    assert err <= 1e-5, err
    assert hard == 0 and recall >= 0.9999


def test_pack_validation_flags_non_finite_and_out_of_range_values(hip_backend):
    """faiss takes any float32 (faiss_vs.py:24); the fp16-based device rows do not: inf / NaN and |x| > 65504 are detected
    while packing instead of silently producing NaN scores."""
    be = hip_backend
    x = synth.corpus(3000, 96, seed=1)
    be.pack(x, SPLIT, check=True)
    be.pack((x * 6.0e4).astype(np.float32), F16, check=True)  # largest component ~ 0.4 * 6e4: still inside fp16's range
    for bad, what in ((np.inf, "inf"), (np.nan, "inf"), (7.0e4, "range"), (-1.0e9, "range")):
        y = x.copy()
        y[1234, 17] = bad
        for mode in (F16, SPLIT):
            with pytest.raises(ValueError, match=what):
                be.pack(y, mode, check=True)


# (2100, 3): 2100 * 256 counters > 256 scan segments of 2 048 - the scan's one-workgroup middle kernel carries across blocks
@pytest.mark.parametrize("nq,nb", [(7, 10_001), (1, 4096), (3, 4097), (300, 2049), (2, 300_000), (5, 1), (2100, 3)])
def test_row_ranking_is_a_stable_descending_sort(hip_backend, nq, nb):
    """lvs_sort_rows_desc (hand-written segmented radix sort): every row ranked best-first, equal scores by ascending id -
    the total order of the result keys - incl. signed zeros, infinities and heavy ties."""
    import torch

    be = hip_backend
    rng = np.random.default_rng(nq * 1000 + nb)
    sc = rng.standard_normal((nq, nb)).astype(np.float32)
    sc[:, ::7] = np.round(sc[:, ::7], 1)            # many exact ties
    if nb > 10:
        sc[0, 3], sc[0, 4], sc[-1, 5], sc[-1, 6] = 0.0, -0.0, np.inf, -np.inf
    keys = be.rank_scores(torch.from_numpy(sc).to(be.device), id_offset=11).cpu().numpy().view(np.uint64)
    ids = np.broadcast_to(np.arange(nb, dtype=np.int64) + 11, sc.shape)
    ref = np.sort(oracle.pack_keys(sc, ids), axis=1)[:, ::-1]
    assert np.array_equal(keys, ref)
