"""Host side of the row selector of the IVF list scans and of ``HipVS(ids_probe=True)``, on the CPU: every case of
ivf_select_cases.py through ``SelectOracleBackend`` (the case is what it claims to be, its filtered reference stays under
the near-tie cap, and the assertions the GPU test makes pass on a backend that is right by construction), the routing rules
of ``HipVS.__call__`` one by one, ``ops.sem_search`` / ``ops.sem_sim_join`` on a filtered frame, ``HipBackend.row_bitmap``'s
layout, and the ``*_keys_sel`` entry points' argument checks.  The device path is covered by tests/test_gpu_ivf_select.py."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import ivf_edge_cases as E
import ivf_select_cases as S
import synth
from ivf_refine_oracle_backend import RefineOracleBackend
from ivf_select_oracle_backend import SelectOracleBackend, bitmap_mask, bitmap_words, filter_lists
from lotus_amd import HipVS, METRIC_INNER_PRODUCT, METRIC_L2, _capi
from lotus_amd.backend import HipBackend

SEL_CALL = {"IVF16,Flat": "ivf_search_sel", "IVF16,SQ8": "ivf_sq8_search_sel", "IVF16,PQ8": "ivf_pq_search_sel"}


# ---- the cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", S.PARAMS, ids=[f"{n}-{m}" for n, m in S.PARAMS])
def test_case_is_what_it_claims(name, mode):
    be = SelectOracleBackend()
    sc = S.build(name)
    res = S.run_sel(be, sc, mode)
    S.preconditions(be, sc, mode, res)
    S.check_result(sc, mode, res)


@pytest.mark.parametrize("mode", S.MODES)
def test_all_selected_and_complement(mode):
    be = SelectOracleBackend()
    S.all_selected_is_the_plain_search(be, mode)
    S.complement_merges_to_the_plain_search(be, mode)


@pytest.mark.parametrize("mode", (S.SQ8, S.PQ))
def test_refine_over_a_selection(mode):
    be = SelectOracleBackend()
    res = S.refine_over_a_selection(be, mode)
    S.preconditions(be, S.build("refine-50"), mode, res)


def test_every_family_meets_every_mode():
    fams = {"random", "last", "skipped", "word", "fewer", "shared"}
    for m in S.MODES:
        assert fams <= {n.split("-")[0] for n, mm in S.PARAMS if mm == m}
    # lengths on both sides of every scan's block and workgroup size, empty lists and a long one
    for b in (16, 32, 64, 128, 512):
        assert {b - 1, b, b + 1} <= set(S.LENGTHS)
    assert S.LENGTHS.count(0) >= 2 and max(S.LENGTHS) >= 1500


def test_filter_lists_and_bitmap_words():
    off, rows = E.deal([5, 0, 7, 3], 1)
    mask = np.zeros(15, bool)
    mask[[0, 3, 4, 14]] = True
    off_f, rows_f = filter_lists(off, rows, mask)
    assert off_f[-1] == 4 and sorted(rows_f.tolist()) == [0, 3, 4, 14]
    for l in range(4):
        want = [r for r in rows[off[l]:off[l + 1]].tolist() if mask[r]]
        assert rows_f[off_f[l]:off_f[l + 1]].tolist() == want
    w = bitmap_words([0, 31, 32, 70], 71)
    assert w.tolist() == [0x80000001, 1, 1 << 6] and np.nonzero(bitmap_mask(w, 71))[0].tolist() == [0, 31, 32, 70]


# ---- row_bitmap ------------------------------------------------------------------------------------------------------------
class _HostBitmap(HipBackend):
    """``HipBackend.row_bitmap`` itself with the upload left out (no GPU here)."""

    def __init__(self):
        pass

    def to_device(self, arr):
        import torch

        return torch.from_numpy(np.ascontiguousarray(arr))


def test_row_bitmap_layout_and_distinct_count():
    import torch

    be = _HostBitmap()
    rng = np.random.default_rng(3)
    for n, ids in ((333, rng.choice(333, 100, replace=False)), (64, [0, 31, 32, 63]), (65, [64]), (1, [0]), (40, []),
                   (1000, [5, 5, 999, 7, 5]), (0, [])):
        words, distinct = be.row_bitmap(np.asarray(ids, np.int64), n)
        assert words.dtype == torch.uint32 and int(words.numel()) == -(-n // 32)
        assert distinct == len(set(np.asarray(ids).tolist()))
        assert np.array_equal(words.numpy(), bitmap_words(ids, n))  # the kernels' rule, bit by bit; nothing set at or past n
    twin, count = SelectOracleBackend().row_bitmap(np.array([5, 5, 999, 7]), 1000)
    assert count == 3 and np.array_equal(twin.numpy(), be.row_bitmap(np.array([5, 999, 7]), 1000)[0].numpy())


# ---- HipVS routing ---------------------------------------------------------------------------------------------------------
N, D_, NLIST, NPROBE = 2000, 32, 16, 2  # the scan scores about N * NPROBE / NLIST = 250 rows per query


@pytest.fixture(scope="module")
def rows():
    return synth.corpus(N, D_, seed=11), synth.queries(synth.corpus(N, D_, seed=11), 12, seed=12)[0]


def store(rows, fs="IVF16,Flat", **kw):
    vs = HipVS(backend=SelectOracleBackend(), factory_string=fs, nprobe=NPROBE, **kw)
    vs.index(None, rows[0], "sel", persist=False)
    vs.backend.calls.clear()
    return vs


def names(vs):
    return [c[0] for c in vs.backend.calls]


def subset(m, seed=0):
    return np.sort(np.random.default_rng(seed).choice(N, m, replace=False))


def took_lists(vs, fs="IVF16,Flat"):
    took = SEL_CALL[fs] in names(vs)
    assert took != ("gather" in names(vs))  # one path or the other
    vs.backend.calls.clear()
    return took


def test_default_is_off(rows):
    vs = store(rows)
    assert vs.ids_probe is False
    vs(rows[1], 10, ids=subset(1000))
    assert not took_lists(vs)


@pytest.mark.parametrize("fs", list(SEL_CALL))
def test_on_takes_the_mode_s_scan_and_returns_the_given_ids(rows, fs):
    vs = store(rows, fs, ids_probe=True)
    ids = subset(1000)
    out = vs(rows[1], 10, ids=ids)
    sel_call = [c for c in vs.backend.calls if c[0] == SEL_CALL[fs]][0]
    assert sel_call[1:] == (12, 10, NPROBE, 1000)
    assert took_lists(vs, fs)
    I = np.asarray(out.indices)
    assert I.shape == (12, 10) and np.isin(I[I >= 0], ids).all() and (I >= 0).any()
    # the probed lists' selected rows under the filtered-lists rule, through the plain store's probes
    _, off, lrows = vs.ivf_lists()
    probe = vs.ivf_probe(rows[1])
    mask = np.zeros(N, bool)
    mask[ids] = True
    off_f, rows_f = filter_lists(off, lrows, mask)
    for q in range(12):
        allowed = np.concatenate([rows_f[off_f[l]:off_f[l + 1]] for l in probe[q]])
        got = I[q][I[q] >= 0]
        assert np.isin(got, allowed).all() and len(got) == min(10, len(allowed))


def test_duplicates_stay_exact(rows):
    vs = store(rows, ids_probe=True)
    ids = np.concatenate([subset(999), subset(999)[:1]])
    out = vs(rows[1], 10, ids=ids)
    assert "row_bitmap" in names(vs) and not took_lists(vs)  # the bitmap's count told
    assert (np.asarray(out.indices) >= 0).all()


def test_k_57_stays_exact(rows):
    vs = store(rows, ids_probe=True)
    big = subset(1500)
    vs(rows[1], 56, ids=big)
    assert took_lists(vs)
    vs(rows[1], 57, ids=big)  # beyond the one-pass list scan
    assert not took_lists(vs)


def test_k_must_be_below_the_number_of_ids(rows):
    """K < len(ids) on its own: nlist = 16 = nprobe would score every row, so take a store where the rule is met by few ids."""
    vs = HipVS(backend=SelectOracleBackend(), factory_string="IVF200,Flat", nprobe=1, ids_probe=True)
    vs.index(None, rows[0], "sel200", persist=False)  # 10 rows scored per query: 11 ids pass the rows-scored rule
    ids = subset(40, seed=7)
    for K, want in ((39, True), (40, False), (41, False)):
        vs.backend.calls.clear()
        vs(rows[1], K, ids=ids)
        assert took_lists(vs) == want, K


def test_rows_scored_rule_on_both_sides_of_equality(rows):
    vs = store(rows, ids_probe=True)
    assert N * NPROBE == 250 * NLIST
    for m, want in ((249, False), (250, False), (251, True)):  # len(ids) * nlist > n * nprobe, strictly
        vs(rows[1], 10, ids=subset(m, seed=m))
        assert took_lists(vs) == want, m
    vs(rows[1], 10, ids=subset(251), nprobe=3)  # the per-call nprobe moves the threshold to 375
    assert not took_lists(vs)
    vs(rows[1], 10, ids=subset(376), nprobe=3)
    assert took_lists(vs)


def test_full_range_ids_are_the_plain_search(rows):
    vs = store(rows, ids_probe=True)
    vs(rows[1], 10, ids=list(range(N)))
    assert "ivf_search" in names(vs) and "ivf_search_sel" not in names(vs) and "row_bitmap" not in names(vs)
    vs.backend.calls.clear()
    vs(rows[1], 10)
    assert "ivf_search" in names(vs) and "row_bitmap" not in names(vs)


def test_per_call_override_and_bad_types(rows):
    on, off = store(rows, ids_probe=True), store(rows)
    ids = subset(1000)
    on(rows[1], 10, ids=ids, ids_probe=False)
    assert not took_lists(on)
    off(rows[1], 10, ids=ids, ids_probe=True)
    assert took_lists(off)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="ids_probe"):
            HipVS(backend=SelectOracleBackend(), factory_string="IVF16,Flat", ids_probe=bad)
        with pytest.raises(ValueError, match="ids_probe"):
            off(rows[1], 10, ids=ids, ids_probe=bad)
    HipVS(backend=SelectOracleBackend(), ids_probe=True)  # a Flat store takes and ignores it


def test_backend_without_row_bitmap_is_refused():
    with pytest.raises(ValueError, match="row_bitmap"):
        HipVS(backend=RefineOracleBackend(), factory_string="IVF16,Flat", ids_probe=True)
    HipVS(backend=RefineOracleBackend(), factory_string="IVF16,Flat")  # without it the older double is fine


@pytest.mark.parametrize("fs,first", [("IVF16,SQ8,Refine(Flat)", "ivf_sq8_search_sel"), ("IVF16,PQ8,Refine(Flat)", "ivf_pq_search_sel")])
def test_refine_store_scans_at_kc_then_reranks(rows, fs, first):
    vs = store(rows, fs, ids_probe=True, k_factor=3)
    ids = subset(1000)
    out = vs(rows[1], 10, ids=ids)
    calls = [c for c in vs.backend.calls if c[0] in (first, "refine_keys")]
    assert [c[0] for c in calls] == [first, "refine_keys"] and calls[0][2] == 30 and calls[1][1:] == (12, 30, 10)
    I, Dd = np.asarray(out.indices), np.asarray(out.distances)
    assert np.isin(I[I >= 0], ids).all()
    x16 = rows[0].astype(np.float32)
    for q in range(12):  # exact scores of the very rows returned (hi|lo storage: fp32-accurate)
        at = I[q] >= 0
        np.testing.assert_allclose(Dd[q][at], x16[I[q][at]].astype(np.float64) @ rows[1][q].astype(np.float64), atol=1e-5)


def test_tie_order_is_by_row_on_the_probe_path_and_by_position_on_the_exact_path():
    """The documented difference: equal scores come out in ascending row order through the lists, in the order of their
    position in ``ids`` on the exact path; for ascending ids the two are one."""
    x = synth.corpus(400, 32, seed=21)
    x[300:340] = x[300]  # forty equal rows
    q = x[300:301]
    ids_desc = np.arange(399, 99, -1)
    for probe in (True, False):
        vs = HipVS(backend=SelectOracleBackend(), factory_string="IVF4,Flat", nprobe=2, ids_probe=probe, storage="fp32")
        vs.index(None, x, "ties", persist=False)
        I = np.asarray(vs(q, 5, ids=ids_desc).indices)[0]
        assert I.tolist() == ([300, 301, 302, 303, 304] if probe else [339, 338, 337, 336, 335])
        assert np.asarray(vs(q, 5, ids=np.sort(ids_desc)).indices)[0].tolist() == [300, 301, 302, 303, 304]


# ---- ops on a filtered frame -----------------------------------------------------------------------------------------------
def test_ops_on_a_filtered_frame_return_rows_of_the_frame_only(tmp_path):
    from lotus_amd import ops

    xb = synth.corpus(600, 32, seed=31)
    xq = synth.queries(xb, 8, seed=32)[0]
    vs = HipVS(backend=SelectOracleBackend(), factory_string="IVF24,Flat", nprobe=1, ids_probe=True)
    right = ops.sem_index(pd.DataFrame({"R": [f"r{i}" for i in range(600)], "year": np.arange(600) % 7}), "R",
                          str(tmp_path / "r"), vs=vs, embeddings=xb)
    kept = right[right.year > 1]  # 5 of 7 rows: 428 ids against 600 / 24 = 25 rows scored
    kept.attrs["index_dirs"] = right.attrs["index_dirs"]
    left = pd.DataFrame({"L": [f"l{i}" for i in range(8)]})

    class PassThroughRM:
        def convert_query_to_query_vector(self, q):
            return xq

    vs.backend.calls.clear()
    out = ops.sem_sim_join(left, kept, "L", "R", 30, rm=PassThroughRM(), vs=vs)
    assert "ivf_search_sel" in names(vs) and "gather" not in names(vs)
    assert set(out["R"]) <= set(kept["R"]) and 0 < len(out) < 8 * 30  # padded slots are dropped: single lists hold < 30 kept rows
    assert not out["R"].isna().any()
    vs.backend.calls.clear()
    hit = ops.sem_search(kept, "R", xq[:1], 30, vs=vs, return_scores=True)
    assert "ivf_search_sel" in names(vs)
    assert set(hit.index) <= set(kept.index) and 0 < len(hit) < 30 and not hit["R"].isna().any()


# ---- C entry points --------------------------------------------------------------------------------------------------------
def test_sel_entry_points_are_exported_and_validate_like_their_plain_twins():
    lib = _capi.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its argument checks first
    tail = dict(xq=p, xq_pack=0, nq=4, xqn=None, d=64, metric=0, nprobe=4, k=10, out=p, probe=None, ws=p, wsb=1 << 20, st=None)
    heads = {
        "lvs_ivf_search_keys": dict(xb=p, xb_pack=0, nb=1000, bn=None, off=p, rows=p, nlist=16, c=p, c_pack=0, cn=None),
        "lvs_ivf_sq8_search_keys": dict(codes=p, rn=None, vmin=p, vdiff=p, off=p, rows=p, nb=1000, nlist=16, c=p, c_pack=0,
                                        cn=None, c32=p),
        "lvs_ivf_pq_search_keys": dict(codes=p, beta=None, books=p, M=8, ksub=256, off=p, rows=p, nb=1000, nlist=16, c=p,
                                       c_pack=0, cn=None, c32=p),
    }
    assert {n + "_sel" for n in heads} <= set(_capi.declared_symbols()) & set(_capi.SIGNATURES)
    for name, head in heads.items():
        assert len(_capi.SIGNATURES[name + "_sel"][1]) == len(_capi.SIGNATURES[name][1]) + 1
        plain_fn, sel_fn = getattr(lib, name), getattr(lib, name + "_sel")

        def both(**kw):
            a = dict(head, **tail)
            a.update(kw)
            rc = plain_fn(*a.values())
            msg = lib.lvs_last_error()
            b = {}
            for key, v in a.items():  # sel_bits follows rows
                b[key] = v
                if key == "rows":
                    b["sel"] = p
            rc_sel = sel_fn(*b.values())
            return rc, msg, rc_sel, lib.lvs_last_error()

        for kw in (dict(metric=3), dict(nprobe=0), dict(nprobe=17), dict(k=0), dict(k=57), dict(xq_pack=5), dict(c_pack=5),
                   dict(nlist=0), dict(out=None), dict(rows=None), dict(metric=1), dict(d=0), dict(nb=-1)):
            rc, msg, rc_sel, msg_sel = both(**kw)
            assert rc == rc_sel == _capi.EINVAL and msg == msg_sel and msg, (name, kw, msg, msg_sel)
        rc, msg, rc_sel, msg_sel = both(wsb=16)
        assert rc == rc_sel == _capi.ENOMEM and msg == msg_sel
        assert both(nq=0)[::2] == (_capi.OK, _capi.OK)
