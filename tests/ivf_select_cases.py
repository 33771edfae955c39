"""Planted inputs for the row selector of the three IVF list scans (``sel=`` of ``ivf_search`` / ``ivf_sq8_search`` /
``ivf_pq_search``, the ``*_keys_sel`` entry points) and the one driver that runs them through a backend.  No test lives
here: test_ivf_select_host.py runs every case through ``SelectOracleBackend`` (is the case what it claims to be?),
test_gpu_ivf_select.py through ``HipBackend``.

A case is a case of ivf_edge_cases.py plus a selection: row numbers, or raw selector words where the bits past the last
row matter.  The reference is the existing rule on FILTERED lists: the unselected row numbers are dropped from every list,
the offsets recomputed (``filter_lists``), and ``ivf_reference`` / ``sq8_reference`` / ``pq_reference`` applied with the
probes of the search itself - the coarse step does not see the selector.

Bars: ivf_edge_cases.py's - 1e-5 on scores, a tie gap of 2e-5 (``synth.compare_topk``), every returned id rescored on the
CPU with (probed rows) x (selected rows) as the allowed set (``synth.check_ids_by_rescoring``), and at most 15 % of the
filtered reference's slots near a tie (``NEAR_TIE_CAP``, asserted per case by the host test)."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

import ivf_edge_cases as E
import synth
from ivf_edge_cases import F16, FLAT, IP, L2, PQ, SPLIT, SQ8
from ivf_oracle_backend import ivf_reference
from ivf_pq_oracle_backend import pq_reference
from ivf_refine_oracle_backend import refine_reference
from ivf_select_oracle_backend import bitmap_mask, bitmap_words, filter_lists
from ivf_sq8_oracle_backend import sq8_reference

MODES = (FLAT, SQ8, PQ)
NQ = 100


@dataclass
class SelCase:
    base: E.Case
    ids: Optional[np.ndarray] = None      # the selected rows ...
    words: Optional[np.ndarray] = None    # ... or the selector's words as given to the device
    pre: Optional[Callable] = None        # pre(sc, mode, res): asserts about the inputs and the reference alone
    post: Optional[Callable] = None       # post(sc, mode, res): the case's own assertions on the backend's result

    def selector(self):
        n = self.base.xb.shape[0]
        return self.words if self.words is not None else bitmap_words(self.ids, n)


# ---- the driver ------------------------------------------------------------------------------------------------------------
class _Selecting:
    """``be`` with ``sel=`` added to its three IVF searches, so that ``ivf_edge_cases.run_case`` drives a selected search;
    keeps what the last search was given and returned (the refine case re-ranks those keys)."""

    def __init__(self, be, words):
        self._be, self._words, self.seen = be, words, None

    def __getattr__(self, name):
        return getattr(self._be, name)

    def _run(self, fn, a, kw, q_at):
        out = fn(*a, sel=self._be.to_device(self._words), **kw)
        self.seen = dict(corpus=a[0], queries=a[q_at], keys=out[0] if kw.get("want_probe") else out)
        return out

    def ivf_search(self, *a, **kw):
        return self._run(self._be.ivf_search, a, kw, 2)

    def ivf_sq8_search(self, *a, **kw):
        return self._run(self._be.ivf_sq8_search, a, kw, 3)

    def ivf_pq_search(self, *a, **kw):
        return self._run(self._be.ivf_pq_search, a, kw, 3)


def run_sel(be, sc, mode):
    """``ivf_edge_cases.run_case`` with the case's selector in the search, and the reference over the filtered lists in
    D_ref / I_ref (the unfiltered one stays in D_all / I_all).  Adds ``mask`` (bool [n], the selected rows), ``off_f`` /
    ``rows_f`` (the filtered lists) and ``seen`` (corpus, queries and keys of the search)."""
    case = sc.base
    n = case.xb.shape[0]
    words = sc.selector()
    sb = _Selecting(be, words)
    res = E.run_case(sb, case, mode)
    mask = bitmap_mask(words, n)
    h = res["h"]
    off_f, rows_f = filter_lists(h["off"], h["rows"], mask)
    if mode == FLAT:
        D_ref, I_ref = ivf_reference(res["xref"], res["q"], case.k, case.metric, h["c"], off_f, rows_f, res["probe"])
    else:
        D_ref, I_ref = (sq8_reference if mode == SQ8 else pq_reference)(res["xref"], res["q"], case.k, case.metric, off_f,
                                                                        rows_f, res["probe"])
    res.update(D_all=res["D_ref"], I_all=res["I_ref"], D_ref=np.asarray(D_ref, np.float64) * res["scale"], I_ref=I_ref,
               mask=mask, off_f=off_f, rows_f=rows_f, seen=sb.seen)
    return res


def preconditions(be, sc, mode, res):
    """Asserts about the inputs and the filtered reference alone."""
    case = sc.base
    n = case.xb.shape[0]
    nlist = case.centroids.shape[0]
    assert 1 <= case.k <= 56 and 1 <= case.nprobe <= min(nlist, 2048)
    assert E.fits(be, case, mode)
    h = res["h"]
    assert h["off"][0] == 0 and h["off"][-1] == n and np.array_equal(np.sort(h["rows"].astype(np.int64)), np.arange(n))
    assert len(sc.selector()) == -(-n // 32)
    assert res["off_f"][-1] == res["mask"].sum() and res["mask"][res["rows_f"].astype(np.int64)].all()
    at = res["I_ref"] >= 0
    assert res["mask"][res["I_ref"][at]].all() and (res["I_ref"] < n).all()
    share = E.near_tie_share(res["D_ref"], res["I_ref"], case.tie_gap)
    assert share <= E.NEAR_TIE_CAP, f"near-tie share {share:.3f}: take another seed or a smaller k"
    if sc.pre is not None:
        sc.pre(sc, mode, res)


def check_result(sc, mode, res):
    """What every case holds a backend's result to (the kernel's name is asserted by the GPU test)."""
    case, bar = sc.base, res["bar"]
    err, hard, _ = synth.compare_topk(res["D_ref"], res["I_ref"], res["D"], res["I"], atol=bar, tie_gap=case.tie_gap)
    assert err <= bar and hard == 0, (err, hard)
    assert np.array_equal(res["I"] == -1, res["I_ref"] == -1)
    got = res["I"][res["I"] >= 0]
    assert (got < case.xb.shape[0]).all() and res["mask"][got].all()
    probe, nlist = res["probe"], case.centroids.shape[0]
    assert ((probe >= 0) & (probe < nlist)).all() and all(len(set(p.tolist())) == len(p) for p in probe)
    assert synth.compare_topk(res["Dp"], res["Ip"], res["Dp"], probe, tie_gap=case.tie_gap)[1] == 0  # the selector is no part of it
    score_fn, allowed = E.rescoring_args(res["xref"], res["q"], case.metric, res["off_f"], res["rows_f"], probe, res["scale"])
    synth.check_ids_by_rescoring(score_fn, res["D"], res["I"], allowed, bar)
    if sc.post is not None:
        sc.post(sc, mode, res)


def _bits(D):
    return np.ascontiguousarray(D, np.float32).view(np.uint32)


def all_selected_is_the_plain_search(be, mode):
    """Case 1: with every row selected the keys - scores bit for bit, and ids - are the unselected search's.  -> both results."""
    sc = build("random-50")
    n = sc.base.xb.shape[0]
    plain = E.run_case(be, sc.base, mode)
    full = run_sel(be, SelCase(sc.base, ids=np.arange(n)), mode)
    assert (plain["I"] >= 0).all()
    assert np.array_equal(plain["I"], full["I"]) and np.array_equal(_bits(plain["D"]), _bits(full["D"]))
    return plain, full


def complement_merges_to_the_plain_search(be, mode):
    """Case 7: the keys of a search over S and of one over its complement, merged, are the unselected search's keys."""
    sc = build("random-10")
    case = sc.base
    n = case.xb.shape[0]
    plain = E.run_case(be, case, mode)
    a = run_sel(be, sc, mode)
    b = run_sel(be, SelCase(case, ids=np.setdiff1d(np.arange(n), sc.ids)), mode)
    assert not (a["mask"] & b["mask"]).any() and (a["mask"] | b["mask"]).all()
    D = np.concatenate([a["D"], b["D"]], axis=1)
    I = np.concatenate([a["I"], b["I"]], axis=1)
    for q in range(I.shape[0]):
        at = np.nonzero(I[q] >= 0)[0]
        better = D[q, at] if case.metric == IP else -D[q, at]
        order = at[np.lexsort((I[q, at], -better))][:case.k]
        assert np.array_equal(I[q, order], plain["I"][q]) and np.array_equal(_bits(D[q, order]), _bits(plain["D"][q])), q
    return plain, a, b


def refine_over_a_selection(be, mode, k=10):
    """Case 9: the selected scan at kc candidates, then ``refine_keys``: ids inside S, exact scores, the order of
    ``refine_reference`` over the scan's own candidates.  -> the first stage's result."""
    sc = build("refine-50")
    case = sc.base
    res = run_sel(be, sc, mode)
    check_result(sc, mode, res)
    seen = res["seen"]
    keys = be.refine_keys(seen["corpus"], seen["queries"], seen["keys"], k, case.metric)
    D, I = be.keys_to_result(keys, case.metric, score_exp=be.score_exp_of(seen["corpus"], seen["queries"]))
    be.synchronize()
    D, I = D.cpu().numpy(), I.cpu().numpy()
    h = res["h"]
    D_ref, I_ref = refine_reference(h["x"], res["q"], res["I"], k, case.metric)
    D_ref = D_ref * res["scale"]
    assert E.near_tie_share(D_ref, I_ref, case.tie_gap) <= E.NEAR_TIE_CAP
    err, hard, _ = synth.compare_topk(D_ref, I_ref, D, I, atol=case.bar, tie_gap=case.tie_gap)
    assert err <= case.bar and hard == 0, (err, hard)
    assert (I >= 0).all() and res["mask"][I].all()
    score_fn, allowed = E.rescoring_args(h["x"], res["q"], case.metric, res["off_f"], res["rows_f"], res["probe"], res["scale"])
    synth.check_ids_by_rescoring(score_fn, D, I, allowed, case.bar)
    return res


# ---- the data --------------------------------------------------------------------------------------------------------------
# list lengths around each scan's block and workgroup sizes (Flat 32 / 128, SQ8 16 / 64, PQ 64 / 512), two empty lists, one long
LENGTHS = [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 0, 0, 1500]


def _base(lengths, metric, pack, seed, d=64, k=10, nprobe=None, xq=None, c=None, **kw):
    n, nlist = int(sum(lengths)), len(lengths)
    xb = synth.corpus(n, d, seed=seed)
    c = synth.corpus(nlist, d, seed=seed + 1) if c is None else c
    off, rows = E.deal(lengths, seed + 2)
    xq = synth.queries(xb, NQ, seed=seed + 3)[0] if xq is None else xq
    return E.Case(xb, xq, c, metric, pack, k, nlist if nprobe is None else nprobe, offsets=off, rows=rows, **kw)


def _list(case, l):
    return case.rows[case.offsets[l]:case.offsets[l + 1]].astype(np.int64)


def _shared_tiles(sc, mode, res):
    """Case 8: every list is probed by all the queries - more than 32 pairs (Flat: several 32-pair work items on one list)
    and more than 16 (SQ8) share the list's selector bits."""
    assert sc.base.nprobe == sc.base.centroids.shape[0] and res["probe"].shape[0] > 32


def random_selection(frac, metric, pack, seed, d=64, nprobe=None, k=10):
    """Case 2: a random share of the rows over the planted lengths."""
    base = _base(LENGTHS, metric, pack, seed, d=d, nprobe=nprobe, k=k)
    n = base.xb.shape[0]
    ids = np.sort(np.random.default_rng(seed + 4).choice(n, max(1, int(round(frac * n))), replace=False))

    def pre(sc, mode, res):
        assert np.array_equal(np.diff(res["h"]["off"]), LENGTHS)
        assert abs(res["mask"].mean() - frac) < 0.01
        if nprobe is None:
            _shared_tiles(sc, mode, res)

    return SelCase(base, ids=ids, pre=pre)


def last_row_only(metric, pack):
    """Case 3: of three lists only the last row is selected, and no length is a multiple of a block (37, 70, 300 against 16,
    32 and 64): the lanes past the end repeat exactly that row.  It comes back once; the other slots are empty."""
    base = _base([37, 70, 300, 200], metric, pack, 1301)
    ids = np.sort([_list(base, l)[-1] for l in range(3)])

    def pre(sc, mode, res):
        assert ((res["I_ref"] >= 0).sum(axis=1) == 3).all()

    def post(sc, mode, res):
        assert ((res["I"] >= 0).sum(axis=1) == 3).all()
        assert all(np.array_equal(np.sort(r[:3]), ids) for r in res["I"])

    return SelCase(base, ids=ids, pre=pre, post=post)


def skipped_blocks(metric, pack):
    """Case 4: a list without a selected row, a list whose three selected rows sit at positions 70, 75 and 90 (one middle
    block of every scan: every block before and after it is skipped), a half-selected list and a fully selected one."""
    base = _base([200, 200, 100, 107], metric, pack, 1401)
    rng = np.random.default_rng(1402)
    ids = np.sort(np.concatenate([_list(base, 1)[[70, 75, 90]], rng.choice(_list(base, 2), 50, replace=False), _list(base, 3)]))

    def pre(sc, mode, res):
        assert not res["mask"][_list(base, 0)].any() and res["mask"][_list(base, 1)].sum() == 3
        assert np.array_equal(np.diff(res["off_f"]), [0, 3, 50, 107])

    return SelCase(base, ids=ids, pre=pre)


def word_edges(which, metric, pack):
    """Case 5: selections at the edges of the selector's 32-bit words.  "last": only row nb - 1 of nb = 333 rows (13 bits
    into the last word), with the 19 bits past it all ones - they are no rows and nothing at or past nb may come back."""
    base = _base([100, 33, 120, 80], metric, pack, 1501, k=5, ksub=64)
    n = base.xb.shape[0]
    ids = {"31": [31], "32": [32], "31-32-63-64": [31, 32, 63, 64], "last": [n - 1]}[which]
    words = bitmap_words(ids, n)
    if which == "last":
        assert n % 32 == 13
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(13)

    def pre(sc, mode, res):
        assert np.array_equal(np.nonzero(res["mask"])[0], ids)
        assert all(np.array_equal(np.sort(r[r >= 0]), ids) for r in res["I_ref"])

    def post(sc, mode, res):
        assert all(np.array_equal(np.sort(r[r >= 0]), ids) for r in res["I"])

    return SelCase(base, words=words, pre=pre, post=post)


def fewer_than_k(metric, pack):
    """Case 6: every query probes the one list it was drawn around (nprobe = 1).  The lists hold 3, 0, 12, 120 (all), 1, 0, 0
    and 0 selected rows against k = 10: queries of lists 0 and 4 get padded results, queries of lists 1 and 5-7 - whose
    selected rows all lie in unprobed lists - nothing at all."""
    nlist, per, d = 8, 120, 64
    c = synth.corpus(nlist, d, seed=1602)
    noise = synth.corpus(NQ, d, seed=1603)
    home = np.arange(NQ) % nlist
    xq = c[home] + np.float32(0.2) * noise
    xq = (xq / np.linalg.norm(xq, axis=1, keepdims=True)).astype(np.float32)
    base = _base([per] * nlist, metric, pack, 1601, nprobe=1, xq=xq, c=c)
    want = [3, 0, 12, per, 1, 0, 0, 0]
    ids = np.sort(np.concatenate([_list(base, l)[:w] for l, w in enumerate(want)]))

    def pre(sc, mode, res):
        assert np.array_equal(res["probe"][:, 0], home) and np.array_equal(res["Ip"][:, 0], home)
        assert np.array_equal((res["I_ref"] >= 0).sum(axis=1), np.minimum(10, np.array(want)[home]))

    def post(sc, mode, res):
        assert np.array_equal((res["I"] >= 0).sum(axis=1), np.minimum(10, np.array(want)[home]))

    return SelCase(base, ids=ids, pre=pre, post=post)


def shared_tiles(metric, pack):
    """Case 8 on its own: three lists, each probed by all 100 queries, 30 % of the rows selected."""
    base = _base([500, 300, 200], metric, pack, 1801)
    ids = np.sort(np.random.default_rng(1802).choice(1000, 300, replace=False))
    return SelCase(base, ids=ids, pre=_shared_tiles)


def refine_half(metric, pack):
    """Case 9's first stage: half of the rows selected, 24 candidates per query."""
    return random_selection(0.5, metric, pack, 1901, k=24)


def _entry(fn, *args, modes=MODES, **kw):
    return functools.partial(fn, *args, **kw), modes


CASES = {
    "random-50": _entry(random_selection, 0.5, IP, F16, 1001, nprobe=6),
    "random-10": _entry(random_selection, 0.1, L2, SPLIT, 1101),
    "random-1-d128": _entry(random_selection, 0.01, IP, SPLIT, 1201, d=128),
    "last-row-l2-f16": _entry(last_row_only, L2, F16),
    "last-row-ip-split": _entry(last_row_only, IP, SPLIT),
    "skipped-blocks-ip-split": _entry(skipped_blocks, IP, SPLIT),
    "skipped-blocks-l2-f16": _entry(skipped_blocks, L2, F16),
    "word-31": _entry(word_edges, "31", IP, F16),
    "word-32": _entry(word_edges, "32", L2, SPLIT),
    "word-31-32-63-64": _entry(word_edges, "31-32-63-64", IP, SPLIT),
    "word-last": _entry(word_edges, "last", L2, F16),
    "fewer-than-k-ip-f16": _entry(fewer_than_k, IP, F16),
    "fewer-than-k-l2-split": _entry(fewer_than_k, L2, SPLIT),
    "shared-tiles-l2-f16": _entry(shared_tiles, L2, F16),
}
PARAMS = [(name, mode) for name, (_, modes) in CASES.items() for mode in modes]
EXTRA = {"refine-50": _entry(refine_half, L2, SPLIT, modes=(SQ8, PQ))}  # driven by refine_over_a_selection


@functools.lru_cache(maxsize=4)
def build(name):
    return (CASES.get(name) or EXTRA[name])[0]()
