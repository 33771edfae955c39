"""Which route a ``HipVS`` call takes, held as the exact sequence of backend methods it calls, on the CPU with
``SelectOracleBackend`` behind a recording proxy: a table of calls over a Flat store, the three IVF modes and a
``Refine(Flat)`` store, each with ``ids_probe`` off and on (a label ending in "+"), the pipelined host route, and which of
two faults - or a fault and an early return - wins.  The sequences are literals: ``python tests/test_vs_routes_host.py``
prints the table of sequences from the code it runs against."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import synth
from ivf_pq_oracle_backend import PqOracleBackend
from ivf_select_oracle_backend import SelectOracleBackend
from lotus_amd import HipVS
from lotus_amd.vs import FLT_MAX
from test_ivf_pq_host import _quick_train

N, D_, NQ, NPROBE = 2100, 32, 12, 2  # K = N is past _capi.MAX_K; the 16 lists' scan scores about N * NPROBE / 16 = 262 rows
FACTORIES = ("Flat", "IVF16,Flat", "IVF16,SQ8", "IVF16,PQ8", "IVF16,SQ8,Refine(Flat)")
LABELS = tuple(fs + plus for fs in FACTORIES for plus in ("", "+"))


class Recorder:
    """Forwards everything to ``be`` and keeps the name of every public method that is CALLED through it.  A name the backend
    does not have - or one in ``hidden`` - is an ``AttributeError``, so ``hasattr`` answers as the wrapped backend does."""

    def __init__(self, be):
        self.be, self.names, self.hidden = be, [], set()

    def __getattr__(self, name):
        if name in self.hidden:
            raise AttributeError(name)
        value = getattr(self.be, name)
        if name.startswith("_") or not callable(value):
            return value

        def call(*a, **k):
            self.names.append(name)
            return value(*a, **k)

        return call


XB = synth.corpus(N, D_, seed=11)
XQ = synth.queries(XB, NQ, seed=12)[0]
_stores = {}


def store(label):
    if label not in _stores:
        fs, probe = label.rstrip("+"), label.endswith("+")
        vs = HipVS(backend=Recorder(SelectOracleBackend()), factory_string=fs, nprobe=NPROBE, ids_probe=probe, k_factor=3)
        with pytest.MonkeyPatch.context() as mp:  # the codebooks' training is not the subject here
            mp.setattr(PqOracleBackend, "ivf_pq_train", _quick_train)
            vs.index(None, XB, label, persist=False)
        _stores[label] = vs
    return _stores[label]


def subset(m, seed=0):
    return np.sort(np.random.default_rng(seed).choice(N, m, replace=False))


BIG = np.float32(1e4)  # components of about 0.2 * 1e4 are beyond fp16's range under the index's scale (unit rows: 2^7)


def one_big():
    q = XQ.copy()
    q[3] *= BIG
    return q


def no_row_bitmap(vs):
    vs.backend.hidden.add("row_bitmap")
    try:
        return vs(XQ, 10, ids=subset(1000))
    finally:
        vs.backend.hidden.clear()


# name -> (the call, rows and columns of its result; None: ``scores()``, a matrix)
CALLS = {
    "plain": (lambda vs: vs(XQ, 10), (NQ, 10)),
    "ids every row in order": (lambda vs: vs(XQ, 10, ids=list(range(N))), (NQ, 10)),
    "subset": (lambda vs: vs(XQ, 10, ids=subset(1000)), (NQ, 10)),
    "subset with a duplicate": (lambda vs: vs(XQ, 10, ids=np.concatenate([subset(999), subset(999)[:1]])), (NQ, 10)),
    "subset, K = len(ids)": (lambda vs: vs(XQ, 40, ids=subset(40)), (NQ, 40)),
    "subset, K > len(ids)": (lambda vs: vs(XQ, 50, ids=subset(40)), (NQ, 50)),
    "subset below the rows-scored rule": (lambda vs: vs(XQ, 10, ids=subset(100)), (NQ, 10)),
    "subset, no row_bitmap": (no_row_bitmap, (NQ, 10)),
    "subset, nprobe 3": (lambda vs: vs(XQ, 10, ids=subset(300), nprobe=3), (NQ, 10)),
    "K = 57": (lambda vs: vs(XQ, 57), (NQ, 57)),
    "K = 57, subset": (lambda vs: vs(XQ, 57, ids=subset(1000)), (NQ, 57)),
    "K = n": (lambda vs: vs(XQ, N), (NQ, N)),
    "K = n, ids": (lambda vs: vs(XQ, N, ids=subset(2060)), (NQ, N)),
    "K = 0": (lambda vs: vs(XQ, 0), (NQ, 0)),
    "no queries": (lambda vs: vs(XQ[:0], 10), (0, 10)),
    "empty ids": (lambda vs: vs(XQ, 10, ids=[]), (NQ, 10)),
    "nprobe above nlist": (lambda vs: vs(XQ, 10, nprobe=40), (NQ, 10)),
    "k_factor 6": (lambda vs: vs(XQ, 10, k_factor=6), (NQ, 10)),
    "return_device": (lambda vs: vs(XQ, 10, return_device=True), (NQ, 10)),
    "return_device, K > len(ids)": (lambda vs: vs(XQ, 50, ids=subset(40), return_device=True), (NQ, 50)),
    "one query out of range": (lambda vs: vs(one_big(), 10), (NQ, 10)),
    "one query out of range, return_device": (lambda vs: vs(one_big(), 10, return_device=True), (NQ, 10)),
    "all queries out of range": (lambda vs: vs(XQ * BIG, 10), (NQ, 10)),
    "scores": (lambda vs: vs.scores(XQ), None),
    "scores, ids": (lambda vs: vs.scores(XQ, ids=subset(1000)), None),
    "scores, ids every row in order": (lambda vs: vs.scores(XQ, ids=np.arange(N)), None),
    "scores, one query out of range": (lambda vs: vs.scores(one_big()), None),
}
ON_DEVICE = {"return_device", "one query out of range, return_device"}  # K > len(ids) comes back padded, on the host

ALL = "every store"

# call -> {the recorded names: the stores that record them}, from the parent of the commit that added this file
EXPECTED = {
    'plain': {
        'pack score_exp_of search_keys keys_to_result':
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result':
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result':
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result':
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result':
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'ids every row in order': {
        'pack score_exp_of search_keys keys_to_result':
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result':
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result':
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result':
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result':
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'subset': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits row_bitmap pack score_exp_of ivf_search keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits row_bitmap pack score_exp_of ivf_sq8_search keys_to_result':
            'IVF16,SQ8+',
        'ivf_pq_fits row_bitmap pack score_exp_of ivf_pq_search keys_to_result':
            'IVF16,PQ8+',
        'ivf_sq8_fits row_bitmap pack score_exp_of ivf_sq8_search refine_keys keys_to_result':
            'IVF16,SQ8,Refine(Flat)+',
    },
    'subset with a duplicate': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits row_bitmap pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits row_bitmap pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits row_bitmap pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'subset, K = len(ids)': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'subset, K > len(ids)': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'subset below the rows-scored rule': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'subset, no row_bitmap': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'subset, nprobe 3': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'K = 57': {
        'pack score_exp_of search_keys keys_to_result':
            ALL,
    },
    'K = 57, subset': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            ALL,
    },
    'K = n': {
        'pack score_exp_of slice_rows scores rank_scores keys_to_result':
            ALL,
    },
    'K = n, ids': {
        'pack score_exp_of slice_rows to_device gather scores rank_scores to_device keys_to_result':
            ALL,
    },
    'K = 0': {
        '':
            ALL,
    },
    'no queries': {
        '':
            ALL,
    },
    'empty ids': {
        '':
            ALL,
    },
    'nprobe above nlist': {
        'pack score_exp_of search_keys keys_to_result':
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result':
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result':
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result':
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result':
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'k_factor 6': {
        'pack score_exp_of search_keys keys_to_result':
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result':
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result':
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result':
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result':
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'return_device': {
        'pack score_exp_of search_keys keys_to_result':
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result':
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result':
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result':
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result':
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'return_device, K > len(ids)': {
        'pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'Flat Flat+ IVF16,Flat IVF16,SQ8 IVF16,PQ8 IVF16,SQ8,Refine(Flat)',
        'ivf_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,SQ8+ IVF16,SQ8,Refine(Flat)+',
        'ivf_pq_fits pack score_exp_of to_device gather to_device search_keys to_device keys_to_result':
            'IVF16,PQ8+',
    },
    'one query out of range': {
        'pack score_exp_of search_keys keys_to_result ' * 3:
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result ' * 3:
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result ' * 3:
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result ' * 3:
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result ' * 3:
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'one query out of range, return_device': {
        'pack score_exp_of search_keys keys_to_result ' * 3:
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result ' * 3:
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result ' * 3:
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result ' * 3:
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result ' * 3:
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'all queries out of range': {
        'pack score_exp_of search_keys keys_to_result ' * 2:
            'Flat Flat+',
        'ivf_fits pack score_exp_of ivf_search keys_to_result ' * 2:
            'IVF16,Flat IVF16,Flat+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search keys_to_result ' * 2:
            'IVF16,SQ8 IVF16,SQ8+',
        'ivf_pq_fits pack score_exp_of ivf_pq_search keys_to_result ' * 2:
            'IVF16,PQ8 IVF16,PQ8+',
        'ivf_sq8_fits pack score_exp_of ivf_sq8_search refine_keys keys_to_result ' * 2:
            'IVF16,SQ8,Refine(Flat) IVF16,SQ8,Refine(Flat)+',
    },
    'scores': {
        'pack scores':
            ALL,
    },
    'scores, ids': {
        'pack to_device gather scores':
            ALL,
    },
    'scores, ids every row in order': {
        'pack scores':
            ALL,
    },
    'scores, one query out of range': {
        'pack pack scores pack scores':
            ALL,
    },
}

# call -> the routes of the plans it makes (a call that is searched again makes several; "none": empty ``ids``, no plan) on the
# Flat stores, on the IVF stores with ``ids_probe`` off, and on those with it on
ROUTES = {
    "plain": ("flat", "ivf", "ivf"),
    "ids every row in order": ("flat", "ivf", "ivf"),
    "subset": ("subset", "subset", "ivf"),
    "subset with a duplicate": ("subset", "subset", "subset"),
    "subset, K = len(ids)": ("subset", "subset", "subset"),
    "subset, K > len(ids)": ("subset", "subset", "subset"),
    "subset below the rows-scored rule": ("subset", "subset", "subset"),
    "subset, no row_bitmap": ("subset", "subset", "subset"),
    "subset, nprobe 3": ("subset", "subset", "subset"),
    "K = 57": ("flat", "flat", "flat"),
    "K = 57, subset": ("subset", "subset", "subset"),
    "K = n": ("rank_all", "rank_all", "rank_all"),
    "K = n, ids": ("rank_all", "rank_all", "rank_all"),
    "K = 0": ("", "", ""),
    "no queries": ("", "", ""),
    "empty ids": ("none", "none", "none"),
    "nprobe above nlist": ("flat", "ivf", "ivf"),
    "k_factor 6": ("flat", "ivf", "ivf"),
    "return_device": ("flat", "ivf", "ivf"),
    "return_device, K > len(ids)": ("subset", "subset", "subset"),
    "one query out of range": ("flat " * 3, "ivf " * 3, "ivf " * 3),
    "one query out of range, return_device": ("flat " * 3, "ivf " * 3, "ivf " * 3),
    "all queries out of range": ("flat " * 2, "ivf " * 2, "ivf " * 2),
    "scores": ("", "", ""),
    "scores, ids": ("", "", ""),
    "scores, ids every row in order": ("", "", ""),
    "scores, one query out of range": ("", "", ""),
}


def run(name, label):
    vs = store(label)
    vs.backend.names.clear()
    return vs, CALLS[name][0](vs)


def stores_of(name):
    return {label: seq for seq, labels in EXPECTED[name].items() for label in (LABELS if labels is ALL else labels.split())}


CASES = [(name, label) for name in CALLS for label in LABELS]


@pytest.mark.parametrize("name,label", CASES, ids=[f"{n}-{l}" for n, l in CASES])
def test_backend_calls(name, label):
    vs, out = run(name, label)
    assert vs.backend.names == stores_of(name)[label].split()
    shape = CALLS[name][1]
    if shape is None:
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape[0] == NQ
        return
    host = name not in ON_DEVICE
    for a, dtype in ((out.distances, "float32"), (out.indices, "int64")):
        assert isinstance(a, np.ndarray) == host and tuple(a.shape) == shape and str(a.dtype).endswith(dtype)
    if name == "subset, K > len(ids)":
        assert (out.indices[:, 40:] == -1).all() and (out.distances[:, 40:] == -FLT_MAX).all() and (out.indices[:, :40] >= 0).all()
    if name == "empty ids":
        assert (out.indices == -1).all() and (out.distances == -FLT_MAX).all()


@pytest.mark.parametrize("name,label", CASES, ids=[f"{n}-{l}" for n, l in CASES])
def test_route_strings(name, label, monkeypatch):
    routes = plan_routes(monkeypatch, lambda: run(name, label))
    assert routes == ROUTES[name][0 if label.startswith("Flat") else 1 + label.endswith("+")].split()


def plan_routes(monkeypatch, fn):
    routes, orig = [], HipVS._plan_call

    def spy(self, *a, **k):
        plan = orig(self, *a, **k)
        routes.append("none" if plan is None else plan.route)
        return plan

    monkeypatch.setattr(HipVS, "_plan_call", spy)
    fn()
    return routes


# ---- the pipelined host route ------------------------------------------------------------------------------------------------
def pipelined_store():
    be = SelectOracleBackend()

    def search_host_pipelined(packed, q, k, metric, id_offset=0, normalize=False, exp=0):
        queries = be.pack(q, packed.mode, normalize=normalize, exp=exp, check="lazy")
        keys = be.search_keys(packed, queries, k, metric, id_offset=id_offset)
        D, I = be.keys_to_result(keys, metric, None, score_exp=be.score_exp_of(packed, queries))
        return D.numpy(), I.numpy(), int(queries.flags.item())

    be.search_host_pipelined, be.CALL_PIPELINE_MIN_QUERIES = search_host_pipelined, 4
    vs = HipVS(backend=Recorder(be), storage="fp16")
    vs.index(None, XB, "pipelined", persist=False)
    vs.backend.names.clear()
    return vs


def test_pipelined_route_is_one_backend_call():
    vs = pipelined_store()
    q16 = XQ.astype(np.float16)
    out = vs(q16, 10)
    assert vs.backend.names == ["search_host_pipelined"]
    for args, kw in (((q16[:3], 10), {}), ((q16, 10), {"return_device": True}), ((q16, 10), {"ids": subset(1000)}),
                     ((q16, N), {}), ((q16, N + 1), {})):  # too few queries, a device result, ids, K = N, a padded result
        vs.backend.names.clear()
        vs(*args, **kw)
        assert "search_host_pipelined" not in vs.backend.names and "pack" in vs.backend.names
    vs.backend.names.clear()
    again = vs(q16, 10, ids=np.arange(N))  # every row in order is the plain call
    assert vs.backend.names == ["search_host_pipelined"]
    vs.backend.hidden.add("search_host_pipelined")
    plain = vs(q16, 10)
    for o in (again, plain):
        assert np.array_equal(o.indices, out.indices) and np.array_equal(o.distances, out.distances)


def test_pipelined_route_string(monkeypatch):
    vs = pipelined_store()
    assert plan_routes(monkeypatch, lambda: vs(XQ.astype(np.float16), 10)) == ["pipelined"]


# ---- which fault wins --------------------------------------------------------------------------------------------------------
BAD_IDS = [0, N]
WIDE = np.zeros((3, D_ + 1), np.float32)
IVF, FLAT = "IVF16,SQ8,Refine(Flat)+", "Flat"

# (store, arguments, keywords, the exception and a piece of its text - or the shape of the padded result that comes back, or
# "searched")
PRECEDENCE = [
    (None, (WIDE, -1), {}, (ValueError, "Index not loaded")),
    (IVF, (WIDE, -1), {}, (ValueError, "query dimension 33 does not match index dimension 32")),
    (IVF, (WIDE, 0), {}, (ValueError, "query dimension")),
    (IVF, (XQ, -1), {"ids": BAD_IDS}, (ValueError, "K must be >= 0")),
    (IVF, (XQ, 0), {"ids": BAD_IDS}, (NQ, 0)),
    (IVF, (XQ[:0], 5), {"ids": BAD_IDS}, (0, 5)),
    (IVF, (XQ, 0), {"nprobe": 0, "k_factor": 0, "ids_probe": 1}, (NQ, 0)),
    (IVF, (XQ, 5), {"ids": BAD_IDS, "nprobe": 0}, (IndexError, "ids out of range for the loaded index")),
    (IVF, (XQ, 5), {"ids": BAD_IDS, "k_factor": 0}, (IndexError, "ids out of range")),
    (FLAT, (XQ, 5), {"ids": [-1], "ids_probe": 1}, (IndexError, "ids out of range")),
    (IVF, (XQ, 5), {"ids": [], "nprobe": 0}, (NQ, 5)),
    (IVF, (XQ, 5), {"ids": [], "k_factor": 0}, (NQ, 5)),
    (FLAT, (XQ, 5), {"ids": [], "ids_probe": 1}, (NQ, 5)),
    (IVF, (XQ, 5), {"nprobe": 0}, (ValueError, "nprobe must be an int >= 1")),
    (FLAT, (XQ, 5), {"nprobe": 0}, "searched"),  # validated only for a store with lists
    (FLAT, (XQ, 5), {"k_factor": 0}, (ValueError, "k_factor must be a finite number >= 1")),
    (FLAT, (XQ, 5), {"ids_probe": 1}, (ValueError, "ids_probe must be a bool")),
    (IVF, (XQ, 5), {"nprobe": 0, "k_factor": 0, "ids_probe": 1}, (ValueError, "nprobe")),
    (IVF, (XQ, 5), {"k_factor": 0, "ids_probe": 1}, (ValueError, "k_factor")),
    (FLAT, (XQ, 5), {"nprobe": 0, "k_factor": 0, "ids_probe": 1}, (ValueError, "k_factor")),
]


@pytest.mark.parametrize("label,args,kw,wins", PRECEDENCE, ids=[str(i) for i in range(len(PRECEDENCE))])
def test_precedence(label, args, kw, wins):
    vs = HipVS(backend=SelectOracleBackend()) if label is None else store(label)
    if wins == "searched":
        assert (vs(*args, **kw).indices >= 0).all()
        return
    if isinstance(wins[0], int):
        out = vs(*args, **kw)
        assert out.distances.shape == out.indices.shape == wins
        assert (out.indices == -1).all() and (out.distances == -FLT_MAX).all()
        return
    with pytest.raises(wins[0], match=wins[1]):
        vs(*args, **kw)


def test_nothing_to_search_returns_before_the_layout(monkeypatch):
    vs = store(FLAT)

    def boom(*a, **k):
        raise AssertionError("_layout was reached")

    monkeypatch.setattr(vs, "_layout", boom)
    for args, kw in (((XQ, 0), {}), ((XQ[:0], 5), {}), ((XQ, 5), {"ids": []})):
        vs.backend.names.clear()
        assert vs(*args, **kw).indices.shape == (len(args[0]), args[1]) and vs.backend.names == []
    with pytest.raises(AssertionError, match="_layout"):
        vs(XQ, 5)


def test_ids_of_the_other_entry_points(monkeypatch):
    """``scores``, ``packed_rows`` and ``kmeans`` take ``ids`` as ``__call__`` does."""
    vs = store(FLAT)
    ent = vs._current()
    for fn in (lambda ids: vs.scores(XQ, ids=ids), vs.packed_rows, lambda ids: vs.kmeans(None, 4, niter=1, ids=ids)):
        for bad in ([-1], BAD_IDS, np.arange(1, N + 1)):
            with pytest.raises(IndexError, match="ids out of range for the loaded index"):
                fn(bad)
    with pytest.raises(ValueError, match="query dimension 33"):
        vs.scores(WIDE, ids=BAD_IDS)
    assert vs.packed_rows() is ent.packed and vs.packed_rows(np.arange(N)) is ent.packed and vs.packed_rows(list(range(N))) is ent.packed
    back = np.arange(N)[::-1]
    assert vs.packed_rows(back) is not ent.packed and vs.packed_rows(back).n == N and vs.packed_rows([]).n == 0
    monkeypatch.setattr(ent, "hi", N - 1)  # a shard: refused before ``ids`` is looked at
    with pytest.raises(ValueError, match="packed_rows needs an unsharded index"):
        vs.packed_rows(BAD_IDS)


def test_recorder_answers_hasattr_as_the_backend_does():
    rec = Recorder(SelectOracleBackend())
    assert hasattr(rec, "row_bitmap") and not hasattr(rec, "search_host_pipelined") and not hasattr(rec, "to_host")
    rec.to_device(np.zeros(2))
    assert rec.names == ["to_device"] and rec.calls == []  # fetched, not called: not recorded
    rec.hidden.add("row_bitmap")
    assert not hasattr(rec, "row_bitmap")


if __name__ == "__main__":
    class Repeated(str):
        __repr__ = str.__str__

    print("EXPECTED = {")
    for name in CALLS:
        seqs = {}
        for label in LABELS:
            seqs.setdefault(" ".join(run(name, label)[0].backend.names), []).append(label)
        print(f"    {name!r}: {{")
        for seq, labels in seqs.items():
            words = seq.split()
            for r in (3, 2):  # a call that is searched again records its names over again
                if words and words == words[:len(words) // r] * r:
                    seq = Repeated(f"{' '.join(words[:len(words) // r]) + ' '!r} * {r}")
                    break
            print(f"        {seq!r}:\n            {'ALL' if len(labels) == len(LABELS) else repr(' '.join(labels))},")
        print("    },")
    print("}")
