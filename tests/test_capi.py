"""The C-ABI library builds for gfx950 without a GPU, loads, and exports exactly what include/lotus_hip.h declares.
No compute call is made here."""
import ast
import contextlib
import ctypes
import glob
import os
import subprocess
import types

import pytest

from lotus_amd import _capi


def test_library_exports_every_declared_symbol():
    lib = _capi.load()
    declared = _capi.declared_symbols()
    assert len(declared) >= 14
    assert set(declared) == set(_capi.SIGNATURES) == set(_capi.PROTOTYPES), "ctypes table and header out of sync"
    for name in declared:
        assert hasattr(lib, name), name
        assert (getattr(lib, name).restype, list(getattr(lib, name).argtypes)) == _capi.SIGNATURES[name], name


# ---- the header is the table: its parser, on the real header and on small ones ------------------------------------------------
I32, I64, F32, F64, VP = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
# the header's whole vocabulary of parameter types: four scalars, pointers to nine base types, the two callback typedefs
PARAMETER_TYPES = ({"int32_t", "int64_t", "float", "double", "lvs_all_gather_fn", "lvs_all_reduce_fn"}
                   | {const + base + "*" for const in ("", "const ")
                      for base in ("void", "char", "float", "double", "int32_t", "int64_t", "uint8_t", "uint32_t", "uint64_t")})


def test_the_header_parses_to_83_prototypes_and_2_callbacks():
    protos = _capi.PROTOTYPES
    assert len(protos) == 83 and sorted(_capi.CALLBACKS) == ["lvs_all_gather_fn", "lvs_all_reduce_fn"]
    spelled = {t for p in protos.values() for t in p.types}
    assert spelled <= PARAMETER_TYPES and len(spelled) == 22, spelled - PARAMETER_TYPES
    for name, p in protos.items():
        assert len(p.argtypes) == len(p.names) == len(p.types) and len(set(p.names)) == len(p.names), name
        for ctype, spelling in zip(p.argtypes, p.types):  # scalars keep their width, everything else is an address
            assert ctype is {"int32_t": I32, "int64_t": I64, "float": F32, "double": F64}.get(spelling, VP), (name, spelling)
        assert _capi.SIGNATURES[name] == (p.restype, list(p.argtypes))
    assert {p.restype for p in protos.values()} == {I32, I64, ctypes.c_char_p}
    assert all((p.restype is I64) == name.endswith("_workspace_bytes") for name, p in protos.items() if name != "lvs_last_error")


def test_the_entries_where_a_wrong_type_would_hurt_most():
    protos = _capi.PROTOTYPES
    p = protos["lvs_ivf_range_search"]
    assert len(p.names) == 29
    assert [n for n, t in zip(p.names, p.argtypes) if t is F32] == ["threshold"]
    assert [n for n, t in zip(p.names, p.argtypes) if t is I64] == ["nb", "nq", "capacity", "workspace_bytes"]
    p = protos["lvs_flat_search_keys_hi_banded"]
    at = p.names.index("kc")
    assert p.names[at:at + 3] == ("kc", "band_scale", "band_slack") and p.argtypes[at:at + 3] == (I32, F32, F32)
    assert [n for n, t in zip(p.names, p.argtypes) if t is F32] == ["band_scale", "band_slack"]
    p = protos["lvs_search_sharded"]
    assert (p.names[0], p.types[0], p.argtypes[0]) == ("all_gather", "lvs_all_gather_fn", VP)
    assert protos["lvs_kmeans_iteration"].types[0] == "lvs_all_reduce_fn"
    assert protos["lvs_last_error"] == _capi.Prototype(ctypes.c_char_p, (), (), ())
    assert protos["lvs_flat_search_keys"].names == (
        "xb", "xb_pack", "nb", "xq", "xq_pack", "nq", "d", "metric", "k", "xb_norms_sq", "xq_norms_sq", "id_offset", "row_ids",
        "out_keys", "workspace", "workspace_bytes", "stream")
    assert protos["lvs_flat_search_keys"].argtypes == (VP, I32, I64, VP, I32, I64, I32, I32, I32, VP, VP, I64, VP, VP, VP, I64, VP)


def test_parser_on_small_headers():
    protos, callbacks, defines = _capi.parse_header("""
        /* lvs_x(int32_t a); in a comment declares nothing */
        // nor does lvs_y(int32_t a); here
        #ifndef H
        #define H
        #define LVS_SEVEN 7 /* a comment
                               over two lines */
        #define LVS_MINUS (-3)
        extern "C" {
        typedef int32_t (*lvs_cb_fn)(void* ctx, int64_t n);
        int64_t
        lvs_split(const void* a,   /* a comment between parameters */
                  int64_t n, float
                  scale, lvs_cb_fn cb);
        const char* lvs_nothing(void);
        int32_t lvs_empty();
        }
        #endif
    """)
    assert defines == {"LVS_SEVEN": 7, "LVS_MINUS": -3}
    assert list(protos) == ["lvs_split", "lvs_nothing", "lvs_empty"]
    assert protos["lvs_split"] == _capi.Prototype(I64, (VP, I64, F32, VP), ("a", "n", "scale", "cb"),
                                                  ("const void*", "int64_t", "float", "lvs_cb_fn"))
    assert protos["lvs_nothing"] == _capi.Prototype(ctypes.c_char_p, (), (), ()) and protos["lvs_empty"].names == ()
    assert list(callbacks) == ["lvs_cb_fn"]
    assert (callbacks["lvs_cb_fn"]._restype_, callbacks["lvs_cb_fn"]._argtypes_) == (I32, (VP, I64))
    for bad, names in [("int32_t lvs_sized(size_t n);", ("lvs_sized", "size_t n")),          # a type outside the vocabulary
                       ("int32_t lvs_unnamed(int32_t);", ("lvs_unnamed", "int32_t")),        # no parameter name
                       ("int32_t lvs_deep(float** rows);", ("lvs_deep", "float** rows")),
                       ("int32_t lvs_later(lvs_late_fn cb);", ("lvs_later", "lvs_late_fn")),   # a callback type nobody declared
                       ("int32_t lvs_twice(int32_t a, float a);", ("lvs_twice",)),
                       ("float lvs_ret(int32_t a);", ("lvs_ret", "float")),
                       ("struct lvs_s { int a; };", ("struct",))]:
        with pytest.raises(ValueError) as e:
            _capi.parse_header(bad)
        assert all(n in str(e.value) for n in names), (bad, str(e.value))


# ---- the binder, against a stub in place of the library ------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


def _stub_backend():
    from lotus_amd.backend import HipBackend

    be = object.__new__(HipBackend)
    be.lib, be.device = _StubLib(), None
    be.torch = types.SimpleNamespace(cuda=types.SimpleNamespace(device=lambda dev: contextlib.nullcontext()))
    return be


def test_binder_orders_keywords_as_the_header_does():
    be = _stub_backend()
    # lvs_merge_keys(parts, nparts, nq, k, out_keys, stream)
    be._c("lvs_merge_keys", stream=6, k=4, out_keys=5, nq=3, parts=1, nparts=2)
    be._c("lvs_merge_keys", 1, 2, 3, stream=6, out_keys=5, k=4)   # positional, then the rest by name
    be._c("lvs_merge_keys", 1, 2, 3, 4, 5, stream=6)
    be._c("lvs_merge_keys", 1, 2, 3, 4, 5, 6)
    assert be.lib.calls == [("lvs_merge_keys", (1, 2, 3, 4, 5, 6))] * 4
    args = (object(), None, 2.5)
    assert _capi.bind("lvs_merge_keys", args, {}) is args  # a positional call is handed on as it is, whatever its length
    assert _capi.bind("lvs_abi_version", (), {}) == ()
    # the longest entry, every argument by name in reverse order
    names = _capi.PROTOTYPES["lvs_ivf_range_search"].names
    assert _capi.bind("lvs_ivf_range_search", (), {n: i for i, n in reversed(list(enumerate(names)))}) == tuple(range(29))
    for kw, complaint in [(dict(parts=1, nparts=2, nq=3, k=4, out_keys=5), "missing parameter 'stream'"),
                          (dict(parts=1, nparts=2, nq=3, k=4, out_keys=5, stream=6, streem=6), "unknown parameter 'streem'"),
                          (dict(parts=1, nparts=2, nq=3, k=4, out_keys=5, streem=6), "missing parameter 'stream'")]:
        with pytest.raises(TypeError, match="lvs_merge_keys: " + complaint):
            be._c("lvs_merge_keys", **kw)
    with pytest.raises(TypeError, match="lvs_merge_keys: parameter 'nparts' given twice"):
        be._c("lvs_merge_keys", 1, 2, nparts=2, nq=3, k=4, out_keys=5, stream=6)
    with pytest.raises(TypeError, match="lvs_merge_keys: unknown parameter 'extra'"):
        be._c("lvs_merge_keys", 1, 2, 3, 4, 5, 6, extra=7)
    with pytest.raises(TypeError, match="lvs_abi_version: unknown parameter 'x'"):
        be._c("lvs_abi_version", x=1)
    assert len(be.lib.calls) == 4  # none of the refused calls reached the library
    # the product's own calls bind in _call: a wrapper around _c (ws_guard.exact_workspace) sees positional arguments only
    seen, plain_c = [], be._c
    be._c = lambda name, *args: seen.append((name, args)) or plain_c(name, *args)
    be._call("lvs_merge_keys", stream=6, k=4, out_keys=5, nq=3, parts=1, nparts=2)
    be._call("lvs_merge_keys", 1, 2, 3, 4, stream=6, out_keys=5)
    assert seen == be.lib.calls[4:] == [("lvs_merge_keys", (1, 2, 3, 4, 5, 6))] * 2
    with pytest.raises(TypeError, match="lvs_merge_keys: missing parameter 'stream'"):
        be._call("lvs_merge_keys", 1, 2, 3, 4, out_keys=5)
    assert len(seen) == 2


def _c_calls(tree):
    """(entry name, call node) of every ``<anything>._c("lvs_...", ...)`` or ``._call("lvs_...", ...)`` in a module."""
    for node in ast.walk(tree):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("_c", "_call") and node.args
                and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str)):
            yield node.args[0].value, node


OPERANDS = ("xb", "xb_pack", "nb", "xb_norms_sq", "xq", "xq_pack", "nq", "xq_norms_sq", "d")  # what backend._operands names


def test_every_call_of_the_product_names_its_entry_s_parameters():
    """A misspelt, missing or doubled keyword in lotus_amd/*.py fails here, without a device."""
    root = os.path.dirname(os.path.abspath(_capi.__file__))
    seen = 0
    for path in sorted(glob.glob(os.path.join(root, "*.py"))):
        for entry, node in _c_calls(ast.parse(open(path).read())):
            where = f"{os.path.basename(path)}:{node.lineno} {entry}"
            assert entry in _capi.PROTOTYPES, where
            names = _capi.PROTOTYPES[entry].names
            positional, given = node.args[1:], [k.arg for k in node.keywords if k.arg is not None]
            assert not any(isinstance(a, ast.Starred) for a in positional), where
            splats = [k.value for k in node.keywords if k.arg is None]
            blocks = [v for v in splats if isinstance(v, ast.Call) and getattr(v.func, "id", "") == "_operands"]
            given += OPERANDS * len(blocks)  # the operand block goes only where the entry declares all nine
            assert len(set(given)) == len(given) and set(given) <= set(names[len(positional):]), \
                (where, set(given) - set(names[len(positional):]))
            if len(blocks) == len(splats):  # no other ** splat: the call spells out every parameter
                assert len(positional) + len(given) == len(names), (where, set(names[len(positional):]) - set(given))
                assert len(names) < 6 or not positional, where + ": six or more arguments go by name"
            seen += 1
    assert seen >= 40


def test_operand_block():
    from lotus_amd.backend import PackedRows, _operands

    t = types.SimpleNamespace(data_ptr=lambda: 64)
    block = _operands(PackedRows(rows=t, norms=t, n=3, d=8, mode=0), PackedRows(rows=t, norms=t, n=2, d=8, mode=1))
    assert block == dict(xb=64, xb_pack=0, nb=3, xb_norms_sq=64, xq=64, xq_pack=1, nq=2, xq_norms_sq=64, d=8)
    assert tuple(block) == OPERANDS
    assert len([name for name, p in _capi.PROTOTYPES.items() if set(OPERANDS) <= set(p.names)]) >= 12


def test_constants_equal_the_header_s_defines():
    d = _capi.DEFINES
    for name in ("OK", "EINVAL", "ENOMEM", "EDEVICE", "EUNSUPPORTED", "DTYPE_F32", "DTYPE_F16", "METRIC_IP", "METRIC_L2", "PACK_F16",
                 "PACK_SPLIT", "MAX_K", "NEAREST3_MAX_ROWS", "ABI_VERSION", "BUILD_TUNING", "BUILD_COUNT_EVENTS",
                 "PACK_FLAG_NONFINITE", "PACK_FLAG_RANGE"):
        assert getattr(_capi, name) == d["LVS_" + name], name
    assert (_capi.EINVAL, _capi.EUNSUPPORTED, _capi.MAX_K, _capi.ABI_VERSION) == (-1, -4, 2048, 7)
    from lotus_amd.backend import HipBackend

    assert HipBackend.KERNEL_NAMES.keys() == {v for n, v in d.items() if n.startswith("LVS_KERNEL_")}
    gather, reduce_ = _capi.CALLBACKS["lvs_all_gather_fn"], _capi.CALLBACKS["lvs_all_reduce_fn"]
    assert (gather._restype_, gather._argtypes_) == (I32, (VP, VP, VP, I64, VP))
    assert (reduce_._restype_, reduce_._argtypes_) == (I32, (VP, VP, I64, I32, VP))


def test_host_out_parameters_take_byref_arrays_and_string_buffers():
    lib = _capi.load()
    assert _capi.device_count() >= 0
    name, cus, hbm = ctypes.create_string_buffer(64), I32(-5), I64(-5)
    st = lib.lvs_device_info(1 << 20, name, 64, ctypes.byref(cus), ctypes.byref(hbm))  # no such device: refused, not a TypeError
    assert st != _capi.OK
    tot, launches, calls, kernel = F64(-1), I64(-1), I64(-1), I32(-1)
    assert lib.lvs_timing_read(ctypes.byref(tot), ctypes.byref(launches)) == _capi.OK and launches.value == 0
    assert lib.lvs_timing_read_calls(ctypes.byref(tot), ctypes.byref(launches), ctypes.byref(calls), ctypes.byref(kernel)) == _capi.OK
    assert (tot.value, launches.value, calls.value) == (0.0, 0, 0)
    coef = (F32 * 5)()
    assert lib.lvs_nearest_bound_coef(_capi.METRIC_L2, _capi.PACK_SPLIT, 64, 0, coef) == _capi.OK and coef[1] > 0  # an array as it is


def test_shared_object_is_gfx950_code():
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", _capi.LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:  # tool missing: fall back to a byte search
        blob = open(_capi.LIB_PATH, "rb").read()
        assert b"gfx950" in blob
    else:
        blob = open(_capi.LIB_PATH, "rb").read()
        assert b"gfx950" in blob and b"lvs_tile_kernel" in blob


def test_host_side_entry_points_without_a_gpu():
    lib = _capi.load()
    assert lib.lvs_abi_version() == _capi.ABI_VERSION == 7 and lib.lvs_build_flags() == 0
    assert lib.lvs_packed_ld(768, _capi.PACK_F16) == 768
    assert lib.lvs_packed_ld(100, _capi.PACK_F16) == 128
    assert lib.lvs_packed_ld(384, _capi.PACK_SPLIT) == 768
    assert lib.lvs_packed_ld(0, _capi.PACK_F16) < 0 and lib.lvs_packed_ld(8, 7) < 0
    ws = lib.lvs_flat_search_workspace_bytes(100000, 1000000, 768, 10, 0, 0)
    assert 100000 * 10 * 8 <= ws < 1 << 30
    assert lib.lvs_flat_search_workspace_bytes(-1, 10, 8, 1, 0, 0) < 0
    assert lib.lvs_flat_search_workspace_bytes(10, 10, 8, 1, 5, 0) < 0  # bad pack mode
    # argument validation happens before any device work
    st = lib.lvs_flat_search_keys(None, 0, 10, None, 0, 10, 8, 5, 3, None, None, 0, None, None, None, 0, None)
    assert st == _capi.EINVAL and b"metric" in lib.lvs_last_error()
    st = lib.lvs_merge_keys(None, 2, 5, 100, None, None)
    assert st == _capi.EINVAL
    assert lib.lvs_flat_search_keys(None, 0, 10, None, 0, 0, 8, 0, 3, None, None, 0, None, None, None, 0, None) == 0
    # the sharded search: scratch = both all-gather images + this shard's lists + the search's own scratch; pooled thresholds
    # only for fp16 rows, k <= 56 and more than one rank (decided from the arguments, identically on every rank)
    one = lib.lvs_search_sharded_workspace_bytes(1, 100000, 1000000, 768, 10, 0, 0, 20)
    assert ws <= one < ws + 2 * 100000 * 10 * 8 + 4096
    w8 = lib.lvs_search_sharded_workspace_bytes(8, 100000, 125000, 768, 10, 0, 0, 20)
    w8_unseeded = lib.lvs_search_sharded_workspace_bytes(8, 100000, 125000, 768, 10, 0, 0, 0)
    assert w8 - w8_unseeded >= 9 * 20 * 100000 * 4 and w8_unseeded >= 9 * 100000 * 10 * 8
    assert lib.lvs_search_sharded_workspace_bytes(8, 100000, 125000, 768, 10, _capi.PACK_SPLIT, 0, 20) < w8  # hi|lo rows: no pool
    assert lib.lvs_search_sharded_workspace_bytes(0, 10, 10, 8, 1, 0, 0, 0) < 0
    st = lib.lvs_search_sharded(None, None, 2, None, 0, 10, None, 0, 10, 8, 0, 3, None, None, 0, 0, None, None, 0, None)
    assert st == _capi.EINVAL and b"all-gather" in lib.lvs_last_error()
    assert lib.lvs_search_sharded(None, None, 1, None, 0, 10, None, 0, 0, 8, 0, 3, None, None, 0, 0, None, None, 0, None) == 0
    assert lib.lvs_rccl_available() in (0, 1)
    assert lib.lvs_search_sharded_rccl(None, None, 0, 10, None, 0, 10, 8, 0, 3, None, None, 0, 0, None, None, 0, None) != 0


def _ivf_search_calls(lib):
    """name -> call(nq, d, metric, nprobe, k, M) of the three IVF searches with NULL buffers, nb = 1000, nlist = 64, fp16"""
    def flat(nq, d, metric, nprobe, k, M):
        return lib.lvs_ivf_search_keys(None, 0, 1000, None, None, None, 64, None, 0, None, None, 0, nq, None, d, metric, nprobe, k,
                                       None, None, None, 0, None)

    def sq8(nq, d, metric, nprobe, k, M):
        return lib.lvs_ivf_sq8_search_keys(None, None, None, None, None, None, 1000, 64, None, 0, None, None, None, 0, nq, None, d,
                                           metric, nprobe, k, None, None, None, 0, None)

    def pq(nq, d, metric, nprobe, k, M):
        return lib.lvs_ivf_pq_search_keys(None, None, None, M, 256, None, None, 1000, 64, None, 0, None, None, None, 0, nq, None,
                                          d, metric, nprobe, k, None, None, None, 0, None)

    return {"flat": flat, "sq8": sq8, "pq": pq}


def test_ivf_search_argument_checks_without_a_gpu():
    # every answer below is decided before the NULL-buffer check and before a device is touched
    lib = _capi.load()
    for name, call in _ivf_search_calls(lib).items():
        assert call(10, 64, 5, 8, 10, 8) == _capi.EINVAL and b"metric" in lib.lvs_last_error(), name
        assert call(10, 64, 0, 65, 10, 8) == _capi.EINVAL and b"nprobe=65" in lib.lvs_last_error(), name  # nprobe > nlist
        assert call(10, 64, 0, 8, 57, 8) == _capi.EINVAL and b"k=57" in lib.lvs_last_error(), name
        assert call(10, 64, 0, 8, 56, 8) == _capi.EINVAL and b"NULL buffer" in lib.lvs_last_error(), name  # the checks passed
        assert call(0, 64, 0, 8, 10, 8) == _capi.OK, name  # no queries: nothing to do
        assert call(0, 64, 5, 8, 10, 8) == _capi.EINVAL, name  # ... but the arguments are still checked
    pq = _ivf_search_calls(lib)["pq"]
    assert pq(10, 64, 0, 8, 10, 7) == _capi.EINVAL and b"divide" in lib.lvs_last_error()  # M does not divide d
    assert pq(10, 64, 0, 65, 10, 7) == _capi.EINVAL and b"divide" in lib.lvs_last_error()  # M is reported ahead of nprobe
    assert pq(10, 64, 0, 8, 10, 0) == _capi.EINVAL and b"M=0" in lib.lvs_last_error()


# recorded from the library before the three searches shared their layout code; negative: LVS_EINVAL (-1) / LVS_EUNSUPPORTED (-4)
IVF_WORKSPACE_BYTES = {
    "flat": [
        ((1, 64, 8, 768, 10, 0), 24576),
        ((100, 4096, 32, 768, 16, 0), 7994368),
        ((16384, 4096, 32, 768, 17, 1), 83019776),
        ((100000, 4096, 2048, 1088, 56, 0), 486691584),
        ((100000, 64, 32, 2240, 16, 0), 77744384),
        ((0, 1, 1, 64, 1, 0), 8448),
        ((100, 64, 65, 768, 10, 0), -1),
        ((100, 64, 8, 768, 57, 0), -1),
        ((100, 64, 8, 768, 10, 2), -1),
        ((100, 64, 8, 1152, 16, 1), 2121728),
        ((100, 64, 8, 1152, 17, 1), 2128128),
        ((100, 64, 8, 2368, 56, 0), -4),
        ((100, 64, 8, 2432, 16, 0), 2121728),
        ((100, 64, 8, 3072, 10, 0), -4),
    ],
    "sq8": [
        ((1, 64, 8, 768, 10, 0), 24576),
        ((100, 4096, 32, 768, 16, 0), 7994368),
        ((16384, 4096, 32, 768, 17, 1), 83019776),
        ((100000, 4096, 2048, 1088, 56, 0), 486691584),
        ((100000, 64, 32, 2240, 16, 0), 77744384),
        ((0, 1, 1, 64, 1, 0), 8448),
        ((100, 64, 65, 768, 10, 0), -1),
        ((100, 64, 8, 768, 57, 0), -1),
        ((100, 64, 8, 768, 10, 2), -1),
        ((100, 64, 8, 1152, 16, 1), 2121728),
        ((100, 64, 8, 1152, 17, 1), 2128128),
        ((100, 64, 8, 2368, 56, 0), 2377728),
        ((100, 64, 8, 2432, 16, 0), 2121728),
        ((100, 64, 8, 3072, 10, 0), -4),
    ],
    "pq": [
        ((1, 64, 8, 768, 64, 10, 0), 87552),
        ((100, 4096, 32, 768, 64, 16, 0), 14468096),
        ((16384, 4096, 32, 768, 96, 17, 1), 422592768),
        ((100000, 4096, 2048, 1088, 64, 56, 0), 513771776),
        ((100000, 64, 32, 1272, 159, 16, 0), 342892800),
        ((100, 64, 8, 1600, 160, 10, 0), -4),
        ((100, 64, 8, 768, 7, 10, 0), -1),
        ((100, 64, 8, 768, 0, 10, 0), -1),
        ((100, 64, 65, 768, 64, 10, 0), -1),
        ((0, 1, 1, 64, 1, 1, 0), 7936),
    ],
}


def test_ivf_workspace_sizes_without_a_gpu():
    # scratch sizes are part of the contract with callers that size their own buffers: (nq, nlist, nprobe, d, k, pack) -> bytes
    lib = _capi.load()
    flat, sq8, pq = (lib.lvs_ivf_search_workspace_bytes, lib.lvs_ivf_sq8_search_workspace_bytes,
                     lib.lvs_ivf_pq_search_workspace_bytes)
    for args, want in IVF_WORKSPACE_BYTES["flat"]:
        assert flat(*args) == want, args
    for args, want in IVF_WORKSPACE_BYTES["sq8"]:
        assert sq8(*args) == want, args
    for args, want in IVF_WORKSPACE_BYTES["pq"]:  # (nq, nlist, nprobe, d, M, k, pack)
        assert pq(*args) == want, args


def test_missing_library_fails_loudly(monkeypatch):
    import pytest

    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/liblotus_hip.so")
    with pytest.raises(_capi.LotusHipError):
        _capi.load()


def test_no_product_module_imports_the_oracle():
    root = os.path.dirname(os.path.abspath(_capi.__file__))
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f


def test_workspace_sizes_cover_every_routing_decision():
    """`lvs_flat_search_workspace_bytes` is pure host arithmetic: it must accept every shape the search accepts and be
    large enough for the path the search will take (k <= 15, 16..56, and the two-phase path beyond 56, whose lists and
    buckets dominate)."""
    lib = _capi.load()
    f = lambda nq, nb, d, k, bm=0, qm=0: lib.lvs_flat_search_workspace_bytes(nq, nb, d, k, bm, qm)  # noqa: E731
    base = f(100_000, 1_000_000, 768, 10)
    assert base > 100_000 * 4 + 11 * 100_000 * 10 * 8 // 2  # thresholds + per-slab candidate lists
    assert f(100_000, 1_000_000, 768, 24) > 0 and f(100_000, 1_000_000, 768, 56) > 0
    big = f(100_000, 1_000_000, 768, 100)
    # two-phase: >= 2k/15 slabs x 15 keys per query of lists + a 512-slot bucket per query, 8 B each
    assert big >= 100_000 * (14 * 15 + 512) * 8
    assert f(100_000, 1_000_000, 768, 2048) >= 100_000 * 4096 * 8
    assert f(1, 1_000_000, 768, 1000) < 1 << 30          # one query: small
    assert f(0, 1000, 64, 5) >= 0 and f(10, 0, 64, 5) >= 0  # empty sides are legal
    assert f(10, 1000, 0, 5) < 0 and f(10, 1000, 64, -1) < 0  # bad shapes are refused
    # beyond 24 GB the two-phase path is not planned: the call falls back to selection passes and their small workspace
    assert f(4_000_000, 1_000_000, 768, 2048) < 24 << 30
    # pack modes are part of the contract (ABI 2); sizes must never shrink below the fp16 case
    for k in (1, 10, 56, 100):
        assert f(5000, 300_000, 384, k, 1, 1) >= f(5000, 300_000, 384, k, 0, 0) > 0


KNOBS = ["LVS_DEBUG_HOT", "LVS_STREAM_DEBUG", "LVS_GQ", "LVS_NSLAB", "LVS_TOP1", "LVS_TWO_PHASE", "LVS_SMALLQ",
         "LVS_LEAD", "LVS_L2_MIN_TILES", "LVS_STREAM", "LVS_STREAM_WGS", "LVS_COUNT", "LVS_TWO_PHASE_SLOTS"]


def test_shipped_library_has_no_tuning_or_debug_knob():
    """one stray LVS_* environment variable must not be able to change (or corrupt) results.
    The shipped .so contains none of the knob names and reports build flags 0; the names only exist in the separate
    `make tuning` build."""
    blob = open(_capi.LIB_PATH, "rb").read()
    for name in KNOBS:
        assert (name.encode() + b"\0") not in blob, name
    assert _capi.load().lvs_build_flags() == 0
    # the only getenv left is rocPRIM's own (ROCPRIM_USE_ATOMIC_BLOCK_ID, header-inlined into the two sort users)
    out = subprocess.run(["nm", "-D", "--undefined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "atoll" not in out and "atoi" not in out


def test_tuning_build_is_refused_by_default(tmp_path):
    import pytest

    csrc = os.path.join(os.path.dirname(_capi.LIB_PATH), "csrc")
    r = subprocess.run(["make", "-C", csrc, "tuning", "-j4"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    tuning = os.path.join(os.path.dirname(_capi.LIB_PATH), "liblotus_hip_tuning.so")
    blob = open(tuning, "rb").read()
    assert b"LVS_DEBUG_HOT\0" in blob
    lib = ctypes.CDLL(tuning)
    lib.lvs_build_flags.restype = ctypes.c_int32
    assert lib.lvs_build_flags() & _capi.BUILD_TUNING
    saved, saved_path = _capi._lib, _capi.LIB_PATH
    try:
        _capi._lib, _capi.LIB_PATH = None, tuning
        with pytest.raises(_capi.LotusHipError, match="tuning build"):
            _capi.load()
        assert _capi.load(tuning).lvs_build_flags() & _capi.BUILD_TUNING  # explicit path: allowed (tools/)
    finally:
        _capi._lib, _capi.LIB_PATH = saved, saved_path


def test_merge_keys_accepts_long_lists_from_many_parts():
    """8 shards x k > 512 used to be rejected.  Argument validation only (no GPU here)."""
    lib = _capi.load()
    assert lib.lvs_merge_keys(None, 8, 0, 1000, None, None) == 0          # nq == 0: nothing to do, accepted
    assert lib.lvs_merge_keys(None, 8, 5, 4000, None, None) == _capi.EINVAL  # NULL buffers / k beyond LVS_MAX_K


def test_block_to_item_deal_covers_every_item_once(tmp_path):
    """The tile kernel's blockIdx -> (query tile, slab) deal (lvs_tile.h): every item exactly once for 1 716 combinations of
    query tiles x slabs x XCD group shape, and the planner's per-XCD round count equals a direct count (host code only)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "mapping_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-w",
                    os.path.join(root, "tests", "native", "mapping_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("ok "), out


def test_planner_invariants_hold_over_the_grid():
    """The flat search's host planner (lotus_amd/csrc/lvs_plan.h) compiled alone by the host compiler (tests/native/plan_check.cpp):
    over 147 840 shapes the slabs cut the tiles, the offsets are aligned and ascending, lvs_flat_search_workspace_bytes is the
    largest layout, and the region the routed path writes holds what its launch geometry says it writes, chunk by chunk."""
    import plan_native

    out = plan_native.run()
    assert out.returncode == 0 and out.stdout.startswith("ok 147840 shapes"), out.stdout[-1000:]
    # ... and the second grid: the searches through the lists, the bucket sort and the threshold join's launches
    assert out.stdout.splitlines()[1].startswith("ok 22732 ivf and bucket shapes (3878 with a halved chunk), 3456 joins"), out.stdout[-1000:]
    # the library answers with the same function
    lib = _capi.load()
    have = {ln.split("|")[0]: int(ln.rsplit(" ", 1)[1]) for ln in plan_native.run("--dump").stdout.splitlines() if "| bytes " in ln}
    for mode, fn in enumerate((lib.lvs_ivf_search_workspace_bytes, lib.lvs_ivf_sq8_search_workspace_bytes)):
        for (nq, nlist, nprobe, d, k, pack) in [(40000, 8200, 2048, 64, 56, 0), (16385, 4097, 257, 64, 17, 1), (255, 1, 16, 64, 1, 0)]:
            assert fn(nq, nlist, nprobe, d, k, pack) == have[f"ivf mode={mode} nq={nq} nlist={nlist} nprobe={nprobe} d={d} M=1 k={k} pack={pack} "]
    assert lib.lvs_ivf_pq_search_workspace_bytes(10001, 40, 4, 636, 159, 56, 1) == have["ivf mode=2 nq=10001 nlist=40 nprobe=4 d=636 M=159 k=56 pack=1 "]
    assert lib.lvs_ivf_range_workspace_bytes(32769, 30000, 2048, 1216, 1) == have["ivf mode=3 nq=32769 nlist=30000 nprobe=2048 d=1216 M=1 k=0 pack=1 "]
    assert lib.lvs_kmeans_accumulate_workspace_bytes(1000000, 24576) == have["bucket n=1000000 k=24576 "]
    for (nq, nb, d, k, bp, qp) in [(100_000, 1_000_000, 768, 10, 0, 0), (100_000, 1_000_000, 768, 2048, 0, 0), (256, 1_000_000, 1536, 10, 1, 1),
                                   (1, 10_000_000, 8, 2048, 0, 0), (0, 0, 8, 1, 0, 0), (65236, 10_000_000, 768, 10, 0, 1)]:
        assert lib.lvs_flat_search_workspace_bytes(nq, nb, d, k, bp, qp) == have[f"nq={nq} nb={nb} d={d} k={k} pack={bp}/{qp} hi=0 "]


def test_permutation_prefix_equals_the_full_permutation():
    """lvs_rand_perm_prefix_host (O(m)) against lvs_rand_perm_host and the oracle's restatement of faiss rand_perm."""
    import numpy as np

    import oracle

    lib = _capi.load()
    for n, m, seed in [(1, 1, 3), (2, 1, 0), (10, 10, 1234), (1000, 7, 1), (1000, 999, 2), (100003, 256, 1234),
                       (100003, 4096, 1235), (300000, 262144, 99), (5, 0, 1)]:
        full = np.empty(n, np.int64)
        assert lib.lvs_rand_perm_host(n, seed, full.ctypes.data) == 0
        pre = np.full(max(m, 1), -1, np.int64)
        assert lib.lvs_rand_perm_prefix_host(n, seed, m, pre.ctypes.data) == 0
        assert np.array_equal(pre[:m], full[:m]), (n, m, seed)
        if n <= 100003:
            assert np.array_equal(full, oracle.rand_perm(n, seed))
    assert lib.lvs_rand_perm_prefix_host(10, 1, 11, None) == _capi.EINVAL
