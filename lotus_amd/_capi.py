"""ctypes binding of ``liblotus_hip.so`` (C ABI in ``include/lotus_hip.h``).

The binding is deliberately thin: every function takes raw device addresses (ints) and sizes.  Loading fails
loudly when the library has not been built; there is no fallback implementation."""
from __future__ import annotations

import ctypes
import operator
import os
import re
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblotus_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lotus_hip.h")

OK, EINVAL, ENOMEM, EDEVICE, EUNSUPPORTED = 0, -1, -2, -3, -4
DTYPE_F32, DTYPE_F16 = 0, 1
METRIC_IP, METRIC_L2 = 0, 1
PACK_F16, PACK_SPLIT = 0, 1
MAX_K = 2048
NEAREST3_MAX_ROWS = 16384
IVF_MAX_K = 56  # largest k of the one-pass list scan (lvs_ivf_search_keys)
ABI_VERSION = 7
BUILD_TUNING, BUILD_COUNT_EVENTS = 1, 2
PACK_FLAG_NONFINITE, PACK_FLAG_RANGE = 1, 2

_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = ("void", "char", "float", "double", "int32_t", "int64_t", "uint8_t", "uint32_t", "uint64_t")


class Prototype(NamedTuple):
    """One function (or callback typedef) of the header: what ctypes needs, and the parameter names in order."""

    restype: type
    argtypes: tuple
    names: tuple
    types: tuple  # every parameter's type as the header spells it ("const float*", "int64_t", "lvs_all_gather_fn")


def parse_header(text: str):
    """-> (prototypes, callbacks, defines) of a header written like include/lotus_hip.h: ``ret lvs_name(type name, ...);`` and
    ``typedef int32_t (*lvs_name_fn)(...);`` between comments and preprocessor lines.  Not a C parser: a statement or a type
    outside that vocabulary raises ``ValueError`` naming the prototype."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    prototypes, callbacks = {}, {}

    def param(decl: str, where: str):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl.strip())
        if m is None:
            raise ValueError(f"{where}: cannot read the parameter {decl.strip()!r} (a type and a name are needed)")
        const, base, star, name = m.groups()
        if star and base in _POINTEES:
            return ctypes.c_void_p, name, f"{'const ' if const else ''}{base}*"
        if not star and not const and base in _SCALARS:
            return _SCALARS[base], name, base
        if not star and not const and base in callbacks:
            return ctypes.c_void_p, name, base  # callers cast their CFUNCTYPE object
        raise ValueError(f"{where}: unknown type of the parameter {decl.strip()!r}")

    for stmt in (s.strip() for s in text.split(";")):
        if not stmt:
            continue
        m = re.fullmatch(r"(typedef\s+)?([\w\s\*]+?)\s*(?:\(\s*\*\s*(lvs_\w+)\s*\)|\b(lvs_\w+))\s*\(([^()]*)\)", stmt)
        if m is None or bool(m.group(1)) != bool(m.group(3)):
            raise ValueError(f"cannot read the declaration {' '.join(stmt.split())[:80]!r}")
        name = m.group(3) or m.group(4)
        ret = " ".join(m.group(2).replace("*", " * ").split())
        if ret in ("int32_t", "int64_t"):
            restype = _SCALARS[ret]
        elif ret == "const char *" and not m.group(1):
            restype = ctypes.c_char_p
        else:
            raise ValueError(f"{name}: unknown return type {ret!r}")
        decls = [] if m.group(5).strip() in ("", "void") else m.group(5).split(",")
        params = [param(d, name) for d in decls]
        proto = Prototype(restype, tuple(p[0] for p in params), tuple(p[1] for p in params), tuple(p[2] for p in params))
        if len(set(proto.names)) != len(proto.names):
            raise ValueError(f"{name}: a parameter name is used twice")
        if m.group(1):
            callbacks[name] = ctypes.CFUNCTYPE(proto.restype, *proto.argtypes)
        else:
            prototypes[name] = proto
    return prototypes, callbacks, defines


with open(HEADER_PATH) as _f:
    # PROTOTYPES: every function of the header; CALLBACKS: its callback typedefs as CFUNCTYPEs; DEFINES: its integer #defines
    PROTOTYPES, CALLBACKS, DEFINES = parse_header(_f.read())
SIGNATURES = {name: (p.restype, list(p.argtypes)) for name, p in PROTOTYPES.items()}  # name -> (restype, argtypes)


class LotusHipError(RuntimeError):
    """A C-ABI call returned a non-zero status."""


_lib = None


def declared_symbols() -> list[str]:
    """Function names declared in include/lotus_hip.h."""
    return sorted(PROTOTYPES)


_tails = {}  # (entry, positional arguments given) -> (how many parameters remain, kw -> their values in header order)


def _tail(name: str, npos: int):
    rest = PROTOTYPES[name].names[npos:]
    get = operator.itemgetter(*rest) if len(rest) > 1 else (lambda kw: (kw[rest[0]],)) if rest else (lambda kw: ())
    _tails[name, npos] = len(rest), get
    return _tails[name, npos]


def bind(name: str, args: tuple, kw: dict) -> tuple:
    """The arguments of entry ``name`` in the header's order: ``args`` as given, then ``kw`` by the header's parameter names.
    A name that is missing, unknown or already given by position raises ``TypeError``; nothing is dropped or defaulted."""
    if not kw:
        return args
    names = PROTOTYPES[name].names
    n, get = _tails.get((name, len(args))) or _tail(name, len(args))
    try:
        tail = get(kw)
    except KeyError as e:
        raise TypeError(f"{name}: missing parameter {e.args[0]!r}") from None
    if len(kw) != n:
        extra = next(k for k in kw if k not in names[len(args):])
        raise TypeError(f"{name}: parameter {extra!r} given twice" if extra in names else f"{name}: unknown parameter {extra!r}")
    return args + tail


def load(path: str | None = None):
    """dlopen the library and bind every declared symbol.  Raises if the library is missing.

    ``path`` selects another build explicitly (development: the ``make tuning`` library with the LVS_* knobs); the
    default library must be the shipped build - one that reports tuning knobs is refused."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    explicit = path is not None
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise LotusHipError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). lotus_amd has no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.  The device buffers and streams this library receives come
    # from torch, so both must share ONE HIP runtime: load torch's first, then our NEEDED libamdhip64.so.7 resolves to
    # the copy already in the process.  (Loaded the other way round, our kernels run on a second runtime that knows
    # nothing about torch's context: "no ROCm-capable device is detected".)
    try:
        import torch  # noqa: F401
    except Exception:  # symbol checks still work without torch
        pass
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.lvs_abi_version() != ABI_VERSION:
        raise LotusHipError(f"ABI version mismatch: library reports {lib.lvs_abi_version()}, binding is {ABI_VERSION}")
    if (lib.lvs_build_flags() & BUILD_TUNING) and not explicit:
        raise LotusHipError(f"{path} is a tuning build (environment knobs that can corrupt results); rebuild with `make`")
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != OK:
        msg = load().lvs_last_error().decode("utf-8", "replace")
        raise LotusHipError(f"{what or 'lotus_hip call'} failed with status {status}: {msg}")


def device_count() -> int:
    n = ctypes.c_int32(0)
    st = load().lvs_device_count(ctypes.byref(n))
    return int(n.value) if st == OK else 0
