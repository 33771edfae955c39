"""tests/native/plan_check.cpp - the host planners (lotus_amd/csrc/lvs_plan.h: flat search and threshold join; lvs_ivf_plan.h: the
searches through the lists) as a program - built once per session with the host C++ compiler (no HIP, no GPU)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def exe():
    tmp = tempfile.mkdtemp(prefix="plan_check_")
    atexit.register(shutil.rmtree, tmp, True)
    out = os.path.join(tmp, "plan_check")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "plan_check.cpp"), "-o", out], check=True)
    return out


def run(*args, stdin=None):
    return subprocess.run([exe(), *args], input=stdin, capture_output=True, text=True)


def ask(questions):
    """--query mode: one question per line ("rq_fits nq nb dpad k", "grouped nq blocks", "chunks nq maximum", ...) -> the
    answers, each a list of ints (None for "none")."""
    out = run("--query", stdin="".join(q + "\n" for q in questions))
    assert out.returncode == 0 and "?" not in out.stdout, out.stdout[-500:]
    answers = [None if ln.strip() == "none" else [int(v) for v in ln.split()] for ln in out.stdout.splitlines()]
    assert len(answers) == len(questions)
    return answers


def bound_coefs(cases):
    """lvs_bound.h's lvs_nearest_bound_coef on every (metric, pack, d, exp_sum) of ``cases`` -> per case the five float32 bit
    patterns as a tuple of ints (None: refused)."""
    return [None if a is None else tuple(a) for a in ask([f"bound_coef {m} {p} {d} {e}" for m, p, d, e in cases])]


IVF_MODE = {"Flat": 0, "SQ8": 1, "PQ": 2, "range": 3}  # LVS_IVF_* of lvs_ivf_plan.h


@functools.lru_cache(maxsize=None)
def ivf_limits():
    """(IVF_WS_BUDGET, IVF_CHUNK_MAX): the scratch budget of one search through the lists and its largest chunk of queries.  The
    tests' one source of the two constants."""
    return tuple(ask(["ivf_limits"])[0])


def ivf_chunk(mode, nq, nlist, nprobe, d, k, pack, M=1):
    """(chunk, last chunk or 0, declared bytes) of a search through the lists (mode: a key of IVF_MODE); None: refused."""
    ans = ask([f"ivf_chunk {IVF_MODE[mode]} {nq} {nlist} {nprobe} {d} {M} {k} {pack}"])[0]
    return None if ans is None else tuple(ans)
