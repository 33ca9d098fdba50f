"""Building, loading and running tests/csrc/g2_split_host_shim.hip: the pair-split G2 mixed addition (csrc/g2split.cuh) with the lane
pair emulated on the host, compiled with ZK_FQU_CHECK.  The records and their exact checkers are tests/madd_lazy_cases.py's G2 ones
(the shim takes the same record layouts), so the split addition is held to the same expected points, formulas and stored bounds as
the one-lane addition.  check_all(lc) is what tests/test_g2_split_host.py runs in a child process: an operand assertion aborts
the process, and the parent reports the message instead of dying with it."""
import ctypes as C
import os
import subprocess

import numpy as np

import madd_lazy_cases as MC
import prim_cases as PC

SRC = os.path.join(PC.ROOT, "tests", "csrc", "g2_split_host_shim.hip")
LIB = os.path.join(PC.OUT_DIR, "libg2_split_host_shim.so")
HEADERS = ["ff.cuh", "ffu.cuh", "ec.cuh", "g2split.cuh"]
OP = {"madd": 0, "chain": 2, "vs": 4}            # + 1: the form without the spare carry passes


def build_shim():
    """Compiles the shim when it is stale (mtime rule of the other shims); returns the library's path."""
    deps = [SRC] + [os.path.join(PC.INC, h) for h in HEADERS]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(PC.OUT_DIR, exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-fvisibility=hidden", "-DZK_FQU_CHECK",
                               "-I", PC.INC, "-o", LIB, SRC])
    return LIB


def load_shim():
    lib = C.CDLL(build_shim())
    lib.g2_split_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.g2_split_run.restype = C.c_int
    lib.g2_split_words.argtypes = [C.c_int, C.c_int]
    assert lib.g2_split_check_active() == 1
    assert lib.g2_split_run(99, 0, None, None) == -1 and lib.g2_split_words(6, 0) == -1
    return lib


def run(lib, op, inp):
    """inp: (n, in_words) uint32 -> (n, out_words) uint32"""
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    assert inp.ndim == 2 and inp.shape[1] == lib.g2_split_words(op, 0), (op, inp.shape)
    out = np.zeros((inp.shape[0], lib.g2_split_words(op, 1)), dtype=np.uint32)
    rc = lib.g2_split_run(op, inp.shape[0], inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, "g2_split_run(op %d) returned %d" % (op, rc)
    return out


def exceptional_cases_present(inp, expected):
    """the four exceptional cases of the addition occur in the chain records: a chain that starts AT its first base and adds it
    (the doubling), one that cancels to infinity, one that restarts from infinity (the start of a run), both signs; the base at
    infinity is among the single additions (MC.point_cases)"""
    seen = set()
    for i in range(inp.shape[0]):
        choices = MC.chain_choices(int(inp[i, -1]))
        seen.update("neg" if neg else "pos" for _, neg in choices)
        if i % 5 == 0 and choices[0] == (0, False):
            seen.add("doubling")
        for s, e in enumerate(expected[i]):
            if e is None:
                seen.add("cancel")
                if s + 1 < MC.CHAIN_STEPS and expected[i][s + 1] is not None:
                    seen.add("restart")
    return seen


def check_all(lc):
    """every check of the split addition in one form (lc = 1: without the spare carry passes); returns a summary line"""
    lib = load_shim()
    # single additions on curve points: both signs, P + P, P - P, either or both operands at infinity, coordinates at the stored maxima
    inp, expected = MC.point_cases("g2")
    assert inp[:, -1].any() and not inp[:, -1].all()
    base_inf = int((~inp[:, 4 * 28:6 * 28].any(axis=1)).sum())
    assert base_inf > 0
    MC.check_points("g2", inp, expected, run(lib, OP["madd"] + lc, inp))
    # the formulas at worst-case limbs: every output coordinate exact, normalised and inside the stored bounds
    winp, meta = MC.worst_limb_cases("g2")
    MC.check_worst("g2", meta, run(lib, OP["madd"] + lc, winp))
    # chains from accumulators at the stored maxima, the point after every step
    cinp, cexp = MC.chain_cases("g2")
    seen = exceptional_cases_present(cinp, cexp)
    assert seen == {"neg", "pos", "doubling", "cancel", "restart"}, seen
    stats = MC.check_chain("g2", cinp, cexp, run(lib, OP["chain"] + lc, cinp))
    assert stats["steps"] == MC.CHAIN_LANES * MC.CHAIN_STEPS
    # ... and coordinate by coordinate against the one-lane addition on the same chains, as residues
    diff = run(lib, OP["vs"] + lc, cinp)
    assert not diff.any(), "split and one-lane additions differ as residues: lanes %s" % sorted(set(np.nonzero(diff)[0].tolist()))
    return "ok points=%d base_inf=%d worst=%d chain_steps=%d inf_steps=%d" % (len(inp), base_inf, len(meta), stats["steps"], stats["inf"])
