"""Shared by tests/test_linear_host.py and tests/test_linear_batch_gpu.py: the model of the linear-equations route in Python big
integers mod r (solver, assignment, matrices, failing rows — by the index formulas of include/zkg16.h), the input families, and the
host-compiled shim of csrc/linear_dev.cuh.  Not a test module."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "linear_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "liblinear_host_shim.so")
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
U64_MAX = (1 << 64) - 1
SENTINEL = 0xA5A5A5A5A5A5A5A5
N_MAX = 1024
OK, BAD_ARG, BAD_HANDLE, UNSUPPORTED, UNSATISFIED = 0, 1, 6, 7, 8          # include/zkg16.h: zkg16_status


# ------------------------------------------------------------------------------------------------ the model
def dims(n):
    return dict(num_instance=1 + n * (n + 1), num_witness=n * (2 * n + 1), num_constraints=n * (n + 1),
                nnz=(2 * n * n + 2 * n, n * n + n, n * n))


def solve(a, b):
    """linear_equations.rs:20-41: x = 0, then x[i] = (b[i] - sum_j a[i][j] x[j]) / a[i][i] over the whole row, in request order."""
    n = len(b)
    x = [0] * n
    for i in range(n):
        s = sum(int(a[i][j]) * x[j] for j in range(n)) % R_MOD
        x[i] = (int(b[i]) - s) * pow(int(a[i][i]), -1, R_MOD) % R_MOD
    return x


def assignment(a, b):
    """The full assignment z (canonical ints), the instance first."""
    n = len(b)
    x = solve(a, b)
    ni = 1 + n * (n + 1)
    z = [None] * (3 * n * n + 2 * n + 1)
    z[0] = 1
    for i in range(n):
        for j in range(n):
            z[1 + i * (n + 1) + j] = int(a[i][j])
            z[ni + i * (2 * n + 1) + 1 + 2 * j] = x[j]
            z[ni + i * (2 * n + 1) + 2 + 2 * j] = int(a[i][j]) * x[j] % R_MOD
        z[1 + i * (n + 1) + n] = int(b[i])
        z[ni + i * (2 * n + 1)] = 0
    assert None not in z
    return z


def matrices(n):
    """(A, B, C) as lists of rows of (coefficient, column), columns in the exported order."""
    ni = 1 + n * (n + 1)
    A, B, Cm = [], [], []
    for i in range(n):
        w0 = ni + i * (2 * n + 1)
        for j in range(n):
            A.append([(1, 1 + i * (n + 1) + j)])
            B.append([(1, w0 + 1 + 2 * j)])
            Cm.append([(1, w0 + 2 + 2 * j)])
        A.append([(R_MOD - 1, 1 + i * (n + 1) + n), (1, w0)] + [(1, w0 + 2 + 2 * j) for j in range(n)])
        B.append([(1, 0)])
        Cm.append([])
    return A, B, Cm


def failing_rows(a, b):
    """The equality rows i (n + 1) + n of the i with (U x)_i != 0, U the strict upper triangle of a."""
    n = len(b)
    x = solve(a, b)
    return [i * (n + 1) + n for i in range(n) if sum(int(a[i][j]) * x[j] for j in range(i + 1, n)) % R_MOD]


def rows_unsatisfied(a, b):
    """The same list from the matrices and the assignment alone: every row of (A z) (B z) = C z evaluated."""
    n = len(b)
    z = assignment(a, b)
    ev = lambda row: sum(c * z[col] for c, col in row) % R_MOD
    A, B, Cm = matrices(n)
    return [r for r in range(n * (n + 1)) if ev(A[r]) * ev(B[r]) % R_MOD != ev(Cm[r])]


def mont(v):
    m = (int(v) << 256) % R_MOD
    return [(m >> (64 * j)) & U64_MAX for j in range(4)]


def mont_limbs(values):
    """Python ints -> [len, 4] u64 Montgomery limbs"""
    return np.array([mont(v) for v in values], dtype=np.uint64).reshape(-1, 4)


def csr(rows):
    """rows of (coefficient, column) -> (row_ptr u64, col u32, coeff [nnz, 4] Montgomery)"""
    rp, col, cf = [0], [], []
    for row in rows:
        for c, j in row:
            col.append(j)
            cf.append(mont(c))
        rp.append(len(col))
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), np.array(cf, dtype=np.uint64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ the inputs
def _entry(rng):
    return (0, 1, U64_MAX, rng.getrandbits(64))[rng.randrange(4)]


def system(n, kind, seed):
    """One request: entries from {0, 1, 2^64 - 1, random 64-bit}, the diagonal never zero.
    "lower": nothing above the diagonal — satisfied.  "dense": every entry above the diagonal non-zero (n >= 2 has some).
    "zero_b": dense with b all zero — x = 0, satisfied whatever a is."""
    rng = random.Random(1000 * n + seed)
    a = [[_entry(rng) for _ in range(n)] for _ in range(n)]
    b = [0 if kind == "zero_b" else _entry(rng) for _ in range(n)]
    for i in range(n):
        a[i][i] = a[i][i] or 1 + rng.getrandbits(63)
        for j in range(i + 1, n):
            a[i][j] = 0 if kind == "lower" else a[i][j] or 1 + rng.getrandbits(63)
    return np.array(a, dtype=np.uint64).reshape(n, n), np.array(b, dtype=np.uint64)


def dense_unsatisfied(n, seed=0):
    """A dense request (n >= 2) whose failing-row list is non-empty: the first seed at or after `seed` for which the model says so."""
    assert n >= 2
    for s in range(seed, seed + 64):
        a, b = system(n, "dense", s)
        if failing_rows(a, b):
            return a, b
    raise AssertionError("no unsatisfied dense system of size %d in 64 seeds" % n)


KINDS = ("lower", "dense", "zero_b", "lower", "dense")


def requests(n, k, seed=0):
    """k requests of size n, kinds cycling through KINDS -> (a [k, n, n], b [k, n], kinds)."""
    sys_ = [system(n, KINDS[i % len(KINDS)], seed + i) for i in range(k)]
    return np.stack([s[0] for s in sys_]), np.stack([s[1] for s in sys_]), [KINDS[i % len(KINDS)] for i in range(k)]


def lower_requests(n, k, seed=0):
    sys_ = [system(n, "lower", seed + i) for i in range(k)]
    return np.stack([s[0] for s in sys_]), np.stack([s[1] for s in sys_])


# ------------------------------------------------------------------------------------------------ the shim
def load_shim():
    """tests/csrc/linear_host_shim.hip (the kernels' lane functions compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("linear_dev.cuh", "ff.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = C.CDLL(SHIM_OUT)
    lib.lin_solve_lanes.restype = C.c_int
    lib.lin_solve_lanes.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lin_fill.restype = None
    lib.lin_fill.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib
