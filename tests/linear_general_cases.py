"""Shared by tests/test_linear_general_host.py and tests/test_linear_general_gpu.py: the model of the linear route's second solver
(option "linear_solver" = 1) — Gaussian elimination mod r in Python big integers, with the status rule stated on the columns of a
alone —, the case set, and the host-compiled shim of csrc/linear_elim_dev.cuh.  The circuit, its layout and the forward solver's
model are tests/linear_cases.py's.  Not a test module."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np

import linear_cases as LC
from linear_cases import CSRC, R_MOD, ROOT, U64_MAX

SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "linear_general_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "liblinear_general_host_shim.so")


# ------------------------------------------------------------------------------------------------ the model
def first_dependent_column(a):
    """The smallest c for which columns 0..c of a are linearly dependent mod r, or None when all n are independent.  Column by
    column: column c is reduced by the basis of the columns before it (each basis vector has a leading 1 in a row of its own);
    what is left is zero exactly when column c lies in their span."""
    n = len(a)
    basis = []                                              # (row of the leading 1, vector)
    for c in range(n):
        v = [int(a[i][c]) % R_MOD for i in range(n)]
        for lead, w in basis:
            if v[lead]:
                f = v[lead]
                v = [(x - f * y) % R_MOD for x, y in zip(v, w)]
        lead = next((i for i in range(n) if v[i]), None)
        if lead is None:
            return c
        inv = pow(v[lead], -1, R_MOD)
        basis.append((lead, [x * inv % R_MOD for x in v]))
    return None


def status(a):
    """What the kernel and the host solver report: 0, or 1 + first_dependent_column."""
    c = first_dependent_column(a)
    return 0 if c is None else 1 + c


def solve(a, b):
    """x with a x = b mod r by Gauss-Jordan elimination (the LAST row with a non-zero entry as the pivot — not the kernel's choice: the
    solution does not depend on it) -> list of ints, or None for a singular a."""
    n = len(b)
    m = [[int(a[i][j]) % R_MOD for j in range(n)] + [int(b[i]) % R_MOD] for i in range(n)]
    for c in range(n):
        p = next((i for i in range(n - 1, c - 1, -1) if m[i][c]), None)
        if p is None:
            return None
        m[c], m[p] = m[p], m[c]
        inv = pow(m[c][c], -1, R_MOD)
        m[c] = [v * inv % R_MOD for v in m[c]]
        for i in range(n):
            if i != c and m[i][c]:
                f = m[i][c]
                m[i] = [(v - f * w) % R_MOD for v, w in zip(m[i], m[c])]
    return [m[i][n] for i in range(n)]


def assignment(a, b):
    """The full assignment z (canonical ints) with the eliminated x: linear_cases.assignment's layout."""
    n = len(b)
    x = solve(a, b)
    ni = 1 + n * (n + 1)
    z = [0] * (3 * n * n + 2 * n + 1)
    z[0] = 1
    for i in range(n):
        for j in range(n):
            z[1 + i * (n + 1) + j] = int(a[i][j])
            z[ni + i * (2 * n + 1) + 1 + 2 * j] = x[j]
            z[ni + i * (2 * n + 1) + 2 + 2 * j] = int(a[i][j]) * x[j] % R_MOD
        z[1 + i * (n + 1) + n] = int(b[i])
    return z


# ------------------------------------------------------------------------------------------------ the cases
def _arr(a, b):
    return np.array(a, dtype=np.uint64).reshape(len(b), len(b)), np.array(b, dtype=np.uint64)


def dense(n, seed, zero_b=False):
    """Random 64-bit entries everywhere (from n = 5 on the eliminated entries wrap mod r: they grow by 64 bits and more per column).
    Non-singular only once the model has said so: solvable() asserts it for every case it hands out."""
    rng = random.Random(7000 * n + seed)
    a = [[rng.getrandbits(64) for _ in range(n)] for _ in range(n)]
    b = [0 if zero_b else rng.getrandbits(64) for _ in range(n)]
    return _arr(a, b)


def _rhs(n, seed):
    rng = random.Random(31 * n + seed)
    return [rng.getrandbits(64) for _ in range(n)]


def zero_corner(n, seed=1):
    """a[0][0] = 0 in a dense system: column 0 needs a row exchange (n >= 2)."""
    a, b = dense(n, seed)
    a[0, 0] = 0
    return a, b


def last_row_leads(n, seed=2):
    """Column 0 is zero except in the last row (n >= 2)."""
    a, b = dense(n, seed)
    a[: n - 1, 0] = 0
    return a, b


def late_zero_pivot():
    """[[1,2,3],[2,4,7],[1,1,1]]: the entry (1, 1) becomes zero only after column 0 has been eliminated."""
    return _arr([[1, 2, 3], [2, 4, 7], [1, 1, 1]], [5, 6, 7])


def permutation(n, seed=3):
    rng = random.Random(11 * n + seed)
    p = list(range(n))
    rng.shuffle(p)
    if n > 1 and p == sorted(p):
        p = p[1:] + p[:1]
    return _arr([[1 if p[i] == j else 0 for j in range(n)] for i in range(n)], _rhs(n, seed))


def identity(n, seed=4):
    return _arr([[1 if i == j else 0 for j in range(n)] for i in range(n)], _rhs(n, seed))


def all_max(n):
    """Every entry of a and b is 2^64 - 1 except a's diagonal, which is 2^64 - 2 (a = max (J - I) + (max - 1) I is non-singular)."""
    a = [[U64_MAX - 1 if i == j else U64_MAX for j in range(n)] for i in range(n)]
    return _arr(a, [U64_MAX] * n)


@functools.lru_cache(maxsize=None)
def solvable(n):
    """The non-singular cases of size n -> [(name, a, b, x)], x the model's solution as [n, 4] Montgomery limbs — which exists, so the
    model has confirmed that a is non-singular.  Up to n = 8 every family; above it (where one big-integer elimination takes a good
    part of a second) the dense, row-exchange, permutation and lower-triangular ones.  Made once per size and shared, read-only."""
    out = []
    for name, a, b in _solvable(n):
        x = solve(a, b)
        assert x is not None, (n, name)
        out.append((name, *_frozen(a, b, mont_limbs(x))))
    return out


def _frozen(*arrays):
    for arr in arrays:
        arr.setflags(write=False)
    return arrays


def _solvable(n):
    out = [("dense", *dense(n, 0)), ("lower", *LC.system(n, "lower", 5))]
    if n >= 2:
        out += [("zero_corner", *zero_corner(n)), ("permutation", *permutation(n))]
    if n == 3:
        out.append(("late_zero_pivot", *late_zero_pivot()))
    if n <= 8:
        out += [("zero_b", *dense(n, 1, zero_b=True)), ("identity", *identity(n)), ("all_max", *all_max(n))]
        if n >= 2:
            out.append(("last_row_leads", *last_row_leads(n)))
    return out


@functools.lru_cache(maxsize=None)
def singular(n):
    """Singular systems of size n -> [(name, a, b, c)] with c from the column rule: a zero column at 0 and at n - 1, and up to n = 8
    also two equal rows and a row that is the sum of two others (above it the row sum alone).  Shared, read-only."""
    out = []

    def add(name, a):
        c = first_dependent_column(a)
        assert c is not None, name
        out.append((name, *_frozen(np.array(a, dtype=np.uint64), np.array(_rhs(n, 9), dtype=np.uint64)), c))
    base = dense(n, 6)[0]
    z0 = base.copy()
    z0[:, 0] = 0
    add("zero_column_0", z0)
    zl = base.copy()
    zl[:, n - 1] = 0
    add("zero_column_last", zl)
    if 2 <= n <= 8:
        eq = base.copy()
        eq[n - 1] = eq[0]
        add("equal_rows", eq)
    if n >= 3:
        # small entries, so that the sum of two rows is still a row of u64 values
        rng = random.Random(n)
        sm = [[rng.getrandbits(62) for _ in range(n)] for _ in range(n)]
        sm[1] = [sm[0][j] + sm[n - 1][j] for j in range(n)]
        add("row_sum", sm)
    assert out[0][3] == 0 and out[1][3] == n - 1
    return out


SIZES = (1, 2, 3, 8, 63, 64, 65)


def mont_limbs(values):
    return LC.mont_limbs(values)


# ------------------------------------------------------------------------------------------------ the shim
def load_shim():
    """tests/csrc/linear_general_host_shim.hip (the elimination kernel's phase functions compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("linear_elim_dev.cuh", "linear_dev.cuh", "ff.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = C.CDLL(SHIM_OUT)
    lib.lin_elim_lanes.restype = C.c_uint32
    lib.lin_elim_lanes.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    return lib
