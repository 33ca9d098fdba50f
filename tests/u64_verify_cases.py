"""Shared by tests/test_verify_u64_host.py and tests/test_verify_u64_gpu.py: the u64 form of batched verification (keys whose public
inputs are plain 64-bit values).  The host build of the device header, the multiplier-sum cases with their Python-integer answers,
keys with known logs for the prepared input X (the oracle's fixed_base of g_0 + sum v_c g_{1+c} is the expected point) and
simulated statements whose verdicts are known by construction (sim_proofs.SimKey).  Not a test module."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import sim_proofs as S
from helpers import *

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "u64_inputs_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "libu64_inputs_host_shim.so")
R = S.R
M64 = (1 << 64) - 1


def load_shim():
    """tests/csrc/u64_inputs_host_shim.hip (the device header compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("u64_inputs_dev.cuh", "prime_inputs_dev.cuh", "pairing_dev.cuh", "ffu.cuh", "ff.cuh", "ec.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = C.CDLL(SHIM_OUT)
    for name in ("u6_sum_slices", "u6_slice_len"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_size_t]
    lib.u6_group_lanes.restype = C.c_uint
    lib.u6_group_lanes.argtypes = [C.c_size_t]
    lib.u6_rho_sums.restype = None
    lib.u6_rho_sums.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.u6_prepared_input.restype = C.c_int
    lib.u6_prepared_input.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_void_p]
    return lib


# the slices of the sums kernels as u64_inputs_dev.cuh cuts them (the shim's u6_slice_len is asserted equal): at least 128 proofs
# a slice, at most 256 slices
def slice_len(k):
    s = min((k + 127) // 128, 256)
    return (k + s - 1) // s if s else 0


# ------------------------------------------------------------------------------------------------ multiplier sums
EDGE = [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
SUM_MS = (1, 2, 63, 64, 65, 257)
SUM_KS = (1, 63, 64, 65, 300)


def values_of(k, m, seed):
    """k x m values: the edge values mixed with random ones so that every column and every row meets both"""
    rng = random.Random(seed)
    pool = EDGE + [None] * 3
    return np.array([[(lambda v: rng.getrandbits(64) if v is None else v)(pool[(5 * p + 2 * c + seed) % len(pool)]) for c in range(m)] for p in range(k)],
                    dtype=np.uint64).reshape(k, m)


def live_masks(k):
    """(name, live bytes or None): all, the first dead, the last dead, a whole slice dead"""
    per = slice_len(k)
    first, last, sl = np.ones(k, np.uint8), np.ones(k, np.uint8), np.ones(k, np.uint8)
    first[0] = 0
    last[k - 1] = 0
    lo = per if k > per else 0                  # the second slice where there is one, else the only one
    sl[lo:lo + per] = 0
    return [("all", None), ("first_dead", first), ("last_dead", last), ("slice_dead", sl)]


def py_sums(values, rhos, live=None):
    """the m + 1 sums over the live proofs, Python integers"""
    k, m = values.shape
    keep = [i for i in range(k) if live is None or live[i]]
    cols = values.astype(object)
    return [sum(rhos[i] for i in keep)] + [sum(rhos[i] * cols[i, c] for i in keep) for c in range(m)]


def sum_cases(ms=SUM_MS, ks=SUM_KS):
    """(name, values [k, m], rho integers, live): sim_proofs.RHO_EDGES as multipliers under each live mask, and the all-maximal case"""
    for m in ms:
        for k in ks:
            vals = values_of(k, m, 7 * m + k)
            rhos = [S.RHO_EDGES[(3 * i + k + m) % len(S.RHO_EDGES)] for i in range(k)]
            for name, live in live_masks(k):
                yield "m%d_k%d_%s" % (m, k, name), vals, rhos, live
    for m, k in ((1, 1), (65, 300), (257, 65)):
        yield "m%d_k%d_all_maximal" % (m, k), np.full((k, m), M64, dtype=np.uint64), [2**128 - 1] * k, None


_WANT = {}


def sums_want(name, values, rhos, live):
    """py_sums, computed once per case and shared"""
    if name not in _WANT:
        _WANT[name] = py_sums(values, rhos, live)
    return _WANT[name]


def sums_ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def boundary_case():
    """K = 65,537 at m = 2: past one pass of 65,536 proofs and, with 256 slices of 257 proofs, a last slice that is short"""
    k, m = 65537, 2
    rng = random.Random(65537)
    vals = np.array([[rng.getrandbits(64), EDGE[i % len(EDGE)]] for i in range(k)], dtype=np.uint64)
    rhos = [rng.getrandbits(128) | 1 for _ in range(k)]
    live = np.ones(k, np.uint8)
    live[[0, 65535, 65536]] = 0
    return vals, rhos, live


# ------------------------------------------------------------------------------------------------ the prepared input X
X_MS = (1, 2, 3, 6, 12, 30, 56, 64, 65, 72, 129)          # L = 1, 2, 4, 8, 16, 32, 64, 64, and 64 with two and three columns a lane
X_FAMILIES = ("random", "small", "g0_inf", "x_inf")


class XCase:
    """a key's points with known logs and rows of values: gabc [1 + m, 12], values [rows, m], the expected X [rows, 12] and its
    infinity flags, from the oracle's fixed_base of g_0 + sum v_c g_{1+c}"""

    def __init__(self, oracle, family, m, rows, seed):
        rng = random.Random(seed)
        self.family, self.m = family, m
        if family == "small":
            # logs and values so small that accumulators meet the bases as equal, opposite and infinite points in any order
            g = [rng.choice((0, 1, -1, 2, -2, 3, -3)) % R for _ in range(m + 1)]
            vals = [[rng.randrange(4) for _ in range(m)] for _ in range(rows)]
        else:
            g = [rng.randrange(1, R) for _ in range(m + 1)]
            pool = EDGE + [None] * 4
            vals = [[(lambda v: rng.getrandbits(64) if v is None else v)(pool[(3 * p + 5 * c) % len(pool)]) for c in range(m)] for p in range(rows)]
        if rows > 1:
            vals[1] = [0] * m                                   # an all-zero row: X = gamma_abc[0]
        if family == "g0_inf":
            g[0] = 0
        if family == "x_inf":
            # g_0 = -sum v_c g_{1+c} of row 0: X is the point at infinity for that row and its copies
            vals[0] = [rng.getrandbits(64) | 1 for _ in range(m)]
            g[0] = -sum(v * gi for v, gi in zip(vals[0], g[1:])) % R
            for p in range(2, rows, 5):
                vals[p] = list(vals[0])
        self.g = g
        self.values = np.array(vals, dtype=np.uint64).reshape(rows, m)
        self.logs = [(g[0] + sum(v * gi for v, gi in zip(row, g[1:]))) % R for row in vals]
        gabc, ginf = oracle.fixed_base("g1", G1_GEN_LIMBS, fr_canon_vec(g))
        self.gabc = np.ascontiguousarray(gabc, dtype=np.uint64).reshape(m + 1, 12)
        assert [bool(f) for f in ginf] == [v == 0 for v in g] and not self.gabc[np.asarray(ginf).astype(bool)].any()
        want, winf = oracle.fixed_base("g1", G1_GEN_LIMBS, fr_canon_vec(self.logs))
        self.want = np.ascontiguousarray(want, dtype=np.uint64).reshape(rows, 12)
        self.want_inf = np.asarray(winf, dtype=np.uint8).reshape(rows)
        assert [bool(f) for f in self.want_inf] == [v == 0 for v in self.logs] and not self.want[self.want_inf.astype(bool)].any()
        if family == "x_inf":
            assert self.want_inf[0] and (rows < 3 or self.want_inf[2])
        if family == "g0_inf" and rows > 1:
            assert self.want_inf[1]                             # the zero row under gamma_abc[0] = O
        if rows > 1 and family in ("random", "x_inf"):
            assert np.array_equal(self.want[1], self.gabc[0])


_XCASES = {}


def x_case(oracle, family, m, rows):
    """XCase, made once per (family, m, rows) and shared"""
    key = (family, m, rows)
    if key not in _XCASES:
        _XCASES[key] = XCase(oracle, family, m, rows, 1000 * X_FAMILIES.index(family) + m)
    return _XCASES[key]


# ------------------------------------------------------------------------------------------------ simulated statements
def u64_inputs(key, k, seed):
    """k input vectors of plain 64-bit values for a key: edges and random ones mixed"""
    rng = random.Random(seed)
    pool = EDGE + [None] * 4
    return [[(lambda v: rng.getrandbits(64) if v is None else v)(pool[(7 * p + 3 * i + 11) % len(pool)]) for i in range(key.ni - 1)] for p in range(k)]


NEGATIVE_KINDS = ("off_by_one", "exchanged", "top_bit", "c_dropped", "other_rows_values")


def negative(key, stmts, i, kind):
    """the negative twin of statement i of the given kind, invalid by construction (sim_proofs asserts it on the integers)"""
    s = stmts[i]
    m = key.ni - 1
    if kind == "off_by_one":
        c = next(c for c in range(m) if s.z[c] < M64 and key.g[c + 1])
        return key.bumped(s, c, kind)
    if kind == "exchanged" and m >= 2:
        a, b = next((a, b) for a in range(m) for b in range(a + 1, m) if key.x(S.swap(s.z, a, b)) != key.x(s.z))
        return key.exchanged(s, a, b, kind)
    if kind == "top_bit":
        z = list(s.z)
        z[m - 1] ^= 1 << 63
        assert 0 <= z[m - 1] <= M64 and key.x(z) != key.x(s.z)
        return key.invalid(s.but(kind, z=z))
    if kind == "other_rows_values" and len(stmts) > 1:
        other = stmts[(i + 1) % len(stmts)]
        assert key.x(other.z) != key.x(s.z)
        return key.invalid(s.but(kind, z=other.z))
    return key.c_dropped(s, "c_dropped")


class U64Sim:
    """a key of num_instance = m + 1 points with known logs and k statements under it whose inputs are u64; `where`: the positions
    replaced by negative twins, the kinds cycled -> batch (verify_batch_cases.Batch), values [k, m] uint64, want [k] bool"""

    def __init__(self, oracle, m, k, where, seed):
        self.key = S.random_key(oracle, m + 1, seed)
        rng = random.Random(seed + 7)
        valid = [self.key.ordinary(z, rng) for z in u64_inputs(self.key, k, seed)]
        self.stmts = list(valid)
        self.kinds = {}
        for n, i in enumerate(where):
            self.kinds[i] = NEGATIVE_KINDS[n % len(NEGATIVE_KINDS)]
            self.stmts[i] = negative(self.key, valid, i, self.kinds[i])
        self.batch, self.want = self.key.batch(self.stmts)
        self.values = np.array([s.z for s in self.stmts], dtype=np.uint64).reshape(k, m)
        assert list(np.flatnonzero(~self.want)) == sorted(where)
        # the values are the batch's public inputs
        assert all(fr_from_mont_vec(self.batch.pubs[i]) == [int(v) for v in self.values[i]] for i in (0, k - 1))


def expand(values):
    """values [k, m] uint64 -> [k, m, 4] Montgomery: what the host form makes of them"""
    values = np.asarray(values, dtype=np.uint64)
    return np.array([fr_mont(int(v)) for v in values.reshape(-1)], dtype=np.uint64).reshape(values.shape + (4,))
