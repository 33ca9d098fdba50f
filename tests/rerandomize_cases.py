"""Shared by tests/test_rerandomize_host.py and tests/test_rerandomize_gpu.py: the case table of proof re-randomisation
(ark-groth16 rerandomize_proof: A' = r1^-1 A, B' = r1 B + r1 r2 delta, C' = C + r2 A), the host build of the device header and the
synthetic limbs of the compress lane.  Not a test module.

With the trapdoor known (sim_proofs.SimKey) a proof is its three logs (a, b, c) and delta is a log too, so the expected result is
known in the exponent, independently of any ladder:

    a' = a / r1        b' = r1 b + r1 r2 delta        c' = c + r2 a        (mod r)

and the expected points are the oracle's fixed_base of those integers.  Every case asserts on the integers that it is the case its
name says before it is handed out, and that its verdict (SimKey.verdict) is the original's."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import pyref as P
import sim_proofs as S
from helpers import *

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "rerandomize_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "librerandomize_host_shim.so")
R = S.R
Q = P.Q_MOD


def load_shim():
    """tests/csrc/rerandomize_host_shim.hip (the device header compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("rerandomize_dev.cuh", "pairing_each_dev.cuh", "pairing_dev.cuh", "ffu.cuh", "ff.cuh", "ec.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = C.CDLL(SHIM_OUT)
    vp = C.c_void_p
    lib.rr_scalars.restype = None
    lib.rr_scalars.argtypes = [vp, vp, vp]
    lib.rr_g1_lane.restype = None
    lib.rr_g1_lane.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.rr_g2_lane.restype = None
    lib.rr_g2_lane.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.rr_compress.restype = None
    lib.rr_compress.argtypes = [C.c_int, vp, vp, C.c_size_t, vp]
    return lib


# ------------------------------------------------------------------------------------------------ the case table
MULTIPLIERS = [v for v in S.EDGES if v]          # 1 (A' = A), r - 1 (A' = -A), zero low limbs, zero high limbs, 2^32 - 1, 2^64, (r +- 1) / 2
assert 1 in MULTIPLIERS and R - 1 in MULTIPLIERS and 2**32 - 1 in MULTIPLIERS and 2**64 in MULTIPLIERS and (R - 1) // 2 in MULTIPLIERS and (R + 1) // 2 in MULTIPLIERS


class Case:
    """a statement, its multipliers and the logs of the re-randomised proof"""

    def __init__(self, key, name, stmt, r1, r2):
        assert 0 < r1 < R and 0 < r2 < R
        self.name, self.stmt, self.r1, self.r2 = name, stmt, r1, r2
        self.a = stmt.a * S.inv(r1) % R
        self.b = (r1 * stmt.b + r1 * r2 * key.delta) % R
        self.c = (stmt.c + r2 * stmt.a) % R
        self.after = stmt.but(name + "_after", a=self.a, b=self.b, c=self.c, c_unflagged=False)
        # both sides of the equation gain r2 a delta: the verdict is the original's, valid or not
        assert key.verdict(self.after) == key.verdict(stmt)


def key_of(oracle):
    return S.random_key(oracle, 2, 7101)


def case_table(key):
    """-> [Case], the order fixed (the GPU tests pad and slice it)"""
    rng = random.Random(7102)
    d, inv = key.delta, S.inv
    wide = lambda: S.wide(rng)
    z = lambda: [wide()]
    out = []
    add = lambda name, stmt, r1, r2: out.append(Case(key, name, stmt, r1, r2))

    # ---- ordinary statements, valid and invalid
    for i in range(2):
        s = key.ordinary(z(), rng, "valid%d" % i)
        assert key.verdict(s)
        add(s.name, s, wide(), wide())
    for i in range(2):
        s = S.negative_twin(key, key.ordinary(z(), rng), i)
        assert not key.verdict(s)
        add("invalid%d_%s" % (i, s.name), s, wide(), wide())

    # ---- r1 at its edges
    for v in MULTIPLIERS:
        c = Case(key, "r1_%x" % v, key.ordinary(z(), rng), v, wide())
        if v == 1:
            assert c.a == c.stmt.a
        if v == R - 1:
            assert c.a == R - c.stmt.a
        out.append(c)
    # ---- r2 at its edges, and r1 r2 = 1
    for v in MULTIPLIERS:
        out.append(Case(key, "r2_%x" % v, key.ordinary(z(), rng), wide(), v))
    r1 = wide()
    c = Case(key, "r1_r2_product_one", key.ordinary(z(), rng), r1, inv(r1))
    assert c.r1 * c.r2 % R == 1 and c.b == (c.r1 * c.stmt.b + d) % R
    out.append(c)

    # ---- degenerate sums, each built by solving for a log; the statements stay valid (c or b solved from the equation)
    def with_b(name, b, zz):
        a = rng.randrange(1, R)
        s = S.Stmt(name, zz, a, b, (a * b - key.t(zz)) * inv(d))
        assert key.verdict(s)
        return s

    def with_c_of_a(name, factor, zz):
        """c = factor a: a b = t + factor a delta, so b = (t + factor a delta) / a"""
        a = rng.randrange(1, R)
        s = S.Stmt(name, zz, a, (key.t(zz) + factor * a * d) * inv(a), factor * a)
        assert key.verdict(s) and s.c == factor * a % R
        return s

    r1, r2 = wide(), wide()
    c = Case(key, "b_prime_infinity", with_b("b_is_minus_r2_delta", -r2 * d, z()), r1, r2)
    assert c.b == 0 and c.stmt.b != 0
    out.append(c)
    c = Case(key, "b_equals_delta", with_b("b_is_delta", d, z()), wide(), wide())
    assert c.stmt.b == d                                   # B + delta is a doubling
    out.append(c)
    c = Case(key, "b_equals_minus_delta", with_b("b_is_minus_delta", -d, z()), wide(), wide())
    assert (c.stmt.b + d) % R == 0 and c.b == c.r1 * (c.r2 - 1) * d % R      # B + delta = O
    out.append(c)
    r2 = wide()
    c = Case(key, "c_prime_infinity", with_c_of_a("c_is_minus_r2_a", -r2, z()), wide(), r2)
    assert c.c == 0 and c.stmt.c != 0
    out.append(c)
    r2 = wide()
    c = Case(key, "c_equals_r2_a", with_c_of_a("c_is_r2_a", r2, z()), wide(), r2)
    assert c.stmt.c == r2 * c.stmt.a % R and c.c == 2 * c.stmt.c % R          # the last addition is a doubling
    out.append(c)

    # ---- points at infinity
    c = Case(key, "a_infinity", key.ab_zero(z(), rng, "a"), wide(), wide())
    assert c.stmt.a == 0 and c.a == 0 and c.c == c.stmt.c                    # A' = O and C' = C
    out.append(c)
    c = Case(key, "b_infinity", key.ab_zero(z(), rng, "b"), wide(), wide())
    assert c.stmt.b == 0 and c.b == c.r1 * c.r2 * d % R                      # B' = r1 r2 delta
    out.append(c)
    c = Case(key, "c_infinity", key.c_zero(z(), rng), wide(), wide())
    assert c.stmt.c == 0 and c.c == c.r2 * c.stmt.a % R                      # C' = r2 A
    out.append(c)
    zz = z()
    s = S.Stmt("a_and_b_infinity", zz, 0, 0, -key.t(zz) * inv(d))
    assert key.verdict(s)
    c = Case(key, "a_and_b_infinity", s, wide(), wide())
    assert c.a == 0 and c.b == c.r1 * c.r2 * d % R and c.c == s.c
    out.append(c)
    c = Case(key, "c_infinity_unflagged", key.c_zero(z(), rng, unflagged=True), wide(), wide())
    assert c.stmt.c == 0 and c.stmt.c_unflagged
    out.append(c)
    assert len({c.name for c in out}) == len(out)
    return out


class Table:
    """the case table as arrays: the batch in (proofs, infs, pubs), r1 / r2 [k, 4] Montgomery, the expected batch out (want, want_inf
    from the oracle's fixed_base of the expected logs) and the verdicts"""

    def __init__(self, oracle, key, cases):
        self.key, self.cases = key, cases
        self.batch, self.verdicts = key.batch([c.stmt for c in cases])
        after, after_verdicts = key.batch([c.after for c in cases])
        assert np.array_equal(self.verdicts, after_verdicts)
        self.want, self.want_inf = after.proofs, after.infs
        self.r1 = np.array([fr_mont(c.r1) for c in cases], dtype=np.uint64).reshape(-1, 4)
        self.r2 = np.array([fr_mont(c.r2) for c in cases], dtype=np.uint64).reshape(-1, 4)
        self.delta = np.ascontiguousarray(key.vk["delta_g2"], dtype=np.uint64).reshape(24)
        for i, c in enumerate(cases):
            assert list(self.want_inf[i]) == [c.a == 0, c.b == 0, c.c == 0]

    @property
    def k(self):
        return len(self.cases)


_TABLES = {}


def table(oracle, k=None):
    """the whole case table, or (k given) its first cases / the table padded with ordinary valid statements up to k proofs; made once
    per k and shared, never changed"""
    if "key" not in _TABLES:
        _TABLES["key"] = key_of(oracle)
        _TABLES["cases"] = case_table(_TABLES["key"])
    key, cases = _TABLES["key"], _TABLES["cases"]
    if k not in _TABLES:
        if k is None or k == len(cases):
            use = cases
        elif k < len(cases):
            use = cases[:k]
        else:
            rng = random.Random(7200 + k)
            pad = S.valid_statements(key, k - len(cases), 7300 + k)
            use = cases + [Case(key, "pad%d" % i, s, S.wide(rng), S.wide(rng)) for i, s in enumerate(pad)]
        _TABLES[k] = Table(oracle, key, use)
    return _TABLES[k]


# ------------------------------------------------------------------------------------------------ refusals
def refusal_calls(t):
    """(name, what to change, the text zkg16_last_error must hold) for the refusals every form shares"""
    k = t.k
    zero, unreduced = np.zeros(4, dtype=np.uint64), np.array(limbs(R, 4), dtype=np.uint64)
    above = np.full(4, MASK64, dtype=np.uint64)
    for which in ("r1", "r2"):
        for at in (0, k // 2, k - 1):
            for kind, v in (("zero", zero), ("not below r", unreduced), ("not below r", above)):
                yield "%s_%d_%s" % (which, at, kind.split()[0]), (which, at, v), "%s of proof %d is %s" % (which, at, kind)
    yield "zero_delta", ("delta", None, None), "delta_g2"
    yield "k_zero", ("k", None, None), "no proofs"
    for name in ("delta", "proofs", "r1", "r2", "out", "out_inf"):
        yield "null_" + name, ("null", name, None), "null pointer"


# ------------------------------------------------------------------------------------------------ the compress lane
HALF = (Q - 1) // 2


def sign_rule_points():
    """synthetic limbs around the sign rule (the stage takes any limbs below q; none of these is on a curve) ->
    (g1 [n, 12], g2 [m, 24]).  A reduced x has a top byte of at most 0x1a, so its five low bits are never all set: the x values
    here fill the top byte as far as a value below q can (q - 1: 0x1a, 2^380 - 1: 0x0f, and 0x19ff..ff)."""
    xs = [1, Q - 1, 2**380 - 1, (0x19 << 376) | (2**376 - 1)]
    ys = [1, HALF, HALF + 1, Q - 1]
    g1 = [np.concatenate([fq_mont(x), fq_mont(y)]) for x in xs for y in ys]
    g2 = []
    for x in xs[:3]:
        for y0, y1 in [(HALF, 0), (HALF + 1, 0), (1, 0), (Q - 1, 0), (1, HALF), (Q - 1, HALF), (1, HALF + 1), (Q - 1, HALF + 1), (0, 1), (0, Q - 1)]:
            g2.append(np.concatenate([fq_mont(x), fq_mont(Q - x), fq_mont(y0), fq_mont(y1)]))
    return np.array(g1, dtype=np.uint64).reshape(-1, 12), np.array(g2, dtype=np.uint64).reshape(-1, 24)


def points_of(tbl):
    """the G1 and G2 points of a table's expected proofs with their flags -> (g1 [2k, 12], g1_inf, g2 [k, 24], g2_inf)"""
    g1 = np.ascontiguousarray(np.concatenate([tbl.want[:, 0:12], tbl.want[:, 36:48]]), dtype=np.uint64)
    g1_inf = np.ascontiguousarray(np.concatenate([tbl.want_inf[:, 0], tbl.want_inf[:, 2]]), dtype=np.uint8)
    g2 = np.ascontiguousarray(tbl.want[:, 12:36], dtype=np.uint64)
    return g1, g1_inf, g2, np.ascontiguousarray(tbl.want_inf[:, 1], dtype=np.uint8)
