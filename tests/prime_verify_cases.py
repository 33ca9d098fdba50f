"""Shared by tests/test_verify_prime_host.py and tests/test_verify_prime_gpu.py: the prime form of batched verification (one extended
key of 260 points for every request of a trapdoor; inputs x, the 256 digest bits, n, j made from 16 bytes).  The host build of the
device header, the (x, j) and multiplier cases with their Python-integer answers, and simulated statements under a key with known
logs (sim_proofs.SimKey, g[258] = v_n, g[259] = -v_j).  Not a test module."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np

import sim_proofs as S
from helpers import *

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "prime_inputs_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "libprime_inputs_host_shim.so")
R = S.R
M64 = (1 << 64) - 1


def load_shim():
    """tests/csrc/prime_inputs_host_shim.hip (the device header compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("prime_inputs_dev.cuh", "ff.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = C.CDLL(SHIM_OUT)
    lib.pi_digest.restype = None
    lib.pi_digest.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.pi_public_inputs.restype = None
    lib.pi_public_inputs.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    lib.pi_rho_sums.restype = None
    lib.pi_rho_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.pi_ext_scalar.restype = C.c_uint64
    lib.pi_ext_scalar.argtypes = [C.c_uint, C.c_uint64, C.c_uint64]
    return lib


# ------------------------------------------------------------------------------------------------ (x, j)
EDGE = [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
EDGE_PAIRS = [(x, j) for x in EDGE for j in EDGE]
CARRY_PAIRS = [(x, j) for x, j in EDGE_PAIRS if x + j > M64]
assert (M64, 1) in CARRY_PAIRS and (2**63, 2**63) in CARRY_PAIRS and (M64, M64) in CARRY_PAIRS


def random_pairs(n, seed):
    rng = random.Random(seed)
    return [(rng.getrandbits(64), rng.getrandbits(rng.choice((1, 8, 33, 64)))) for _ in range(n)]


def pairs_of(k, seed=5):
    """k pairs: the edge pairs first, then random ones"""
    return (EDGE_PAIRS + random_pairs(max(k - len(EDGE_PAIRS), 0), seed))[:k]


def py_digest(x, j):
    """-> (SHA-256 of x + j as 32 little-endian bytes, the digest as a little-endian integer mod 2^20): hashlib"""
    d = hashlib.sha256((x + j).to_bytes(32, "little")).digest()
    return d, int.from_bytes(d, "little") & 0xFFFFF


def ext_ints(x, j):
    """the 259 inputs of a request under the extended key, as integers: x, bit_0 .. bit_255, n, j"""
    d, n = py_digest(x, j)
    return [x] + [(d[t >> 3] >> (t & 7)) & 1 for t in range(256)] + [n, j]


def py_sums(pairs, rhos, live=None):
    """the 260 sums over the live proofs, Python integers"""
    out = [0] * 260
    for i, ((x, j), r) in enumerate(zip(pairs, rhos)):
        if live is not None and not live[i]:
            continue
        out[0] += r
        for c, v in enumerate(ext_ints(x, j)):
            if v:
                out[1 + c] += r * v
    return out


def py_sums_large(pairs, rhos, live=None):
    """py_sums for a large batch in a time a test can afford: the 256 bit columns as one exact integer matrix product (digest bits
    x the multipliers' 16-bit pieces, every entry below 2^16 K), the four other columns as Python integers.  Checked against
    py_sums by tests/test_verify_prime_host.py"""
    k = len(pairs)
    keep = [i for i in range(k) if live is None or live[i]]
    assert k < 1 << 32
    digs = [py_digest(*pairs[i]) for i in keep]
    bits = np.unpackbits(np.frombuffer(b"".join(d for d, _ in digs), dtype=np.uint8).reshape(len(keep), 32), axis=1, bitorder="little") if keep else np.zeros((0, 256), np.uint8)
    pieces = np.array([[(rhos[i] >> (16 * p)) & 0xFFFF for p in range(8)] for i in keep], dtype=np.uint64).reshape(len(keep), 8)
    cols = bits.T.astype(np.uint64) @ pieces
    out = [sum(rhos[i] for i in keep), sum(rhos[i] * pairs[i][0] for i in keep)]
    out += [sum(int(cols[t, p]) << (16 * p) for p in range(8)) for t in range(256)]
    out += [sum(rhos[i] * n for i, (_, n) in zip(keep, digs)), sum(rhos[i] * pairs[i][1] for i in keep)]
    return out


SUM_KS = (1, 2, 63, 64, 65, 257, 1000)


def sum_cases(ks=SUM_KS):
    """(name, pairs, rho integers, live bytes or None): every multiplier 2^128 - 1 on x = j = 2^64 - 1 (full carries), and the
    multipliers of sim_proofs.RHO_EDGES on the edge pairs under a live mask that is all set, all clear and alternating"""
    for k in ks:
        yield "k%d_full_carries" % k, [(M64, M64)] * k, [2**128 - 1] * k, None
        pairs = pairs_of(k, seed=k)
        rhos = [S.RHO_EDGES[(3 * i + k) % len(S.RHO_EDGES)] for i in range(k)]
        for name, live in (("all_set", np.ones(k, np.uint8)), ("all_clear", np.zeros(k, np.uint8)), ("alternating", (np.arange(k) % 2).astype(np.uint8))):
            yield "k%d_%s" % (k, name), pairs, rhos, live


_WANT = {}


def sums_want(name, pairs, rhos, live):
    """py_sums, computed once per case and shared"""
    if name not in _WANT:
        _WANT[name] = py_sums(pairs, rhos, live)
    return _WANT[name]


def u64s(vals):
    return np.array(list(vals), dtype=np.uint64)


def sums_ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(260, 4)]


# ------------------------------------------------------------------------------------------------ simulated statements
class Claim:
    """a request as the verifier is handed it: the (x, j) it claims and the proof's statement with the inputs of that claim"""

    def __init__(self, name, x, j, stmt):
        self.name, self.x, self.j, self.stmt = name, x, j, stmt


class PrimeSim:
    """An extended key with known logs and K requests under it.  g[0 .. 257]: the template's, g[258] = v_n, g[259] = -v_j; request
    (x, j)'s own 258-point key has g_0 + n v_n - j v_j in front."""

    def __init__(self, oracle, seed):
        rng = random.Random(seed)
        self.oracle = oracle
        self.v_n, self.v_j = rng.randrange(1, R), rng.randrange(1, R)
        self.key = S.SimKey(oracle, [rng.randrange(1, R) for _ in range(258)] + [self.v_n, -self.v_j % R], seed + 1)
        self.rng = random.Random(seed + 2)

    def valid(self, x, j):
        s = self.key.ordinary(ext_ints(x, j), self.rng)
        assert self.key.verdict(s)
        return Claim("valid", x, j, s)

    def claimed(self, c, name, x, j):
        """the proof of c handed in with another (x, j): invalid, asserted on the integers"""
        assert 0 <= x <= M64 and 0 <= j <= M64
        s = self.key.invalid(c.stmt.but(name, z=ext_ints(x, j)))
        return Claim(name, x, j, s)

    def negatives(self, claims, where):
        """the claims with those at `where` replaced by negatives, the kinds cycled; an exchange also replaces the next claim"""
        out = list(claims)
        taken = set()
        for n, i in enumerate(where):
            if i in taken:
                continue
            c = claims[i]
            kind = n % 5
            if kind == 2 and not (c.j >= 1 and c.x < M64):
                kind = 0
            if kind == 3 and (i + 1 >= len(claims) or i + 1 in where):
                kind = 1
            if kind == 0:
                out[i] = self.claimed(c, "j_plus_1", c.x, c.j + 1)
            elif kind == 1:
                out[i] = self.claimed(c, "x_plus_1", c.x + 1, c.j)
            elif kind == 2:
                # the same sum, so the same digest and n: x and j enter on their own, not only through the hash
                assert py_digest(c.x + 1, c.j - 1) == py_digest(c.x, c.j)
                out[i] = self.claimed(c, "x_plus_1_j_minus_1", c.x + 1, c.j - 1)
            elif kind == 3:
                d = claims[i + 1]
                out[i], out[i + 1] = self.claimed(c, "exchanged", d.x, d.j), self.claimed(d, "exchanged", c.x, c.j)
                taken.add(i + 1)
            else:
                out[i] = Claim("c_dropped", c.x, c.j, self.key.c_dropped(c.stmt))
        return out

    def batch(self, claims):
        """-> (verify_batch_cases.Batch under the extended key, xs, js, the by-construction verdicts)"""
        b, want = self.key.batch([c.stmt for c in claims])
        return b, u64s(c.x for c in claims), u64s(c.j for c in claims), want

    def own_pvk(self, x, j):
        """the prepared 258-point key of request (x, j): the template's with gamma_abc_g1[0] = (g_0 + n v_n - j v_j) G1"""
        n = py_digest(x, j)[1]
        g0 = (self.key.g[0] + n * self.v_n - j * self.v_j) % R
        pt, inf = self.oracle.fixed_base("g1", G1_GEN_LIMBS, fr_canon_vec([g0]))
        assert not inf[0]
        gabc = np.concatenate([np.asarray(pt, dtype=np.uint64).reshape(1, 12), np.asarray(self.key.pvk["gamma_abc_g1"], dtype=np.uint64).reshape(260, 12)[1:258]])
        return dict(self.key.pvk, gamma_abc_g1=gabc)


# pairs for simulated batches: j >= 1 and x below 2^64 - 1 often enough that every kind of negative occurs
def sim_pairs(k, seed=77):
    rng = random.Random(seed)
    fixed = [(12345, 9), (0, 3), (M64 - 1, 18), (99, 4), (2**32, 2**32 - 1), (7, 0), (M64, 1), (2**63, 2**63)]
    return (fixed + [(rng.getrandbits(64) >> 1, 1 + rng.getrandbits(20)) for _ in range(max(k - len(fixed), 0))])[:k]
