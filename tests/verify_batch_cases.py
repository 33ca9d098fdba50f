"""Shared by tests/test_verify_batch.py and tests/test_verify_batch_gpu.py: a small Groth16 key, K valid proofs of K different
assignments made by the CPU oracle, the tampering the issue lists, and the per-proof reference verdicts (a loop of
zkg16_verify_prepared).  Not a test module."""
import ctypes
import os
import random
import subprocess

import numpy as np

import pyref as P
import synth
from helpers import *


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "pairing_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "libpairing_host_shim.so")
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")


def load_shim():
    """tests/csrc/pairing_host_shim.hip (the device pairing header compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("pairing_dev.cuh", "pairing_fast.inc", "ffu.cuh", "ff.cuh", "ec.cuh", "hostff.hpp")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = ctypes.CDLL(SHIM_OUT)
    lib.pd_member.restype = ctypes.c_int
    lib.pd_scale128.restype = ctypes.c_int
    return lib


def host_miller(shim, g1, g2):
    """-> (the device header's Miller value computed on the host, pairing_fast.inc's), 72 u64 each"""
    od, oh = np.zeros(72, np.uint64), np.zeros(72, np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    shim.pd_miller(vp(np.ascontiguousarray(g1, dtype=np.uint64)), vp(np.ascontiguousarray(g2, dtype=np.uint64)), vp(od), vp(oh))
    return od, oh


def draw_rho(rng, k):
    """k non-zero 128-bit multipliers from a seeded generator (tests only: a service draws them from the OS)."""
    out = np.zeros((k, 2), dtype=np.uint64)
    for i in range(k):
        v = rng.randrange(1, 1 << 128)
        out[i, 0], out[i, 1] = v & MASK64, v >> 64
    return out


class Batch:
    """pvk + K proofs (proofs [K, 48], infs [K, 3], pubs [K, ni - 1, 4])."""

    def __init__(self, pvk, pubs, proofs, infs):
        self.pvk, self.pubs, self.proofs, self.infs = pvk, pubs, proofs, infs

    @property
    def k(self):
        return self.proofs.shape[0]

    def copy(self):
        return Batch(self.pvk, self.pubs.copy(), self.proofs.copy(), self.infs.copy())

    def head(self, k):
        return Batch(self.pvk, self.pubs[:k].copy(), self.proofs[:k].copy(), self.infs[:k].copy())

    def tiled(self, k):
        reps = (k + self.k - 1) // self.k
        return Batch(self.pvk, np.tile(self.pubs, (reps, 1, 1))[:k].copy(), np.tile(self.proofs, (reps, 1))[:k].copy(), np.tile(self.infs, (reps, 1))[:k].copy())

    def loop(self):
        """what zkg16_verify_prepared says of each proof alone"""
        from zksnark_finalproject_amd.device import verify_prepared
        return np.array([verify_prepared(self.pvk, self.pubs[i], self.proofs[i], self.infs[i]) for i in range(self.k)], dtype=bool)


def make_batch(oracle, k, steps=12, seed=2024):
    """The host Fibonacci synthesis (one circuit, every (a, b) another assignment) under a known-trapdoor key from the oracle,
    proved k times by the oracle with k different assignments and (r, s).  a, b < 2^30 and 12 steps: every public input is below
    2^40 and num_instance is 4.  Full-width inputs, other key shapes and statements with a point at infinity: tests/sim_proofs.py."""
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    from zksnark_finalproject_amd.device import pvk_prepare
    rng = random.Random(seed)
    circs = [fibonacci_circuit(rng.randrange(1 << 30), rng.randrange(1 << 30), steps) for _ in range(k)]
    c0 = circs[0]
    pk, meta = synth.make_pk(oracle, c0.r1cs, c0.num_vars, rng)
    gabc, ginf = oracle.fixed_base("g1", meta["g1"], oracle.fr_to_canonical(meta["logs"]["gabc"]))
    assert not np.any(ginf)
    gamma_g2 = oracle.point_mul("g2", meta["g2"], fr_canon(meta["trap"]["gamma"]))[0]
    vk = dict(alpha_g1=pk["alpha_g1"], beta_g2=pk["beta_g2"], gamma_g2=gamma_g2, delta_g2=pk["delta_g2"], gamma_abc_g1=gabc)
    pvk = pvk_prepare(vk)
    proofs, infs = [], []
    for c in circs:
        p, f = oracle.prove(pk, fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng)), c.r1cs, c.z)
        proofs.append(p)
        infs.append(f)
    pubs = np.array([c.public_inputs for c in circs], dtype=np.uint64).reshape(k, c0.num_instance - 1, 4)
    return Batch(pvk, pubs, np.array(proofs, dtype=np.uint64).reshape(k, 48), np.array(infs, dtype=np.uint8).reshape(k, 3))


def rerandomised(oracle, base, k, rng):
    """k valid proofs from a few: (A, B, C) -> (t A, t^-1 B, C) is again a valid proof of the same statement for every t != 0"""
    proofs = np.zeros((k, 48), dtype=np.uint64)
    infs = np.zeros((k, 3), dtype=np.uint8)
    pubs = np.zeros((k,) + base.pubs.shape[1:], dtype=np.uint64)
    for i in range(k):
        j = i % base.k
        proofs[i], infs[i], pubs[i] = base.proofs[j], base.infs[j], base.pubs[j]
        if i >= base.k:
            t = rng.randrange(1, P.R_MOD)
            proofs[i, 0:12] = oracle.point_mul("g1", base.proofs[j, 0:12], fr_canon(t))[0]
            proofs[i, 12:36] = oracle.point_mul("g2", base.proofs[j, 12:36], fr_canon(pow(t, -1, P.R_MOD)))[0]
    return Batch(base.pvk, pubs, proofs, infs)


def to_wire(b):
    """a limb batch as it travels: [k, 192] bytes (A 48 | B 96 | C 48).  The wire form has one encoding of the point at infinity,
    so all-zero limbs without a flag (which the limb entry points read as infinity) travel as infinity too."""
    from zksnark_finalproject_amd import wire
    k = b.k
    inf = lambda lo, hi, j: (b.infs[:, j].astype(bool) | ~b.proofs[:, lo:hi].any(axis=1)).astype(np.uint8)
    a = np.frombuffer(wire.points_compress("g1", b.proofs[:, 0:12], inf(0, 12, 0)), dtype=np.uint8).reshape(k, 48)
    bb = np.frombuffer(wire.points_compress("g2", b.proofs[:, 12:36], inf(12, 36, 1)), dtype=np.uint8).reshape(k, 96)
    c = np.frombuffer(wire.points_compress("g1", b.proofs[:, 36:48], inf(36, 48, 2)), dtype=np.uint8).reshape(k, 48)
    return np.ascontiguousarray(np.concatenate([a, bb, c], axis=1))


def g2_outside_subgroup():
    """A point of the twist that is not in the prime-order subgroup (the construction of
    test_wire.py::test_native_codecs_equal_python_rules): a random x with a point, which the validating decoder refuses."""
    from zksnark_finalproject_amd import wire
    rng = random.Random(99)
    while True:
        x0, x1 = rng.randrange(P.Q_MOD), rng.randrange(P.Q_MOD)
        cand = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
        cand[0] |= 0x80
        try:
            pt, inf = wire.g2_decompress(bytes(cand), validate=False)
        except ValueError:
            continue
        try:
            wire.g2_decompress(bytes(cand))
        except ValueError:
            return np.asarray(pt, dtype=np.uint64).reshape(24)


def g1_add(oracle, p, q):
    r, inf = oracle.point_add("g1", p, q)
    assert not inf
    return np.asarray(r, dtype=np.uint64).reshape(12)


TAMPERS = ("c_plus_g", "public_input", "swap_a", "b_outside_subgroup", "a_off_curve", "a_infinity")


def positions(k):
    """{0}, {K-1}, {two in the middle}, {all}; duplicates collapse for tiny K"""
    out = [(0,), (k - 1,), tuple(sorted({k // 2, max(k // 2 - 1, 0)})), tuple(range(k))]
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


def tamper(oracle, batch, kind, where, torsion=None):
    """a copy of the batch with the proofs at `where` tampered"""
    b = batch.copy()
    k = b.k
    if kind == "swap_a" and len(where) == k > 1:      # every A against its neighbour's: a rotation (pairwise swaps would undo each other)
        b.proofs[:, 0:12] = np.roll(batch.proofs[:, 0:12], 1, axis=0)
        return b
    for i in where:
        if kind == "c_plus_g":
            b.proofs[i, 36:48] = g1_add(oracle, batch.proofs[i, 36:48], G1_GEN_LIMBS)
        elif kind == "public_input":
            b.pubs[i, 0] = fr_mont(P.fr_from_mont(unlimbs(batch.pubs[i, 0])) + 1)
        elif kind == "swap_a":
            j = (i + 1) % k                          # A_i <-> A_j (K = 1: nobody to swap with, A <- 2A)
            if k > 1:
                b.proofs[[i, j], 0:12] = b.proofs[[j, i], 0:12]
            else:
                b.proofs[i, 0:12] = g1_add(oracle, batch.proofs[i, 0:12], batch.proofs[i, 0:12])
        elif kind == "b_outside_subgroup":
            b.proofs[i, 12:36] = torsion
        elif kind == "a_off_curve":
            b.proofs[i, 0] ^= np.uint64(1)
        elif kind == "a_infinity":
            b.proofs[i, 0:12] = 0
            b.infs[i, 0] = 1
        else:
            raise ValueError(kind)
    return b
