"""Shared by tests/test_sponge_chains_host.py and tests/test_sponge_chains_gpu.py: the host-compiled shim of csrc/sponge_chain_dev.cuh,
the request sets and the layout of a MatrixCircuit assignment.  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "sponge_chain_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "libsponge_chain_host_shim.so")
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SENTINEL = 0xA5A5A5A5A5A5A5A5
NEVER = (1 << 32) + 1           # option "sponge_chains_min": above 2^32 = the chains never run on the device
PERM_WITNESSES, FIRST_PERM_SKIPPED = 265, 5


def load_shim():
    """tests/csrc/sponge_chain_host_shim.hip (the chain kernel's lane function compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("sponge_chain_dev.cuh", "poseidon_params.inc", "ff.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = C.CDLL(SHIM_OUT)
    lib.sc_walk.restype = None
    lib.sc_walk.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def requests(n, k=5, seed=200):
    """k <= 5 requests, the set of test_matrix_batch_gpu.py: every entry 2^64 - 1 (c's entries need the third limb), all zero, a
    random one, another, the first random one again."""
    rng = np.random.default_rng(seed + n)
    a = rng.integers(0, 1 << 63, size=(5, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(5, n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 63, size=(5, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(5, n, n), dtype=np.uint64)
    a[0] = b[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    a[1] = b[1] = 0
    a[4], b[4] = a[2], b[2]
    return a[:k], b[:k]


def many_requests(n, k, seed=300):
    """k requests: requests(n) repeated, every repeat after the first with its random entries drawn again"""
    parts = [requests(n, 5, seed + 7 * i) for i in range((k + 4) // 5)]
    return np.concatenate([p[0] for p in parts])[:k], np.concatenate([p[1] for p in parts])[:k]


def layout(n):
    """offsets of a MatrixCircuit assignment (csrc/witness.hip: MatrixWitnessLayout): the three sponge gadgets and the total"""
    nn = n * n
    perms = (nn + 1) // 2
    hw = perms * PERM_WITNESSES - FIRST_PERM_SKIPPED
    off_ha = 4 + 2 * nn
    off_hb = off_ha + hw
    off_hc = off_hb + hw + nn + nn * (n + 1)
    return dict(perms=perms, hw=hw, off=(off_ha, off_hb, off_hc), total=off_hc + hw)


def mont_limbs(values):
    """Python ints -> [len, 4] u64 Montgomery limbs"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (v << 256) % R_MOD
        out[i] = [(m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    return out


def unlimbs(row):
    return sum(int(v) << (64 * j) for j, v in enumerate(row))


def chain_values(a, b):
    """the elements the three chains of request (a, b) absorb, as Python ints: a, b row-major and c = a b over the integers"""
    n = a.shape[0]
    ai = [[int(x) for x in row] for row in a]
    bi = [[int(x) for x in row] for row in b]
    c = [sum(ai[i][k] * bi[k][j] for k in range(n)) for i in range(n) for j in range(n)]
    return [sum(ai, []), sum(bi, []), c]
