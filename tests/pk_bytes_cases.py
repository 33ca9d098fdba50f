"""Shared by tests/test_pk_bytes_host.py and tests/test_pk_bytes_gpu.py: the host-compiled shim of csrc/pk_bytes_dev.cuh, a host-made
Fibonacci-12 key, the offsets of a serialized proving key's sections and byte-level tampering.  Not a test module."""
import ctypes
import os
import random
import subprocess

import numpy as np

import pyref as P
import synth
from helpers import *

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "pk_bytes_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "libpk_bytes_host_shim.so")
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
QUERIES = (("a_query", 48), ("b_g1_query", 48), ("b_g2_query", 96), ("h_query", 48), ("l_query", 48))
WORDS = {1: 28, 2: 56}
LIMBS = {1: 12, 2: 24}
SIZE = {1: 48, 2: 96}


def load_shim():
    """tests/csrc/pk_bytes_host_shim.hip (the lane functions compiled for the host, bound assertions live), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("pk_bytes_dev.cuh", "decompress_dev.cuh", "pairing_dev.cuh", "ffu.cuh", "ff.cuh", "ec.cuh")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = ctypes.CDLL(SHIM_OUT)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.pkb_decode.argtypes = [ctypes.c_int, vp, sz, vp, vp, vp, vp]
    lib.pkb_convert.argtypes = [ctypes.c_int, vp, vp, sz, vp]
    lib.pkb_encode.argtypes = [ctypes.c_int, vp, sz, vp]
    lib.pkb_read.argtypes = [ctypes.c_int, vp, sz, vp, vp]
    lib.pkb_fq2_sqrt.argtypes = [ctypes.c_int, vp, vp]
    lib.pkb_fq2_sqrt.restype = ctypes.c_int
    for name in ("pkb_decode", "pkb_convert", "pkb_encode", "pkb_read"):
        getattr(lib, name).restype = None
    return lib


def shim_decode(shim, group, data):
    """-> (limbs [n, 12 | 24], inf [n], status [n], words [n, 28 | 56]) of n encodings back to back"""
    n = len(data) // SIZE[group]
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    limbs = np.full((n, LIMBS[group]), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    inf = np.full(n, 7, dtype=np.uint8)
    status = np.full(n, -1, dtype=np.int32)
    words = np.full((n, WORDS[group]), 0xA5A5A5A5, dtype=np.uint32)
    shim.pkb_decode(group, raw.ctypes.data, n, limbs.ctypes.data, inf.ctypes.data, status.ctypes.data, words.ctypes.data)
    return limbs, inf, status, words


def shim_convert(shim, group, limbs, inf):
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, LIMBS[group])
    inf = np.ascontiguousarray(inf, dtype=np.uint8)
    words = np.zeros((limbs.shape[0], WORDS[group]), dtype=np.uint32)
    shim.pkb_convert(group, limbs.ctypes.data, inf.ctypes.data, limbs.shape[0], words.ctypes.data)
    return words


def shim_encode(shim, group, words):
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, WORDS[group])
    out = np.zeros(words.shape[0] * SIZE[group], dtype=np.uint8)
    shim.pkb_encode(group, words.ctypes.data, words.shape[0], out.ctypes.data)
    return out.tobytes()


def shim_read(shim, group, words):
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, WORDS[group])
    limbs = np.zeros((words.shape[0], LIMBS[group]), dtype=np.uint64)
    inf = np.zeros(words.shape[0], dtype=np.uint8)
    shim.pkb_read(group, words.ctypes.data, words.shape[0], limbs.ctypes.data, inf.ctypes.data)
    return limbs, inf


def host_fibonacci_key(oracle, steps=12, seed=77):
    """A Groth16 key of the FibonacciCircuit of `steps` rounds made on the host by the oracle's points -> (pk dict, vk dict)."""
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    circ = fibonacci_circuit(3, 5, steps)
    rng = random.Random(seed)
    pk, meta = synth.make_pk(oracle, circ.r1cs, circ.num_vars, rng)
    gamma = oracle.fixed_base("g2", meta["g2"], fr_canon_vec([meta["trap"]["gamma"]]))[0][0]
    gabc = oracle.fixed_base("g1", meta["g1"], oracle.fr_to_canonical(meta["logs"]["gabc"]))[0]
    vk = dict(alpha_g1=pk["alpha_g1"], beta_g2=pk["beta_g2"], gamma_g2=gamma, delta_g2=pk["delta_g2"], gamma_abc_g1=gabc)
    return pk, vk


def sections(ni, m, n_h):
    """name -> (offset of its first point, bytes per point, points) in a serialized key of these dimensions; the single points too"""
    out = dict(alpha_g1=(0, 48, 1), beta_g2=(48, 96, 1), gamma_g2=(144, 96, 1), delta_g2=(240, 96, 1), gamma_abc_g1=(344, 48, ni))
    pos = 344 + 48 * ni
    out["beta_g1"], out["delta_g1"] = (pos, 48, 1), (pos + 48, 48, 1)
    pos += 96
    for (name, size), n in zip(QUERIES, (m, m, m, n_h, m - ni)):
        out[name] = (pos + 8, size, n)
        pos += 8 + size * n
    out["end"] = (pos, 0, 0)
    return out


def prefix_offsets(ni, m, n_h):
    """offsets of the five query length prefixes and of gamma_abc_g1's (first)"""
    s = sections(ni, m, n_h)
    return [336] + [s[name][0] - 8 for name, _ in QUERIES]


def with_point(raw, section, index, enc):
    """raw with the encoding of point `index` of a section replaced"""
    at, size, n = section
    assert index < n and len(enc) == size
    b = bytearray(raw)
    b[at + size * index:at + size * (index + 1)] = enc
    return bytes(b)


def pk_equal(a, b):
    """two pk dicts (Device.pk_load's shape, flags optional = none set): every array equal"""
    for name, flag, _ in (("a_query", "a_inf", 0), ("b_g1_query", "b_g1_inf", 0), ("b_g2_query", "b_g2_inf", 0), ("h_query", "h_inf", 0), ("l_query", "l_inf", 0)):
        x, y = np.asarray(a[name], dtype=np.uint64), np.asarray(b[name], dtype=np.uint64)
        if x.shape[0] != y.shape[0] or x.reshape(-1).tobytes() != y.reshape(-1).tobytes():
            return False
        fx = np.zeros(x.shape[0], np.uint8) if a.get(flag) is None else np.asarray(a[flag], dtype=np.uint8)
        fy = np.zeros(y.shape[0], np.uint8) if b.get(flag) is None else np.asarray(b[flag], dtype=np.uint8)
        if not np.array_equal(fx, fy):
            return False
    return all(np.array_equal(np.asarray(a[k], dtype=np.uint64).reshape(-1), np.asarray(b[k], dtype=np.uint64).reshape(-1))
               for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2"))
