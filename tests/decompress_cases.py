"""Shared by tests/test_decompress_dev.py and tests/test_verify_wire_gpu.py: the host-compiled shim of csrc/decompress_dev.cuh, the
library's host decoders with their statuses, and the encodings a decoder must refuse, one per status.  Not a test module."""
import ctypes
import os
import random
import subprocess

import numpy as np

import pyref as P
from helpers import *

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_SRC = os.path.join(ROOT, "tests", "csrc", "decompress_host_shim.hip")
SHIM_OUT = os.path.join(ROOT, "tests", "csrc", "build", "libdecompress_host_shim.so")
CSRC = os.path.join(ROOT, "zksnark-finalproject_amd", "csrc")
Q = P.Q_MOD
SIZE = {"g1": 48, "g2": 96}
WIDTH = {"g1": 12, "g2": 24}


def load_shim():
    """tests/csrc/decompress_host_shim.hip (the device decompression header compiled for the host), built when stale."""
    deps = [SHIM_SRC] + [os.path.join(CSRC, f) for f in ("decompress_dev.cuh", "pairing_dev.cuh", "pairing_fast.inc", "ffu.cuh", "ff.cuh", "ec.cuh", "hostff.hpp")]
    if not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        os.makedirs(os.path.dirname(SHIM_OUT), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SHIM_OUT, SHIM_SRC])
    lib = ctypes.CDLL(SHIM_OUT)
    for name in ("dc_consts_check", "dc_fq_sqrt", "dc_fq2_sqrt", "dc_decompress"):
        getattr(lib, name).restype = ctypes.c_int
    lib.dc_decompress.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


def _decode_with(fn, group, data, validate, lead=()):
    n = len(data) // SIZE[group]
    assert len(data) == n * SIZE[group]
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.full((n, WIDTH[group]), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)       # a decoder must write every limb, failed points included
    inf = np.full(n, 7, dtype=np.uint8)
    status = np.full(n, -1, dtype=np.int32)
    rc = fn(*lead, raw.ctypes.data, n, out.ctypes.data, inf.ctypes.data, 1 if validate else 0, status.ctypes.data)
    return out, inf, status, rc


def host_decode(group, data, validate=True):
    """zkg16_g1_decompress / zkg16_g2_decompress on points back to back -> (limbs, inf, status, return code); nothing raises."""
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    fn = lib.zkg16_g1_decompress if group == "g1" else lib.zkg16_g2_decompress
    return _decode_with(lambda raw, n, out, inf, v, st: fn(raw, n, out, inf, v, ctypes.cast(st, ctypes.POINTER(ctypes.c_int))), group, data, validate)


def shim_decode(shim, group, data, validate=True):
    """the same through the device header run on the host; the return code is the number of points that failed"""
    return _decode_with(shim.dc_decompress, group, data, validate, lead=(1 if group == "g1" else 2,))


def legendre(a):
    """1 residue, -1 non-residue, 0 zero"""
    s = pow(a % Q, (Q - 1) // 2, Q)
    return -1 if s == Q - 1 else s


def valid_points(oracle, group, n, seed):
    """n subgroup points -> (limbs [n, 12 | 24], their encodings back to back); both sign bits occur"""
    from zksnark_finalproject_amd import wire
    rng = random.Random(seed)
    gen = G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS
    pts = oracle.fixed_base(group, gen, fr_canon_vec([rng.randrange(1, P.R_MOD) for _ in range(n)]))[0]
    return pts, wire.points_compress(group, pts)


def _g1_rhs(x):
    return (x ** 3 + 4) % Q


def _g2_rhs(x0, x1):
    a0, a1 = (x0 * x0 - x1 * x1) % Q, 2 * x0 * x1 % Q
    return (a0 * x0 - a1 * x1 + 4) % Q, (a0 * x1 + a1 * x0 + 4) % Q


def _fq2_has_root(a0, a1):
    """a1 == 0 always has a root (a0 or -a0 is a residue); otherwise iff the norm is a residue"""
    return True if a1 == 0 else legendre(a0 * a0 + a1 * a1) == 1


def hostile(group, good, seed=5):
    """{name: (encoding, status the validating decoder gives)} from one good encoding of the group: every status from 1 to 5, x == q
    exactly, and for G2 the flag bits and a value >= q in the x.c0 half (only the first byte carries flags)."""
    from zksnark_finalproject_amd import wire
    from zksnark_finalproject_amd.device import point_check
    rng = random.Random(seed)
    size = SIZE[group]
    out = {}
    out["not_compressed"] = (bytes([good[0] & 0x7F]) + good[1:], 1)
    out["infinity_stray_byte"] = (bytes([0xC0]) + bytes(size - 2) + b"\x01", 2)
    out["infinity_with_sign"] = (bytes([0xE0]) + bytes(size - 1), 2)
    q_enc = bytearray(Q.to_bytes(48, "big"))
    q_enc[0] |= 0x80
    out["x_is_q"] = (bytes(q_enc) + (good[48:] if group == "g2" else b""), 3)
    top = bytearray((2 ** 381 - 1).to_bytes(48, "big"))
    top[0] |= 0x80
    out["x_all_ones"] = (bytes(top) + (good[48:] if group == "g2" else b""), 3)
    if group == "g2":
        out["c0_is_q"] = (good[:48] + Q.to_bytes(48, "big"), 3)
        for bit in (0x80, 0x40, 0x20):
            out["c0_flag_%02x" % bit] = (good[:48] + bytes([good[48] | bit]) + good[49:], 3)
    # seeded x values until one has no point, and one has a point outside the subgroup
    while "no_point" not in out or "outside_subgroup" not in out:
        if group == "g1":
            x = rng.randrange(Q)
            has = legendre(_g1_rhs(x)) >= 0
            enc = bytearray(x.to_bytes(48, "big"))
        else:
            x0, x1 = rng.randrange(Q), rng.randrange(Q)
            has = _fq2_has_root(*_g2_rhs(x0, x1))
            enc = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
        enc[0] |= 0x80 | (0x20 if rng.random() < 0.5 else 0)
        if not has:
            out.setdefault("no_point", (bytes(enc), 4))
        elif "outside_subgroup" not in out:
            pt, _ = (wire.g1_decompress if group == "g1" else wire.g2_decompress)(bytes(enc), validate=False)
            if not point_check(group, pt):
                out["outside_subgroup"] = (bytes(enc), 5)
    return out
