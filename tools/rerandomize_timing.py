"""Re-randomising proofs: the device forms against the host form and against what a caller had before, on Fibonacci-1000 proofs from
zkg16_prove_batch (GPU box).
   python tools/rerandomize_timing.py [--ks 1,8,64,...] [--runs 3] [--out profiles/rerandomize_timing.txt]
For every K, ms per proof of
  (1) a loop of host decode (zkg16_g1 / g2_decompress, validating), four zkg16_scalar_mul_* calls and host encode
      (zkg16_points_compress) on one thread — the baseline a caller has today; it lacks the two point additions (the ABI has none
      on the host), so it is a lower bound of that route;
  (2) zkg16_rerandomize_batch_host on 1 thread and on 8 threads;
  (3) zkg16_rerandomize_batch on limbs (option rerandomize_min = 1 so that every K runs the kernels);
  (4) zkg16_rerandomize_batch_wire from bytes to bytes, with the zkg16_rerandomize_timings split;
the median of --runs rounds with the routes alternated in every round, and the spread (min .. max).  The host routes cost the same
per proof at every K, so (1) and (2) on one thread are timed on at most --cap1 proofs of a batch and (2) on eight threads on at
most --cap8; the device routes always take the whole batch.  Every result is checked against the host form's.  The last line is the
default of rerandomize_min the table gives: the smallest K at which both device forms beat the host form on eight threads in every
round (max of the device rounds below min of the host rounds)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from verify_batch_timing import make_proofs
from zksnark_finalproject_amd import Device, wire
from zksnark_finalproject_amd.device import draw_rerandomizers, rerandomize_batch_host

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def limbs4(v):
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


def canonical(mont_rows):
    inv = pow(1 << 256, -1, R)
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) * inv % R for row in mont_rows]


def loop_baseline(lib, delta, raw, r1, r2):
    """decode, four scalar multiplications, encode, proof by proof; the scalars are prepared outside the timed loop"""
    n = raw.shape[0]
    c1, c2 = canonical(r1[:n]), canonical(r2[:n])
    ks = [(limbs4(pow(a, -1, R)), limbs4(b), limbs4(a), limbs4(a * b % R)) for a, b in zip(c1, c2)]
    pa, pb, pc = np.zeros(12, np.uint64), np.zeros(24, np.uint64), np.zeros(12, np.uint64)
    oa, ob, od, oc = np.zeros(12, np.uint64), np.zeros(24, np.uint64), np.zeros(24, np.uint64), np.zeros(12, np.uint64)
    fl, st, inf = np.zeros(1, np.uint8), C.c_int(0), C.c_uint8(0)
    out = np.zeros(192, np.uint8)
    t0 = time.perf_counter()
    for i in range(n):
        b = raw[i]
        lib.zkg16_g1_decompress(b[0:48].ctypes.data, 1, pa.ctypes.data, fl.ctypes.data, 1, C.byref(st))
        lib.zkg16_g2_decompress(b[48:144].ctypes.data, 1, pb.ctypes.data, fl.ctypes.data, 1, C.byref(st))
        lib.zkg16_g1_decompress(b[144:192].ctypes.data, 1, pc.ctypes.data, fl.ctypes.data, 1, C.byref(st))
        k = ks[i]
        lib.zkg16_scalar_mul_g1(pa, k[0], oa, C.byref(inf))
        lib.zkg16_scalar_mul_g1(pa, k[1], oc, C.byref(inf))
        lib.zkg16_scalar_mul_g2(pb, k[2], ob, C.byref(inf))
        lib.zkg16_scalar_mul_g2(delta, k[3], od, C.byref(inf))
        lib.zkg16_points_compress(1, oa.ctypes.data, None, 1, out[0:48].ctypes.data)
        lib.zkg16_points_compress(2, ob.ctypes.data, None, 1, out[48:144].ctypes.data)
        lib.zkg16_points_compress(1, oc.ctypes.data, None, 1, out[144:192].ctypes.data)
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,64,256,1024,4096,16384")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cap1", type=int, default=128)
    ap.add_argument("--cap8", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerandomize_timing.txt"))
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    dev = Device(0)
    dev.set_option("rerandomize_min", 1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    pvk, pubs, proofs, infs, prove_ms = make_proofs(dev, max(ks))
    delta = np.ascontiguousarray(pvk["delta_g2"], dtype=np.uint64).reshape(24)
    say("Fibonacci-1000 proofs from zkg16_prove_batch (%d made, %.3f ms per proof in that one call); median of %d rounds [min .. max], routes alternated; "
        "host routes on one thread timed on at most %d proofs of a batch, on eight threads on at most %d" % (proofs.shape[0], prove_ms, a.runs, a.cap1, a.cap8))
    say("K | (1) decode + 4 scalar_mul + encode loop, 1 thread ms/proof | (2) batch_host 1 thread | (2) batch_host 8 threads | (3) rerandomize_batch device | "
        "(4) rerandomize_batch_wire device | (4) split ms per call: upload, decode+membership, G1 kernel, G2 kernel, compress, read-back, total | h8/(3) | h8/(4)")
    res = {}
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))
    for k in ks:
        p, f = proofs[:k], infs[:k]
        raw = np.frombuffer(b"".join(wire.proof_serialize_compressed(p[i], f[i]) for i in range(k)), dtype=np.uint8).reshape(k, 192).copy()
        r1, r2 = draw_rerandomizers(k), draw_rerandomizers(k)
        n1, n8 = min(k, a.cap1), min(k, a.cap8)
        want, want_inf = rerandomize_batch_host(delta, p[:n8], f[:n8], r1[:n8], r2[:n8], threads=8)          # warm, and the reference
        out, oinf = dev.rerandomize_batch(delta, p, f, r1, r2)                                               # warm: buffers of this K, code objects
        assert np.array_equal(out[:n8], want) and np.array_equal(oinf[:n8], want_inf)
        t1, th1, th8, t3, t4, brk = [], [], [], [], [], []
        for _ in range(a.runs):
            t1.append(loop_baseline(dev.lib, delta, raw[:n1], r1, r2))
            t0 = time.perf_counter()
            rerandomize_batch_host(delta, p[:n1], f[:n1], r1[:n1], r2[:n1], threads=1)
            th1.append((time.perf_counter() - t0) * 1e3 / n1)
            t0 = time.perf_counter()
            rerandomize_batch_host(delta, p[:n8], f[:n8], r1[:n8], r2[:n8], threads=8)
            th8.append((time.perf_counter() - t0) * 1e3 / n8)
            t0 = time.perf_counter()
            out, oinf = dev.rerandomize_batch(delta, p, f, r1, r2)
            t3.append((time.perf_counter() - t0) * 1e3 / k)
            assert dev.rerandomize_timings()["host_form"] == 0
            t0 = time.perf_counter()
            new, st = dev.rerandomize_batch_wire(delta, raw, r1, r2)
            t4.append((time.perf_counter() - t0) * 1e3 / k)
            t = dev.rerandomize_timings()
            assert t["host_form"] == 0 and not st.any()
            brk.append([t[n] for n in ("upload_ms", "decode_ms", "g1_ms", "g2_ms", "compress_ms", "readback_ms", "total_ms")])
        assert np.array_equal(out[:n8], want) and np.array_equal(oinf[:n8], want_inf)
        assert new[:n1].tobytes() == b"".join(wire.proof_serialize_compressed(want[i], want_inf[i]) for i in range(n1))
        b = np.median(np.array(brk), axis=0)
        res[k] = (th8, t3, t4)
        say("%d | %s | %s | %s | %s | %s | %s | %.2f | %.2f" % (k, fmt(t1), fmt(th1), fmt(th8), fmt(t3), fmt(t4), ", ".join("%.2f" % v for v in b),
                                                                np.median(th8) / np.median(t3), np.median(th8) / np.median(t4)))
    wins = [k for k in ks if max(res[k][1]) < min(res[k][0]) and max(res[k][2]) < min(res[k][0])]
    # a default must hold from its K on: the smallest K from which every larger measured K wins too
    first = None
    for k in reversed(ks):
        if k in wins:
            first = k
        else:
            break
    say("both device forms beat batch_host on 8 threads in every round (max of (3) and of (4) below min of (2) on 8 threads) at K = %s; "
        "default of rerandomize_min from this table: %s" % (wins, first if first else "never"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
