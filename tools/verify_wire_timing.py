"""Batched verification from wire bytes: where the decoding should happen, on Fibonacci-1000 proofs from zkg16_prove_batch (GPU box).
   python tools/verify_wire_timing.py [--ks 8,64,...] [--runs 3] [--out profiles/verify_wire_timing_r9.txt]
The proofs start as they travel (192 compressed bytes each; base64 is outside every timed section).  For every K, ms per proof of
  (a) the per-proof route of handlers.verify_proofs before zkg16_verify_batch_wire: a Python loop of wire.proof_deserialize_compressed,
      then zkg16_verify_batch;
  (b) whole-batch host decode (g1_decompress_many for A and C, g2_decompress_many for B) + zkg16_verify_batch_host on 8 threads;
  (c) the same whole-batch host decode + zkg16_verify_batch;
  (d) zkg16_verify_batch_wire, with the decode kernels' ms beside the Miller kernel's (zkg16_verify_batch_timings);
the median of --runs rounds with the four alternated in every round, and the spread (min .. max) of the rounds.  Options
verify_batch_min = verify_wire_min = 1, so that every K runs the kernels.  Every verdict is checked."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from verify_batch_timing import make_proofs
from zksnark_finalproject_amd import Device, wire
from zksnark_finalproject_amd.device import draw_rho, verify_batch_host


def to_wire(proofs, infs):
    k = proofs.shape[0]
    a = np.frombuffer(wire.points_compress("g1", proofs[:, 0:12], infs[:, 0]), dtype=np.uint8).reshape(k, 48)
    b = np.frombuffer(wire.points_compress("g2", proofs[:, 12:36], infs[:, 1]), dtype=np.uint8).reshape(k, 96)
    c = np.frombuffer(wire.points_compress("g1", proofs[:, 36:48], infs[:, 2]), dtype=np.uint8).reshape(k, 48)
    return np.ascontiguousarray(np.concatenate([a, b, c], axis=1))


def decode_loop(raw):
    """what verify_proofs did per entry"""
    out = [wire.proof_deserialize_compressed(raw[i].tobytes()) for i in range(raw.shape[0])]
    return np.array([p for p, _ in out], dtype=np.uint64), np.array([f for _, f in out], dtype=np.uint8)


def decode_whole(raw):
    k = raw.shape[0]
    ac, iac = wire.g1_decompress_many(np.ascontiguousarray(raw[:, [*range(0, 48), *range(144, 192)]]).tobytes(), 2 * k)
    bb, ib = wire.g2_decompress_many(np.ascontiguousarray(raw[:, 48:144]).tobytes(), k)
    ac, iac = ac.reshape(k, 2, 12), iac.reshape(k, 2)
    return (np.ascontiguousarray(np.concatenate([ac[:, 0], bb, ac[:, 1]], axis=1)),
            np.ascontiguousarray(np.stack([iac[:, 0], ib, iac[:, 1]], axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="8,64,256,1024,4096,16384")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_wire_timing_r9.txt"))
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    dev = Device(0)
    dev.set_option("verify_batch_min", 1)
    dev.set_option("verify_wire_min", 1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    pvk, pubs, proofs, infs, prove_ms = make_proofs(dev, max(ks))
    raw_all = to_wire(proofs, infs)
    say("Fibonacci-1000 proofs from zkg16_prove_batch (%d made, %.3f ms per proof in that one call), compressed to 192 bytes each; median of %d rounds "
        "[min .. max], methods alternated" % (proofs.shape[0], prove_ms, a.runs))
    say("K | (a) per-proof decode loop + verify_batch ms/proof | (a) its decode share | (b) whole-batch host decode + batch_host 8 threads | "
        "(b, c) the host decode alone | (c) whole-batch host decode + verify_batch | (d) verify_batch_wire | (d) decode kernels ms per call | "
        "(d) scaling+Miller kernel ms per call | (d) total ms per call | (d) proofs/s from bytes | best of (b, c) / (d)")
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))
    res = {}
    for k in ks:
        raw, z = np.ascontiguousarray(raw_all[:k]), pubs[:k]
        rho = draw_rho(k)
        assert dev.verify_batch_wire(pvk, z, raw, rho=rho) is True                # warm: buffers of this K, code objects
        p, f = decode_whole(raw)
        assert np.array_equal(p, proofs[:k]) and np.array_equal(f, infs[:k])
        assert dev.verify_batch(pvk, z, p, f, rho=rho) is True
        ta, tad, tb, th, tc, td, dec, mil, tot = [], [], [], [], [], [], [], [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            p, f = decode_loop(raw)
            t1 = time.perf_counter()
            assert dev.verify_batch(pvk, z, p, f, rho=rho) is True
            ta.append((time.perf_counter() - t0) * 1e3 / k)
            tad.append((t1 - t0) * 1e3 / k)
            t0 = time.perf_counter()
            p, f = decode_whole(raw)
            t1 = time.perf_counter()
            assert verify_batch_host(pvk, z, p, f, rho=rho, threads=8) is True
            tb.append((time.perf_counter() - t0) * 1e3 / k)
            th.append((t1 - t0) * 1e3 / k)
            t0 = time.perf_counter()
            p, f = decode_whole(raw)
            assert dev.verify_batch(pvk, z, p, f, rho=rho) is True
            tc.append((time.perf_counter() - t0) * 1e3 / k)
            t0 = time.perf_counter()
            assert dev.verify_batch_wire(pvk, z, raw, rho=rho) is True
            td.append((time.perf_counter() - t0) * 1e3 / k)
            t = dev.verify_batch_timings()
            assert t["host_form"] == 0
            dec.append(t["decode_ms"])
            mil.append(t["miller_ms"])
            tot.append(t["total_ms"])
        res[k] = (tb, tc, td)
        best = min(np.median(tb), np.median(tc))
        say("%d | %s | %.4f | %s | %.4f | %s | %s | %.2f | %.2f | %.2f | %.0f | %.2f" %
            (k, fmt(ta), np.median(tad), fmt(tb), np.median(th), fmt(tc), fmt(td), np.median(dec), np.median(mil), np.median(tot), 1e3 / np.median(td),
             best / np.median(td)))
    wins = [k for k in ks if max(res[k][2]) < min(min(res[k][0]), min(res[k][1]))]
    say("verify_batch_wire beats the best of (b) and (c) in every round (max of (d) below the min of both) at K = %s; smallest: %s" %
        (wins, wins[0] if wins else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
