"""Batched verification against the single-proof verifier, on Fibonacci-1000 proofs from zkg16_prove_batch (GPU box).
   python tools/verify_batch_timing.py [--ks 1,8,64,...] [--runs 3] [--out profiles/verify_batch_timing_r8.txt]
For every K, ms per proof of
  (a) a loop of zkg16_verify_prepared on one thread — the single-proof verifier, the baseline;
  (b) zkg16_verify_batch_host on 1 thread and on 8 threads;
  (c) zkg16_verify_batch (kernels on the ctx; option verify_batch_min = 1 so that every K runs them) with its
      zkg16_verify_batch_timings breakdown;
the median of --runs rounds with the four alternated in every round, and the spread (min .. max) of the rounds.  One more line:
K = 1024 with a single bad proof and per-proof flags asked for (what bisecting costs).  Every verdict is checked.  The last
lines set verify-batch proofs/s beside the prove-batch proofs/s of profiles/batch_timing_r7.txt."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from zksnark_finalproject_amd import Device
from zksnark_finalproject_amd.device import draw_rho, pvk_prepare, scalar_mul, verify_batch_host

DISTINCT = 8


def make_proofs(dev, kmax):
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    trap, g1, g2 = bench.draw_key_inputs(42)
    rng = np.random.default_rng(1)
    cs = [fibonacci_circuit(int(a), int(b), 1000) for a, b in rng.integers(0, 1 << 20, size=(DISTINCT, 2))]
    rh = dev.r1cs_load(cs[0].r1cs, cs[0].num_vars)
    ph, vk = dev.setup_resident(rh, cs[0].num_instance, trap, g1, g2)
    dev.pk_precompute(ph, 0, 0)
    pool = np.array([dev.witness_load(c.z) for c in cs], dtype=np.uint64)
    whs = np.resize(pool, kmax)
    prng = np.random.default_rng(7)
    rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=kmax)]).reshape(kmax, 4)
    ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=kmax)]).reshape(kmax, 4)
    t0 = time.perf_counter()
    proofs, infs = dev.prove_batch(ph, rh, whs, rs, ss)
    prove_ms = (time.perf_counter() - t0) * 1e3 / kmax
    pubs = np.array([cs[i % DISTINCT].public_inputs for i in range(kmax)], dtype=np.uint64).reshape(kmax, -1, 4)
    for w in pool:
        dev.witness_free(int(w))
    dev.pk_free(ph)
    dev.r1cs_free(rh)
    return pvk_prepare(vk), pubs, proofs, infs, prove_ms


def loop_single(lib, pvk, pubs, proofs, infs):
    """zkg16_verify_prepared proof by proof, arguments prepared outside the timed loop"""
    gabc = np.ascontiguousarray(pvk["gamma_abc_g1"], dtype=np.uint64).reshape(-1, 12)
    g = np.ascontiguousarray(pvk["gamma_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    d = np.ascontiguousarray(pvk["delta_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    ab = np.ascontiguousarray(pvk["alpha_beta"], dtype=np.uint64)
    ok = C.c_int(0)
    good = 0
    t0 = time.perf_counter()
    for i in range(proofs.shape[0]):
        lib.zkg16_verify_prepared(gabc, gabc.shape[0], pubs[i].ctypes.data, ab, g, d, g.shape[0], proofs[i], infs[i], C.byref(ok))
        good += ok.value
    return (time.perf_counter() - t0) * 1e3, good == proofs.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,8,64,256,1024,4096,16384")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_timing_r8.txt"))
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    dev = Device(0)
    dev.set_option("verify_batch_min", 1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    pvk, pubs, proofs, infs, prove_ms = make_proofs(dev, max(ks + [1024]))
    say("Fibonacci-1000 proofs from zkg16_prove_batch (%d made, %.3f ms per proof in that one call); median of %d rounds [min .. max], methods alternated" %
        (proofs.shape[0], prove_ms, a.runs))
    say("K | (a) verify_prepared loop, 1 thread ms/proof | (b) batch_host 1 thread | (b) batch_host 8 threads | (c) verify_batch device | "
        "(c) breakdown ms per call: membership, scaling+Miller, product, MSM, host equation, bisect, total | (c) proofs/s | a/b1 | b8/c")
    res = {}
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))
    for k in ks:
        p, f, z = proofs[:k], infs[:k], pubs[:k]
        rho = draw_rho(k)
        assert dev.verify_batch(pvk, z, p, f, rho=rho) is True                  # warm: buffers of this K, code objects
        assert verify_batch_host(pvk, z, p, f, rho=rho, threads=8) is True
        ta, tb1, tb8, tc, brk = [], [], [], [], []
        for _ in range(a.runs):
            ms, ok = loop_single(dev.lib, pvk, z, p, f)
            assert ok
            ta.append(ms / k)
            t0 = time.perf_counter()
            assert verify_batch_host(pvk, z, p, f, rho=rho, threads=1) is True
            tb1.append((time.perf_counter() - t0) * 1e3 / k)
            t0 = time.perf_counter()
            assert verify_batch_host(pvk, z, p, f, rho=rho, threads=8) is True
            tb8.append((time.perf_counter() - t0) * 1e3 / k)
            t0 = time.perf_counter()
            assert dev.verify_batch(pvk, z, p, f, rho=rho) is True
            tc.append((time.perf_counter() - t0) * 1e3 / k)
            t = dev.verify_batch_timings()
            assert t["host_form"] == 0
            brk.append([t[n] for n in ("membership_ms", "miller_ms", "product_ms", "msm_ms", "host_ms", "bisect_ms", "total_ms")])
        b = np.median(np.array(brk), axis=0)
        res[k] = (ta, tb1, tb8, tc)
        say("%d | %s | %s | %s | %s | %s | %.0f | %.2f | %.2f" % (k, fmt(ta), fmt(tb1), fmt(tb8), fmt(tc), ", ".join("%.2f" % v for v in b),
                                                                1e3 / np.median(tc), np.median(ta) / np.median(tb1), np.median(tb8) / np.median(tc)))
    # one bad proof at K = 1024, per-proof flags wanted
    k = 1024
    p, f, z = proofs[:k].copy(), infs[:k], pubs[:k]
    p[700, 36:48] = scalar_mul("g1", p[700, 36:48], np.array([2, 0, 0, 0], dtype=np.uint64))[0]      # 2 C: still in the subgroup, so only the equation tells
    want = np.ones(k, dtype=bool)
    want[700] = False
    rho = draw_rho(k)
    rows = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        ok, each = verify_batch_host(pvk, z, p, f, rho=rho, each=True, threads=8)
        th = (time.perf_counter() - t0) * 1e3
        assert ok is False
        flagged = np.flatnonzero(~each)
        t0 = time.perf_counter()
        okd, eachd = dev.verify_batch(pvk, z, p, f, rho=rho, each=True)
        td = (time.perf_counter() - t0) * 1e3
        assert okd is False and np.array_equal(each, eachd)
        t = dev.verify_batch_timings()
        rows.append((th, td, t["bisect_ms"]))
    assert list(flagged) == [700], flagged
    r = np.median(np.array(rows), axis=0)
    say("K = 1024, one bad proof (C doubled: it passes membership), per-proof flags: batch_host 8 threads %.2f ms per call, verify_batch %.2f ms per call "
        "(bisecting %.2f ms of it); flagged: %s" % (r[0], r[1], r[2], [int(i) for i in flagged]))
    # the comparison that motivates the work
    prove = None
    try:
        with open(os.path.join(ROOT, "profiles", "batch_timing_r7.txt")) as fh:
            for line in fh:
                c = [x.strip() for x in line.split("|")]
                if c[0] == "Fibonacci-1000" and c[1] == "64":
                    prove = float(c[5])
    except OSError:
        pass
    for k in (64, 1024):
        if k in res:
            ta, tb1, tb8, tc = res[k]
            say("K = %d: verify_batch %.0f proofs/s, batch_host on 8 threads %.0f proofs/s, verify_prepared loop %.0f proofs/s; prove_batch of Fibonacci-1000 "
                "at K = 64 (profiles/batch_timing_r7.txt): %s proofs/s" % (k, 1e3 / np.median(tc), 1e3 / np.median(tb8), 1e3 / np.median(ta),
                                                                         "%.0f" % prove if prove else "not found"))
    wins = [k for k in ks if k in res and max(res[k][3]) < min(res[k][2])]
    say("verify_batch beats batch_host on 8 threads in every round (max of (c) below min of (b8)) at K = %s; smallest: %s" % (wins, wins[0] if wins else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
