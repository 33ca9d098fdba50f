"""The linear route's two solvers on the same requests: forward substitution (option "linear_solver" = 0, the default) against
Gaussian elimination (1) (GPU box).
   python tools/linear_elim_timing.py [--ns 8,32,64] [--ks 1,8,64] [--runs 3] [--out profiles/linear_elim_timing.txt]
Per (n, K), ms per request of
   assignment pass   Device.witness_linear_batch of K (upload, the solve or elimination kernel, the fill kernel, x and the status words
                     read back, the handles registered) under either solver: the call, and of it the device part (timings_ms[1]);
   batch entry       Device.prove_linear_batch of K under either solver, on one tabled key;
   host              circuits.linear_solve_general_host of the K systems plus the general host mirror (zkg16_circuit_linear_general,
                     which eliminates once more) per request — no upload on the host side;
on LOWER-TRIANGULAR systems of random 64-bit entries, the only inputs both solvers accept (they give the same x, and the proofs of
the two batch entries are compared byte for byte in every round); and of the elimination's assignment pass on DENSE systems of the
same size, which the forward solver leaves unsatisfied.  The legs are alternated in every round and the median of --runs rounds is
reported with [min .. max]."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from zksnark_finalproject_amd import Device, handlers
from zksnark_finalproject_amd.circuits import linear_circuit_handle, linear_solve_general_host


def med(v):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))


def systems(n, k, seed, lower):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 1 << 63, size=(k, n, n), dtype=np.uint64)
    if lower:
        a *= np.tril(np.ones((n, n), dtype=np.uint64))
    b = rng.integers(0, 1 << 63, size=(k, n), dtype=np.uint64)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="8,32,64")
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_elim_timing.txt"))
    arg = ap.parse_args()
    ns = [int(v) for v in arg.ns.split(",")]
    ks = [int(v) for v in arg.ks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = Device(0)
    say("Linear equations, forward substitution (solver 0) against elimination (solver 1), tabled key, %d rounds, legs alternated; "
        "ms per request: median [min .. max]" % arg.runs)
    say("n | K | assignment pass, solver 0: call, of which device | assignment pass, solver 1: call, of which device | x (call 1 / call 0) | "
        "batch entry (prove_linear_batch), solver 0 | batch entry, solver 1 | x (1 / 0) | host (linear_solve_general_host + general "
        "mirror) | x (host / assignment pass 1) | assignment pass, solver 1, dense requests: call, of which device")
    prng = np.random.default_rng(7)
    for n in ns:
        key = handlers.linear_key(dev, n, random.Random(0))
        ph, rh = key["ph"], key["rh"]
        dev.pk_precompute(ph, 0, 0)
        for k in ks:
            a, b = systems(n, k, 100 * n + k, True)
            a_de, b_de = systems(n, k, 200 * n + k, False)
            x_de, st_de = linear_solve_general_host(a_de, b_de)
            if x_de is None:
                raise SystemExit("a dense system of size %d is singular mod r (status %s): pick another seed" % (n, list(st_de)))
            rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)

            def host_assign():
                linear_solve_general_host(a, b)
                for i in range(k):
                    linear_circuit_handle(a[i], b[i], solver="elimination").close()

            def dev_assign(aa, bb, solver):
                t0 = time.perf_counter()
                whs, x, ms = dev.witness_linear_batch(aa, bb, solver=solver)
                for w in whs:
                    dev.witness_free(int(w))
                return (time.perf_counter() - t0) * 1e3 / k, ms["device_ms"] / k, x

            def prove(solver):
                t0 = time.perf_counter()
                proofs, inf, _, _ = dev.prove_linear_batch(ph, rh, a, b, rs, ss, solver=solver)
                return (time.perf_counter() - t0) * 1e3 / k, proofs, inf
            # warm: workspaces of this K, both kernels
            for solver in ("forward", "elimination"):
                prove(solver)
                dev_assign(a, b, solver)
            w0, w0d, w1, w1d, p0, p1, wh, wd, wdd = ([] for _ in range(9))
            ok = True
            for _ in range(arg.runs):
                t, d, x0 = dev_assign(a, b, "forward")
                w0.append(t); w0d.append(d)
                t, d, x1 = dev_assign(a, b, "elimination")
                w1.append(t); w1d.append(d)
                t, proofs0, inf0 = prove("forward")
                p0.append(t)
                t, proofs1, inf1 = prove("elimination")
                p1.append(t)
                t0 = time.perf_counter()
                host_assign()
                wh.append((time.perf_counter() - t0) * 1e3 / k)
                t, d, xd = dev_assign(a_de, b_de, "elimination")
                wd.append(t); wdd.append(d)
                ok = ok and np.array_equal(x0, x1) and np.array_equal(proofs0, proofs1) and np.array_equal(inf0, inf1) and np.array_equal(xd, x_de)
            m = lambda v: float(np.median(v))
            say("%d | %d | %s, %.4f | %s, %.4f | %.2f | %s | %s | %.2f | %s | %.2f | %s, %.4f%s" % (
                n, k, med(w0), m(w0d), med(w1), m(w1d), m(w1) / m(w0), med(p0), med(p1), m(p1) / m(p0), med(wh), m(wh) / m(w1),
                med(wd), m(wdd), "" if ok else " | RESULTS DIFFER"))
        dev.pk_free(ph)
        dev.r1cs_free(rh)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
