"""K linear-equation requests of one size: the batched request entry against the two per-request loops (GPU box).
   python tools/linear_batch_timing.py [--ns 8,32] [--ks 1,8,64] [--runs 3] [--out profiles/linear_batch_timing.txt]
Per (n, K), ms per request of
   batch entry     one Device.prove_linear_batch of K (zkg16_prove_linear_batch), with its timings_ms;
   handler loop    K calls of handlers.prove_linear_equations, the reference's shape: host solve + synthesis, circuit_load, a setup of
                   its own key, the proof, the verification, the key encodings, each time (its cost per request does not depend on K:
                   at most --loop-cap requests are run and the mean is reported);
   resident loop   host solve + synthesis + circuit_load + prove_resident per request on a key kept resident;
and, separately, of the assignment pass alone: Device.witness_linear_batch of K (upload, the solve and fill kernels, x read back, the
handles registered) against circuits.linear_solve_host of the K systems plus the host mirror (zkg16_circuit_linear, which solves once
more) per request — no upload on the host side.  The resident loop and the batch entry share one tabled key; the legs are alternated
in every round and the median of --runs rounds is reported with [min .. max].  Every batch is checked byte for byte against the
resident loop's proofs of the round.  The requests are lower-triangular (satisfied) systems of random 64-bit entries."""
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
from zksnark_finalproject_amd.circuits import linear_circuit_handle, linear_solve_host


def med(v):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))


def systems(n, k, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 1 << 63, size=(k, n, n), dtype=np.uint64)
    a *= np.tril(np.ones((n, n), dtype=np.uint64))
    b = rng.integers(0, 1 << 63, size=(k, n), dtype=np.uint64)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="8,32")
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=8, help="requests of the handler loop actually run per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_batch_timing.txt"))
    arg = ap.parse_args()
    ns = [int(v) for v in arg.ns.split(",")]
    ks = [int(v) for v in arg.ks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = Device(0)
    say("Linear equations, tabled key, %d rounds, legs alternated; ms per request: median [min .. max]" % arg.runs)
    say("n | K | batch entry (prove_linear_batch) | handler loop (prove_linear_equations, own key) | resident loop (solve + synthesis + "
        "circuit_load + prove_resident) | x handler loop | x resident loop | batch entry timings_ms per request: host checks / assignment "
        "passes / proving / whole call | assignment pass alone: device (witness_linear_batch: call, of which device) | host "
        "(linear_solve_host + mirror)")
    prng = np.random.default_rng(7)
    for n in ns:
        key = handlers.linear_key(dev, n, random.Random(0))
        ph, rh = key["ph"], key["rh"]
        dev.pk_precompute(ph, 0, 0)
        for k in ks:
            a, b = systems(n, k, 100 * n + k)
            rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            n_loop = min(k, arg.loop_cap)

            def resident(i):
                rh_i, wh_i = dev.circuit_load(linear_circuit_handle(a[i], b[i]))
                try:
                    return dev.prove_resident(ph, rh_i, wh_i, rs[i], ss[i])
                finally:
                    dev.witness_free(wh_i)
                    dev.r1cs_free(rh_i)

            def host_assign():
                linear_solve_host(a, b)
                for i in range(k):
                    linear_circuit_handle(a[i], b[i]).close()

            def dev_assign():
                whs, _, ms = dev.witness_linear_batch(a, b)
                for w in whs:
                    dev.witness_free(int(w))
                return ms
            # warm: workspaces of this K, the handler's path, the loop's path
            dev.prove_linear_batch(ph, rh, a, b, rs, ss)
            handlers.prove_linear_equations(dev, a[0], b[0])
            resident(0)
            dev_assign()
            loop, res, bat, parts, wdev, wdev_ms, whost = [], [], [], [], [], [], []
            ok = True
            for _ in range(arg.runs):
                t0 = time.perf_counter()
                proofs, inf, _, ms = dev.prove_linear_batch(ph, rh, a, b, rs, ss)
                bat.append((time.perf_counter() - t0) * 1e3 / k)
                parts.append([ms["host_check_ms"] / k, ms["witness_ms"] / k, ms["prove_ms"] / k, ms["call_ms"] / k])

                t0 = time.perf_counter()
                for i in range(n_loop):
                    handlers.prove_linear_equations(dev, a[i], b[i])
                loop.append((time.perf_counter() - t0) * 1e3 / n_loop)

                t0 = time.perf_counter()
                singles = [resident(i) for i in range(k)]
                res.append((time.perf_counter() - t0) * 1e3 / k)
                ok = ok and all(np.array_equal(proofs[i], singles[i][0]) and np.array_equal(inf[i], singles[i][1]) for i in range(k))

                t0 = time.perf_counter()
                ms = dev_assign()
                wdev.append((time.perf_counter() - t0) * 1e3 / k)
                wdev_ms.append(ms["device_ms"] / k)

                t0 = time.perf_counter()
                host_assign()
                whost.append((time.perf_counter() - t0) * 1e3 / k)
            mb = float(np.median(bat))
            pm = np.median(np.array(parts), axis=0)
            say("%d | %d | %s | %s | %s | %.1f | %.2f | %.4f / %.4f / %.4f / %.4f | %s, %.4f | %s%s" % (
                n, k, med(bat), med(loop), med(res), float(np.median(loop)) / mb, float(np.median(res)) / mb, pm[0], pm[1], pm[2], pm[3],
                med(wdev), float(np.median(wdev_ms)), med(whost), "" if ok else " | PROOFS DIFFER"))
            if n_loop < k:
                say("  (handler loop: %d of the %d requests run per round)" % (n_loop, k))
        dev.pk_free(ph)
        dev.r1cs_free(rh)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
