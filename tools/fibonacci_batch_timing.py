"""K Fibonacci requests of one round count: the batched request entry against the two per-request loops (GPU box).
   python tools/fibonacci_batch_timing.py [--steps 1000] [--ks 1,8,64,1024] [--runs 3] [--out profiles/fibonacci_batch_timing.txt]
Per K, ms per request of
   handler loop    K calls of handlers.prove_fibonacci: host synthesis, circuit_load, a setup, the proof, the key encodings, each time
                   (its cost per request does not depend on K: at most --loop-cap requests are run and the mean is reported);
   resident loop   the same loop with the key kept resident: host synthesis + circuit_load + prove_resident per request;
   batch entry     one Device.prove_fibonacci_batch of K (zkg16_prove_fibonacci_batch), with its timings_ms;
   prove_batch     one Device.prove_batch of K on witness handles built beforehand: what DESIGN 2.8 measures, for the same key and K.
The resident loop, the batch entry and prove_batch share one tabled key; the legs are alternated in every round and the median of
--runs rounds is reported with [min .. max].  Every batch is checked byte for byte against the resident loop's proofs of the round."""
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
from zksnark_finalproject_amd.circuits import fibonacci_circuit_handle


def med(v):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--ks", default="1,8,64,1024")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=64, help="requests of the handler loop actually run per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fibonacci_batch_timing.txt"))
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = Device(0)
    steps = a.steps
    key = handlers.fibonacci_key(dev, steps, random.Random(42))
    ph, rh = key["ph"], key["rh"]
    dev.pk_precompute(ph, 0, 0)
    say("Fibonacci-%d, tabled key, %d rounds, legs alternated; ms per request: median [min .. max]" % (steps, a.runs))
    say("K | handler loop (prove_fibonacci) | resident loop (synthesis + circuit_load + prove_resident) | batch entry (prove_fibonacci_batch) | "
        "prove_batch on handles built beforehand | x handler loop | x resident loop | batch entry timings_ms per request: coefficients / "
        "assignment passes / proving / whole call")
    rng = np.random.default_rng(1)
    prng = np.random.default_rng(7)
    for k in ks:
        ab = rng.integers(0, 1 << 63, size=(k, 2), dtype=np.uint64)
        av, bv = np.ascontiguousarray(ab[:, 0]), np.ascontiguousarray(ab[:, 1])
        rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
        ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
        n_loop = min(k, a.loop_cap)

        def resident(i):
            rh_i, wh_i = dev.circuit_load(fibonacci_circuit_handle(int(av[i]), int(bv[i]), steps))
            try:
                return dev.prove_resident(ph, rh_i, wh_i, rs[i], ss[i])
            finally:
                dev.witness_free(wh_i)
                dev.r1cs_free(rh_i)
        # warm: workspaces of this K, the handler's path, the loop's path
        dev.prove_fibonacci_batch(ph, rh, steps, av, bv, rs, ss)
        handlers.prove_fibonacci(dev, int(av[0]), int(bv[0]), steps)
        resident(0)
        whs, _, _ = dev.witness_fibonacci_batch(steps, av, bv)
        dev.prove_batch(ph, rh, whs, rs, ss)
        loop, res, bat, pre, parts = [], [], [], [], []
        ok = True
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for i in range(n_loop):
                handlers.prove_fibonacci(dev, int(av[i]), int(bv[i]), steps)
            loop.append((time.perf_counter() - t0) * 1e3 / n_loop)

            t0 = time.perf_counter()
            singles = [resident(i) for i in range(k)]
            res.append((time.perf_counter() - t0) * 1e3 / k)

            t0 = time.perf_counter()
            proofs, inf, _, ms = dev.prove_fibonacci_batch(ph, rh, steps, av, bv, rs, ss)
            bat.append((time.perf_counter() - t0) * 1e3 / k)
            parts.append([ms["host_coeffs_ms"] / k, ms["witness_ms"] / k, ms["prove_ms"] / k, ms["call_ms"] / k])
            ok = ok and all(np.array_equal(proofs[i], singles[i][0]) and np.array_equal(inf[i], singles[i][1]) for i in range(k))

            t0 = time.perf_counter()
            dev.prove_batch(ph, rh, whs, rs, ss)
            pre.append((time.perf_counter() - t0) * 1e3 / k)
        for w in whs:
            dev.witness_free(int(w))
        mb = float(np.median(bat))
        pm = np.median(np.array(parts), axis=0)
        say("%d | %s | %s | %s | %s | %.1f | %.2f | %.4f / %.4f / %.4f / %.4f%s" % (
            k, med(loop), med(res), med(bat), med(pre), float(np.median(loop)) / mb, float(np.median(res)) / mb, pm[0], pm[1], pm[2], pm[3],
            "" if ok else " | PROOFS DIFFER"))
        if n_loop < k:
            say("  (handler loop: %d of the %d requests run per round)" % (n_loop, k))
    dev.pk_free(ph)
    dev.r1cs_free(rh)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
