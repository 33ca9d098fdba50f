"""What checking an assignment against its R1CS costs on the device (GPU box).
   python tools/r1cs_check_timing.py [--runs 3] [--out profiles/r1cs_check_timing.txt]
Three legs, each the median of --runs rounds after a warm-up round, the sides of a leg alternated inside every round, with the
spread (min .. max):
  (1) zkg16_r1cs_check alone (one sparse product, the check kernel, one read-back of two words; wall ms per call) beside
      zkg16_bench_witness_map (the whole witness map, device ms per run) on the PrimeCircuit of (99, 4) and the 32x32 MatrixCircuit,
      with the device ms per launch of spmv_kernel and r1cs_check_kernel from the kernel timers;
  (2) zkg16_prime_check_batch beside zkg16_prove_prime_batch on the same K requests, K = 8 and 64 (wall ms per call);
  (3) zkg16_prove_resident and zkg16_prove_batch (K = 8) on the 32x32 MatrixCircuit with option "check_satisfied" off and on
      (wall ms per call; the same proof bytes, asserted).
Every verdict is compared with what the leg expects (satisfied assignments throughout, except the unsatisfied first-found
candidates among the prime requests, which leg (2) counts)."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from zksnark_finalproject_amd import Device, handlers
from zksnark_finalproject_amd.circuits import prime_dims, prime_search

NONE = (1 << 64) - 1


def wall_ms(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def med(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def rounds(sides, runs):
    """sides: name -> callable returning ms.  One warm-up round, then `runs` rounds with the sides in turn -> name -> [ms]"""
    got = {name: [] for name in sides}
    for r in range(runs + 1):
        for name, fn in sides.items():
            ms = fn()
            if r:
                got[name].append(ms)
    return got


def kernel_ms(dev, fn, names):
    dev.kernel_timing(True)
    dev.kernel_stats_reset()
    fn()
    out = {}
    for n in names:
        st = dev.kernel_stats(n)
        out[n] = st["ms"] / st["launches"] if st["launches"] else 0.0
    dev.kernel_timing(False)
    return out


def leg_single(dev, say, runs, title, rh, wh, nc, log_n):
    assert dev.r1cs_check(rh, wh) == (0, NONE)
    dev.r1cs_check(rh, wh)          # the handle's second use builds the dictionary and the row order
    got = rounds({"check": lambda: wall_ms(lambda: dev.r1cs_check(rh, wh), 10)[0],
                  "witness_map": lambda: dev.bench_witness_map(rh, wh, iters=10)}, runs)
    k = kernel_ms(dev, lambda: [dev.r1cs_check(rh, wh) for _ in range(10)], ("spmv_kernel", "r1cs_check_kernel"))
    say("%s: %d constraints, domain 2^%d" % (title, nc, log_n))
    say("  zkg16_r1cs_check, wall ms per call          %s" % med(got["check"]))
    say("  zkg16_bench_witness_map, device ms per run  %s" % med(got["witness_map"]))
    say("  device ms per launch: spmv_kernel %.4f, r1cs_check_kernel (with its two-word fill) %.4f" % (k["spmv_kernel"], k["r1cs_check_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_check_timing.txt"))
    a = ap.parse_args()
    dev = Device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("r1cs_check_timing: one MI355X, %d rounds after a warm-up, sides alternated; median (min .. max)" % a.runs)
    # ---- (1)
    say("(1) the check alone beside the witness map")
    d = prime_dims(4)
    rh, wh = dev.r1cs_prime(99, 4), dev.witness_prime(99, 4)
    leg_single(dev, say, a.runs, "PrimeCircuit (99, 4)", rh, wh, d["num_constraints"], (d["num_constraints"] + d["num_instance"] - 1).bit_length())
    dev.witness_free(wh)
    dev.r1cs_free(rh)
    n = 32
    rng = np.random.default_rng(32)
    shape = handlers._matrix_shape(dev, n)
    mats = rng.integers(0, 1 << 32, size=(2, 8, n, n), dtype=np.uint64)
    whs, _, _ = dev.witness_matrix_batch(mats[0], mats[1])
    leg_single(dev, say, a.runs, "MatrixCircuit 32x32", shape.rh, int(whs[0]), shape.num_constraints,
               (shape.num_constraints + shape.num_instance - 1).bit_length())
    # ---- (2)
    say("(2) zkg16_prime_check_batch beside zkg16_prove_prime_batch, wall ms per call")
    prng = random.Random(20260)
    key = handlers.prime_template_key(dev, prng)
    xs, js, x = [], [], 1000
    while len(xs) < 64:
        f = prime_search(x, 64)
        if f["found"]:
            xs.append(x)
            js.append(f["j"])
        x += 1
    xs, js = np.array(xs, dtype=np.uint64), np.array(js, dtype=np.uint64)
    for k in (8, 64):
        rs, ss = handlers._draw_rs_batch(prng, k)
        g0 = key["vk"]["gamma_abc_g1"][0]
        verdicts = dev.prime_check_batch(key["rh"], xs[:k], js[:k])
        got = rounds({"check": lambda: wall_ms(lambda: dev.prime_check_batch(key["rh"], xs[:k], js[:k]), 3)[0],
                      "prove": lambda: wall_ms(lambda: dev.prove_prime_batch(key["ph"], key["rh"], key["corr"], g0, xs[:k], js[:k], rs, ss,
                                                                             public_inputs=False), 3)[0]}, a.runs)
        assert dev.prime_check_batch(key["rh"], xs[:k], js[:k]) == verdicts
        say("  K = %-3d check %s   prove %s   (%d of the %d first-found candidates unsatisfied)"
            % (k, med(got["check"]), med(got["prove"]), sum(1 for v in verdicts if v[0]), k))
    dev.pk_free(key["ph"])
    dev.r1cs_free(key["rh"])
    # ---- (3)
    say("(3) option check_satisfied off / on, MatrixCircuit 32x32, wall ms per call")
    import bench
    trap, g1, g2 = bench.draw_key_inputs(7)
    ph, _ = dev.setup_resident(shape.rh, shape.num_instance, trap, g1, g2)
    rs, ss = handlers._draw_rs_batch(random.Random(3), 8)

    def side(value, fn, reps):
        def run():
            dev.set_option("check_satisfied", value)
            try:
                return wall_ms(fn, reps)[0]
            finally:
                dev.set_option("check_satisfied", 0)
        return run
    one = lambda: dev.prove_resident(ph, shape.rh, int(whs[0]), rs[0], ss[0])
    many = lambda: dev.prove_batch(ph, shape.rh, whs, rs, ss)
    ref_one, ref_many = one(), many()
    dev.set_option("check_satisfied", 1)
    on_one, on_many = one(), many()
    assert dev.last_check() == [(0, NONE)] * 8
    dev.set_option("check_satisfied", 0)
    assert np.array_equal(ref_one[0], on_one[0]) and np.array_equal(ref_many[0], on_many[0])
    got = rounds({"resident off": side(0, one, 10), "resident on": side(1, one, 10), "batch off": side(0, many, 3), "batch on": side(1, many, 3)}, a.runs)
    say("  zkg16_prove_resident     off %s   on %s" % (med(got["resident off"]), med(got["resident on"])))
    say("  zkg16_prove_batch K = 8  off %s   on %s" % (med(got["batch off"]), med(got["batch on"])))
    for w in whs:
        dev.witness_free(int(w))
    dev.pk_free(ph)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
