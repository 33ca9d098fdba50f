"""zkg16_prove_batch against one caller and two callers on one ctx, per shape, on tabled resident keys (GPU box).
   python tools/batch_timing.py [shape ...] [--ks 1,2,4,...] [--runs 3]      shapes: fib1000 8 16 prime 32 46 (matrix n)
For every shape and K: ms per proof of one caller proving K proofs in turn (zkg16_prove_resident), of two threads proving K/2
each on one ctx (two lanes), and of one zkg16_prove_batch of K; the median of --runs rounds, the three alternated in every
round.  Every batch is checked byte for byte against the single proofs of the round."""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from zksnark_finalproject_amd import Device

DISTINCT = 8            # distinct assignments per shape (cycled to K)


def shape_setup(dev, shape, tables=True):
    """-> (description, r1cs handle, pk handle, witness handles)"""
    trap, g1, g2 = bench.draw_key_inputs(42)
    rng = np.random.default_rng(1)
    if shape.isdigit():
        n = int(shape)
        rh = dev.r1cs_matrix(n)
        ph, _ = dev.setup_resident(rh, 4, trap, g1, g2)
        whs = [dev.witness_matrix(rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64),
                                  rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64))[0] for _ in range(DISTINCT)]
        desc = "matrix %dx%d" % (n, n)
    elif shape.startswith("fib"):
        from zksnark_finalproject_amd.circuits import fibonacci_circuit
        steps = int(shape[3:])
        cs = [fibonacci_circuit(int(a), int(b), steps) for a, b in rng.integers(0, 1 << 20, size=(DISTINCT, 2))]
        rh = dev.r1cs_load(cs[0].r1cs, cs[0].num_vars)
        ph, _ = dev.setup_resident(rh, cs[0].num_instance, trap, g1, g2)
        whs = [dev.witness_load(c.z) for c in cs]
        desc = "Fibonacci-%d" % steps
    elif shape == "prime":
        from zksnark_finalproject_amd.circuits import prime_circuit
        c = prime_circuit(0x123456789ABCDEF, 32)
        rh = dev.r1cs_load(c.r1cs, c.num_vars)
        ph, _ = dev.setup_resident(rh, c.num_instance, trap, g1, g2)
        whs = [dev.witness_load(c.z) for _ in range(DISTINCT)]
        desc = "PrimeCircuit (one assignment x 8)"
    else:
        raise SystemExit("unknown shape " + shape)
    if tables:
        dev.pk_precompute(ph, 0, 0)
    return desc, rh, ph, np.array(whs, dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["fib1000", "8", "16", "prime", "32", "46"])
    ap.add_argument("--ks", default="1,2,4,8,16,32,64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-proofs", type=int, default=0, help="skip K above this (0: none)")
    ap.add_argument("--reduce-modes", action="store_true",
                    help="instead: the batch alone with option reduce_mode 0 (default), 5 (bit-sliced wherever it applies), 6 (never), "
                         "alternated, plain key and tabled key")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    dev = Device(0)
    dev.set_option("lanes", 2)
    print("shape | K | one caller ms/proof | two callers ms/proof | batch ms/proof | batch proofs/s | x one caller | x two callers", flush=True)
    if a.reduce_modes:
        return reduce_modes(dev, a, ks)
    for shape in a.shapes:
        desc, rh, ph, pool = shape_setup(dev, shape)
        prng = np.random.default_rng(7)
        for k in ks:
            if a.max_proofs and k > a.max_proofs:
                continue
            whs = np.resize(pool, k)
            rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            dev.prove_batch(ph, rh, whs, rs, ss)                       # warm: workspaces of this K
            dev.prove_resident(ph, rh, int(whs[0]), rs[0], ss[0])
            one, two, bat = [], [], []
            ok = True
            for _ in range(a.runs):
                t0 = time.perf_counter()
                singles = [dev.prove_resident(ph, rh, int(whs[i]), rs[i], ss[i]) for i in range(k)]
                one.append((time.perf_counter() - t0) * 1e3 / k)

                def half(lo, hi):
                    for i in range(lo, hi):
                        dev.prove_resident(ph, rh, int(whs[i]), rs[i], ss[i])
                ts = [threading.Thread(target=half, args=(0, (k + 1) // 2)), threading.Thread(target=half, args=((k + 1) // 2, k))]
                t0 = time.perf_counter()
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                two.append((time.perf_counter() - t0) * 1e3 / k)

                t0 = time.perf_counter()
                proofs, inf = dev.prove_batch(ph, rh, whs, rs, ss)
                bat.append((time.perf_counter() - t0) * 1e3 / k)
                ok = ok and all(np.array_equal(proofs[i], singles[i][0]) and np.array_equal(inf[i], singles[i][1]) for i in range(k))
            m1, m2, mb = (float(np.median(v)) for v in (one, two, bat))
            print("%s | %d | %.3f | %.3f | %.3f | %.0f | %.2f | %.2f%s" % (desc, k, m1, m2, mb, 1e3 / mb, m1 / mb, m2 / mb,
                  "" if ok else " | PROOFS DIFFER"), flush=True)
        for w in set(int(w) for w in pool):
            dev.witness_free(w)
        dev.pk_free(ph)
        dev.r1cs_free(rh)
    dev.close()


def reduce_modes(dev, a, ks):
    """ms per proof of the batch with the reduction forms the bit-sliced caps choose between (plain key, then tabled)."""
    print("shape | key | K | default ms/proof | bit-sliced (5) | work-efficient (6)", flush=True)
    for shape in a.shapes:
        desc, rh, ph, pool = shape_setup(dev, shape, tables=False)
        for key in ("plain", "tabled"):
            if key == "tabled":
                dev.pk_precompute(ph, 0, 0)
            prng = np.random.default_rng(7)
            for k in ks:
                whs = np.resize(pool, k)
                rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
                ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
                res = {0: [], 5: [], 6: []}
                ref = None
                for mode in (0, 5, 6):
                    dev.set_option("reduce_mode", mode)
                    dev.prove_batch(ph, rh, whs, rs, ss)                # warm
                for _ in range(a.runs):
                    for mode in (0, 5, 6):
                        dev.set_option("reduce_mode", mode)
                        t0 = time.perf_counter()
                        p, _ = dev.prove_batch(ph, rh, whs, rs, ss)
                        res[mode].append((time.perf_counter() - t0) * 1e3 / k)
                        ref = p if ref is None else ref
                        assert np.array_equal(p, ref)
                dev.set_option("reduce_mode", 0)
                print("%s | %s | %d | %.3f | %.3f | %.3f" % (desc, key, k, *(float(np.median(res[m])) for m in (0, 5, 6))), flush=True)
        for w in set(int(w) for w in pool):
            dev.witness_free(w)
        dev.pk_free(ph)
        dev.r1cs_free(rh)
    dev.close()


if __name__ == "__main__":
    main()
