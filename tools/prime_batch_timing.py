"""K prime requests: the per-request path against the template key and the batched entries (GPU box).
   python tools/prime_batch_timing.py [--ks 1,2,4,...,64] [--runs 3] [--legs a,b,c,w] [--out profiles/prime_batch_timing.txt]
For K distinct candidates (first-found primes of x = 1000, 1001, ...), ms per request as the median of --runs rounds
[min .. max] after one warm-up round, the legs alternated in every round:
   leg a  K x the device path of handlers.prove_prime: r1cs_prime, witness_prime, setup_resident, prove_resident, frees
   leg b  K x (template key: r1cs_prime_template + setup_resident, then prove_prime_batch with k = 1)
   leg c  one prove_prime_batch on a template key that is already resident, with its four timings per request
          (host inputs / assignment passes / proving / whole call)
   leg w  the assignments alone: K x witness_prime against one witness_prime_batch
Legs b and c are checked byte for byte against leg a's proofs and gamma_abc_g1[0] of the round.  --legs a uses nothing the
batched entries added: run it on a build of the parent commit for the baseline (its rows go under the same header)."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from zksnark_finalproject_amd import Device
from zksnark_finalproject_amd.circuits import prime_dims, prime_search
from zksnark_finalproject_amd.device import scalar_mul
from zksnark_finalproject_amd.handlers import _fr_mont
from zksnark_finalproject_amd.workloads import R_MOD, g1_generator, g2_generator


def fmt(v):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8,16,32,64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,w")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    legs = a.legs.split(",")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    cands, x = [], 1000
    while len(cands) < max(ks):
        f = prime_search(x, 64)
        if f["found"]:
            cands.append((x, f["j"]))
        x += 1
    rng = random.Random(7)
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    kk = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), kk)[0], scalar_mul("g2", g2_generator(), kk)[0]
    rs_all = np.stack([_fr_mont(rng.randrange(R_MOD)) for _ in cands])
    ss_all = np.stack([_fr_mont(rng.randrange(R_MOD)) for _ in cands])
    ni = prime_dims(1)["num_instance"]
    dev = Device(0)
    batched = any(l in legs for l in "bc")
    if batched:
        from zksnark_finalproject_amd.circuits import prime_key_corrections
        corr, _ = prime_key_corrections(trap, g1)
        t_rh = dev.r1cs_prime_template()
        t_ph, t_vk = dev.setup_resident(t_rh, ni, trap, g1, g2)
    emit("K | leg a: K x (r1cs_prime + witness_prime + setup_resident + prove_resident) | leg b: K x (template key + prove_prime_batch k = 1) | "
         "leg c: one prove_prime_batch | leg c inputs / assignment / proving / call | a / b | a / c | leg w: K x witness_prime | "
         "one witness_prime_batch | ratio     (ms per request, median [min .. max])")
    for k in ks:
        xs = np.array([c[0] for c in cands[:k]], dtype=np.uint64)
        js = np.array([c[1] for c in cands[:k]], dtype=np.uint64)
        rs, ss = rs_all[:k], ss_all[:k]

        def leg_a():
            t0 = time.perf_counter()
            proofs, g0 = [], []
            for i in range(k):
                rh, wh = dev.r1cs_prime(int(xs[i]), int(js[i])), dev.witness_prime(int(xs[i]), int(js[i]))
                ph, vk = dev.setup_resident(rh, ni, trap, g1, g2)
                proofs.append(dev.prove_resident(ph, rh, wh, rs[i], ss[i])[0])
                g0.append(vk["gamma_abc_g1"][0])
                for f, h in ((dev.pk_free, ph), (dev.witness_free, wh), (dev.r1cs_free, rh)):
                    f(h)
            return (time.perf_counter() - t0) * 1e3 / k, (np.stack(proofs), np.stack(g0)), None

        def leg_b():
            t0 = time.perf_counter()
            proofs, g0 = [], []
            for i in range(k):
                rh = dev.r1cs_prime_template()
                ph, vk = dev.setup_resident(rh, ni, trap, g1, g2)
                p, _, g, _, _ = dev.prove_prime_batch(ph, rh, corr, vk["gamma_abc_g1"][0], xs[i:i + 1], js[i:i + 1], rs[i:i + 1], ss[i:i + 1],
                                                      public_inputs=False)
                proofs.append(p[0])
                g0.append(g[0])
                dev.pk_free(ph)
                dev.r1cs_free(rh)
            return (time.perf_counter() - t0) * 1e3 / k, (np.stack(proofs), np.stack(g0)), None

        def leg_c():
            t0 = time.perf_counter()
            p, _, g, _, ms = dev.prove_prime_batch(t_ph, t_rh, corr, t_vk["gamma_abc_g1"][0], xs, js, rs, ss, public_inputs=False)
            return (time.perf_counter() - t0) * 1e3 / k, (p, g), [ms[n] / k for n in ("host_inputs_ms", "witness_ms", "prove_ms", "call_ms")]

        def leg_w():
            t0 = time.perf_counter()
            for i in range(k):
                dev.witness_free(dev.witness_prime(int(xs[i]), int(js[i])))
            t1 = time.perf_counter()
            one = None
            if hasattr(dev, "witness_prime_batch"):
                for h in dev.witness_prime_batch(xs, js):
                    dev.witness_free(int(h))
                one = (time.perf_counter() - t1) * 1e3 / k
            return (t1 - t0) * 1e3 / k, None, one
        run = dict(a=leg_a, b=leg_b, c=leg_c, w=leg_w)
        for l in legs:                                      # warm-up: workspaces, staging and the dictionary of this K
            run[l]()
        t = {l: [] for l in legs}
        split, one = [], []
        ok = True
        for _ in range(a.runs):
            ref = None
            for l in legs:
                ms, res, extra = run[l]()
                t[l].append(ms)
                if l == "c":
                    split.append(extra)
                if l == "w" and extra is not None:
                    one.append(extra)
                if res is not None:
                    ref = res if ref is None else ref
                    ok = ok and np.array_equal(res[0], ref[0]) and np.array_equal(res[1], ref[1])
        med = {l: float(np.median(t[l])) for l in legs}
        cell = lambda l: fmt(t[l]) if l in legs else "-"
        emit("%d | %s | %s | %s | %s | %s | %s | %s | %s | %s%s" % (
            k, cell("a"), cell("b"), cell("c"),
            " / ".join("%.3f" % float(np.median([s[i] for s in split])) for i in range(4)) if split else "-",
            "%.2f" % (med["a"] / med["b"]) if "a" in legs and "b" in legs else "-",
            "%.2f" % (med["a"] / med["c"]) if "a" in legs and "c" in legs else "-",
            cell("w"), fmt(one) if one else "-", "%.2f" % (med["w"] / float(np.median(one))) if one else "-",
            "" if ok else " | PROOFS DIFFER"))
    if batched:
        dev.pk_free(t_ph)
        dev.r1cs_free(t_rh)
    dev.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
