"""Verifying K proofs of the prime handler made under one trapdoor (GPU box).
   python tools/verify_prime_timing.py [--ks 64,1024,16384] [--runs 3] [--distinct 1024] [--out profiles/verify_prime_timing.txt]
The proofs come from zkg16_prove_prime_batch on one template key (--distinct of them, each a first-found prime of its x, less those
whose proof zkg16_verify_each refuses; a larger K repeats them, every entry with its own multiplier) and start as they travel, 192 compressed bytes each.  For every K, ms per proof of
  (a) a loop of handlers.verify_prime, each proof under its own key as handlers.prove_primes returns it (base64 of the compressed
      key); the loop is timed on the first min(K, 64) proofs, its cost per proof does not depend on K;
  (b) what a caller could do without the prime form: the 259 public inputs of every proof built on the host (zkg16_prime_ext_inputs,
      native; 8.3 KB of limbs per proof) and handed to zkg16_verify_batch_wire under the extended key;
  (c) zkg16_verify_prime_batch_wire: 16 bytes per proof, the inputs and their multiplier sums made on the device,
      with the inputs kernel's and the sums kernels' ms per call (zkg16_verify_batch_timings [11], [12]);
the median of --runs rounds with the three alternated in every round, and the spread (min .. max).  verify_wire_min = 1, so that
every K runs the kernels.  Every verdict is checked."""
import argparse
import base64
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from verify_wire_timing import to_wire
from zksnark_finalproject_amd import Device, handlers, wire
from zksnark_finalproject_amd.circuits import prime_ext_inputs, prime_search
from zksnark_finalproject_amd.device import draw_rho, pvk_prepare


def make_proofs(dev, n, chunk=512):
    """n proofs of first-found primes on one template key -> (key dict, xs, js, proofs, infs, g0, ms per proof of the proving calls)"""
    rng = random.Random(20260)
    key = handlers.prime_template_key(dev, rng)
    xs, js, x = [], [], 1000
    while len(xs) < n:
        f = prime_search(x, 64)
        if f["found"]:
            xs.append(x)
            js.append(f["j"])
        x += 1
    xs, js = np.array(xs, dtype=np.uint64), np.array(js, dtype=np.uint64)
    proofs, infs, g0s, ms = [], [], [], 0.0
    try:
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            rs, ss = handlers._draw_rs_batch(rng, hi - lo)
            t0 = time.perf_counter()
            p, f, g0, _, _ = dev.prove_prime_batch(key["ph"], key["rh"], key["corr"], key["vk"]["gamma_abc_g1"][0], xs[lo:hi], js[lo:hi], rs, ss,
                                                   public_inputs=False)
            ms += (time.perf_counter() - t0) * 1e3
            proofs.append(p)
            infs.append(f)
            g0s.append(g0)
    finally:
        dev.pk_free(key["ph"])
        dev.r1cs_free(key["rh"])
    proofs, infs, g0s = np.concatenate(proofs), np.concatenate(infs), np.concatenate(g0s)
    # A candidate the search finds is not always one whose circuit is satisfied (the Fermat verdict is the native one): the proofs of
    # the others do not verify.  They are told apart by the per-proof verifier on host-built inputs, which shares nothing with the
    # prime form's front, and left out
    z = np.stack([prime_ext_inputs(int(x), int(j)) for x, j in zip(xs, js)])
    good = np.flatnonzero(dev.verify_each(pvk_prepare(key["ext_vk"]), z, proofs, infs))
    return key, xs[good], js[good], proofs[good], infs[good], g0s[good], ms / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="64,1024,16384")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_prime_timing.txt"))
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    dev = Device(0)
    dev.set_option("verify_batch_min", 1)
    dev.set_option("verify_wire_min", 1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    asked = min(max(ks), a.distinct)
    key, xs_all, js_all, proofs, infs, g0, prove_ms = make_proofs(dev, asked)
    n = proofs.shape[0]
    raw_all = to_wire(proofs, infs)
    pvk = pvk_prepare(key["ext_vk"])
    # (a)'s keys, as prove_primes sends them: the template's bytes with gamma_abc_g1[0] (bytes 344 .. 392) replaced
    loop_n = min(n, 64)
    vk_bytes = wire.vk_serialize_compressed(key["vk"])
    own = [base64.standard_b64encode(vk_bytes[:344] + wire.points_compress("g1", g0[i]) + vk_bytes[392:]).decode() for i in range(loop_n)]
    b64 = [base64.standard_b64encode(raw_all[i].tobytes()).decode() for i in range(loop_n)]
    say("PrimeCircuit proofs from zkg16_prove_prime_batch on one template key (%d proved at %.3f ms per proof, %d of them verify by zkg16_verify_each and are "
        "used; larger K repeats them), 192 bytes each; median of %d rounds [min .. max], methods alternated" % (asked, prove_ms, n, a.runs))
    say("K | (a) handlers.verify_prime loop ms/proof (first %d proofs) | (b) host-built inputs + verify_batch_wire ms/proof | (b) its host inputs share | "
        "(c) verify_prime_batch_wire ms/proof | (c) inputs kernel ms per call [11] | (c) sums kernels ms per call [12] | (c) scaling+Miller kernel ms per call | "
        "(c) total ms per call | (c) proofs/s | (b) / (c)" % loop_n)
    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))
    res = {}
    for k in ks:
        reps = (k + n - 1) // n
        raw = np.ascontiguousarray(np.tile(raw_all, (reps, 1))[:k])
        xs, js = np.ascontiguousarray(np.tile(xs_all, reps)[:k]), np.ascontiguousarray(np.tile(js_all, reps)[:k])
        rho = draw_rho(k)
        assert dev.verify_prime_batch_wire(pvk, xs, js, raw, rho=rho) is True              # warm: buffers of this K, code objects
        ta, tb, tbi, tc, t11, t12, mil, tot = [], [], [], [], [], [], [], []
        for _ in range(a.runs):
            m = min(k, loop_n)
            t0 = time.perf_counter()
            for i in range(m):
                assert handlers.verify_prime(own[i], int(xs[i]), int(js[i]), b64[i])["valid"] is True
            ta.append((time.perf_counter() - t0) * 1e3 / m)
            t0 = time.perf_counter()
            z = np.empty((k, 259, 4), dtype=np.uint64)
            for i in range(k):
                z[i] = prime_ext_inputs(int(xs[i]), int(js[i]))
            t1 = time.perf_counter()
            assert dev.verify_batch_wire(pvk, z, raw, rho=rho) is True
            tb.append((time.perf_counter() - t0) * 1e3 / k)
            tbi.append((t1 - t0) * 1e3 / k)
            assert dev.verify_batch_timings()["host_form"] == 0
            t0 = time.perf_counter()
            assert dev.verify_prime_batch_wire(pvk, xs, js, raw, rho=rho) is True
            tc.append((time.perf_counter() - t0) * 1e3 / k)
            t = dev.verify_batch_timings(prime=True)
            assert t["host_form"] == 0
            t11.append(t["prime_inputs_ms"])
            t12.append(t["prime_sums_ms"])
            mil.append(t["miller_ms"])
            tot.append(t["total_ms"])
        res[k] = (tb, tc)
        say("%d | %s | %s | %.4f | %s | %.3f | %.3f | %.2f | %.2f | %.0f | %.2f" %
            (k, fmt(ta), fmt(tb), np.median(tbi), fmt(tc), np.median(t11), np.median(t12), np.median(mil), np.median(tot), 1e3 / np.median(tc),
             np.median(tb) / np.median(tc)))
    wins = [k for k in ks if max(res[k][1]) < min(res[k][0])]
    say("verify_prime_batch_wire beats (b) in every round (max of (c) below the min of (b)) at K = %s" % wins)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
