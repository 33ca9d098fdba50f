"""Per-proof verdicts on the device against bisecting, on Fibonacci-1000 proofs from zkg16_prove_batch (GPU box).
   python tools/verify_each_timing.py [--runs 3] [--other-lib PATH] [--out profiles/verify_each_timing_r10.txt]
Three tables, every figure the median of --runs rounds with the methods alternated in every round, spread (min .. max) stated:
  1. T_each(K): wall ms of zkg16_verify_each at K = 64, 1024, 4096, 16384 beside eight host threads looping zkg16_verify_prepared;
  2. t_range: ms per range test of bisecting to the end (option verify_each_after above 2K) at K = 1024 and 16384, one bad proof
     and 1 % bad, from zkg16_verify_batch_timings [5] / [10] — and the default ceil(T_each(1024) / t_range(1024)) they give;
  3. the bad-proof sweep: zkg16_verify_batch with ok_each at K = 1024 and 16384 with 0, 1, 1 %, 10 % and 50 % of the proofs bad
     (C doubled: it passes membership, so only the equation tells), this build at the default option against --other-lib (a build
     of the parent commit: the same ABI without the per-proof pass), alternated, the one that goes first changing with the round;
     for 0 and 1 bad proof the breakdown of both builds.
Every verdict is checked."""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import verify_batch_timing as VBT
from zksnark_finalproject_amd import Device, _lib
from zksnark_finalproject_amd.device import draw_rho, scalar_mul


def other_device(path):
    """a Device on another build of the library (the symbols it has)"""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    d = Device.__new__(Device)
    d.lib = lib
    d.ctx = C.c_void_p()
    ids = (C.c_int * 1)(0)
    rc = lib.zkg16_init(ids, 1, C.byref(d.ctx))
    assert rc == 0, rc
    return d


def loop_eight_threads(lib, pvk, pubs, proofs, infs):
    gabc = np.ascontiguousarray(pvk["gamma_abc_g1"], dtype=np.uint64).reshape(-1, 12)
    g = np.ascontiguousarray(pvk["gamma_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    d = np.ascontiguousarray(pvk["delta_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    ab = np.ascontiguousarray(pvk["alpha_beta"], dtype=np.uint64)
    k = proofs.shape[0]

    def part(t):
        ok = C.c_int(0)
        good = 0
        for i in range(t, k, 8):
            lib.zkg16_verify_prepared(gabc, gabc.shape[0], pubs[i].ctypes.data, ab, g, d, g.shape[0], proofs[i], infs[i], C.byref(ok))
            good += ok.value
        return good
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=8) as ex:
        good = sum(ex.map(part, range(8)))
    return (time.perf_counter() - t0) * 1e3, good == k


def spoil(proofs, k, n_bad, seed):
    """-> (proofs with n_bad of the first k having C doubled, the expected verdicts)"""
    p = proofs[:k].copy()
    want = np.ones(k, dtype=bool)
    if n_bad:
        two = np.array([2, 0, 0, 0], dtype=np.uint64)
        for i in np.random.default_rng(seed).choice(k, size=n_bad, replace=False):
            p[i, 36:48] = scalar_mul("g1", p[i, 36:48], two)[0]
            want[i] = False
    return p, want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ks", default="64,1024,4096,16384")
    ap.add_argument("--sweep-ks", default="1024,16384")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--parts", default="1,2,3", help="which of the three tables to measure")
    ap.add_argument("--max-bad-percent", type=int, default=50, help="table 3: leave out the rows with more bad proofs than this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_each_timing_r10.txt"))
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    sweep_ks = [int(k) for k in a.sweep_ks.split(",")]
    dev = Device(0)
    dev.set_option("verify_batch_min", 1)
    other = other_device(a.other_lib) if a.other_lib else None
    if other:
        other.set_option("verify_batch_min", 1)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    fmt = lambda v: "%.2f [%.2f .. %.2f]" % (float(np.median(v)), min(v), max(v))
    pvk, pubs, proofs, infs, _ = VBT.make_proofs(dev, max(ks + sweep_ks))
    say("Fibonacci-1000 proofs from zkg16_prove_batch (%d made); median of %d rounds [min .. max], methods alternated in every round" % (proofs.shape[0], a.runs))

    parts = [int(x) for x in a.parts.split(",")]
    say("1. K | zkg16_verify_each ms per call | eight host threads looping zkg16_verify_prepared ms | ratio")
    t_each = {}
    for k in (ks if 1 in parts else []):
        p, f, z = proofs[:k], infs[:k], pubs[:k]
        assert dev.verify_each(pvk, z, p, f).all()                         # warm
        te, tl = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            got = dev.verify_each(pvk, z, p, f)
            te.append((time.perf_counter() - t0) * 1e3)
            assert got.all()
            ms, ok = loop_eight_threads(dev.lib, pvk, z, p, f)
            assert ok
            tl.append(ms)
        t_each[k] = te
        say("%d | %s | %s | %.1f" % (k, fmt(te), fmt(tl), np.median(tl) / np.median(te)))

    say("2. K | bad proofs | bisecting to the end: ms [5] | range tests [10] | t_range = [5] / [10] ms")
    t_range = {}
    dev.set_option("verify_each_after", 1 << 30)
    for k in (sweep_ks if 2 in parts else []):
        for n_bad in (1, max(k // 100, 1)):
            p, want = spoil(proofs, k, n_bad, 100 + n_bad)
            rho = draw_rho(k)
            tb, nr = [], []
            for _ in range(a.runs):
                ok, each = dev.verify_batch(pvk, pubs[:k], p, infs[:k], rho=rho, each=True)
                assert ok is False and np.array_equal(each, want)
                t = dev.verify_batch_timings()
                assert t["each_ms"] == 0
                tb.append(t["bisect_ms"])
                nr.append(t["range_tests"])
            per = [x / y for x, y in zip(tb, nr)]
            t_range.setdefault(k, []).append(float(np.median(per)))
            say("%d | %d | %s | %d | %s" % (k, n_bad, fmt(tb), int(np.median(nr)), "%.3f [%.3f .. %.3f]" % (float(np.median(per)), min(per), max(per))))
    dev.set_option("verify_each_after", 0)
    if 1024 in t_each and 1024 in t_range:
        te, tr = float(np.median(t_each[1024])), t_range[1024][0]
        say("default of verify_each_after: ceil(T_each(1024) / t_range(1024, one bad proof)) = ceil(%.2f / %.3f) = %d" % (te, tr, int(np.ceil(te / tr))))

    say("3. K | bad proofs | this build, default option: verify_batch with ok_each ms per call | per-proof pass ms [9] | range tests [10] | other build ms per call | other / this")
    for k in (sweep_ks if 3 in parts else []):
        for n_bad in (0, 1, max(k // 100, 1), k // 10, k // 2):
            if n_bad > 1 and 100 * n_bad > a.max_bad_percent * k:
                continue
            p, want = spoil(proofs, k, n_bad, 200 + n_bad)
            rho = draw_rho(k)
            tn, to, e9, e10, brk = [], [], [], [], {"this": [], "other": []}
            names = ("membership_ms", "miller_ms", "product_ms", "msm_ms", "host_ms", "bisect_ms")

            def one(d, times, tag):
                t0 = time.perf_counter()
                ok, each = d.verify_batch(pvk, pubs[:k], p, infs[:k], rho=rho, each=True)
                times.append((time.perf_counter() - t0) * 1e3)
                assert ok is (n_bad == 0) and np.array_equal(each, want)
                t = d.verify_batch_timings()
                brk[tag].append([t[n] for n in names])
                return t
            for r in range(a.runs):
                # who goes first alternates with the round
                order = [("this", dev, tn), ("other", other, to)] if other else [("this", dev, tn)]
                for tag, d, times in (order if r % 2 == 0 else order[::-1]):
                    t = one(d, times, tag)
                    if tag == "this":
                        e9.append(t["each_ms"])
                        e10.append(t["range_tests"])
            say("%d | %d | %s | %.2f | %d | %s | %s" % (k, n_bad, fmt(tn), float(np.median(e9)), int(np.median(e10)), fmt(to) if to else "-",
                                                      "%.2f" % (np.median(to) / np.median(tn)) if to else "-"))
            if n_bad <= 1:
                for tag in brk:
                    if brk[tag]:
                        say("    %s build, ms per call: %s" % (tag, ", ".join("%s %.2f" % (n[:-3], v) for n, v in zip(names, np.median(np.array(brk[tag]), axis=0)))))
    if other:
        other.close()
    dev.close()


if __name__ == "__main__":
    main()
