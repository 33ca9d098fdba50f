"""Setup-and-prove requests: the key route (zkg16_setup_resident + zkg16_prove_resident) against the trapdoor route
(zkg16_prove_trapdoor), through the handlers, on one MI355X (GPU box).
   python tools/trapdoor_timing.py [--rounds 3] [--reps 3] [--cases matrix32,matrix128,prime,fib1000,linear8,linear32,fib1000x64,linear8x64,linear32x64]
                                   [--out profiles/trapdoor_timing.txt] [--tree CHECKOUT]
Per case, ms per request of the handler call with route="key" and with route="trapdoor": every round runs --reps requests on one
route, then on the other (alternated; the order flips from round to round), the figure of a round is the mean of its requests, and
the table gives the median of the rounds with [min .. max].  matrix128 and the batches make ONE call per route and round whatever
--reps says (a batch call's figure is divided by K); the column "calls per round" says which.  Two figures per route: the whole handler call (host synthesis, encoding
and, for linear, the handler's own verification included) and setup_time + proving_time as the record reports them.  Matrix requests
run on resident matrices (the shape cache, warmed before the rounds) with prove_matrix's overlap of the assignment and the setup.
Batches of K = 64: prove_fibonaccis / prove_linear_equations_batch with key=None, so the key route sets its key up in the same call.
Every trapdoor record is compared with the key route's (proof, vk) before anything is timed.
--tree: import the package from another checkout (a build of the parent commit, which has no route keyword) and time its key route
alone; the A/B file profiles/trapdoor_ab_parent.txt is made from such runs alternated with this tree's."""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cases", default="matrix32,matrix128,prime,fib1000,linear8,linear32,fib1000x64,linear8x64,linear32x64")
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=None)
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.tree) if ARGS.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zksnark_finalproject_amd import Device, handlers  # noqa: E402

PARENT = ARGS.tree is not None
ROUTES = ("key",) if PARENT else ("key", "trapdoor")


def lower(n, seed):
    rng = np.random.default_rng(seed)
    a = np.tril(rng.integers(1, 1 << 63, (n, n), dtype=np.uint64))
    return a, rng.integers(0, 1 << 63, n, dtype=np.uint64)


def make_case(dev, name):
    """-> (call(route, seed) -> (record or list of records), requests per call)"""
    kw = lambda route: {} if PARENT else dict(route=route)
    if name.startswith("matrix"):
        n = int(name[6:])
        rng = np.random.default_rng(n)
        a, b = rng.integers(0, 1 << 63, (n, n), dtype=np.uint64), rng.integers(0, 1 << 63, (n, n), dtype=np.uint64)
        return (lambda route, seed: handlers.prove_matrix(dev, n, a, b, seed=seed, **kw(route))), 1
    if name == "prime":
        return (lambda route, seed: handlers.prove_prime(dev, 12345, 32, seed=seed, **kw(route))), 1
    if name.startswith("fib") and "x" not in name:
        rounds = int(name[3:])
        return (lambda route, seed: handlers.prove_fibonacci(dev, 3, 5, rounds, seed=seed, **kw(route))), 1
    if name.startswith("linear") and "x" not in name:
        a, b = lower(int(name[6:]), 5)
        return (lambda route, seed: handlers.prove_linear_equations(dev, a, b, seed=seed, **kw(route))), 1
    what, k = name.split("x")
    k = int(k)
    if what.startswith("fib"):
        rounds = int(what[3:])
        reqs = [(3 + i, 5 + 2 * i) for i in range(k)]
        return (lambda route, seed: handlers.prove_fibonaccis(dev, reqs, rounds, seed=seed, **kw(route))), k
    systems = [lower(int(what[6:]), 100 + i) for i in range(k)]
    return (lambda route, seed: handlers.prove_linear_equations_batch(dev, systems, seed=seed, **kw(route))), k


def reported(rec):
    """setup_time + proving_time of a record (ms per request of the call)"""
    if isinstance(rec, list):
        d = rec[0]["_detail"]
        return (rec[0].get("setup_time", d.get("setup_time", 0.0)) / len(rec) + rec[0]["proving_time"]) * 1e3      # proving_time is per request already
    d = rec["_detail"]
    return (d["setup_time"] + d["proving_time"]) * 1e3


def main():
    dev = Device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))
    say("%s; median of %d rounds [min .. max]; a round's figure is the mean of its calls per route (column 3: %d, or 1 for matrix128 and for "
        "the batches, whose one call is divided by K), routes alternated" %
        ("parent build, key route alone" if PARENT else "key route against trapdoor route", ARGS.rounds, ARGS.reps))
    say("case | route | calls per round | handler call ms/request | setup_time + proving_time ms/request" + ("" if PARENT else " | key / trapdoor (call) | route that answered"))
    for name in ARGS.cases.split(","):
        call, k = make_case(dev, name)
        reps = 1 if k > 1 or name == "matrix128" else ARGS.reps
        first = {r: call(r, 1) for r in ROUTES}                       # warm: shape cache, code objects, buffers — and the comparison
        if not PARENT:
            a, b = first["key"], first["trapdoor"]
            pairs = list(zip(a, b)) if isinstance(a, list) else [(a, b)]
            assert all(x["proof"] == y["proof"] and x["vk"] == y["vk"] for x, y in pairs), name
        wall = {r: [] for r in ROUTES}
        rep = {r: [] for r in ROUTES}
        answered = set()
        for rnd in range(ARGS.rounds):
            for r in (ROUTES if rnd % 2 == 0 else ROUTES[::-1]):
                w, p = [], []
                for i in range(reps):
                    t0 = time.perf_counter()
                    rec = call(r, 10 + rnd * reps + i)
                    w.append((time.perf_counter() - t0) * 1e3 / k)
                    p.append(reported(rec))
                    if r == "trapdoor":
                        answered.add((rec[0] if isinstance(rec, list) else rec)["_detail"]["route"])
                wall[r].append(float(np.mean(w)))
                rep[r].append(float(np.mean(p)))
        for r in ROUTES:
            extra = ""
            if not PARENT and r == "trapdoor":
                extra = " | %.2f | %s" % (np.median(wall["key"]) / np.median(wall["trapdoor"]), ",".join(sorted(answered)))
            say("%s | %s | %d | %s | %s%s" % (name, r, reps, fmt(wall[r]), fmt(rep[r]), extra))
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
