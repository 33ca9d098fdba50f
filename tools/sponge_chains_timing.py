"""The Poseidon sponge chains of a batch on host threads against the chain kernel (option "sponge_chains_min"), on tabled resident keys
(GPU box).
   python tools/sponge_chains_timing.py [n ...] [--ks 64,128,...] [--runs 3] [--legs witness,prove,hash] [--routes host,device]
For every size n and batch size K, ms per call (the whole batch) of
   witness   one witness_matrix_batch (handles freed inside the timed region)      3K chains
   prove     one prove_matrix_batch                                               3K chains per sub-batch
   hash      matrix_hash_batch against zkg16_matrix_hash_batch_host on 8 threads  K chains
each with the chains on the host ("sponge_chains_min" = never) and on the device (= 1), as the median of --runs rounds [min .. max], the
two routes alternated in every round.  A route WINS a cell when its slowest round is faster than the other's fastest.  Public inputs,
proofs and hashes of the two routes are compared byte for byte.  Before the table: t_perm, the time one wave needs for one permutation —
the chain kernel's device time for 64 chains (one wave) divided by the permutations of a chain.
The last line is the default of "sponge_chains_min" the table gives: per leg and n the smallest chain count from which the device wins
every measured cell, the largest of those over the sizes and over the two assignment legs, the same for the hash leg, and the larger of
the two — or "never" when some leg at some size has no such count.
--routes host --legs witness,prove runs on a build without the option (the baseline).  --summarise FILE prints that last line for a
table this tool wrote earlier (no GPU)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

NEVER = (1 << 32) + 1


def fmt(v):
    return "%.2f [%.2f .. %.2f]" % (float(np.median(v)), min(v), max(v)) if v else "-"


def verdict(host, device):
    if not host or not device:
        return "-"
    if max(device) < min(host):
        return "device %.2fx" % (float(np.median(host)) / float(np.median(device)))
    if max(host) < min(device):
        return "host %.2fx" % (float(np.median(device)) / float(np.median(host)))
    return "within spread"


def default_from(rows):
    """rows: (n, K, {leg: verdict}) -> the line that states the default the table gives"""
    per_leg = {}
    for leg, mult in (("witness", 3), ("prove", 3), ("hash", 1)):
        worst = 0
        for n in sorted(set(r[0] for r in rows)):
            cells = sorted((mult * k, v[leg].startswith("device")) for nn, k, v in rows if nn == n and v.get(leg, "-") != "-")
            if not cells:
                continue
            first = None
            for chains, wins in reversed(cells):
                if not wins:
                    break
                first = chains
            if first is None:
                worst = None
                break
            worst = max(worst, first)
        per_leg[leg] = worst
    said = ", ".join("%s: %s" % (l, "never" if c is None else "not measured" if c == 0 else "from %d chains" % c) for l, c in per_leg.items())
    if any(c is None or c == 0 for c in per_leg.values()):
        return "default of sponge_chains_min from this table: never (per leg, over every measured n — " + said + ")"
    return "default of sponge_chains_min from this table: %d (per leg, over every measured n — %s)" % (max(per_leg.values()), said)


def summarise(path):
    rows = []
    for line in open(path):
        c = [x.strip() for x in line.split("|")]
        if len(c) >= 12 and c[0].isdigit() and c[1].isdigit():
            rows.append((int(c[0]), int(c[1]), dict(witness=c[5], prove=c[8], hash=c[11])))
    print(default_from(rows))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2])
    import bench
    from zksnark_finalproject_amd import Device, _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[8, 16, 32])
    ap.add_argument("--ks", default="64,128,256,512,1024,4096")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--legs", default="witness,prove,hash")
    ap.add_argument("--routes", default="host,device")
    ap.add_argument("--max-gb", type=float, default=96.0, help="skip the assignment legs of a cell whose K assignments exceed this")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    legs = a.legs.split(",")
    routes = a.routes.split(",")
    dev = Device(0)
    lib = _lib.load()

    def route(r):
        if routes != ["host"]:                      # a build without the option has only the host route
            dev.set_option("sponge_chains_min", NEVER if r == "host" else 1)

    if "device" in routes:
        dev.kernel_timing(True)
        route("device")
        for n in a.sizes:
            m = np.random.default_rng(n).integers(0, 1 << 63, size=(64, n, n), dtype=np.uint64)
            dev.matrix_hash_batch(m)
            dev.kernel_stats_reset()
            for _ in range(a.runs):
                dev.matrix_hash_batch(m)
            st = dev.kernel_stats("wit_chain_batch_kernel")
            launches, ms = st["launches"], st["ms"]
            perms = (n * n + 1) // 2
            print("t_perm at n = %d: %.4f ms (one wave of 64 chains, %d permutations each, %.3f ms per call, %d launches)"
                  % (n, ms / a.runs / perms, perms, ms / a.runs, launches), flush=True)
        dev.kernel_timing(False)
    print("n | K | chains (assignments / hashes) | witness host | witness device | wins | prove host | prove device | wins | "
          "hash host 8 threads | hash device | wins     (ms per call, median [min .. max])", flush=True)
    rows = []
    for n in a.sizes:
        trap, g1, g2 = bench.draw_key_inputs(42)
        rh = dev.r1cs_matrix(n)
        ph, _ = dev.setup_resident(rh, 4, trap, g1, g2)
        dev.pk_precompute(ph, 0, 0)
        nc, nw = C.c_size_t(), C.c_size_t()
        assert lib.zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), None) == 0
        total = 4 + nw.value
        rng = np.random.default_rng(n)
        prng = np.random.default_rng(7)
        for k in ks:
            am = rng.integers(0, 1 << 63, size=(k, n, n), dtype=np.uint64)
            bm = rng.integers(0, 1 << 63, size=(k, n, n), dtype=np.uint64)
            rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
            fits = k * total * 32 <= a.max_gb * (1 << 30)

            def witness(r):
                route(r)
                t0 = time.perf_counter()
                whs, pubs, _ = dev.witness_matrix_batch(am, bm)
                for w in whs:
                    dev.witness_free(int(w))
                return (time.perf_counter() - t0) * 1e3, pubs

            def prove(r):
                route(r)
                t0 = time.perf_counter()
                proofs, _, pubs, _ = dev.prove_matrix_batch(ph, rh, am, bm, rs, ss)
                return (time.perf_counter() - t0) * 1e3, np.concatenate([proofs.reshape(-1), pubs.reshape(-1)])

            def hash_(r):
                t0 = time.perf_counter()
                if r == "host":
                    out = np.zeros((k, 4), dtype=np.uint64)
                    assert lib.zkg16_matrix_hash_batch_host(n, am.ctypes.data, k, 8, out.ctypes.data) == 0
                else:
                    route(r)
                    out = dev.matrix_hash_batch(am)
                return (time.perf_counter() - t0) * 1e3, out
            run = dict(witness=witness, prove=prove, hash=hash_)
            t = {(l, r): [] for l in legs for r in routes}
            ok = True
            for rnd in range(a.runs + 1):               # round 0 warms workspaces and staging of this K
                for l in legs:
                    if l != "hash" and not fits:
                        continue
                    ref = None
                    for r in (routes if rnd % 2 else routes[::-1]):
                        ms, res = run[l](r)
                        if rnd:
                            t[(l, r)].append(ms)
                        ref = res if ref is None else ref
                        ok = ok and np.array_equal(res, ref)
            cells = []
            for l in ("witness", "prove", "hash"):
                h, d = t.get((l, "host"), []), t.get((l, "device"), [])
                cells += [fmt(h), fmt(d), verdict(h, d)]
            rows.append((n, k, dict(zip(("witness", "prove", "hash"), cells[2::3]))))
            print("%d | %d | %d / %d | %s%s%s" % (n, k, 3 * k, k, " | ".join(cells), "" if fits else " | assignments beyond --max-gb",
                                                 "" if ok else " | RESULTS DIFFER"), flush=True)
        dev.pk_free(ph)
        dev.r1cs_free(rh)
    dev.close()
    if routes == ["host", "device"]:
        print(default_from(rows), flush=True)


if __name__ == "__main__":
    main()
