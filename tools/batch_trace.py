"""Kernel trace of zkg16_prove_batch alone (GPU box), apart from the setup and from single proofs.
   run:      rocprofv3 --kernel-trace -d DIR -o NAME -- python tools/batch_trace.py run SHAPE K [--calls 3]
             (shape as tools/batch_timing.py; setup, a warm batch, then --calls batches, each after a 300 ms pause)
   analyze:  python tools/batch_trace.py analyze DB OUT_PREFIX
             keeps the kernels of the LAST batch call (the launches after the last pause of > 150 ms) and writes
             OUT_PREFIX.csv (per kernel: launches, summed and wall-union time) and OUT_PREFIX.txt (the call's span, device busy
             time, and the chain of launches that ends last: walking back from the last kernel to the one whose end is
             closest before each kernel's start on any stream — the critical path as the trace shows it)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(shape, k, calls):
    import numpy as np
    import bench
    from batch_timing import shape_setup
    from zksnark_finalproject_amd import Device
    dev = Device(0)
    desc, rh, ph, pool = shape_setup(dev, shape)
    whs = np.resize(pool, k)
    prng = np.random.default_rng(7)
    rs = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
    ss = np.stack([bench.fr_mont(int(v)) for v in prng.integers(1, 1 << 62, size=k)]).reshape(k, 4)
    dev.prove_batch(ph, rh, whs, rs, ss)
    for _ in range(calls):
        time.sleep(0.3)
        t0 = time.perf_counter()
        dev.prove_batch(ph, rh, whs, rs, ss)
        print("%s K=%d: %.3f ms per batch call" % (desc, k, (time.perf_counter() - t0) * 1e3), flush=True)
    dev.close()


def analyze(db, out):
    import csv
    import sqlite3
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end, stream_id from kernels order by start").fetchall()
    cut = 0
    for i in range(1, len(rows)):
        if rows[i][1] - max(r[2] for r in rows[max(0, i - 64):i]) > 150e6:
            cut = i
    ks = rows[cut:]
    t0, t1 = ks[0][1], max(r[2] for r in ks)
    busy, cur_s, cur_e = 0, None, None
    for _, s, e, _ in ks:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    busy += cur_e - cur_s
    per = {}
    for n, s, e, _ in ks:
        p = per.setdefault(n, [0, 0])
        p[0] += 1
        p[1] += e - s
    with open(out + ".csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "PercentOfSpan"])
        for n, (cnt, tot) in sorted(per.items(), key=lambda x: -x[1][1]):
            w.writerow([n, cnt, tot, "%.2f" % (100.0 * tot / (t1 - t0))])
    # critical chain: from the kernel that ends last, step to the kernel whose end is the latest at or before this one's start
    by_end = sorted(ks, key=lambda r: r[2])
    chain, cur = [], max(ks, key=lambda r: r[2])
    while cur is not None:
        chain.append(cur)
        prev = None
        for r in by_end:
            if r[2] <= cur[1] + 2000 and r is not cur:
                prev = r
            elif r[2] > cur[1] + 2000:
                break
        cur = prev if prev is not None and prev[1] < cur[1] else None
    chain.reverse()
    agg = {}
    for n, s, e, _ in chain:
        a = agg.setdefault(n, [0, 0])
        a[0] += 1
        a[1] += e - s
    with open(out + ".txt", "w") as f:
        f.write("one batch call: %d launches, span %.3f ms, device busy (union of kernel intervals) %.3f ms\n" %
                (len(ks), (t1 - t0) / 1e6, busy / 1e6))
        f.write("critical chain: %d launches, %.3f ms of kernel time, %.3f ms of gaps between them\n" %
                (len(chain), sum(e - s for _, s, e, _ in chain) / 1e6, ((t1 - t0) - sum(e - s for _, s, e, _ in chain)) / 1e6))
        f.write("chain by kernel (launches, ms):\n")
        for n, (cnt, tot) in sorted(agg.items(), key=lambda x: -x[1][1]):
            f.write("  %8.3f ms %4d x  %s\n" % (tot / 1e6, cnt, n[:110]))
    print(open(out + ".txt").read())


if __name__ == "__main__":
    if sys.argv[1] == "run":
        calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 3
        run(sys.argv[2], int(sys.argv[3]), calls)
    else:
        analyze(sys.argv[2], sys.argv[3])
