"""Membership of many points: the host loop, the per-point device stage and the key-check kernels, then whole resident keys (GPU box).
   python tools/pk_check_timing.py [--n 1048576] [--runs 3] [--host-cap 4096] [--keys 32,128] [--out profiles/pk_check_timing.txt]
ms per million points, G1 and G2 separately, of
  (a) zkg16_point_check looped on eight host threads (timed on --host-cap points: the cost per point does not depend on the count);
  (b) zkg16_point_check_batch on the n points (upload, membership_kernel, a byte per point back);
  (c) the kernels of zkg16_pk_check on the same n points resident in U-form (zkg16_points_check_bulk: its kernel by device events,
      and beside it the whole call with the upload and conversion in front);
the median of --runs rounds with the three alternated in every round, and the spread.  The points are multiples of the generator
(Device.fixed_base), so every route must find no bad point.  Then, for every n x n MatrixCircuit key of --keys made by
zkg16_setup_resident: zkg16_pk_check of the resident key (wall, and each query's kernel), without and with window tables, next to
what zkg16_setup + zkg16_pk_load of that key cost (the host arrays of a key that large may not fit: then that is what is recorded)."""
import argparse
import ctypes as C
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np

import bench
from zksnark_finalproject_amd import Device
from zksnark_finalproject_amd._lib import Zkg16Error
from zksnark_finalproject_amd.device import PK_QUERIES, point_check
from zksnark_finalproject_amd.workloads import g1_generator, g2_generator

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
WIDTH = {"g1": 12, "g2": 24}


def host_loop(group, pts, threads=8):
    """zkg16_point_check of every point on `threads` host threads (the library call releases the interpreter lock) -> seconds"""
    bad = []

    def work(lo, hi):
        for i in range(lo, hi):
            if not point_check(group, pts[i]):
                bad.append(i)
    n = pts.shape[0]
    th = [threading.Thread(target=work, args=(n * t // threads, n * (t + 1) // threads)) for t in range(threads)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    assert not bad
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-cap", type=int, default=4096)
    ap.add_argument("--keys", default="32,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pk_check_timing.txt"))
    a = ap.parse_args()
    dev = Device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: "%.2f [%.2f .. %.2f]" % (float(np.median(v)), min(v), max(v))
    rng = np.random.default_rng(11)
    say("# %d points per group (multiples of the generator); ms per million points, median of %d rounds [min .. max], routes alternated in every round" % (a.n, a.runs))
    say("# group | (a) zkg16_point_check on 8 host threads (timed on %d points) | (b) zkg16_point_check_batch, whole call | (c) pk_check kernel on resident points "
        "(device events) | (c) zkg16_points_check_bulk whole call (upload + conversion + kernel) | (a)/(c) | (b)/(c)" % min(a.host_cap, a.n))
    for group in ("g1", "g2"):
        k = np.zeros((a.n, 4), dtype=np.uint64)
        k[:, :3] = rng.integers(1, 1 << 63, size=(a.n, 3), dtype=np.uint64)          # 192-bit logs: below r, never zero
        pts, inf = dev.fixed_base(group, g1_generator() if group == "g1" else g2_generator(), k)
        assert not np.any(inf)
        per_m = 1e6 / a.n
        assert dev.point_check_batch(group, pts).all() and dev.points_check_bulk(group, pts) == (0, (1 << 64) - 1)          # warm: buffers, code objects
        cap = min(a.host_cap, a.n)
        ta, tb, tc, tcw = [], [], [], []
        for _ in range(a.runs):
            ta.append(host_loop(group, pts[:cap]) * 1e3 * 1e6 / cap)
            t0 = time.perf_counter()
            ok = dev.point_check_batch(group, pts)
            tb.append((time.perf_counter() - t0) * 1e3 * per_m)
            assert ok.all()
            t0 = time.perf_counter()
            res = dev.points_check_bulk(group, pts)
            tcw.append((time.perf_counter() - t0) * 1e3 * per_m)
            assert res == (0, (1 << 64) - 1)
            tc.append(dev.pk_check_timings()["bulk_kernel_ms"] * per_m)
        say("%s | %s | %s | %s | %s | %.1f | %.2f" % (group, fmt(ta), fmt(tb), fmt(tc), fmt(tcw), np.median(ta) / np.median(tc), np.median(tb) / np.median(tc)))
        del pts
    say("")
    say("# whole resident keys of the n x n MatrixCircuit (zkg16_setup_resident); pk_check: wall ms of the call, median of %d [min .. max], and the kernel of each query "
        "(device events of the median round's neighbour: they run side by side)" % a.runs)
    for n in [int(x) for x in a.keys.split(",") if x]:
        rh = dev.r1cs_matrix(n)
        trap, g1, g2 = bench.draw_key_inputs(100 + n)
        t0 = time.perf_counter()
        ph, _ = dev.setup_resident(rh, 4, trap, g1, g2)
        t_setup = time.perf_counter() - t0
        ni, nc, nvar = C.c_size_t(), C.c_size_t(), C.c_size_t()          # the dimensions alone (Device.r1cs_read copies the matrices back)
        dev._check(dev.lib.zkg16_r1cs_read(dev.ctx, rh, None, None, None, C.byref(ni), C.byref(nc), C.byref(nvar), None))
        nv, domain = nvar.value, 1 << (nc.value + ni.value - 1).bit_length()
        sizes = "a = b_g1 = b_g2 = %d, l = %d, h = %d points" % (nv, nv - 4, domain - 1)

        def check(label):
            tw, parts = [], None
            for _ in range(a.runs):
                t0 = time.perf_counter()
                res = dev.pk_check(ph)
                tw.append((time.perf_counter() - t0) * 1e3)
                assert res["ok"], res
                parts = dev.pk_check_timings()
            g1_pts, g2_pts = 3 * nv - 4 + domain - 1, nv
            say("n=%d %s: pk_check %s ms  (%s; %.2f M G1 + %.2f M G2 points; setup_resident %.2f s)  kernels ms: %s" %
                (n, label, fmt(tw), sizes, g1_pts / 1e6, g2_pts / 1e6, t_setup, ", ".join("%s %.2f" % (q, parts[q]) for q in PK_QUERIES)))
        check("plain key")
        try:
            t0 = time.perf_counter()
            dev.pk_precompute(ph)
            say("n=%d pk_precompute %.2f s, widths %s" % (n, time.perf_counter() - t0, dev.pk_table_bits(ph)))
            check("with window tables (level 0 at the table stride)")
        except Zkg16Error as e:
            say("n=%d window tables not built next to the key: %s" % (n, e))
        dev.pk_free(ph)
        # what loading that key from host arrays costs (zkg16_setup writes them, zkg16_pk_load reads them back in)
        try:
            t0 = time.perf_counter()
            pk, _ = dev.setup(rh, 4, nv, domain, trap, g1, g2)
            t_host_setup = time.perf_counter() - t0
            tl = []
            for opt in (0, 1):
                dev.set_option("pk_validate", opt)
                t0 = time.perf_counter()
                h = dev.pk_load(pk, 4)
                tl.append((time.perf_counter() - t0) * 1e3)
                dev.pk_free(h)
            dev.set_option("pk_validate", 0)
            say("n=%d zkg16_setup to host arrays %.2f s; zkg16_pk_load of them %.1f ms, with option pk_validate = 1 %.1f ms (one round each)" % (n, t_host_setup, tl[0], tl[1]))
            del pk
        except (MemoryError, Zkg16Error) as e:
            dev.set_option("pk_validate", 0)
            say("n=%d pk_load not measured: %s" % (n, e))
        dev.r1cs_free(rh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
