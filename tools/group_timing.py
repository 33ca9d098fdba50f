"""Per-rank timing of a device group (zkg16_group_create / zkg16_prove_group) on the MatrixCircuit, with the witness map split
over the group's witness-map ranks (csrc/group.hip):
   python tools/group_timing.py [--devices 0,0,0,0] [--n 128|46|32] [--tables on|off] [--bw 50] [--reps 3] [--wm-transforms 6|7]
--devices: one ctx per entry (the default puts four ctxs on GPU 0: every number below is then measured on ONE GPU).
Reports per rank
  - the witness-map share's device time with option group_serial = 1 (each step of each rank alone on the device), of which the
    gather kernels, and the bytes gathered per row-pass exchange and in the redistribution of h;
  - the H / z share time: zkg16_prove_partial of the rank's shard minus the replicated witness map it runs there;
  - the group proof's wall time (on one GPU: all ranks share it);
and the predicted group time: the slowest rank = witness-map share - local gathers + exchanged bytes / --bw + H / z share.  The
exchange term is a bandwidth given on the command line: UNMEASURED unless the devices really are different GPUs."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from zksnark_finalproject_amd import Device, DeviceGroup, _lib  # noqa: E402
from zksnark_finalproject_amd.device import group_layout, shard_plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0,0,0,0")
    ap.add_argument("--n", type=int, default=128, choices=[128, 46, 32])
    ap.add_argument("--tables", default="on", choices=["on", "off"])
    ap.add_argument("--bw", type=float, default=50.0, help="GB/s per rank for the exchanges (a prediction input, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--wm-only", action="store_true", help="no keys: the split witness map's share per rank for k = 2 .. len(devices)")
    ap.add_argument("--wm-transforms", type=int, default=6, choices=[6, 7], help="option wm_transforms: one exchange per transform")
    a = ap.parse_args()
    ids = [int(x) for x in a.devices.split(",")]
    G, tables = len(ids), a.tables == "on"
    devs = [Device(i) for i in ids]
    for d in devs:
        d.set_option("wm_transforms", a.wm_transforms)
    T = a.wm_transforms
    rng = np.random.default_rng(a.n)
    am = rng.integers(0, 1 << 20, size=(a.n, a.n), dtype=np.uint64)
    bm = rng.integers(0, 1 << 20, size=(a.n, a.n), dtype=np.uint64)
    trap, g1, g2 = bench.draw_key_inputs(a.n)
    r, s = bench.fr_mont(12345), bench.fr_mont(67890)
    hs = []
    for d in devs:
        rh = d.r1cs_matrix(a.n)
        wh, _, _ = d.witness_matrix(am, bm)
        ph = None if a.wm_only else d.setup_resident(rh, 4, trap, g1, g2)[0]
        hs.append((ph, rh, wh))
    nc, nw = C.c_size_t(), C.c_size_t()
    assert _lib.load().zkg16_matrix_r1cs_dims(a.n, C.byref(nc), C.byref(nw), None) == 0
    nv = 4 + nw.value
    log_n = int(nc.value + 4 - 1).bit_length()
    N = 1 << log_n
    wm_full = devs[0].bench_witness_map(hs[0][1], hs[0][2], iters=5)
    print("MatrixCircuit %dx%d: %d variables, domain 2^%d; devices %s (%s); tables %s" %
          (a.n, a.n, nv, log_n, ids, "ONE GPU: every rank shares it" if len(set(ids)) == 1 else "%d GPUs" % len(set(ids)),
           "-" if a.wm_only else a.tables))
    print("single-ctx witness map (zkg16_bench_witness_map): %.2f ms" % wm_full)
    if a.wm_only:
        for k in range(2, G + 1):
            if not group_layout(log_n, k)["applies"]:
                continue
            g = DeviceGroup(devs[:k])
            g.set_option("group_serial", 1)
            rhs, whs = [h[1] for h in hs[:k]], [h[2] for h in hs[:k]]
            g.witness_map(rhs, whs, N)
            runs = []
            for _ in range(a.reps):
                g.witness_map(rhs, whs, N)
                runs.append(g.rank_stats())
            g.close()
            wm = [float(np.median([run[j]["wm_ms"] for run in runs])) for j in range(k)]
            ex, hb = runs[0][0]["exchange_bytes"], runs[0][0]["h_bytes"]
            xfer = (T * ex + hb) / (a.bw * 1e9) * 1e3
            print("k = %d: wm share per rank (serial, ms) %s; exchange %.1f MB x %d + h %.1f MB per rank -> %.2f ms at %.0f GB/s (UNMEASURED)" %
                  (k, [round(x, 2) for x in wm], ex / 1e6, T, hb / 1e6, xfer, a.bw))
        for d, (_, rh, wh) in zip(devs, hs):
            d.r1cs_free(rh)
            d.witness_free(wh)
        return
    base = devs[0].pk_slice(hs[0][0], 0, nv, 0, N - 1, True)        # the whole key; with its own tables (+79 GB at 128x128) if asked
    if tables:
        devs[0].pk_precompute(base)
    proof1, _ = devs[0].prove_resident(base, hs[0][1], hs[0][2], r, s)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        devs[0].prove_resident(base, hs[0][1], hs[0][2], r, s)
    single = (time.perf_counter() - t0) / a.reps * 1e3
    devs[0].pk_free(base)
    print("single-ctx proof (%s): %.2f ms" % ("window tables" if tables else "plain key", single))

    plans = [0] + [k for k in (G // 2, G) if k >= 2]
    for h_ranks in dict.fromkeys(plans):
        plan, k = shard_plan(G, nv, N - 1, 0.0, h_ranks, window_tables=tables)
        L = group_layout(log_n, k)
        shards = []
        for i, (z_lo, z_hi, h_lo, h_hi, blind) in enumerate(plan):
            sh = devs[i].pk_slice(hs[i][0], z_lo, z_hi, h_lo, h_hi, blind)
            if tables:
                devs[i].pk_precompute(sh)
            shards.append(sh)
        # H / z share per rank: its partial proof alone, less the replicated witness map the partial runs when it has an h range
        share = []
        for i, p in enumerate(plan):
            devs[i].prove_partial(shards[i], hs[i][1], hs[i][2], r, s)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                devs[i].prove_partial(shards[i], hs[i][1], hs[i][2], r, s)
            dt = (time.perf_counter() - t0) / a.reps * 1e3
            share.append(dt - (wm_full if p[3] > p[2] else 0.0))
        g = DeviceGroup(devs)
        rhs = [h[1] for h in hs]
        whs = [h[2] for h in hs]
        proof, _ = g.prove(shards, rhs, whs, r, s)
        assert np.array_equal(proof, proof1), "group proof != single-ctx proof"
        t0 = time.perf_counter()
        for _ in range(a.reps):
            g.prove(shards, rhs, whs, r, s)
        wall = (time.perf_counter() - t0) / a.reps * 1e3
        k_dist = g.last_wm()
        # the witness-map share alone: group_serial = 1, the witness-map ranks only
        wm_idx = [i for i, p in enumerate(plan) if p[3] > p[2]]
        wstats = {}
        if k_dist:
            gw = DeviceGroup([devs[i] for i in wm_idx])
            gw.set_option("group_serial", 1)
            for d in devs:
                d.kernel_timing(True)
            gw.witness_map([rhs[i] for i in wm_idx], [whs[i] for i in wm_idx], N)
            for d in devs:
                d.kernel_stats_reset()
            runs = []
            for _ in range(a.reps):
                gw.witness_map([rhs[i] for i in wm_idx], [whs[i] for i in wm_idx], N)
                runs.append(gw.rank_stats())
            for j, i in enumerate(wm_idx):
                gather_ms = devs[i].kernel_stats("group_gather_kernel")["ms"] / a.reps
                wstats[i] = dict(wm=float(np.median([run[j]["wm_ms"] for run in runs])), gather=gather_ms,
                                 ex=runs[0][j]["exchange_bytes"], h=runs[0][j]["h_bytes"])
            for d in devs:
                d.kernel_timing(False)
            gw.close()
        g.close()
        print("\nplan: G = %d ranks, k = %d witness-map ranks (%s); split witness map: %s (m = %d)" %
              (G, k, "cost model" if h_ranks == 0 else "forced", "k = %d" % k_dist if k_dist else "no, replicated", L["m"]))
        worst = 0.0
        for i, p in enumerate(plan):
            role = "wm+H" if p[3] > p[2] else "z"
            if p[1] > p[0] or p[4]:
                role += "+z"
            if i in wstats:
                w = wstats[i]
                xfer = (T * w["ex"] + w["h"]) / (a.bw * 1e9) * 1e3
                pred = w["wm"] - w["gather"] + xfer + share[i]
                print("  rank %d %-6s wm share %.2f ms (serial; gathers %.2f ms)  exchange %.1f MB x %d + h %.1f MB  H/z share %.2f ms"
                      "  -> predicted %.2f ms (exchanges %.2f ms at %.0f GB/s: UNMEASURED)" %
                      (i, role, w["wm"], w["gather"], w["ex"] / 1e6, T, w["h"] / 1e6, share[i], pred, xfer, a.bw))
            else:
                pred = share[i] + (wm_full if p[3] > p[2] else 0.0)
                print("  rank %d %-6s H/z share %.2f ms%s -> predicted %.2f ms" %
                      (i, role, share[i], " + replicated witness map %.2f ms" % wm_full if p[3] > p[2] else "", pred))
            worst = max(worst, pred)
        print("  group proof wall (measured, %s): %.2f ms" % ("one GPU shared by all ranks" if len(set(ids)) == 1 else "multi-GPU", wall))
        print("  predicted group time (slowest rank): %.2f ms, %.2fx the single-ctx proof" % (worst, single / worst))
        for i, sh in enumerate(shards):
            devs[i].pk_free(sh)
    for d, (ph, rh, wh) in zip(devs, hs):
        d.pk_free(ph)
        d.r1cs_free(rh)
        d.witness_free(wh)
    for d in devs:
        d.close()


if __name__ == "__main__":
    main()
