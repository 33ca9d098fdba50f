"""Window tables with packed against padded entries in one process (development probe, GPU box): one resident key, two whole copies
of it (zkg16_pk_slice), one with tables at table_stride = 1 and one at 2, proofs alternated between them.
   python tools/ab_table_stride.py <matrix_n> [rounds [window_bits_z [window_bits_h]]]
Per round and key: wall ms per proof, and HIP-event averages per launch of the two accumulation kernels (zkg16_kernel_timing = 2)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from zksnark_finalproject_amd import Device
from zksnark_finalproject_amd.device import verify
n = int(sys.argv[1])
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
cz = int(sys.argv[3]) if len(sys.argv) > 3 else 0
ch = int(sys.argv[4]) if len(sys.argv) > 4 else 0
dev = Device(0)
trap, g1, g2 = bench.draw_key_inputs(7)
c, _, desc = bench.synthesize("matrix", n)
rh = dev.r1cs_load(c.r1cs, c.num_vars)
ph, vk = dev.setup_resident(rh, c.num_instance, trap, g1, g2)
wh = dev.witness_load(c.z)
r, s = bench.fr_mont(12345), bench.fr_mont(67890)
ref = dev.prove_resident(ph, rh, wh, r, s)
print(desc, "verified:", verify(vk, c.public_inputs, *ref), flush=True)
n_h = (1 << (c.r1cs["num_constraints"] + c.num_instance - 1).bit_length()) - 1
keys = {}
for mode in (1, 2):
    h = dev.pk_slice(ph, 0, c.num_vars, 0, n_h, True)
    dev.set_option("table_stride", mode)
    t0 = time.perf_counter()
    added = dev.pk_precompute(h, cz, ch)
    print("table_stride=%d: pk_precompute %.2f s, %.3f GB added, widths %s" % (mode, time.perf_counter() - t0, added / 1e9, dev.pk_table_bits(h)), flush=True)
    keys[mode] = h
dev.set_option("table_stride", 0)
dev.pk_free(ph)
reps = 3 if n >= 100 else 8
res = {m: dict(wall=[], g1=[], g2=[]) for m in keys}
same = True
for rnd in range(rounds):
    for mode in ((1, 2) if rnd % 2 == 0 else (2, 1)):
        h = keys[mode]
        out = dev.prove_resident(h, rh, wh, r, s)
        same = same and np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
        t0 = time.perf_counter()
        for _ in range(reps):
            dev.prove_resident(h, rh, wh, r, s)
        wall = (time.perf_counter() - t0) / reps * 1e3
        dev.kernel_stats_reset()
        dev.kernel_timing(2)
        dev.prove_resident(h, rh, wh, r, s)
        dev.kernel_timing(0)
        k1, k2 = dev.kernel_stats("msm_accumulate_g1"), dev.kernel_stats("msm_accumulate_g2")
        a1, a2 = k1["ms"] / max(k1["launches"], 1), k2["ms"] / max(k2["launches"], 1)
        res[mode]["wall"].append(wall); res[mode]["g1"].append(a1); res[mode]["g2"].append(a2)
        print("round %d table_stride=%d  wall %.2f ms/proof   msm_accumulate_g1 avg %.3f ms (%d launches, sum %.2f)   msm_accumulate_g2 avg %.3f ms" %
              (rnd + 1, mode, wall, a1, k1["launches"], k1["ms"], a2), flush=True)
for mode in keys:
    for k in ("wall", "g1", "g2"):
        x = sorted(res[mode][k])
        print("n=%d table_stride=%d %-4s min %.3f median %.3f max %.3f" % (n, mode, k, x[0], x[len(x) // 2], x[-1]), flush=True)
print("proofs identical to the plain key's:", same, flush=True)
