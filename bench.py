#!/usr/bin/env python3
"""bench.py — Groth16 (BLS12-381) proofs/s + constraints/s on the reference's matrix-mul circuit, MI355X HIP path (libzkg16.so).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: setup (synthesis, real key, window tables), W warm-up proofs, K timed
proofs, the pairing check of the last one, the outputs of the last timed proof if --dump-outputs is given, and one JSON line.
Everything else the line can carry (the plain-key figure, the other workloads as legs, the end-to-end request legs, callers in
flight, the CPU baseline, per-stage times, roofline / alu figures) runs only with --full.

--dump-outputs DIR writes what the last timed step returned to its caller: DIR/proof.npy (the 48 proof words A | B | C, affine
Montgomery limbs, each split into its low and high 32-bit halves: float64, shape (48, 2), exact) and DIR/infinity.npy (the three
infinity flags, float64).  The key, the witness and every r, s are seeded, so the same arguments give the same proof on every run.

N > 1 without a torch.distributed environment: this process only spawns
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>` as a CHILD
(before anything touches torch or the GPU) and relays its output and exit code; under torchrun (WORLD_SIZE set) it asserts
WORLD_SIZE == --gpus and fails otherwise, so a 1-GPU number can never be reported as an N-GPU one.

One "step" = one pass of the hot path = one whole Groth16 proof of the workload (the inside of `Groth16::<Bls12_381>::prove`,
/root/reference/src/arkworks/backend/matrix_proof.rs:139-140: 3 SpMV + 7 NTT + 4 G1 MSM + 1 G2 MSM + tail) with the proving
key, the R1CS matrices and the full assignment already resident in HBM (zkg16_prove_resident).
Workload at N = 1 = the LARGEST single-GPU configuration of BASELINE.json: MatrixCircuit 128x128 + Poseidon — 10,706,932
constraints, 8,675,313 witness variables, domain 2^24 — synthesized by the C++ mirror of the reference's circuit on the
reference bench's all-ones inputs (bench/matrix.py:11).  The key is a REAL Groth16 key (zkg16_setup_resident from a seeded
trapdoor), and the last proof of the timed region is VERIFIED with the pairing verifier (zkg16_verify) after the region:
`proof_verified`; a failure exits non-zero.  Extra legs in the same JSON line (N = 1, --full): the 46x46 (largest 2^20 domain) and
32x32 (configs[1]) circuits, each verified; `end_to_end` = what the reference times as `proving_time` (host synthesis + the
host-pointer entry zkg16_prove); `cpu_baseline` = the CPU oracle (a port, oracle/) timed directly on the 32x32 circuit on all
host threads — its proof must equal the GPU's 32x32 proof bit for bit (`oracle_match`) — and on one thread at 16x16.

N > 1 (`--parallel shard`, default): ONE proof over N ranks with rank roles from zkg16_shard_plan (the first k ranks run the
witness map and share h_query; every rank takes the share of the z-side index ranges that lets all finish together), ONE
exchange per proof — an all_gather of 77 words of partial sums over RCCL — and the tail on every rank: strong scaling.
`--parallel replicas`: every rank proves its own proofs on the whole key, no exchange (weak scaling).

Prints ONE JSON line (rank 0).  With --full, `roofline` is for the dominant kernel (msm_accumulate_g1) from HIP-event pairs recorded on
the library's own stream during the timed region; `traffic` / `alu.peak` are read from the profile summaries committed under
profiles/ for this configuration (null when there is none).
"""
import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--matrix-n", type=int, default=128, help="n of the n x n matrix-mul circuit (128 = largest single-GPU config, 2^24 domain)")
    ap.add_argument("--workload", default="matrix", choices=["matrix", "prime"],
                    help="matrix = the reference's MatrixCircuit (metric workload); prime = the reference's PrimeCircuit (configs[4])")
    ap.add_argument("--legs", default="46,32,prime,fib1000",
                    help="N = 1, --full: further workloads measured after the timed region (comma list, '' = none): a number = that matrix size; "
                         "prime = the reference's PrimeCircuit (BASELINE configs[4]); fibN = FibonacciCircuit with N rounds (configs[0])")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and the oracle comparisons of the legs")
    ap.add_argument("--no-e2e", action="store_true", help="--full: skip the end-to-end (host synthesis + host-pointer prove) leg")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, one GPU per rank) | gloo (rehearsal: several ranks on one GPU)")
    ap.add_argument("--cpu-sample-n", type=int, default=32, help="matrix size the CPU baseline proves on all threads")
    ap.add_argument("--cpu-1t-n", type=int, default=16, help="matrix size the CPU baseline proves on one thread")
    ap.add_argument("--parallel", default="shard", choices=["shard", "replicas"],
                    help="N > 1: shard = one proof's index ranges over the ranks (north_star; strong scaling); "
                         "replicas = every rank proves its own proofs on the whole key (no exchange; weak scaling)")
    ap.add_argument("--h-ranks", type=int, default=0, help="N > 1, shard: ranks that run the witness map (0 = cost model; N = equal split)")
    ap.add_argument("--in-flight", type=int, default=2,
                    help="N = 1, --full: after the timed region, also report throughput with this many callers on the one ctx (its lanes share the key; 0 = skip)")
    ap.add_argument("--replicas-leg", action="store_true",
                    help="N > 1, shard: after the timed sharded region also time every rank proving its own proofs on the whole key (weak "
                         "scaling; keeps the whole key + its tables on every rank, so off by default: the timed leg must not be lost to it)")
    ap.add_argument("--no-replicas-leg", action="store_true", help="(default since round 3; accepted for older command lines)")
    ap.add_argument("--tables", default="auto", choices=["auto", "on", "off"],
                    help="auto = window tables for the resident key (zkg16_pk_precompute; with --full the plain key is timed first and "
                         "reported beside it); on = the same without the plain-key proofs (profiling runs); off = plain key only")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure: the plain-key figure (--tables auto), --legs, "
                         "the end-to-end legs, --in-flight, the CPU baseline, per-stage times and the roofline / alu figures")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed proof as DIR/proof.npy and DIR/infinity.npy (float64; see the module docstring)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def spawn_ranks(args):
    """--gpus N > 1 outside torchrun: launch N ranks as a child process, before this process has touched torch or the GPU."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.stderr.write("bench.py: spawning %d ranks: %s\n" % (args.gpus, " ".join(cmd)))
    sys.exit(subprocess.call(cmd, env=env))


def fr_mont(x):
    v = (x << 256) % R_MOD
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def draw_key_inputs(seed):
    """The trapdoor (tau, alpha, beta, gamma, delta) and generators a request would draw from its rng (upstream: generator.rs)."""
    import random
    from zksnark_finalproject_amd.device import scalar_mul
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    rng = random.Random(seed)
    trap = np.stack([fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    return trap, scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]


def synthesize(workload, n, x=None):
    """-> (SynthesizedCircuit, seconds, description).  matrix: all-ones n x n inputs as bench/matrix.py:11."""
    t0 = time.perf_counter()
    if workload.startswith("fib"):
        from zksnark_finalproject_amd.circuits import fibonacci_circuit
        rounds = int(workload[3:] or n)
        circ = fibonacci_circuit(0, 1, rounds)           # bench/fibo.py:26-34: a = 0, b = 1
        desc = ("FibonacciCircuit mirror, %d rounds (BASELINE configs[0]): %d constraints, %d witness vars, domain 2^%d"
                % (rounds, circ.num_constraints, circ.num_witness, circ.domain.bit_length() - 1))
    elif workload == "prime":
        from zksnark_finalproject_amd.circuits import prime_circuit
        circ = prime_circuit(0x123456789ABCDEF if x is None else x, 32, check_satisfied=False)      # (the satisfaction check is a test convenience)
        desc = ("Fermat-prime circuit (PrimeCircuit mirror, BASELINE configs[4]: SHA-256 + 3 Fermat bases, 20-bit modpow): %d constraints, "
                "%d witness vars, domain 2^%d" % (circ.num_constraints, circ.num_witness, circ.domain.bit_length() - 1))
    else:
        from zksnark_finalproject_amd.circuits import matrix_circuit
        ones = np.ones((n, n), dtype=np.uint64)
        circ = matrix_circuit(ones, ones)
        desc = ("matrix-mul %dx%d + Poseidon MatrixCircuit: %d constraints, %d witness vars, domain 2^%d"
                % (n, n, circ.num_constraints, circ.num_witness, circ.domain.bit_length() - 1))
    return circ, time.perf_counter() - t0, desc


def dump_outputs(d, proof, inf):
    """--dump-outputs: the proof words as exact float64 32-bit halves (low, high) and the infinity flags."""
    os.makedirs(d, exist_ok=True)
    w = np.asarray(proof, dtype=np.uint64).reshape(48)
    np.save(os.path.join(d, "proof.npy"), np.stack([w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)], axis=1).astype(np.float64))
    np.save(os.path.join(d, "infinity.npy"), np.asarray(inf, dtype=np.float64).reshape(3))


def profile_lookup(key):
    """Numbers that come from committed profile summaries (profiles/bench_constants_r3.json, else _r2: written by
    tools/pmc_to_json.py from the rocprofv3 --pmc / microbench logs next to it); None when no summary has the entry."""
    for name in ("bench_constants_r3.json", "bench_constants_r2.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                cur = json.load(f)
        except (OSError, ValueError):
            continue
        for k in key:
            if not isinstance(cur, dict) or k not in cur:
                cur = None
                break
            cur = cur[k]
        if cur is not None:
            return cur
    return None


def cpu_baseline(dev, args, gpu_proofs, key_inputs, rs, headline_nc):
    """Times the CPU oracle (a port of the arkworks algorithms; oracle/) directly: the 32x32 MatrixCircuit on all host threads
    (its proof is compared with the GPU's for the same key, r, s) and the 16x16 one on a single thread."""
    sys.path[:0] = [os.path.join(ROOT, "oracle")]
    import oracle as orc
    trap, g1, g2 = key_inputs
    threads = min(os.cpu_count() or 1, 16)

    def host_key(n):
        circ, _, _ = synthesize("matrix", n)
        rh = dev.r1cs_load(circ.r1cs, circ.num_vars)
        pk, vk = dev.setup(rh, circ.num_instance, circ.num_vars, circ.domain, trap, g1, g2)      # untimed: the timed part is the CPU prover alone
        dev.r1cs_free(rh)
        return circ, pk

    out = {"kind": "port", "unit": "proofs/s"}
    n = args.cpu_sample_n
    circ, pk = host_key(n)
    used = orc.set_threads(threads)
    r, s = rs
    t0 = time.perf_counter()
    oproof, oinf = orc.prove(pk, r, s, circ.r1cs, circ.z)
    dt = time.perf_counter() - t0
    out["cores"] = used
    out["measured"] = {"n": n, "constraints": circ.num_constraints, "seconds": dt, "proofs_per_sec": 1.0 / dt,
                       "constraints_per_sec": circ.num_constraints / dt, "cores": used}
    if n in gpu_proofs:             # the GPU's proof of the same circuit under the same key, r, s
        out["oracle_match"] = bool(np.array_equal(oproof, gpu_proofs[n][0]) and np.array_equal(oinf, gpu_proofs[n][1]))
    del pk
    n1 = args.cpu_1t_n
    circ1, pk1 = host_key(n1)
    orc.set_threads(1)
    t0 = time.perf_counter()
    orc.prove(pk1, r, s, circ1.r1cs, circ1.z)
    dt1 = time.perf_counter() - t0
    orc.set_threads(threads)
    out["one_thread"] = {"n": n1, "constraints": circ1.num_constraints, "seconds": dt1, "proofs_per_sec": 1.0 / dt1,
                         "constraints_per_sec": circ1.num_constraints / dt1, "cores": 1}
    # the metric's unit on the headline workload: scaled by constraint count from the all-threads measurement
    out["value"] = (circ.num_constraints / dt) / headline_nc
    out["sample"] = ("MEASURED: oracle prove of the %dx%d MatrixCircuit (%d constraints) in %.2f s on %d threads (OpenMP: one task per MSM "
                     "window, as ark's `parallel` feature) and of the %dx%d one (%d constraints) in %.2f s on 1 thread; %s"
                     % (n, n, circ.num_constraints, dt, used, n1, n1, circ1.num_constraints, dt1,
                        "`value` = that all-threads measurement: it IS the headline circuit (--cpu-sample-n = --matrix-n)" if circ.num_constraints == headline_nc else
                        "SCALED: `value` = the all-threads constraints/s divided by the headline circuit's %d constraints (--cpu-sample-n %d measures "
                        "the headline circuit itself: ~70 s)" % (headline_nc, args.matrix_n)))
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)           # never returns
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: refusing to report a %d-rank run as %d GPUs\n" % (args.gpus, world, world, args.gpus))
        sys.exit(2)
    import torch
    dist = None
    on_gpu = args.dist_backend == "nccl"
    dev_index = local_rank if (world > 1 and on_gpu) else int(os.environ.get("ZKG16_BENCH_DEVICE", "0"))
    if world > 1:
        import torch.distributed as dist
        if on_gpu:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo")
        if dist.get_world_size() != args.gpus:
            sys.stderr.write("bench.py: process group has %d ranks, --gpus %d\n" % (dist.get_world_size(), args.gpus))
            sys.exit(2)
    from zksnark_finalproject_amd import Device
    from zksnark_finalproject_amd.device import shard_plan, verify, z_costs

    dev = Device(dev_index)
    sharded = world > 1 and args.parallel == "shard"
    key_inputs = draw_key_inputs(args.seed)           # same seed on every rank -> the same key on every rank
    trap, g1, g2 = key_inputs

    circ, synth_s, desc = synthesize(args.workload, args.matrix_n)
    shp = dict(nc=circ.num_constraints, num_instance=circ.num_instance, num_witness=circ.num_witness, num_vars=circ.num_vars, domain=circ.domain)
    rh = dev.r1cs_load(circ.r1cs, circ.num_vars)
    t0 = time.perf_counter()
    ph, vk = dev.setup_resident(rh, circ.num_instance, trap, g1, g2)
    setup_s = time.perf_counter() - t0
    plan, h_ranks, full = None, 1, None
    if sharded:
        plan, h_ranks = shard_plan(world, circ.num_vars, circ.domain - 1, 0.0, args.h_ranks, z_costs(circ.r1cs, circ.z, circ.num_instance),
                                   window_tables=args.tables != "off")
        z_lo, z_hi, h_lo, h_hi, blind = plan[rank]
        full = ph
        ph = dev.pk_slice(full, z_lo, z_hi, h_lo, h_hi, blind)      # device-to-device
        if not args.replicas_leg:
            dev.pk_free(full)                                       # the whole key is dropped again
            full = None
    wh = dev.witness_load(circ.z)
    rng = np.random.default_rng(99)
    rs = [(fr_mont(int.from_bytes(rng.bytes(31), "little")), fr_mont(int.from_bytes(rng.bytes(31), "little"))) for _ in range(args.steps + args.warmup + 2)]

    def with_tables(d, pk_h, prove_once, plain_steps=0):
        """Window tables for a key that stays resident; with prove_once (--full) the plain key is timed first (a few proofs) so both
        appear in the line."""
        if args.tables == "off":
            return None
        plain_ms, plain = None, None
        if prove_once is not None and args.tables == "auto":
            for _ in range(max(1, min(args.warmup, 2))):
                prove_once()
            k = max(3, plain_steps)
            torch.cuda.synchronize()
            gc.collect()                 # a cyclic collection that unmaps the previous workload's arrays mid-loop stalls every thread of
            gc.disable()                 # the process (seen: one 50 ms proof among ten 12.4 ms ones)
            t_ = time.perf_counter()
            each = []
            for _ in range(k):
                t1_ = time.perf_counter()
                prove_once()
                each.append((time.perf_counter() - t1_) * 1e3)
            torch.cuda.synchronize()
            plain_ms = (time.perf_counter() - t_) / k * 1e3
            gc.enable()
            if os.environ.get("ZKG16_BENCH_TRACE"):
                sys.stderr.write("plain-key proofs (ms): %s\n" % " ".join("%.2f" % x for x in each))
            plain = {"ms_per_step": plain_ms, "value": 1e3 / plain_ms, "unit": "proofs/s", "steps": k, "median_ms": sorted(each)[k // 2],
                     "note": "the key as the reference's per-request setup produces it (no window tables): the like-for-like figure"}
        t_ = time.perf_counter()
        added = d.pk_precompute(pk_h)
        pre_s = time.perf_counter() - t_
        bz, bh = d.pk_table_bits(pk_h)
        return {"window_bits_z": bz, "window_bits_h": bh, "table_bytes": added, "precompute_s": pre_s, "plain_key_ms_per_proof": plain_ms,
                "plain_key": plain,
                "note": "zkg16_pk_precompute: 2^(c w) multiples of every base kept in HBM, all digits of a scalar in one bucket set per MSM; "
                        "same proofs bit for bit (tests/test_gpu_parity.py::test_window_tables_*); built once per resident key"}
    tables_info = with_tables(dev, ph, (lambda: dev.prove_resident(ph, rh, wh, *rs[0])) if (world == 1 and args.full) else None,
                              plain_steps=args.steps)

    xdev = "cuda" if on_gpu else "cpu"
    if sharded:
        gather_buf = [torch.empty(77, dtype=torch.int64, device=xdev) for _ in range(world)]

    def one_proof(r, s):
        if not sharded:
            return dev.prove_resident(ph, rh, wh, r, s)
        part, pinf = dev.prove_partial(ph, rh, wh, r, s)
        rec = np.concatenate([part.view(np.int64), pinf.astype(np.int64)])
        dist.all_gather(gather_buf, torch.from_numpy(rec).to(xdev))        # the single exchange: 77 words per rank over xGMI
        allrec = torch.stack(gather_buf).cpu().numpy()
        parts = allrec[:, :72].copy().view(np.uint64)
        pinfs = allrec[:, 72:].astype(np.uint8)
        return dev.prove_finish(ph, r, s, parts, pinfs)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    proof = inf = None
    for i in range(args.warmup):
        proof, inf = one_proof(*rs[i])
    if args.full:
        dev.kernel_stats_reset()
        dev.kernel_timing(2)         # async HIP-event pairs around the bucket accumulations (the roofline kernel) on the
                                     # library's own streams; resolved after the timed region
    gc.collect()
    gc.disable()                     # no cyclic collection inside the timed region (see with_tables)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        proof, inf = one_proof(*rs[args.warmup + i])
    barrier()
    dt = time.perf_counter() - t0
    gc.enable()
    if args.full:
        dev.kernel_timing(False)
    per_rank = None
    if world > 1:
        # every rank's own time of the timed region, so that the curve can be read against the per-shard predictions
        # (profiles/shard_timing_r2b.txt): the witness-map ranks are expected to be the floor
        mine = torch.tensor([dt], dtype=torch.float64, device=xdev)
        allt = [torch.empty(1, dtype=torch.float64, device=xdev) for _ in range(world)]
        dist.all_gather(allt, mine)
        per_rank = [float(x.item()) / args.steps * 1e3 for x in allt]
        t = torch.tensor([dt], dtype=torch.float64, device=xdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    # ---- correctness gate, outside the timed region: the last timed proof must satisfy the Groth16 pairing equation for the real key
    verified = verify(vk, circ.public_inputs, proof, inf) if proof is not None else False
    if world > 1:
        flag = torch.tensor([1 if verified else 0], dtype=torch.int64, device=xdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        verified = bool(flag.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, proof, inf)
    stages = term_counts = acc = acc2 = acc_waves = None
    if args.full:
        stages = dev.last_timings()
        term_counts = dev.last_term_counts()      # sorted term-list lengths of the last proof: exact mixed additions per MSM
        acc = dev.kernel_stats("msm_accumulate_g1")
        acc2 = dev.kernel_stats("msm_accumulate_g2")
        acc_waves = dev.last_acc_waves()

    tabled = bool(tables_info and (tables_info["window_bits_z"] or tables_info["window_bits_h"]))
    cfg_key = ("n%d" % args.matrix_n if args.workload == "matrix" else args.workload) + ("_tables" if tabled else "")
    extra_out = {}
    if rank == 0 and world == 1 and args.full:
        # ---- stand-alone witness map and one transform of the workload's domain (second kernel family of the path)
        try:
            log_n = shp["domain"].bit_length() - 1
            dev.bench_ntt(log_n, 1, 1, 2)
            ntt_ms = dev.bench_ntt(log_n, 1, 1, 10)
            gbs = 64.0 * shp["domain"] / (ntt_ms * 1e-3) / 1e9
            extra_out["roofline_ntt"] = {"bound": "hbm", "kernel": "ntt_pass_cols_u + ntt_pass_rows_u (one coset-inverse transform of 2^%d)" % log_n,
                                         "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0, "ms": ntt_ms, "transforms_per_proof": 7,
                                         "traffic": profile_lookup([cfg_key, "ntt_transform_traffic_bytes"]),      # same profile run as roofline.traffic
                                         "note": "64 algorithmic bytes per element (read once, written once); integer-ALU bound too"}
            extra_out["witness_map_standalone_ms"] = dev.bench_witness_map(rh, wh, 3)
        except Exception as e:      # noqa: BLE001 - an extra leg must never cost the contract line
            extra_out["roofline_ntt"] = {"error": repr(e)}

        # ---- end to end = the reference's `proving_time` (matrix_proof.rs:138-145): Groth16::prove re-synthesizes the circuit on
        # the host and hands matrices + assignment to the prover; here: C++ synthesis + zkg16_prove (host pointers, uploads inside)
        if not args.no_e2e:
            try:
                r, s = rs[-1]
                first = None
                for _ in range(2):          # a server's steady state: the second request (the first also allocates the pinned upload ring)
                    t1 = time.perf_counter()
                    c2, syn2, _ = synthesize(args.workload, args.matrix_n)
                    t2 = time.perf_counter()
                    p2, i2 = dev.prove(ph, r, s, c2.r1cs, c2.z)
                    t3 = time.perf_counter()
                    if first is None:
                        first = t3 - t1
                ok2 = verify(vk, c2.public_inputs, p2, i2)
                e2e = {"seconds": t3 - t1, "proofs_per_sec": 1.0 / (t3 - t1), "constraints_per_sec": shp["nc"] / (t3 - t1),
                       "host_synthesis_s": t2 - t1, "prove_host_pointers_s": t3 - t2, "first_request_s": first, "proof_verified": bool(ok2),
                       "what": "the full first-request path: matrices + assignment synthesized on the host, everything uploaded inside zkg16_prove",
                       "note": "host synthesis (C++ mirror, full R1CS + assignment) + zkg16_prove with host pointers (matrices and "
                               "assignment uploaded over PCIe inside the call); the key stays resident, as the reference holds its pk"}
                if args.workload == "matrix":
                    # a server that kept the matrices of this size (they depend on n alone).  Per request only the assignment:
                    # built ON THE DEVICE from the host sponges' entering states (zkg16_witness_matrix), then the resident proof
                    ones = np.ones((args.matrix_n, args.matrix_n), dtype=np.uint64)
                    best = None
                    for _ in range(3):
                        t1 = time.perf_counter()
                        p3, i3, pub2, pms = dev.prove_matrix(ph, rh, ones, ones, r, s)
                        t2 = time.perf_counter()
                        if best is None or t2 - t1 < best[0]:
                            best = (t2 - t1, pms)
                    e2e["cached_matrices"] = {"seconds": best[0], "proofs_per_sec": 1.0 / best[0], "constraints_per_sec": shp["nc"] / best[0],
                                              "host_sponges_ms": best[1]["host_sponges_ms"], "assignment_parts": best[1]["parts"],
                                              "same_proof": bool(np.array_equal(p3, p2)), "public_inputs_match": bool(np.array_equal(pub2, c2.public_inputs)),
                                              "proof_verified": bool(verify(vk, pub2, p3, i3)),
                                              "note": "best of 3: zkg16_prove_matrix on the matrices kept per size — the three native Poseidon sponges "
                                                      "(sequential by construction, hasher.rs:17-27) run on three host threads and feed the device in "
                                                      "growing slices; kernels write z in place and the z-side MSMs run in rounds on the parts that "
                                                      "exist while the sponges still compute the rest; the witness map and H follow the last part"}
                    # the same request without the overlap: assignment on the device first (zkg16_witness_matrix), then the resident proof
                    best = None
                    for _ in range(2):
                        t1 = time.perf_counter()
                        w2, pub3, wms = dev.witness_matrix(ones, ones)
                        t2 = time.perf_counter()
                        p5, i5 = dev.prove_resident(ph, rh, w2, r, s)
                        t3 = time.perf_counter()
                        dev.witness_free(w2)
                        if best is None or t3 - t1 < best[0]:
                            best = (t3 - t1, t2 - t1, t3 - t2, wms)
                    e2e["cached_matrices_two_step"] = {"seconds": best[0], "assignment_on_device_s": best[1], "host_sponges_ms": best[3]["host_sponges_ms"],
                                                       "assignment_kernels_ms": best[3]["device_ms"], "prove_resident_s": best[2],
                                                       "same_proof": bool(np.array_equal(p5, p2))}
                    # a FIRST request with nothing synthesized on the host: the matrices written by kernels (zkg16_r1cs_matrix), then the
                    # overlapped assignment + proof (the key stays resident, as in the legs above)
                    t1 = time.perf_counter()
                    rh_dev = dev.r1cs_matrix(args.matrix_n)
                    t2 = time.perf_counter()
                    p6, i6, pub6, _ = dev.prove_matrix(ph, rh_dev, ones, ones, r, s)
                    t3 = time.perf_counter()
                    dev.r1cs_free(rh_dev)
                    e2e["first_request_device"] = {"seconds": t3 - t1, "matrices_on_device_s": t2 - t1, "prove_matrix_s": t3 - t2,
                                                   "same_proof": bool(np.array_equal(p6, p2)),
                                                   "note": "zkg16_r1cs_matrix (the three CSR matrices written by kernels from one template per "
                                                           "Poseidon-permutation class + matrix_mul's closed form: nothing synthesized on the host, "
                                                           "nothing uploaded) + zkg16_prove_matrix; to be read beside `seconds` / "
                                                           "`host_synthesis_s` above, the same request with host synthesis"}
                    # the reference's WHOLE request (matrix_proof.rs:96-160): the key is regenerated for every request
                    # (Groth16::setup at :129), so no window tables — device setup into a resident key, the streamed proof on it,
                    # proof + prepared key encoded; through the handler mirror, second request of the size (matrices kept)
                    try:
                        from zksnark_finalproject_amd import handlers
                        for it in range(2):
                            t1 = time.perf_counter()
                            hres = handlers.prove_matrix(dev, args.matrix_n, ones, ones, seed=it)
                            t2 = time.perf_counter()
                        hver = handlers.verify_proof(hres["pvk"], hres["_circuit"].public_inputs, hres["proof"])
                        e2e["request_with_setup"] = {"seconds": t2 - t1, "setup_s": hres["setup_time"], "proving_s": hres["proving_time"],
                                                     "verifying_s": hver["verifying_time"], "proof_verified": bool(hver["valid"]),
                                                     "note": "handler mirror: zkg16_setup_resident (fresh trapdoor and generators) + "
                                                             "zkg16_prove_matrix on the plain key + wire encoding; the reference's request "
                                                             "does exactly these steps per call"}
                        del hres
                    except Exception as e:      # noqa: BLE001
                        e2e["request_with_setup"] = {"error": repr(e)}
                    # the round-2 form of the same request, for comparison: assignment built on the host, uploaded over PCIe
                    from zksnark_finalproject_amd.circuits import matrix_witness
                    t1 = time.perf_counter()
                    z2 = matrix_witness(ones, ones, shp["num_vars"])
                    w2 = dev.witness_load(z2)
                    p4, i4 = dev.prove_resident(ph, rh, w2, r, s)
                    t2 = time.perf_counter()
                    dev.witness_free(w2)
                    e2e["cached_matrices_host_assignment"] = {"seconds": t2 - t1, "same_proof": bool(np.array_equal(p4, p2))}
                    del z2
                del c2
                extra_out["end_to_end"] = e2e
            except Exception as e:      # noqa: BLE001
                extra_out["end_to_end"] = {"error": repr(e)}

    # ---- N > 1, shard: the same ranks as independent provers (every rank its own proofs on the whole key, no exchange) — the
    # throughput a server farm would get from N GPUs, beside the one-proof latency the sharded path is about
    replicas = None
    if sharded and args.replicas_leg and full is not None:
        k_r = max(2, min(args.steps, 5))
        dt_r, ok_r, err_r = float("inf"), False, None
        barrier()
        try:
            if args.tables != "off" and args.dist_backend == "nccl":      # (rehearsals put several ranks on one GPU: no room for N tables)
                dev.pk_precompute(full)
            p_r = dev.prove_resident(full, rh, wh, *rs[0])
            torch.cuda.synchronize()
            t_r = time.perf_counter()
            for j in range(k_r):
                p_r = dev.prove_resident(full, rh, wh, *rs[j % len(rs)])
            torch.cuda.synchronize()
            dt_r = time.perf_counter() - t_r
            ok_r = bool(verify(vk, circ.public_inputs, *p_r))
        except Exception as e:      # noqa: BLE001 - every rank still reaches the reduction below
            err_r = repr(e)
        t_all = torch.tensor([dt_r if ok_r else 1e30], dtype=torch.float64, device=xdev)
        dist.all_reduce(t_all, op=dist.ReduceOp.MAX)
        worst = float(t_all.item())
        replicas = ({"value": world * k_r / worst, "unit": "proofs/s", "proofs_per_rank": k_r, "ms_per_proof_per_rank": worst / k_r * 1e3,
                     "scaling": "weak", "proofs_verified": True,
                     "note": "every rank proves its own proofs on the whole key (window tables when each rank has its own GPU), no exchange; "
                             "max over ranks; outside the contract's timed region"} if worst < 1e29 else {"error": err_r or "a rank failed"})
        dev.pk_free(full)

    def callers_on_one_ctx(p_h, r_h, w_h, per, base_rate):
        """several callers on ONE ctx: its lanes share the resident key, the window tables, the matrices and the assignment"""
        import threading
        dev.set_option("lanes", args.in_flight)

        def caller(count):
            for j in range(count):
                dev.prove_resident(p_h, r_h, w_h, *rs[j % len(rs)])
        for count in (1, per):       # the first round creates the lanes and their workspaces
            ths = [threading.Thread(target=caller, args=(count,)) for _ in range(args.in_flight)]
            barrier()
            t1 = time.perf_counter()
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            barrier()
            dt2 = time.perf_counter() - t1
        total = per * args.in_flight
        lanes_used = sorted({l for l, _, _ in dev.lane_log(total)})
        dev.set_option("lanes", 2)
        return {"proofs_in_flight": args.in_flight, "proofs": total, "value": total / dt2, "unit": "proofs/s",
                "ms_per_proof": dt2 / total * 1e3, "lanes_used": lanes_used, "vs_one_at_a_time": (total / dt2) / base_rate,
                "note": "ONE library ctx, %d host threads calling zkg16_prove_resident on the same handles: the ctx's lanes (own streams + "
                        "workspaces each) share the resident key, its window tables, the matrices and the assignment; outside the "
                        "contract's timed region" % args.in_flight}

    in_flight = None
    if world == 1 and args.in_flight > 1 and args.full:
        try:
            in_flight = callers_on_one_ctx(ph, rh, wh, max(args.steps, 4), args.steps / dt)
        except Exception as e:      # noqa: BLE001
            in_flight = {"error": repr(e)}

    # ---- free the headline workload before the smaller legs
    headline_z = circ.z
    headline_gpu_proof = None
    if world == 1 and args.full and not args.no_cpu_baseline and args.workload == "matrix" and args.cpu_sample_n == args.matrix_n:
        headline_gpu_proof = dev.prove_resident(ph, rh, wh, *rs[-1])      # what the CPU baseline's proof of the headline circuit must equal
    for f, h in ((dev.pk_free, ph), (dev.witness_free, wh), (dev.r1cs_free, rh)):
        f(h)
    del circ

    legs = []
    gpu_proofs = {}                 # matrix size -> the GPU's proof for (key_inputs, rs[-1]): what the CPU baseline's proof must equal
    if headline_gpu_proof is not None:
        gpu_proofs[args.matrix_n] = headline_gpu_proof
    if rank == 0 and world == 1 and args.full and args.workload == "matrix":
        for leg in [x.strip() for x in args.legs.split(",") if x.strip()]:
            try:
                wl, n = ("matrix", int(leg)) if leg.isdigit() else (leg, 0)
                c, syn, d_ = synthesize(wl, n)
                r_h = dev.r1cs_load(c.r1cs, c.num_vars)
                t1 = time.perf_counter()
                p_h, v_k = dev.setup_resident(r_h, c.num_instance, trap, g1, g2)
                set_s = time.perf_counter() - t1
                w_h = dev.witness_load(c.z)
                k = max(3, min(args.steps, 20))
                leg_tables = with_tables(dev, p_h, lambda: dev.prove_resident(p_h, r_h, w_h, *rs[0]), plain_steps=k)
                dev.prove_resident(p_h, r_h, w_h, *rs[0])
                torch.cuda.synchronize()
                gc.collect()
                gc.disable()
                t1 = time.perf_counter()
                for j in range(k):
                    pr, pi = dev.prove_resident(p_h, r_h, w_h, *rs[j % (len(rs) - 1)])
                torch.cuda.synchronize()
                d1 = (time.perf_counter() - t1) / k
                gc.enable()
                pr, pi = dev.prove_resident(p_h, r_h, w_h, *rs[-1])
                if wl == "matrix":
                    gpu_proofs[n] = (pr, pi)
                rec = {"workload": d_, "n": n if wl == "matrix" else leg, "ms_per_step": d1 * 1e3, "value": 1.0 / d1, "unit": "proofs/s", "steps": k,
                       "constraints_per_sec": c.num_constraints / d1, "proof_verified": bool(verify(v_k, c.public_inputs, pr, pi)),
                       "setup_resident_s": set_s, "host_synthesis_s": syn, "stage_ms_last_proof": dev.last_timings(),
                       "window_tables": leg_tables}
                if wl == "matrix" and args.in_flight > 1:
                    try:
                        rec["throughput_in_flight"] = callers_on_one_ctx(p_h, r_h, w_h, max(k, 10), 1.0 / d1)
                    except Exception as e:      # noqa: BLE001
                        rec["throughput_in_flight"] = {"error": repr(e)}
                for f, h in ((dev.pk_free, p_h), (dev.witness_free, w_h)):
                    f(h)
                if wl != "matrix" and not args.no_cpu_baseline:
                    # the CPU oracle proves these in seconds: same key (same trapdoor, through the host this time), same r, s ->
                    # the proof bytes must be equal
                    try:
                        sys.path[:0] = [os.path.join(ROOT, "oracle")]
                        import oracle as orc
                        pk_host, _ = dev.setup(r_h, c.num_instance, c.num_vars, c.domain, trap, g1, g2)
                        orc.set_threads(min(os.cpu_count() or 1, 16))
                        t1 = time.perf_counter()
                        op, oi = orc.prove(pk_host, rs[-1][0], rs[-1][1], c.r1cs, c.z)
                        rec["oracle_seconds"] = time.perf_counter() - t1
                        rec["oracle_match"] = bool(np.array_equal(op, pr) and np.array_equal(oi, pi))
                        del pk_host
                    except Exception as e:      # noqa: BLE001
                        rec["oracle_match"] = None
                        rec["oracle_error"] = repr(e)
                dev.r1cs_free(r_h)
                legs.append(rec)
            except Exception as e:      # noqa: BLE001
                legs.append({"n": leg, "error": repr(e)})

    if rank == 0:
        total_proofs = args.steps * (world if (world > 1 and not sharded) else 1)
        out = {
            "metric": "groth16_proofs_per_sec", "value": total_proofs / dt, "unit": "proofs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if (sharded or world == 1) else "weak", "vs_baseline": None, "dtype": "u32",
            "data": "the reference's circuit on its bench driver's inputs (all-ones matrices, bench/matrix.py:11); real Groth16 key from a seeded trapdoor",
            "proof_verified": bool(verified),
            "config": {"workload": desc + "; pk/R1CS/assignment resident in HBM; real key (zkg16_setup_resident)" +
                                   (" with window tables (zkg16_pk_precompute)" if tables_info and (tables_info["window_bits_z"] or tables_info["window_bits_h"]) else "") +
                                   ", last timed proof verified (zkg16_verify)",
                       "parallelism": "1 GPU" if world == 1 else
                                      ("%d GPUs, one proof: %d rank(s) run the witness map and share h_query, z-side index ranges by cost model "
                                       "(zkg16_shard_plan); 1 all_gather(77 words)/proof" % (world, h_ranks) if sharded else
                                       "%d replicas: every GPU proves its own proofs on the whole key, no exchange" % world)},
            "constraints_per_sec": shp["nc"] * total_proofs / dt,
            "setup_resident_s": setup_s, "host_synthesis_s": synth_s,
        }
        if args.full:
            # algorithmic bytes of one G1 bucket-accumulation launch: every (base, scalar) term once = (96 + 32) B per term
            # (SURVEY.md 8d); terms per launch = what the launches of this rank actually processed (event-pair units)
            launches = max(acc["launches"], 1)
            terms_per_launch = acc["units"] / launches
            alg_bytes = 128.0 * terms_per_launch
            avg_ms = acc["ms"] / launches
            achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            traffic = profile_lookup([cfg_key, "msm_accumulate_g1_traffic_bytes"]) if world == 1 else None
            out["stage_ms_last_proof"] = stages
            out["roofline"] = {"bound": "hbm", "kernel": "msm_accumulate_g1", "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                               "frac": achieved / 8000.0, "traffic": traffic,
                               "avg_launch_ms": avg_ms, "launches": acc["launches"], "algorithmic_bytes_per_launch": alg_bytes,
                               "terms_per_launch": terms_per_launch,
                               "note": "integer-ALU bound by construction: one XYZZ mixed addition = 8 products + 2 squarings in Fq (3,542 "
                                       "v_mad_u64_u32) per window per 128 algorithmic bytes; traffic = PMC FETCH+WRITE of the same command from "
                                       "profiles/ (one 96-byte base or table entry gathered per (scalar, window) term); g2 accumulate avg %.3f ms"
                                       % (acc2["ms"] / max(acc2["launches"], 1))}
        if plan is not None:
            out["config"]["shard_plan"] = [{"rank": i, "z": [p[0], p[1]], "h": [p[2], p[3]], "blinding": p[4],
                                            "role": ("witness map + h share" if p[3] > p[2] else "") + (" + " if p[3] > p[2] and p[1] > p[0] else "") +
                                                    ("z share" if p[1] > p[0] else ""),
                                            "ms_per_step": per_rank[i] if per_rank else None} for i, p in enumerate(plan)]
        if per_rank:
            out["per_rank_ms_per_step"] = per_rank
            out["slowest_rank"] = int(np.argmax(per_rank))
        # the bound that does apply: mixed additions per second against the same addition in a bare register-resident loop
        nshard = world if sharded else 1
        if world == 1 and args.full:
            one = fr_mont(1)
            zz = np.asarray(headline_z, dtype=np.uint64).reshape(-1, 4)
            n_one = int(np.all(zz == one, axis=1).sum())
            n_zero = int(np.all(zz == 0, axis=1).sum())
            nz, nh = zz.shape[0], shp["domain"] - 1

            def nwin(n, table_bits):
                if table_bits:
                    return 254 // table_bits + 1
                return 254 // (17 if n >= (1 << 23) else 16 if n >= (1 << 20) else 15 if n >= (1 << 17) else 13 if n >= (1 << 14) else max(4, n.bit_length() - 4)) + 1
            z_entries = (nz - n_one - n_zero) * nwin(nz, tables_info["window_bits_z"] if tables_info else 0) + n_one
            h_entries = nh * nwin(nh, tables_info["window_bits_h"] if tables_info else 0)
            est = (3 * z_entries + h_entries) / 4.0
            # exact: A and L walk the z list, B1 the B list (or the z list), H the h list — lengths read back from the device
            zc, bc, hc = term_counts
            exact = (2 * zc + (bc if bc else zc) + hc) / 4.0
            gadd = exact / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            # the bare register-resident loop at the occupancy the launches actually used (waves per SIMD read back from the plans;
            # launches at different occupancies are weighted by their additions), and the multiplier's own bound beside it
            by_waves = profile_lookup(["alu", "madd_g1_bare_gadd_per_s_by_waves"]) or {}
            lists = [(zc, acc_waves[0], 2.0), ((bc if bc else zc), acc_waves[1] if bc else acc_waves[0], 1.0), (hc, acc_waves[2], 1.0)]
            wsum = sum(cnt * mult for cnt, _, mult in lists)
            peak = None
            if by_waves and wsum > 0 and all(str(w) in by_waves for cnt, w, _ in lists if cnt):
                # time-weighted (harmonic) mean of the bare rates: total additions / sum of (additions / rate)
                peak = wsum / sum(cnt * mult / by_waves[str(w)] for cnt, w, mult in lists if cnt)
            if peak is None:
                peak = profile_lookup(["alu", "madd_g1_bare_gadd_per_s"])
            mad_bound = profile_lookup(["alu", "mad_bound_gadd_per_s"])
            try:
                res_g1, res_g2 = dev.acc_resident_waves()
            except Exception:      # noqa: BLE001
                res_g1 = res_g2 = None
            peak_res = by_waves.get(str(res_g1)) if res_g1 else None
            out["alu"] = {"kernel": "msm_accumulate_g1", "achieved": gadd, "peak": peak, "unit": "G mixed additions/s",
                          "frac": (gadd / peak) if peak else None,
                          "waves_per_simd": {"z": acc_waves[0], "b": acc_waves[1], "h": acc_waves[2]},
                          # the kernel's registers (255) let a SIMD HOLD two waves; a grid sized for four runs them as two rounds.  `frac`
                          # stays against the four-wave row (the stricter reading); the row of the resident occupancy is beside it
                          "resident_waves_per_simd": {"g1": res_g1, "g2": res_g2},
                          "peak_at_resident_waves": peak_res, "frac_at_resident_waves": (gadd / peak_res) if peak_res else None,
                          "mad_bound": mad_bound, "frac_of_mad_bound": (gadd / mad_bound) if mad_bound else None,
                          "additions_per_launch": exact, "term_lists": {"z": zc, "b": bc, "h": hc}, "additions_per_launch_estimate": est,
                          "note": "additions = lengths of the sorted term lists of the last proof, read back from the device "
                                  "(zkg16_last_term_counts): A and L walk the z list, B1 the B list, H the h list; peak = the same XYZZ "
                                  "mixed addition in a bare register-resident loop at the occupancy the launches used (zkg16_last_acc_waves; "
                                  "tools/microbench.hip, the log is named in profiles/bench_constants_r3.json); mad_bound = the measured "
                                  "v_mad_u64_u32 issue rate of the whole chip / 3,542 multiply-adds per mixed addition: the hardware bound "
                                  "of this formula, which the bare loop itself reaches to ~80 %"}
        out.update(extra_out)
        out["window_tables"] = tables_info
        if replicas:
            out["replicas_throughput"] = replicas
        if legs:
            out["legs"] = legs
        if in_flight:
            out["throughput_in_flight"] = in_flight
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(dev, args, gpu_proofs, key_inputs, rs[-1], shp["nc"])
            except Exception as e:      # noqa: BLE001
                out["cpu_baseline"] = {"error": repr(e)}
        print(json.dumps(out), flush=True)
    dev.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if not verified:
        sys.stderr.write("bench.py: the timed proof did NOT verify\n")
        sys.exit(3)
    if rank == 0 and world == 1 and isinstance(locals().get("out", {}).get("cpu_baseline"), dict) and out["cpu_baseline"].get("oracle_match") is False:
        sys.stderr.write("bench.py: the GPU proof of the 32x32 circuit differs from the oracle's\n")
        sys.exit(4)


if __name__ == "__main__":
    main()
