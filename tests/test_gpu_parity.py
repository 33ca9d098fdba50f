"""GPU parity tests proper: the HIP path (through the C ABI, libzkg16.so) against the CPU oracle and the
golden fixtures, bit-exact (all arithmetic is modular integer arithmetic; outputs are canonical)."""
import os
import random

import numpy as np
import pytest

import pyref as P
import stream_cases
import synth
from helpers import *

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


# ---------------------------------------------------------------------------------------------- NTT
def test_ntt_golden(dev):
    for case in load("ntt_kat.json"):
        a = fr_mont_vec([H(x) for x in case["in"]])
        for inv in (0, 1):
            for coset in (0, 1):
                got = fr_from_mont_vec(dev.ntt(a, bool(inv), bool(coset)))
                assert got == [H(x) for x in case["out_inv%d_coset%d" % (inv, coset)]], (case["log_n"], inv, coset)


@pytest.mark.parametrize("log_n", [4, 9, 10, 11, 12, 13, 15, 16])
def test_ntt_vs_oracle(dev, oracle, log_n):
    rng = np.random.default_rng(100 + log_n)
    n = 1 << log_n
    canon = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)     # < 2^254 < r: valid canonical residues
    a = oracle.fr_from_canonical(canon)
    for inv in (False, True):
        for coset in (False, True):
            assert np.array_equal(dev.ntt(a, inv, coset), oracle.ntt(a, inv, coset)), (log_n, inv, coset)


@pytest.mark.parametrize("log_n", [19, 20])
def test_ntt_full_size(dev, oracle, log_n):
    """BASELINE sizes (n=32 -> 2^19, n=46 -> 2^20): oracle equality + the round-trip property."""
    rng = np.random.default_rng(7)
    n = 1 << log_n
    a = oracle.fr_from_canonical(rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64))
    f = dev.ntt(a, False, True)
    assert np.array_equal(f, oracle.ntt(a, False, True))
    assert np.array_equal(dev.ntt(f, True, True), a)
    g = dev.ntt(a, True, False)
    assert np.array_equal(g, oracle.ntt(a, True, False))


@pytest.mark.parametrize("log_n", [23, 24])
def test_ntt_three_pass(dev, oracle, log_n):
    """Domains above 2^22 (the literal 128x128 config needs 2^24): by default two passes over 4096-point tiles (the three-pass
    plan and the other variants are in test_ntt_plans.py): oracle equality + round trip."""
    rng = np.random.default_rng(log_n)
    n = 1 << log_n
    a = oracle.fr_from_canonical(rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64))
    oracle.set_threads(8)
    f = dev.ntt(a, False, True)
    assert np.array_equal(f, oracle.ntt(a, False, True))
    assert np.array_equal(dev.ntt(f, True, True), a)
    if log_n == 23:
        g = dev.ntt(a, True, False)
        assert np.array_equal(g, oracle.ntt(a, True, False))
    oracle.set_threads(1)


# ---------------------------------------------------------------------------------------------- fixed base / MSM
@pytest.mark.parametrize("bits", [0, 5, 14, 16, 18])
def test_fixed_base_vs_oracle(dev, oracle, bits):
    """Window widths by batch size (0), a narrow and the widest ladder-built table, and the two-level tables a large key's
    batches use (16, 18: fixed_base_combine_kernel), forced here on a small batch; digits on either side of each window and
    half-window boundary."""
    rng = random.Random(5)
    ks = [0, 1, 2, 255, 256, 511, 512, (1 << 16) - 1, 1 << 16, (1 << 18) - 1, 1 << 18, (1 << 9) << 18, ((1 << 9) - 1) << 18 | 1,
          (1 << 8) << 16, P.R_MOD - 1] + [P.rand_fr(rng) for _ in range(200)]
    sc = fr_canon_vec(ks)
    dev.set_option("fixed_base_bits", bits)
    try:
        for group, gen in (("g1", G1_GEN_LIMBS), ("g2", G2_GEN_LIMBS)):
            got, ginf = dev.fixed_base(group, gen, sc)
            exp, einf = oracle.fixed_base(group, gen, sc)
            assert np.array_equal(ginf, einf)
            assert np.array_equal(got[einf == 0], exp[einf == 0])
    finally:
        dev.set_option("fixed_base_bits", 0)


def _golden_msm_arrays(case, group, oracle):
    gen = G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS
    w = 12 if group == "g1" else 24
    if case["n"]:
        bases, binf = oracle.fixed_base(group, gen, fr_canon_vec([H(k) for k in case["base_logs"]]))
    else:
        bases, binf = np.zeros((0, w), np.uint64), np.zeros(0, np.uint8)
    return bases, np.array(case["inf"], dtype=np.uint8) | binf, fr_canon_vec([H(s) for s in case["scalars"]])


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_msm_golden(dev, oracle, group):
    enc = g1_limbs if group == "g1" else g2_limbs
    for case in load("msm_kat.json"):
        bases, inf, sc = _golden_msm_arrays(case, group, oracle)
        for c, mode in ((0, 0), (4, 0), (7, 0), (5, 5), (9, 5), (13, 5)):           # mode 5: the bit-sliced bucket reduction on every window
            dev.set_option("window_bits", c)
            dev.set_option("reduce_mode", mode)
            got, ginf = dev.msm(group, bases, sc, inf)
            exp, einf = enc(case["expected_" + group])
            assert ginf == einf and (einf or np.array_equal(got, exp)), (case["name"], c, mode)
    dev.set_option("window_bits", 0)
    dev.set_option("reduce_mode", 0)


def _random_points(dev, group, n, seed):
    rng = np.random.default_rng(seed)
    logs = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    gen = G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS
    pts, inf = dev.fixed_base(group, gen, logs)
    return pts, inf, logs


@pytest.mark.parametrize("group,n,c", [("g1", 1000, 0), ("g1", 5000, 9), ("g1", 70000, 0), ("g1", 70000, 16),
                                       ("g2", 3000, 0), ("g2", 20000, 13)])
def test_msm_random_vs_oracle(dev, oracle, group, n, c):
    pts, inf, _ = _random_points(dev, group, n, 1000 + n)
    rng = np.random.default_rng(n)
    sc = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    sc[:, 3] |= rng.integers(0, 1 << 63, size=n, dtype=np.uint64) & np.uint64(0x3fffffffffffffff)
    dev.set_option("window_bits", c)
    got, ginf = dev.msm(group, pts, sc, inf)
    dev.set_option("window_bits", 0)
    exp, einf = oracle.msm(group, pts, sc, inf)
    assert ginf == einf and np.array_equal(got, exp)


def test_msm_randomised_sizes_and_distributions(dev, oracle):
    """Many (size, scalar width, window bits, run length) combinations against the oracle: the accumulation's segmenting, the
    short / long / folded fix-up paths and the bucket reduction are exercised at shapes no fixed case pins down.  Each base is
    [k]G with a known k, so the expected result is one scalar multiplication of the generator (cheap even for large n)."""
    rng = np.random.default_rng(20261004)
    to_int = lambda a: [unlimbs(r) for r in a]
    for trial in range(24):
        group = "g2" if trial % 6 == 5 else "g1"
        n = int(rng.choice([1, 2, 3, 63, 64, 65, 257, 1000, 4097, 9001, 33333, 70001]))
        bits = int(rng.choice([1, 2, 8, 15, 16, 17, 31, 64, 128, 254]))
        pts, inf, logs = _random_points(dev, group, n, 5000 + trial)
        sc = np.zeros((n, 4), dtype=np.uint64)
        full, rem = divmod(bits, 64)
        for i in range(full):
            sc[:, i] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
        if rem:
            sc[:, full] = rng.integers(0, 1 << rem, size=n, dtype=np.uint64)
        if trial % 4 == 1:
            sc[rng.integers(0, n, size=max(1, n // 3))] = 0            # holes
        c = int(rng.choice([0, 0, 4, 7, 10, 13, 16]))
        seg = int(rng.choice([0, 0, 1, 3, 50]))
        dev.set_option("window_bits", c)
        dev.set_option("min_seg", seg)
        got, ginf = dev.msm(group, pts, sc, inf)
        dev.set_option("window_bits", 0)
        dev.set_option("min_seg", 0)
        total = sum(s * k for s, k in zip(to_int(sc), to_int(logs))) % P.R_MOD
        gen = G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS
        exp, einf = oracle.point_mul(group, gen, fr_canon(total))
        assert ginf == einf and np.array_equal(got, exp), (trial, group, n, bits, c, seg)


@pytest.mark.parametrize("n,c", [(3000, 0), (70000, 0), (70000, 9)])
def test_msm_g2_lazy_products_vs_oracle(dev, oracle, n, c):
    """G2 bucket accumulation with the one-reduction-per-component Fq2 products (option g2_lazy; operands parked in LDS):
    same MSM value as the oracle and as the Karatsuba form, incl. repeated / inverse points (the doubling and cancellation cases)."""
    rng = random.Random(n + c)
    gen = oracle.point_mul("g2", G2_GEN_LIMBS, fr_canon(P.rand_fr(rng)))[0]
    ks = [P.rand_fr(rng) for _ in range(64)]
    pts, _ = oracle.fixed_base("g2", gen, fr_canon_vec(ks))
    bases = pts[np.array([rng.randrange(64) for _ in range(n)])]
    scalars = [rng.choice([0, 1, 2, P.R_MOD - 1, P.rand_fr(rng), P.rand_fr(rng)]) for _ in range(n)]
    sc = fr_canon_vec(scalars)
    want, winf = oracle.msm("g2", bases, sc)
    dev.set_option("window_bits", c)
    try:
        for lazy in (1, 2):                       # 1: one reduction per component (default), 2: Karatsuba
            dev.set_option("g2_lazy", lazy)
            got, ginf = dev.msm("g2", bases, sc)
            assert ginf == winf and np.array_equal(got, want), lazy
    finally:
        dev.set_option("g2_lazy", 0)
        dev.set_option("window_bits", 0)


@pytest.mark.parametrize("kind", ["ones", "bits", "same", "matmul_mix", "top_digit"])
def test_msm_skewed_scalars(dev, oracle, kind):
    """Scalar distributions of the reference's witnesses: ~10% ones, zeros, bit vectors —
    one bucket then spans hundreds of accumulation segments."""
    n = 30000
    pts, inf, _ = _random_points(dev, "g1", n, 77)
    rng = np.random.default_rng(3)
    sc = np.zeros((n, 4), dtype=np.uint64)
    if kind == "ones":
        sc[:, 0] = 1
    elif kind == "bits":
        sc[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
    elif kind == "same":
        sc[:] = fr_canon(0x1234567890abcdef1234567890abcdef)
    elif kind == "matmul_mix":
        sc = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        sc[: n // 10] = 0
        sc[: n // 10, 0] = 1
        sc[n // 10: n // 10 + 200] = 0
    elif kind == "top_digit":
        sc[:] = fr_canon(P.R_MOD - 1)
        sc[::3] = fr_canon((1 << 254) + (1 << 15))
    got, ginf = dev.msm("g1", pts, sc, inf)
    exp, einf = oracle.msm("g1", pts, sc, inf)
    assert ginf == einf and np.array_equal(got, exp)


@pytest.mark.parametrize("kind", ["matmul_mix", "bits"])
def test_msm_known_logs_full_size(dev, oracle, kind):
    """Size-independent property at BASELINE scale (2^19 terms): bases [k_i]G with known k_i, so
    MSM == [sum s_i k_i mod r] G  (SURVEY.md 8c-3).  "bits": one bucket spans the whole accumulation grid (the long fix-up's
    multi-item fold)."""
    n = 1 << 19
    pts, inf, logs = _random_points(dev, "g1", n, 4242)
    rng = np.random.default_rng(9)
    if kind == "bits":
        sc = np.zeros((n, 4), dtype=np.uint64)
        sc[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
    else:
        sc = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        sc[: n // 10] = 0
        sc[: n // 10, 0] = 1
    got, ginf = dev.msm("g1", pts, sc, inf)
    to_int = lambda a: [unlimbs(r) for r in a]
    total = sum(s * k for s, k in zip(to_int(sc), to_int(logs))) % P.R_MOD
    exp, einf = oracle.point_mul("g1", G1_GEN_LIMBS, fr_canon(total))
    assert ginf == einf and np.array_equal(got, exp)


# ---------------------------------------------------------------------------------------------- witness map / prove
def test_witness_map_vs_oracle(dev, oracle):
    rng = random.Random(21)
    for nc, ni, nv in ((27, 3, 14), (3000, 4, 2500)):
        A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
        r1cs = synth.r1cs_arrays(A, B, C, ni)
        zm = fr_mont_vec(z)
        rh, wh = dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
        h = dev.witness_map(rh, wh, 1 << 13)
        assert np.array_equal(h, oracle.witness_map(r1cs, zm)), nc
        dev.r1cs_free(rh)
        dev.witness_free(wh)


def test_witness_map_row_order_and_coefficient_dictionary(dev, oracle):
    """The SpMV's two per-handle structures (csrc/poly.hip): rows ordered by length class (the bit length of the row's non-zero
    count: 0, 1, 2-3, 4-7, ..., longest class first; here classes 0 .. 3, 6 and 9) and the 16-bit coefficient dictionary (here 37
    distinct values, among them 1, -1 and 0; the random systems of the other tests overflow it and exercise the fall-back).
    Witness map == oracle, and == the plain kernel (option spmv_dict 2).  Their limits: tests/test_sparse_limits_gpu.py."""
    rng = random.Random(77)
    nc, ni, nv = 9000, 3, 7000
    pool = [1, P.R_MOD - 1, 0, 2, 3] + [P.rand_fr(rng) for _ in range(32)]
    z = [1] + [P.rand_fr(rng) for _ in range(nv - 1)]
    lens = [0, 1, 1, 1, 2, 5, 40, 300]
    A, B, C = [], [], []
    for i in range(nc):
        rows = []
        for _ in range(3):
            k = lens[rng.randrange(len(lens))] if i % 11 else 1
            cols = sorted(rng.sample(range(nv), k))
            rows.append([(pool[rng.randrange(len(pool))], j) for j in cols])
        A.append(rows[0]); B.append(rows[1]); C.append(rows[2])
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    zm = fr_mont_vec(z)
    rh, wh = dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
    want = oracle.witness_map(r1cs, zm)
    assert np.array_equal(dev.witness_map(rh, wh, 1 << 14), want)
    dev.set_option("spmv_dict", 2)
    try:
        assert np.array_equal(dev.witness_map(rh, wh, 1 << 14), want)
    finally:
        dev.set_option("spmv_dict", 0)
    assert np.array_equal(dev.witness_map(rh, wh, 1 << 14), want)
    assert dev.r1cs_spmv_state(rh)[:2] == (1, 37)          # the dictionary is in use, with every value of the pool
    dev.r1cs_free(rh)
    dev.witness_free(wh)


def test_prove_golden(dev):
    """Whole proofs against the golden Groth16 fixtures (expected A, B, C computed in the exponent by pyref)."""
    for case in load("groth16_kat.json"):
        r1cs, _ = r1cs_from_case(case)
        pk = pk_from_case(case)
        z = fr_mont_vec([H(v) for v in case["z"]])
        ph = dev.pk_load(pk, case["num_inputs"])
        proof, inf = dev.prove(ph, fr_mont(H(case["r"])), fr_mont(H(case["s"])), r1cs, z)
        dev.pk_free(ph)
        assert list(inf) == [0, 0, 0]
        assert np.array_equal(proof[:12], g1_limbs(case["proof"]["a"])[0]), case["name"]
        assert np.array_equal(proof[12:36], g2_limbs(case["proof"]["b"])[0]), case["name"]
        assert np.array_equal(proof[36:], g1_limbs(case["proof"]["c"])[0]), case["name"]


def test_prove_random_vs_oracle_and_exponent(dev, oracle):
    rng = random.Random(99)
    nc, ni, nv = 3000, 4, 2500
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, meta = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zm = fr_mont_vec(z)
    r, s = P.rand_fr(rng), P.rand_fr(rng)
    ph, rh, wh = dev.pk_load(pk, ni), dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
    proof, inf = dev.prove_resident(ph, rh, wh, fr_mont(r), fr_mont(s))
    eproof, einf = oracle.prove(pk, fr_mont(r), fr_mont(s), r1cs, zm)
    assert np.array_equal(inf, einf) and np.array_equal(proof, eproof)
    # independent check: the Groth16 verification equation in the exponent (known trapdoor)
    logs_int = {k: fr_from_mont_vec(meta["logs"][k]) for k in ("a", "b", "l", "h", "gabc")}
    h_int = fr_from_mont_vec(oracle.witness_map(r1cs, zm))
    a, b, c, ok = synth.expected_proof_logs(meta, logs_int, h_int, z, ni, r, s)
    assert ok
    assert np.array_equal(proof[:12], oracle.point_mul("g1", meta["g1"], fr_canon(a))[0])
    assert np.array_equal(proof[12:36], oracle.point_mul("g2", meta["g2"], fr_canon(b))[0])
    assert np.array_equal(proof[36:], oracle.point_mul("g1", meta["g1"], fr_canon(c))[0])
    # index-range sharded key (2 shards on one device) + partial/finish == single-GPU proof
    parts, pinf = [], []
    for k in range(2):
        sh = dev.pk_load(pk, ni, shard_index=k, shard_count=2)
        p, f = dev.prove_partial(sh, rh, wh, fr_mont(r), fr_mont(s))
        parts.append(p)
        pinf.append(f)
        dev.pk_free(sh)
    proof2, inf2 = dev.prove_finish(ph, fr_mont(r), fr_mont(s), np.array(parts), np.array(pinf))
    assert np.array_equal(proof2, proof) and np.array_equal(inf2, inf)
    # every scheduling / tuning option leaves the proof bit-identical (the measured alternatives)
    for opt, vals in (("reduce_mode", (1, 2, 4, 5, 6, 0)), ("fixup_aux", (1, 0)), ("g1_waves", (1, 3, 4, 0)), ("window_bits_h", (9, 0)),
                      ("window_bits", (2, 3, 7, 11, 17, 0)), ("reduce_chunk", (4, 16, 0)), ("wm_concurrent", (0, -1)), ("fuse_pointwise", (0, 1)),
                      ("ntt_mode", (0, 1)), ("ntt_radix", (4, 2, 3, 1)), ("ntt_xcd", (2, 1)), ("sort_mode", (1, 0)), ("acc_pipeline", (3, 1, 2, 0)), ("b_filter", (1, 2, 0)), ("g2_lazy", (2, 0)),
                      ("collect_threads", (1, 2, 0))):
        for v in vals:
            dev.set_option(opt, v)
            p3, i3 = dev.prove_resident(ph, rh, wh, fr_mont(r), fr_mont(s))
            assert np.array_equal(p3, proof) and np.array_equal(i3, inf), (opt, v)
    for f, hnd in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(hnd)


@pytest.mark.parametrize("nc,ni,nv,r,s", [(1, 1, 2, 5, 7), (2, 2, 3, 0, 9), (5, 1, 4, 11, 0), (17, 3, 9, 0, 0), (64, 4, 40, 1, 1),
                                          (300, 2, 1000, P.R_MOD - 1, 2), (1000, 5, 130, 3, P.R_MOD - 1)])
def test_prove_edge_shapes_vs_oracle(dev, oracle, nc, ni, nv, r, s):
    """Degenerate shapes through the whole path: a single constraint, one instance variable (no public input), more
    variables than constraints and the reverse, r and/or s equal to 0, 1, r - 1 (ark-groth16 skips the B1 MSM when r = 0:
    the group element is the same)."""
    rng = random.Random(1000 * nc + nv)
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zm = fr_mont_vec(z)
    ph = dev.pk_load(pk, ni)
    proof, inf = dev.prove(ph, fr_mont(r), fr_mont(s), r1cs, zm)
    dev.pk_free(ph)
    eproof, einf = oracle.prove(pk, fr_mont(r), fr_mont(s), r1cs, zm)
    assert np.array_equal(inf, einf) and np.array_equal(proof, eproof)


def test_request_with_cached_matrices_equals_first_request(dev):
    """The handler mirror keeps a MatrixCircuit's matrices on the device per size and computes only the assignment for later
    requests (zkg16_circuit_matrix_witness): same inputs and seed -> byte-identical proof; other inputs -> a valid proof."""
    from zksnark_finalproject_amd import handlers
    n = 5
    rng = np.random.default_rng(77)
    a = rng.integers(0, 1 << 30, size=(n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 30, size=(n, n), dtype=np.uint64)
    dev.__dict__.pop("_matrix_shapes", None)
    first = handlers.prove_matrix(dev, n, a, b, seed=3)            # synthesizes, exports, uploads, caches
    assert n in dev._matrix_shapes
    again = handlers.prove_matrix(dev, n, a, b, seed=3)            # assignment only
    assert again["proof"] == first["proof"] and again["hash_c"] == first["hash_c"]
    other = handlers.prove_matrix(dev, n, b, a, seed=4)
    assert other["hash_c"] != first["hash_c"]
    assert handlers.verify_proof(other["vk"], other["_circuit"].public_inputs, other["proof"])["valid"] is True
    full = handlers.prove_matrix(dev, n, b, a, seed=4, keep_key=True)     # the un-cached path
    assert full["proof"] == other["proof"]


@pytest.mark.parametrize("n", [32, 46, 128])
def test_full_size_request_verifies(dev, n):
    """BASELINE.json's sizes end to end with a size-independent check: the reference's MatrixCircuit at 32x32 (472,564
    constraints, domain 2^19), 46x46 (domain 2^20) and 128x128 (domain 2^24), synthesized -> device setup -> device proof -> host pairing
    verification == true (the reference's own acceptance test, constraints.rs:231-272), and false for another public input."""
    from zksnark_finalproject_amd import handlers
    rng = np.random.default_rng(n)
    a = rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64)
    res = handlers.prove_matrix(dev, n, a, b, seed=n)
    circ = res["_circuit"]
    assert circ.domain == {32: 1 << 19, 46: 1 << 20, 128: 1 << 24}[n]      # 128: 10.7 M constraints, the 4096-point-tile NTT
    assert handlers.verify_proof(res["vk"], circ.public_inputs, res["proof"])["valid"] is True
    bad = circ.public_inputs.copy()
    bad[2] = bad[0]                     # claim hash_c = hash_a
    assert handlers.verify_proof(res["vk"], bad, res["proof"])["valid"] is False


@pytest.mark.parametrize("ranks,h_ranks", [(2, 0), (4, 0), (4, 1), (8, 0), (8, 8), (3, 2)])
def test_rank_roles_partial_finish_equals_single_proof(dev, oracle, ranks, h_ranks):
    """Multi-GPU rank roles on one device: the plan of zkg16_shard_plan (some ranks run the witness map and share h_query, every
    rank takes a cost-weighted share of the z ranges), each rank's shard cut out of the resident key (zkg16_pk_slice) or loaded from
    the host by range (zkg16_pk_load_range), partial per rank -> finish == the single-GPU proof == the oracle's proof."""
    from zksnark_finalproject_amd.device import shard_plan
    rng = random.Random(4242 + ranks)
    nc, ni, nv = 5000, 3, 4100
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zm = fr_mont_vec(z)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    ph, rh, wh = dev.pk_load(pk, ni), dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
    proof, inf = dev.prove_resident(ph, rh, wh, r, s)
    eproof, einf = oracle.prove(pk, r, s, r1cs, zm)
    assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)
    plan, k = shard_plan(ranks, nv, (1 << 13) - 1, 0.0, h_ranks)
    assert 1 <= k <= ranks and (h_ranks == 0 or k == h_ranks)
    assert sum(p[4] for p in plan) == 1
    parts, pinf = [], []
    for i, (z_lo, z_hi, h_lo, h_hi, blind) in enumerate(plan):
        sh = dev.pk_slice(ph, z_lo, z_hi, h_lo, h_hi, blind) if i % 2 == 0 else dev.pk_load_range(pk, ni, z_lo, z_hi, h_lo, h_hi, blind)
        p, f = dev.prove_partial(sh, rh, wh, r, s)
        if h_hi == h_lo:
            assert f[0] == 1            # no h range: this rank skipped the witness map and the H MSM
        parts.append(p)
        pinf.append(f)
        dev.pk_free(sh)
    proof2, inf2 = dev.prove_finish(ph, r, s, np.array(parts), np.array(pinf))
    assert np.array_equal(proof2, proof) and np.array_equal(inf2, inf)
    for f, hnd in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(hnd)


@pytest.mark.parametrize("cz,ch", [(0, 0), (17, 17), (9, 12), (22, 23), (17, -1), (-1, 19), (24, 20)])
def test_window_tables_same_proof(dev, oracle, cz, ch):
    """zkg16_pk_precompute: window tables 2^(c w) * base next to every base of the five queries, all digits of a scalar in ONE bucket
    set.  The proof must be the plain key's proof == the oracle's, bit for bit, for widths on both sides of the two- / three-pass
    scatter (<= 20 / > 20 bucket bits), for one side only, and for the default (16 bits below 2^16 terms).  A shard cut out of a
    key with tables sees level 0 = the plain query; a shard gets its own tables; a second precompute is refused."""
    from zksnark_finalproject_amd import Zkg16Error
    from zksnark_finalproject_amd.device import shard_plan
    rng = random.Random(977 + 31 * cz + ch)
    nc, ni, nv = 6000, 3, 5200
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    for i in range(ni, nv, 3):                     # the reference's witnesses are full of 0 / 1 / small values: giant buckets
        z[i] = (0, 1, 1, 2, 255)[i % 5]
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zm = fr_mont_vec(z)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    ph, rh, wh = dev.pk_load(pk, ni), dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
    plain = dev.prove_resident(ph, rh, wh, r, s)
    eproof, einf = oracle.prove(pk, r, s, r1cs, zm)
    assert np.array_equal(plain[0], eproof) and np.array_equal(plain[1], einf)
    added = dev.pk_precompute(ph, cz, ch)
    n_h = (1 << 13) - 1
    cz, ch = cz or 16, ch or 16                   # the default widths of queries below 2^16 terms
    assert dev.pk_table_bits(ph) == (max(cz, 0), max(ch, 0))
    want = sum((254 // c) * n * sz for c, n, sz in ((cz, nv + 3, 3 * 112 + 224), (ch, n_h, 112)) if c > 0)
    assert added == want
    tabled = dev.prove_resident(ph, rh, wh, r, s)
    assert np.array_equal(tabled[0], plain[0]) and np.array_equal(tabled[1], plain[1])
    # zkg16_last_term_counts: the sorted term lists of that proof = mixed additions per MSM (what bench.py's `alu` figure divides by)
    zc, bc, hc = dev.last_term_counts()
    digits = lambda c, n: 254 // c + 1 if c > 0 else 254 // (13 if n >= (1 << 14) else max(4, n.bit_length() - 4)) + 1
    assert 0 < zc <= (nv + 3) * digits(cz, nv + 3) and 0 < hc <= n_h * digits(ch, n_h) and bc <= zc
    assert hc > n_h * (digits(ch, n_h) - 2)                  # h is dense: nearly every digit of every scalar is a term
    with pytest.raises(Zkg16Error) as e:
        dev.pk_precompute(ph, cz, ch)
    assert e.value.status == 1
    # rank roles on top: shards of the tabled key, every other one with tables of its own
    plan, _ = shard_plan(3, nv, n_h, 0.0, 2)
    parts, pinf = [], []
    for i, (z_lo, z_hi, h_lo, h_hi, blind) in enumerate(plan):
        sh = dev.pk_slice(ph, z_lo, z_hi, h_lo, h_hi, blind)
        if i != 1:
            dev.pk_precompute(sh, 11 + i, 10)
        pp, ff = dev.prove_partial(sh, rh, wh, r, s)
        parts.append(pp)
        pinf.append(ff)
        dev.pk_free(sh)
    fin = dev.prove_finish(ph, r, s, np.array(parts), np.array(pinf))
    assert np.array_equal(fin[0], plain[0]) and np.array_equal(fin[1], plain[1])
    with pytest.raises(Zkg16Error) as e:
        dev.pk_precompute(987654, 0, 0)
    assert e.value.status == 6
    with pytest.raises(Zkg16Error) as e:
        dev.pk_precompute(ph, 25, 0)
    assert e.value.status == 1
    for f, hnd in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(hnd)


@pytest.mark.parametrize("kind", ["matrix32", "prime"])
def test_window_tables_reference_circuits(dev, oracle, kind):
    """The default table widths on the reference's circuits at BASELINE's 32x32 size and on PrimeCircuit (bit-valued witnesses:
    almost every term falls into bucket 1 of window 0): same proof as the plain key, and it verifies."""
    from zksnark_finalproject_amd import circuits
    from zksnark_finalproject_amd.device import verify
    import bench
    if kind == "prime":
        c = circuits.prime_circuit(5, 32)
    else:
        c, _, _ = bench.synthesize("matrix", 32)
    trap, g1, g2 = bench.draw_key_inputs(11)
    rh = dev.r1cs_load(c.r1cs, c.num_vars)
    ph, vk = dev.setup_resident(rh, c.num_instance, trap, g1, g2)
    wh = dev.witness_load(c.z)
    r, s = fr_mont(1234567), fr_mont(7654321)
    plain = dev.prove_resident(ph, rh, wh, r, s)
    assert dev.pk_precompute(ph) > 0
    tabled = dev.prove_resident(ph, rh, wh, r, s)
    assert np.array_equal(tabled[0], plain[0]) and np.array_equal(tabled[1], plain[1])
    assert verify(vk, c.public_inputs, *tabled)
    for v in (2, 1, 0):         # the B-side term list by a second sort / filtered out of the full list (the default with tables)
        dev.set_option("b_filter", v)
        again = dev.prove_resident(ph, rh, wh, r, s)
        assert np.array_equal(again[0], plain[0]) and np.array_equal(again[1], plain[1]), v
    for f, hnd in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(hnd)


def test_prime_handler_round_trip(dev):
    """prove_prime / verify_prime mirrors (backend/prime_snark.rs:49-146, 165-206): search, PrimeCircuit, device setup, device proof,
    pairing verification through the wire format with the public inputs recovered by re-synthesis; a wrong j does not verify."""
    from zksnark_finalproject_amd import handlers
    res = handlers.prove_prime(dev, 5, 32, check_satisfied=True)
    assert res["found_prime"] and res["satisfied"] is True and int(res["prime_num"]) > 1
    assert handlers.verify_prime(res["vk"], 5, res["j"], res["proof"])["valid"] is True
    other = res["j"] + 1
    try:
        bad = handlers.verify_prime(res["vk"], 5, other, res["proof"])["valid"]
    except Exception:                                   # candidate j + 1 may be below 2 / have a zero base: not constructible upstream either
        bad = False
    assert bad is False
    none = handlers.prove_prime(dev, 5, 0)
    assert none["found_prime"] is False and none["proof"] == ""


def test_error_paths(dev):
    from zksnark_finalproject_amd import Zkg16Error
    # malformed CSR row pointers are rejected on the host (the SpMV kernel walks them unchecked)
    rng = random.Random(5)
    A, B, C, z = synth.random_r1cs(rng, 20, 2, 12)
    good = synth.r1cs_arrays(A, B, C, 2)
    for mut in ("nonzero_start", "decreasing"):
        bad = dict(good)
        rp, col, cf = good["a"]
        rp = rp.copy()
        if mut == "nonzero_start":
            rp[0] = 1
        else:
            rp[5], rp[6] = rp[6] + 1, rp[5]
        bad["a"] = (rp, col, cf)
        with pytest.raises(Zkg16Error) as e:
            dev.r1cs_load(bad, 12)
        assert e.value.status == 1   # ZKG16_ERR_BAD_ARG
    with pytest.raises(Zkg16Error) as e:
        dev.prove_resident(12345, 1, 2, fr_mont(1), fr_mont(2))
    assert e.value.status == 6       # ZKG16_ERR_BAD_HANDLE
    with pytest.raises(Zkg16Error) as e:
        dev.lib.zkg16_ntt.argtypes  # noqa
        dev._check(dev.lib.zkg16_ntt(dev.ctx, np.zeros((1, 4), np.uint64), 40, 0, 0))
    assert e.value.status == 2       # domain too large
    # the matrix request's entry points: sizes that are not a MatrixCircuit, handles of another size, unknown handles
    two = np.ones((2, 2), dtype=np.uint64)
    one = np.ones((1, 1), dtype=np.uint64)
    for call in (lambda: dev.witness_matrix(one, one), lambda: dev.r1cs_matrix(1), lambda: dev.r1cs_matrix(5000)):
        with pytest.raises(Zkg16Error) as e:
            call()
        assert e.value.status == 1
    rh3 = dev.r1cs_matrix(3)
    from zksnark_finalproject_amd.device import scalar_mul
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    trap = np.stack([fr_mont(k + 2) for k in range(5)])
    ph3, _ = dev.setup_resident(rh3, 4, trap, g1_generator(), g2_generator())
    with pytest.raises(Zkg16Error) as e:
        dev.prove_matrix(ph3, rh3, two, two, fr_mont(1), fr_mont(2))      # a 2x2 request on the 3x3 circuit's handles
    assert e.value.status == 1
    with pytest.raises(Zkg16Error) as e:
        dev.prove_matrix(ph3, 999999, np.ones((3, 3), dtype=np.uint64), np.ones((3, 3), dtype=np.uint64), fr_mont(1), fr_mont(2))
    assert e.value.status == 6
    ok = dev.prove_matrix(ph3, rh3, np.ones((3, 3), dtype=np.uint64), np.ones((3, 3), dtype=np.uint64), fr_mont(1), fr_mont(2))
    assert ok[0].any()                                                    # and the ctx still proves after the refusals
    dev.pk_free(ph3)
    dev.r1cs_free(rh3)
    for name, v in (("lanes", 0), ("lanes", 9), ("matrix_parts", 9), ("g2_lazy", 3), ("fixed_base_bits", 3), ("fixed_base_bits", 17),
                    ("fixed_base_bits", 22)):
        with pytest.raises(Zkg16Error):
            dev.set_option(name, v)
    # every option name zkg16_set_option accepts: one accepted value, the nearest rejected value on each bounded side
    try:
        for name, accepted, rejected, _ in OPTION_BOUNDS:
            for v in accepted:
                dev.set_option(name, v)
            for v in rejected:
                with pytest.raises(Zkg16Error) as e:
                    dev.set_option(name, v)
                assert e.value.status == 1, (name, v)        # ZKG16_ERR_BAD_ARG
        with pytest.raises(Zkg16Error) as e:
            dev.set_option("no_such_option", 1)
        assert e.value.status == 7                           # ZKG16_ERR_UNSUPPORTED
    finally:
        for name, _, _, default in OPTION_BOUNDS:
            dev.set_option(name, default)


# (name, accepted values, rejected values, the value that restores the default).  The bounds are those of zkg16_set_option; fixup_aux,
# wm_concurrent and fuse_pointwise take any value.  0 restores the default of sponge_chains_min and of the three verify thresholds.
OPTION_BOUNDS = (
    ("lanes", (1, 8), (0, 9), 2),
    ("window_bits", (2, 20), (-1, 1, 21), 0),
    ("min_seg", (4096,), (-1, 4097), 0),
    ("ntt_mode", (0, 3), (-1, 2, 4), 1),
    ("reduce_mode", (6,), (-1, 7), 0),
    ("g1_waves", (4,), (-1, 5), 0),
    ("fixup_aux", (1,), (), 0),
    ("window_bits_h", (2, 20), (-1, 1, 21), 0),
    ("wm_concurrent", (0,), (), -1),
    ("ntt_radix", (4,), (-1, 5), 0),
    ("ntt_xcd", (2,), (-1, 3), 0),
    ("acc_debug", (15,), (-1, 16), 0),
    ("sort_mode", (1,), (-1, 2), 0),
    ("acc_pipeline", (4,), (-1, 5), 0),
    ("fuse_pointwise", (0,), (), 1),
    ("wm_transforms", (6, 7), (-1, 1, 5, 8), 0),
    ("wm_first", (-1, 2), (-2, 3), -1),
    ("spmv_dict", (2,), (-1, 3), 0),
    ("b_filter", (2,), (-1, 3), 0),
    ("collect_threads", (2,), (-1, 3), 0),
    ("fixed_base_bits", (4, 14, 16, 20), (-1, 3, 15, 21), 0),
    ("g2_lazy", (2,), (-1, 3), 0),
    ("g1_inline", (2,), (-1, 3), 0),
    ("acc_lazy", (0,), (-1, 2), 1),
    ("matrix_parts", (8,), (-1, 9), 0),
    ("matrix_slice_min", (1, 1 << 20), (-1, (1 << 20) + 1), 0),
    ("batch_max", (65535,), (-1, 65536), 0),
    ("matrix_batch_threads", (16,), (-1, 17), 0),
    ("matrix_batch_grid", (65535,), (-1, 65536), 0),
    ("sponge_chains_min", (1, 1 << 40), (-1,), 0),
    ("sponge_chain_segment", (65535,), (-1, 65536), 0),
    ("verify_batch_min", (1 << 30,), (-1, (1 << 30) + 1), 0),
    ("verify_wire_min", (1 << 30,), (-1, (1 << 30) + 1), 0),
    ("verify_each_after", (1 << 30,), (-1, (1 << 30) + 1), 0),
    ("reduce_chunk", (1, 64), (-1, 3, 65), 0),
)


def test_prove_entry_status_codes(dev, oracle):
    """The status codes of zkg16_prove_resident / _partial / _batch on the smallest system the synth helper makes (50 constraints,
    domain 2^6): an unknown handle is reported before any shape check, a key shard is a bad argument to prove_resident and
    unsupported by prove_batch, a witness of the wrong length is a bad argument everywhere; the ctx still proves afterwards."""
    from zksnark_finalproject_amd import Zkg16Error
    BAD_ARG, BAD_HANDLE, UNSUPPORTED = 1, 6, 7
    rng = random.Random(77)
    nc, ni, nv = 50, 3, 40
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zm = fr_mont_vec(z)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    ph, rh, wh = dev.pk_load(pk, ni), dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
    shard = dev.pk_slice(ph, 0, nv // 2, 0, 30, True)
    long_w = dev.witness_load(np.concatenate([zm, zm[:1]]))
    none = 987654321

    def status(call):
        with pytest.raises(Zkg16Error) as e:
            call()
        return e.value.status

    def resident(p, c, w): return lambda: dev.prove_resident(p, c, w, r, s)
    def partial(p, c, w): return lambda: dev.prove_partial(p, c, w, r, s)
    def batch(p, c, ws): return lambda: dev.prove_batch(p, c, ws, np.stack([r] * len(ws)), np.stack([s] * len(ws)))

    try:
        for entry in (resident, partial):
            assert status(entry(none, rh, wh)) == BAD_HANDLE
            assert status(entry(ph, none, wh)) == BAD_HANDLE
            assert status(entry(ph, rh, none)) == BAD_HANDLE
            assert status(entry(ph, rh, long_w)) == BAD_ARG
            assert status(entry(none, rh, long_w)) == BAD_HANDLE      # the handles are looked up before any shape is compared
        assert status(batch(none, rh, [wh])) == BAD_HANDLE
        assert status(batch(ph, none, [wh])) == BAD_HANDLE
        assert status(batch(ph, rh, [wh, none])) == BAD_HANDLE
        assert status(batch(ph, rh, [wh, long_w])) == BAD_ARG
        assert status(batch(ph, rh, [long_w, none])) == BAD_HANDLE
        assert status(resident(shard, rh, wh)) == BAD_ARG
        assert status(batch(shard, rh, [wh])) == UNSUPPORTED
        assert status(batch(shard, rh, [long_w])) == UNSUPPORTED          # the shard is refused before the lengths are compared
        assert status(batch(shard, rh, [none])) == BAD_HANDLE
        part, pinf = dev.prove_partial(shard, rh, wh, r, s)               # prove_partial takes shards
        assert part.shape == (72,) and pinf.shape == (5,)
        proof, inf = dev.prove_resident(ph, rh, wh, r, s)
        eproof, einf = oracle.prove(pk, r, s, r1cs, zm)
        assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)
    finally:
        for w in (wh, long_w):
            dev.witness_free(w)
        for p in (shard, ph):
            dev.pk_free(p)
        dev.r1cs_free(rh)


@pytest.mark.parametrize("kind", ["fib0", "fib10", "fib186", "fib1000", "matrix3", "matrix8", "matrix32", "prime"])
def test_prove_reference_circuits(dev, oracle, kind):
    """The reference's own circuits (C++ mirrors, csrc/circuits.hip) proved on the GPU: bit-identical to the oracle's proof
    and satisfying the Groth16 equation in the exponent (known-trapdoor key).  fib1000 = BASELINE configs[0] literally (the C++
    mirror computes the result in Fr, so the public input matches the circuit where the reference's u128 wraps: SURVEY F8);
    matrix32 = configs[1] at full size: 472,564 constraints, domain 2^19, oracle on all host threads."""
    from zksnark_finalproject_amd.circuits import fibonacci_circuit, matrix_circuit, prime_circuit
    if kind in ("matrix32", "prime"):
        oracle.set_threads(min(os.cpu_count() or 1, 16))
    rng = random.Random(hash(kind) & 0xffff)
    if kind == "prime":
        c = prime_circuit(0x123456789ABCDEF, 32)                        # BASELINE configs[4]: PrimeCircuit (338,296 constraints, nearly all witnesses are bits)
    elif kind.startswith("fib"):
        c = fibonacci_circuit(0, 1, int(kind[3:]))                      # bench/fibo.py:26-34: a=0, b=1, rounds <= 186
    else:
        n = int(kind[6:])
        c = matrix_circuit(np.ones((n, n), dtype=np.uint64), np.ones((n, n), dtype=np.uint64))   # bench/matrix.py:11
    pk, meta = synth.make_pk(oracle, c.r1cs, c.num_vars, rng, point_gen=dev.fixed_base)
    r, s = P.rand_fr(rng), P.rand_fr(rng)
    ph = dev.pk_load(pk, c.num_instance)
    proof, inf = dev.prove(ph, fr_mont(r), fr_mont(s), c.r1cs, c.z)
    dev.pk_free(ph)
    eproof, einf = oracle.prove(pk, fr_mont(r), fr_mont(s), c.r1cs, c.z)
    assert np.array_equal(inf, einf) and np.array_equal(proof, eproof)
    logs_int = {k: fr_from_mont_vec(meta["logs"][k]) for k in ("a", "b", "l", "h", "gabc")}
    h_int = fr_from_mont_vec(oracle.witness_map(c.r1cs, c.z))
    a, b, cc, ok = synth.expected_proof_logs(meta, logs_int, h_int, fr_from_mont_vec(c.z), c.num_instance, r, s)
    assert ok
    assert np.array_equal(proof[:12], oracle.point_mul("g1", meta["g1"], fr_canon(a))[0])
    assert np.array_equal(proof[12:36], oracle.point_mul("g2", meta["g2"], fr_canon(b))[0])
    assert np.array_equal(proof[36:], oracle.point_mul("g1", meta["g1"], fr_canon(cc))[0])


@pytest.mark.parametrize("kind", ["random3000", "matrix3", "random3000-wide", "random20000"])
def test_setup_on_device_vs_oracle(dev, oracle, kind):
    """zkg16_setup (trapdoor -> proving key on the device) == the oracle's key for the same trapdoor and generators
    (ark-groth16 generator.rs semantics), and a proof under that key satisfies the Groth16 equation in the exponent."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    rng = random.Random(31337)
    if kind == "matrix3":
        c = matrix_circuit(np.ones((3, 3), dtype=np.uint64), np.ones((3, 3), dtype=np.uint64))
        r1cs, zm, ni, nv = c.r1cs, c.z, c.num_instance, c.num_vars
        z_int = fr_from_mont_vec(c.z)
    else:
        # column 0 of C holds 6/7 of the rows: one queued slice of the column sums at 3000 rows, three at 20000
        nc, ni, nv = int(kind.split("-")[0][6:]), 4, 2500
        A, B, C, z_int = synth.random_r1cs(rng, nc, ni, nv)
        r1cs = synth.r1cs_arrays(A, B, C, ni)
        zm = fr_mont_vec(z_int)
    state = rng.getstate()
    epk, meta = synth.make_pk(oracle, r1cs, nv, rng)                       # oracle key (CPU fixed-base)
    rng.setstate(state)
    trap_int = {k: P.rand_fr(rng) for k in ("tau", "alpha", "beta", "gamma", "delta")}
    assert trap_int == meta["trap"]
    trap = fr_mont_vec([trap_int[k] for k in ("tau", "alpha", "beta", "gamma", "delta")])
    rh = dev.r1cs_load(r1cs, nv)
    domain = 1 << max(r1cs["num_constraints"] + ni - 1, 0).bit_length()
    dev.set_option("fixed_base_bits", 16 if kind.endswith("-wide") else 0)          # the two-level tables of a large key
    try:
        pk, vk = dev.setup(rh, ni, nv, domain, trap, meta["g1"], meta["g2"])
    finally:
        dev.set_option("fixed_base_bits", 0)
    for k in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query"):
        inf_key = {"a_query": "a_inf", "b_g1_query": "b_g1_inf", "b_g2_query": "b_g2_inf", "l_query": "l_inf"}.get(k)
        if inf_key:
            assert np.array_equal(pk[inf_key], epk[inf_key]), k
            keep = epk[inf_key] == 0
            assert np.array_equal(pk[k][keep], epk[k][keep]), k
        else:
            assert np.array_equal(pk[k], epk[k]), k
    for k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2"):
        assert np.array_equal(pk[k], epk[k]), k
    gabc_exp, _ = oracle.fixed_base("g1", meta["g1"], oracle.fr_to_canonical(meta["logs"]["gabc"]))
    assert np.array_equal(vk["gamma_abc_g1"], gabc_exp)
    assert np.array_equal(vk["gamma_g2"], oracle.point_mul("g2", meta["g2"], fr_canon(trap_int["gamma"]))[0])
    # prove under the device-generated key
    r, s = P.rand_fr(rng), P.rand_fr(rng)
    ph, wh = dev.pk_load(pk, ni), dev.witness_load(zm)
    proof, inf = dev.prove_resident(ph, rh, wh, fr_mont(r), fr_mont(s))
    logs_int = {k: fr_from_mont_vec(meta["logs"][k]) for k in ("a", "b", "l", "h", "gabc")}
    h_int = fr_from_mont_vec(oracle.witness_map(r1cs, zm))
    a, b, cc, ok = synth.expected_proof_logs(meta, logs_int, h_int, z_int, ni, r, s)
    assert ok and list(inf) == [0, 0, 0]
    assert np.array_equal(proof[:12], oracle.point_mul("g1", meta["g1"], fr_canon(a))[0])
    assert np.array_equal(proof[12:36], oracle.point_mul("g2", meta["g2"], fr_canon(b))[0])
    assert np.array_equal(proof[36:], oracle.point_mul("g1", meta["g1"], fr_canon(cc))[0])
    for f, hnd in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(hnd)


def test_circuit_load_equals_export_then_load(dev):
    """zkg16_circuit_load (a synthesized circuit straight to the device through the ctx's pinned staging block) leaves the same bytes
    on the device as zkg16_circuit_export + zkg16_r1cs_load + zkg16_witness_load, and the same proof comes out; twice in a row with
    different sizes (the staging block grows and is reused)."""
    from zksnark_finalproject_amd.circuits import (fibonacci_circuit, fibonacci_circuit_handle, prime_circuit, prime_circuit_handle,
                                                   prime_search)
    from zksnark_finalproject_amd import handlers
    j = prime_search(12345, 32)["j"]
    cases = [(prime_circuit_handle(12345, j), prime_circuit(12345, j, search=False, check_satisfied=False)),
             (fibonacci_circuit_handle(0, 1, 300), fibonacci_circuit(0, 1, 300)),
             (prime_circuit_handle(99, prime_search(99, 32)["j"]), prime_circuit(99, 32, check_satisfied=False))]
    for h, full in cases:
        assert np.array_equal(h.public_inputs, full.public_inputs)
        rh, wh = dev.circuit_load(h)
        h.close()
        got, nv = dev.r1cs_read(rh)
        assert nv == full.num_vars and got["num_inputs"] == full.num_instance and got["num_constraints"] == full.num_constraints
        for m in "abc":
            assert all(np.array_equal(u, v) for u, v in zip(got[m], full.r1cs[m])), m
        assert np.array_equal(dev.witness_read(wh, full.num_vars), full.z)
        dev.r1cs_free(rh)
        dev.witness_free(wh)
    res = handlers.prove_prime(dev, 12345, 32)                # the handler's request path goes through zkg16_circuit_load
    assert handlers.verify_prime(res["pvk"], 12345, res["j"], res["proof"])["valid"] is True
    assert handlers.verify_prime(res["pvk"], 12346, res["j"], res["proof"])["valid"] is False


def test_handler_mirrors_end_to_end(dev, oracle):
    """prove_matrix / prove_fibonacci (handlers.py: synthesize -> device setup -> device prove -> wire encoding): the proof
    the handler returns decodes to exactly the oracle's proof for the same key, r, s."""
    from zksnark_finalproject_amd import handlers, wire
    for res in (handlers.prove_matrix(dev, 4, np.ones((4, 4), dtype=np.uint64), np.ones((4, 4), dtype=np.uint64), keep_key=True),
                handlers.prove_fibonacci(dev, 0, 1, 100, keep_key=True)):
        d, circ = res["_detail"], res["_circuit"]
        proof, inf = wire.decode_proof(res["proof"])
        assert len(wire.proof_serialize_compressed(proof, inf)) == 192
        eproof, einf = oracle.prove(d["pk"], d["r"], d["s"], circ.r1cs, circ.z)
        assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)
        assert res["proving_time"] > 0 and res["setup_time"] > 0
    assert res["num_constraints"] == 101


def test_resident_setup_equals_host_round_trip(dev):
    """zkg16_setup_resident (key built straight into the device layout) gives the same verifying key and the byte-identical
    proof as zkg16_setup -> host -> zkg16_pk_load, for the same trapdoor, generators, r, s."""
    from zksnark_finalproject_amd import handlers
    for n in (3, 6):
        a = np.arange(n * n, dtype=np.uint64).reshape(n, n) % 7
        host = handlers.prove_matrix(dev, n, a, a.T.copy(), seed=5, keep_key=True)
        res = handlers.prove_matrix(dev, n, a, a.T.copy(), seed=5, keep_key=False)
        assert res["proof"] == host["proof"]
        for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1"):
            assert np.array_equal(res["_detail"]["vk"][k], host["_detail"]["vk"][k]), k
        assert handlers.verify_proof(res["_detail"]["vk"], res["_circuit"].public_inputs, res["proof"])["valid"]


def test_setup_prove_verify_with_pairings(dev):
    """setup (device) -> prove (device) -> verify (pure-Python pairings) == true, and false for a wrong public input:
    the reference's own acceptance test (constraints.rs:231-272, fibbonaci.rs:192-232) end to end, with NO oracle involved."""
    import pyref_pairing as PP
    from zksnark_finalproject_amd import handlers, wire
    to1 = lambda l: P.g1_from_limbs([int(v) for v in l])
    to2 = lambda l: P.g2_from_limbs([int(v) for v in l])
    for res in (handlers.prove_matrix(dev, 3, np.ones((3, 3), dtype=np.uint64), 2 * np.ones((3, 3), dtype=np.uint64), seed=5),
                handlers.prove_fibonacci(dev, 0, 1, 50, seed=6)):
        d, circ = res["_detail"], res["_circuit"]
        vk = dict(alpha_g1=to1(d["vk"]["alpha_g1"]), beta_g2=to2(d["vk"]["beta_g2"]), gamma_g2=to2(d["vk"]["gamma_g2"]),
                  delta_g2=to2(d["vk"]["delta_g2"]), gamma_abc_g1=[to1(g) for g in d["vk"]["gamma_abc_g1"]])
        proof, inf = wire.decode_proof(res["proof"])            # through the wire format
        pr = (to1(proof[:12]), to2(proof[12:36]), to1(proof[36:]))
        pub = fr_from_mont_vec(circ.public_inputs)
        assert PP.groth16_verify(vk, pub, pr)
        bad = list(pub)
        bad[-1] = (bad[-1] + 1) % P.R_MOD
        assert not PP.groth16_verify(vk, bad, pr)
        # the product's own host verifier through the handler mirror agrees
        assert handlers.verify_proof(d["vk"], circ.public_inputs, res["proof"])["valid"] is True
        assert handlers.verify_proof(res["vk"], circ.public_inputs, res["proof"])["valid"] is True      # key over the wire
        assert handlers.verify_proof(d["vk"], fr_mont_vec(bad), res["proof"])["valid"] is False


@pytest.mark.parametrize("shards", [3, 8])
def test_sharding_with_empty_shards(dev, oracle, shards):
    """8 ranks on the 5-variable Fibonacci circuit (BASELINE configs[0] shape): most index-range shards are empty or hold a
    single term; partial/finish must still reproduce the single-GPU proof."""
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    rng = random.Random(77)
    c = fibonacci_circuit(0, 1, 20)
    pk, _ = synth.make_pk(oracle, c.r1cs, c.num_vars, rng, point_gen=dev.fixed_base)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    rh, wh = dev.r1cs_load(c.r1cs, c.num_vars), dev.witness_load(c.z)
    ph = dev.pk_load(pk, c.num_instance)
    proof, inf = dev.prove_resident(ph, rh, wh, r, s)
    eproof, einf = oracle.prove(pk, r, s, c.r1cs, c.z)
    assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)
    parts, pinf = [], []
    for k in range(shards):
        sh = dev.pk_load(pk, c.num_instance, shard_index=k, shard_count=shards)
        p_, f_ = dev.prove_partial(sh, rh, wh, r, s)
        parts.append(p_)
        pinf.append(f_)
        dev.pk_free(sh)
    proof2, inf2 = dev.prove_finish(ph, r, s, np.array(parts), np.array(pinf))
    assert np.array_equal(proof2, proof) and np.array_equal(inf2, inf)
    for f, hnd in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(hnd)


def test_concurrent_callers_on_one_ctx(dev, oracle):
    """actix runs one worker per core and each may call prove (src/main.rs:37-43): a ctx runs two proofs at a time on two lanes
    that SHARE the resident key, matrices and assignment (option "lanes"); every caller gets the right proof (== the oracle's),
    proofs on different lanes really overlap (zkg16_lane_log), with lanes = 1 everything is serialised on lane 0, and freeing the
    handles while proofs are in flight is safe."""
    import threading
    rng = random.Random(5)
    nc, ni, nv = 20000, 3, 15000
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zm = fr_mont_vec(z)
    ph, rh, wh = dev.pk_load(pk, ni), dev.r1cs_load(r1cs, nv), dev.witness_load(zm)
    jobs = [(fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))) for _ in range(12)]
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    want = [oracle.prove(pk, r, s, r1cs, zm) for r, s in jobs]
    out = [None] * len(jobs)

    def work(i):
        out[i] = dev.prove_resident(ph, rh, wh, *jobs[i])

    def run_all():
        ts = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for i in range(len(jobs)):
            assert np.array_equal(out[i][0], want[i][0]) and np.array_equal(out[i][1], want[i][1]), i
        return dev.lane_log(len(jobs))

    dev.prove_resident(ph, rh, wh, *jobs[0])                      # warm both the lazy structures and lane 0
    log = run_all()
    assert len(log) == len(jobs) and {l for l, _, _ in log} == {0, 1}, log
    both = [(a, b) for a in log for b in log if a[0] == 0 and b[0] == 1 and a[1] < b[2] and b[1] < a[2]]
    assert both, "no two proofs on different lanes overlapped: %s" % (log,)
    dev.set_option("lanes", 1)
    try:
        log1 = run_all()
        assert {l for l, _, _ in log1} == {0}
        assert all(log1[i][2] <= log1[i + 1][1] + 1e-3 for i in range(len(log1) - 1)), "lanes = 1 must serialise"
    finally:
        dev.set_option("lanes", 2)
    # handles freed under running proofs: the proofs in flight keep their key / matrices / assignment alive
    started = threading.Event()

    def late(i):
        started.set()
        try:
            out[i] = dev.prove_resident(ph, rh, wh, *jobs[i])
        except Exception as e:          # noqa: BLE001 - a caller that arrives after the free gets BAD_HANDLE, never a crash
            out[i] = e
    ts = [threading.Thread(target=late, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    started.wait()
    for f, hnd in ((dev.witness_free, wh), (dev.r1cs_free, rh), (dev.pk_free, ph)):
        f(hnd)
    for t in ts:
        t.join()
    for i in range(4):
        if isinstance(out[i], Exception):
            assert "handle" in str(out[i])
        else:
            assert np.array_equal(out[i][0], want[i][0])


def test_prove_prime_like_bits_workload(dev, oracle):
    """configs[4] shape: every z-side scalar is 0 or 1 (one giant bucket per MSM): GPU proof == oracle proof."""
    from zksnark_finalproject_amd.workloads import prime_like_r1cs
    r1cs, zm, shp = prime_like_r1cs(4000)
    rng = random.Random(12)
    pk, _ = synth.make_pk(oracle, r1cs, shp["num_vars"], rng, point_gen=dev.fixed_base)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    ph = dev.pk_load(pk, shp["num_instance"])
    proof, inf = dev.prove(ph, r, s, r1cs, zm)
    dev.pk_free(ph)
    eproof, einf = oracle.prove(pk, r, s, r1cs, zm)
    assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)


# ---------------------------------------------------------------------------------------------- device witness generation
@pytest.mark.parametrize("n", [2, 5, 33, 46, 128])
def test_witness_matrix_on_device_equals_host_builder(dev, n):
    """zkg16_witness_matrix (scope row f-4 "on GPU"): the MatrixCircuit assignment written by the device kernels from the host
    sponges' entering states == the host builder's (zkg16_circuit_matrix_witness, itself checked against the gadget-level
    synthesis and a Python sponge in tests/test_circuits.py) byte for byte; random full-range u64 inputs (products up to 2^128,
    sums above it), odd n (a last sponge block with one element) and the headline size."""
    from zksnark_finalproject_amd.circuits import matrix_witness
    from zksnark_finalproject_amd.workloads import matmul_shape
    rng = np.random.default_rng(1000 + n)
    a = rng.integers(0, 1 << 63, size=(n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 63, size=(n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, n), dtype=np.uint64)
    nv = matmul_shape(n)["num_witness"] + 4
    want = matrix_witness(a, b, nv)
    wh, pub, ms = dev.witness_matrix(a, b)
    got = dev.witness_read(wh, nv)
    dev.witness_free(wh)
    assert np.array_equal(pub, want[1:4])
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("device assignment differs from the host builder's at %d of %d variables, first %s" % (len(bad), nv, bad[:8]))
    # all-ones inputs, the reference bench's workload (bench/matrix.py:11)
    ones = np.ones((n, n), dtype=np.uint64)
    wh, pub, _ = dev.witness_matrix(ones, ones)
    assert np.array_equal(dev.witness_read(wh, nv), matrix_witness(ones, ones, nv))
    dev.witness_free(wh)


@pytest.mark.parametrize("n", [8, 32])
def test_proof_from_device_witness_equals_proof_from_host_witness(dev, oracle, n):
    """The whole request through the device-built assignment: same key, r, s -> the same proof bytes as with the host-built
    assignment, which equal the oracle's."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    rng_np = np.random.default_rng(5 + n)
    a = rng_np.integers(0, 1 << 40, size=(n, n), dtype=np.uint64)
    b = rng_np.integers(0, 1 << 40, size=(n, n), dtype=np.uint64)
    circ = matrix_circuit(a, b)
    rng = random.Random(11 * n)
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    pk, _ = synth.make_pk(oracle, circ.r1cs, circ.num_vars, rng, point_gen=dev.fixed_base)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    ph = dev.pk_load(pk, circ.num_instance)
    rh = dev.r1cs_load(circ.r1cs, circ.num_vars)
    w_host = dev.witness_load(circ.z)
    w_dev, pub, _ = dev.witness_matrix(a, b)
    assert np.array_equal(pub, circ.public_inputs)
    p_host = dev.prove_resident(ph, rh, w_host, r, s)
    p_dev = dev.prove_resident(ph, rh, w_dev, r, s)
    assert np.array_equal(p_host[0], p_dev[0]) and np.array_equal(p_host[1], p_dev[1])
    eproof, einf = oracle.prove(pk, r, s, circ.r1cs, circ.z)
    assert np.array_equal(p_dev[0], eproof) and np.array_equal(p_dev[1], einf)
    for f, h in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, w_host), (dev.witness_free, w_dev)):
        f(h)


def test_full_size_request_verifies_with_tables(dev):
    """The headline MODE at the headline SIZE: 128x128, resident key -> plain proof -> window tables
    (c = 20 / 22, three-pass scatter, B-list filter, four G1 waves per SIMD, witness map first) -> tabled proof == the plain
    proof bit for bit -> pairing verification; the assignment comes from the device generator."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    from zksnark_finalproject_amd.device import verify
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    from zksnark_finalproject_amd.device import scalar_mul
    n = 128
    ones = np.ones((n, n), dtype=np.uint64)
    circ = matrix_circuit(ones, ones)
    rng = random.Random(128)
    trap = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]
    rh = dev.r1cs_load(circ.r1cs, circ.num_vars)
    ph, vk = dev.setup_resident(rh, circ.num_instance, trap, g1, g2)
    wh, pub, _ = dev.witness_matrix(ones, ones)
    assert np.array_equal(pub, circ.public_inputs)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    plain = dev.prove_resident(ph, rh, wh, r, s)
    dev.pk_precompute(ph)
    assert dev.pk_table_bits(ph) == (20, 22)
    tabled = dev.prove_resident(ph, rh, wh, r, s)
    assert np.array_equal(plain[0], tabled[0]) and np.array_equal(plain[1], tabled[1])
    assert verify(vk, circ.public_inputs, *tabled) is True
    bad = circ.public_inputs.copy()
    bad[2] = bad[0]
    assert verify(vk, bad, *tabled) is False
    for f, h in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(h)


@pytest.mark.parametrize("n", [46, 128])
def test_headline_size_equals_oracle(dev, oracle, n):
    """The headline configuration against the oracle, bit for bit: MatrixCircuit 128x128 (10,706,932 constraints, domain 2^24)
    with random full-range inputs — key from the device setup (host copy), the plain proof, the streamed request
    (zkg16_prove_matrix, assignment from the device) and the proof with window tables all == the CPU oracle's proof for the same
    key, r, s, matrices and assignment (the oracle takes ~70 s on 16 threads for this size) — and the same at 46x46 (1,035,770
    constraints, domain 2^20: north_star's "up to 2^20 constraints")."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    from zksnark_finalproject_amd.device import scalar_mul
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    rng_np = np.random.default_rng(77 + n)
    a = rng_np.integers(0, 1 << 63, size=(n, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    b = rng_np.integers(0, 1 << 63, size=(n, n), dtype=np.uint64)
    circ = matrix_circuit(a, b)
    assert (circ.num_constraints, circ.domain) == {128: (10706932, 1 << 24), 46: (1035770, 1 << 20)}[n]
    rng = random.Random(1000 + n)
    trap = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]
    rh = dev.r1cs_load(circ.r1cs, circ.num_vars)
    pk, vk = dev.setup(rh, circ.num_instance, circ.num_vars, circ.domain, trap, g1, g2)
    ph = dev.pk_load(pk, circ.num_instance)
    wh = dev.witness_load(circ.z)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    plain = dev.prove_resident(ph, rh, wh, r, s)
    streamed = dev.prove_matrix(ph, rh, a, b, r, s)
    dev.pk_precompute(ph)
    tabled = dev.prove_resident(ph, rh, wh, r, s)
    for f, h in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(h)
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    eproof, einf = oracle.prove(pk, r, s, circ.r1cs, circ.z)
    assert list(einf) == [0, 0, 0]
    for name, got in (("plain", plain), ("streamed", streamed[:2]), ("tabled", tabled)):
        assert np.array_equal(got[1], einf) and np.array_equal(got[0], eproof), name


@pytest.mark.parametrize("n,tables,parts", [(8, False, 0), (33, False, 0), (46, True, 0), (46, False, 8), (46, True, 1), (128, True, 0)])
def test_prove_matrix_streamed_equals_two_step(dev, n, tables, parts):
    """zkg16_prove_matrix: the assignment arrives on the device in parts while the z-side MSMs already run on the parts that exist
    (rounds summed bucket-wise, one reduction) -> the same proof bytes as zkg16_witness_matrix + zkg16_prove_resident on the same key,
    r, s; pairing-verified; with and without window tables, several slice counts (parts = 1: no overlap), random full-range inputs."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    from zksnark_finalproject_amd.device import scalar_mul, verify
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    rng_np = np.random.default_rng(4000 + n)
    a = rng_np.integers(0, 1 << 63, size=(n, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    b = rng_np.integers(0, 1 << 63, size=(n, n), dtype=np.uint64)
    circ = matrix_circuit(a, b)
    rng = random.Random(n)
    trap = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]
    rh = dev.r1cs_load(circ.r1cs, circ.num_vars)
    ph, vk = dev.setup_resident(rh, circ.num_instance, trap, g1, g2)
    if tables:
        dev.pk_precompute(ph, 17 if n < 100 else 0, 17 if n < 100 else 0)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    wh, pub, _ = dev.witness_matrix(a, b)
    want = dev.prove_resident(ph, rh, wh, r, s)
    dev.set_option("matrix_parts", parts)
    try:
        for _ in range(2):                       # twice: the second call reuses every workspace of the first
            proof, inf, pub2, ms = dev.prove_matrix(ph, rh, a, b, r, s)
            assert np.array_equal(pub2, circ.public_inputs) and np.array_equal(pub, pub2)
            assert np.array_equal(proof, want[0]) and np.array_equal(inf, want[1]), "streamed proof differs (parts used: %d)" % ms["parts"]
            # the slices that really ran (tests/stream_cases.py): 46x46 runs two whether 0 or 8 are asked for, 8x8 and 33x33 one,
            # 128x128 five; parts = 1 is one slice by definition
            assert ms["parts"] == len(stream_cases.slice_bounds((n * n + 1) // 2, parts)) == (2 if parts == 1 else {8: 2, 33: 2, 46: 3, 128: 6}[n])
    finally:
        dev.set_option("matrix_parts", 0)
    assert verify(vk, circ.public_inputs, proof, inf) is True
    after = dev.prove_resident(ph, rh, wh, r, s)                 # and the ordinary path still works on the same slots afterwards
    assert np.array_equal(after[0], want[0])
    for f, h in ((dev.pk_free, ph), (dev.r1cs_free, rh), (dev.witness_free, wh)):
        f(h)
    with pytest.raises(Exception):
        dev.prove_matrix(ph, rh, a, b, r, s)                     # freed handles


# ---------------------------------------------------------------------------------------------- the MatrixCircuit's R1CS on the device
@pytest.mark.parametrize("n", [2, 5, 9, 33, 46, 128])
def test_r1cs_matrix_on_device_equals_host_synthesis(dev, n):
    """zkg16_r1cs_matrix: the MatrixCircuit's three CSR matrices written by kernels from the plan (one template per Poseidon-
    permutation class with renamed variables + matrix_mul's closed form) == the arrays of the full gadget-level synthesis on the
    host (zkg16_circuit_matrix + zkg16_circuit_export), array for array; even / odd n and the headline size (86.6 M non-zeros)."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    ones = np.ones((n, n), dtype=np.uint64)
    full = matrix_circuit(ones, ones)
    rh = dev.r1cs_matrix(n)
    got, nv = dev.r1cs_read(rh)
    assert nv == full.num_vars and got["num_constraints"] == full.num_constraints and got["num_inputs"] == full.num_instance
    for m in "abc":
        for k, name in enumerate(("row_ptr", "col", "coeff")):
            assert np.array_equal(got[m][k], full.r1cs[m][k]), (m, name)
    del got
    # and it is a working handle: the witness map on it equals the one on the uploaded matrices
    if n <= 46:
        rh2 = dev.r1cs_load(full.r1cs, full.num_vars)
        wh = dev.witness_load(full.z)
        h1 = dev.witness_map(rh, wh, full.domain)
        h2 = dev.witness_map(rh2, wh, full.domain)
        assert np.array_equal(h1, h2)
        dev.r1cs_free(rh2)
        dev.witness_free(wh)
    dev.r1cs_free(rh)


@pytest.mark.parametrize("n", [8, 46])
def test_whole_request_without_host_synthesis(dev, n):
    """A first request with nothing of the circuit built on the host: matrices by zkg16_r1cs_matrix, key by zkg16_setup_resident on
    them, assignment + proof by zkg16_prove_matrix — the proof verifies against the hashes the call returns, equals the proof of the
    host-synthesized flow for the same trapdoor, r, s, and fails for a wrong public input."""
    from zksnark_finalproject_amd.circuits import matrix_circuit
    from zksnark_finalproject_amd.device import scalar_mul, verify
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    rng_np = np.random.default_rng(9000 + n)
    a = rng_np.integers(0, 1 << 50, size=(n, n), dtype=np.uint64)
    b = rng_np.integers(0, 1 << 50, size=(n, n), dtype=np.uint64)
    rng = random.Random(3 * n)
    trap = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    rh = dev.r1cs_matrix(n)
    ph, vk = dev.setup_resident(rh, 4, trap, g1, g2)
    proof, inf, pub, _ = dev.prove_matrix(ph, rh, a, b, r, s)
    assert verify(vk, pub, proof, inf) is True
    bad = pub.copy()
    bad[1] = bad[0]
    assert verify(vk, bad, proof, inf) is False
    circ = matrix_circuit(a, b)                                     # the host-synthesized flow
    rh2 = dev.r1cs_load(circ.r1cs, circ.num_vars)
    ph2, vk2 = dev.setup_resident(rh2, circ.num_instance, trap, g1, g2)
    wh2 = dev.witness_load(circ.z)
    want = dev.prove_resident(ph2, rh2, wh2, r, s)
    assert np.array_equal(pub, circ.public_inputs)
    assert np.array_equal(proof, want[0]) and np.array_equal(inf, want[1])
    for key in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1"):
        assert np.array_equal(np.asarray(vk[key]), np.asarray(vk2[key])), key
    for f, h in ((dev.pk_free, ph), (dev.pk_free, ph2), (dev.r1cs_free, rh), (dev.r1cs_free, rh2), (dev.witness_free, wh2)):
        f(h)


def test_two_streamed_requests_at_once(dev):
    """Two callers, each a whole matrix request (zkg16_prove_matrix) on the same resident key and device-written matrices, different
    inputs: each gets the proof the two-step path gives for its inputs, and both verify."""
    import threading
    from zksnark_finalproject_amd.device import verify
    from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
    n = 40
    rng_np = np.random.default_rng(40)
    inputs = [(rng_np.integers(0, 1 << 60, size=(n, n), dtype=np.uint64), rng_np.integers(0, 1 << 60, size=(n, n), dtype=np.uint64)) for _ in range(4)]
    trap = np.stack([fr_mont(1000 + k) for k in range(5)])
    rh = dev.r1cs_matrix(n)
    ph, vk = dev.setup_resident(rh, 4, trap, g1_generator(), g2_generator())
    r, s = fr_mont(77), fr_mont(99)
    want = []
    for a, b in inputs:
        wh, pub, _ = dev.witness_matrix(a, b)
        want.append((dev.prove_resident(ph, rh, wh, r, s), pub))
        dev.witness_free(wh)
    out = [None] * len(inputs)

    def work(i):
        out[i] = dev.prove_matrix(ph, rh, inputs[i][0], inputs[i][1], r, s)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(inputs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(len(inputs)):
        proof, inf, pub, _ = out[i]
        assert np.array_equal(pub, want[i][1]) and np.array_equal(proof, want[i][0][0]) and np.array_equal(inf, want[i][0][1]), i
        assert verify(vk, pub, proof, inf) is True
    assert {l for l, _, _ in dev.lane_log(len(inputs))} == {0, 1}
    dev.pk_free(ph)
    dev.r1cs_free(rh)
