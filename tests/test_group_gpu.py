"""Device groups (zkg16_group_create / zkg16_witness_map_group / zkg16_prove_group): several ctxs of one process on device 0
prove one proof together, their witness-map ranks splitting the seven NTTs (csrc/group.hip).  The split witness map must give
the single-ctx zkg16_witness_map's h byte for byte at every two-pass size, for every rank count the tiles allow and every NTT
kernel variant; sizes where the split cannot apply take the replicated map (last_wm() == 0).  Group proofs must equal
zkg16_prove_resident's proof (== the oracle's) for plans with witness-map and z-only ranks, with and without window tables, and on
the 128x128 MatrixCircuit (2^24)."""
import contextlib
import random

import numpy as np
import pytest

import pyref as P
import synth
from helpers import fr_mont, fr_mont_vec

pytestmark = pytest.mark.gpu

NDEV = 8
OPT_DEFAULTS = {"ntt_radix": 1, "ntt_mode": 1, "fuse_pointwise": 1}


@pytest.fixture(scope="module")
def devs():
    from zksnark_finalproject_amd import Device
    ds = [Device(0) for _ in range(NDEV)]
    yield ds
    for d in ds:
        d.close()


@contextlib.contextmanager
def group_of(devs):
    from zksnark_finalproject_amd import DeviceGroup
    g = DeviceGroup(devs)
    try:
        yield g
    finally:
        g.close()


@contextlib.contextmanager
def options(devs, opts):
    try:
        for d in devs:
            for k, v in opts.items():
                d.set_option(k, v)
        yield
    finally:
        for d in devs:
            for k in opts:
                d.set_option(k, OPT_DEFAULTS[k])


def rand_fr_limbs(rng, n):
    """n residues below r as 4 x u64 limbs (any residue is some value's Montgomery form)."""
    v = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    v[:, 3] = rng.integers(0, P.R_MOD >> 192, size=n, dtype=np.uint64)
    return v


def big_r1cs(log_n, seed, ni=3):
    """A random (unsatisfied) sparse R1CS whose domain is 2^log_n, and an assignment: enough for the witness map."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    nc = n - ni - int(rng.integers(0, n // 4))
    nv = max(nc // 2, 16)
    r1cs = dict(num_inputs=ni, num_constraints=nc)
    for m in ("a", "b", "c"):
        lens = rng.integers(0, 3 if log_n <= 22 else 2, size=nc, dtype=np.uint64)
        rp = np.zeros(nc + 1, dtype=np.uint64)
        np.cumsum(lens, out=rp[1:])
        nnz = int(rp[-1])
        r1cs[m] = (rp, rng.integers(0, nv, size=nnz, dtype=np.uint32), rand_fr_limbs(rng, nnz))
    return r1cs, nv, rand_fr_limbs(rng, nv)


def allowed_ks(log_n, ks):
    from zksnark_finalproject_amd.device import group_layout
    return [k for k in ks if group_layout(log_n, k)["applies"]]


@contextlib.contextmanager
def loaded(devs, r1cs, nv, z):
    hs = [(d.r1cs_load(r1cs, nv), d.witness_load(z)) for d in devs]
    try:
        yield np.array([h[0] for h in hs], dtype=np.uint64), np.array([h[1] for h in hs], dtype=np.uint64)
    finally:
        for d, (rh, wh) in zip(devs, hs):
            d.r1cs_free(rh)
            d.witness_free(wh)


def assert_same(got, exp, what):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(exp)).any(axis=1))
    assert bad.size == 0, "%s: %d of %d words differ, first at %d" % (what, bad.size, len(exp), bad[0])


# ---------------------------------------------------------------------------------------------- witness map
@pytest.mark.parametrize("log_n", list(range(12, 25)))
def test_split_witness_map_equals_single_ctx(devs, log_n):
    ks = allowed_ks(log_n, (2, 3, 4, 8))
    assert 2 in ks
    r1cs, nv, z = big_r1cs(log_n, 100 + log_n)
    with loaded(devs[: max(ks)], r1cs, nv, z) as (rhs, whs):
        want = devs[0].witness_map(rhs[0], whs[0], 1 << log_n)
        for k in ks:
            with group_of(devs[:k]) as g:
                got = g.witness_map(rhs[:k], whs[:k], 1 << log_n)
                assert g.last_wm() == k
                stats = g.rank_stats()
                assert len(stats) == k and all(s["exchange_bytes"] > 0 and s["h_bytes"] > 0 for s in stats)
            assert_same(got, want, "2^%d, k = %d" % (log_n, k))


VARIANTS = [("radix2", {"ntt_radix": 2}), ("radix3", {"ntt_radix": 3}), ("radix4", {"ntt_radix": 4}), ("saturated", {"ntt_mode": 0}),
            ("three_pass", {"ntt_mode": 3}), ("unfused", {"fuse_pointwise": 0})]


@pytest.mark.parametrize("log_n", [16, 24])
def test_split_witness_map_kernel_variants(devs, log_n):
    k = 4
    r1cs, nv, z = big_r1cs(log_n, 7 * log_n)
    with loaded(devs[:k], r1cs, nv, z) as (rhs, whs):
        want = devs[0].witness_map(rhs[0], whs[0], 1 << log_n)
        with group_of(devs[:k]) as g:
            for name, opts in VARIANTS:
                with options(devs[:k], opts):
                    got = g.witness_map(rhs, whs, 1 << log_n)
                    # ntt_mode 0 and 3 run 2^24 in three passes: no split there
                    split = not (log_n == 24 and opts.get("ntt_mode") in (0, 3))
                    assert g.last_wm() == (k if split else 0), name
                assert_same(got, want, "2^%d %s" % (log_n, name))
            # the third and later calls on a handle run the SpMV over the rows in length-class order: the rank's rows are re-filtered
            assert_same(g.witness_map(rhs, whs, 1 << log_n), want, "2^%d again" % log_n)


@pytest.mark.parametrize("log_n", [10, 25])
def test_replicated_fallback(devs, log_n):
    r1cs, nv, z = big_r1cs(log_n, 5 + log_n)
    with loaded(devs[:2], r1cs, nv, z) as (rhs, whs):
        want = devs[0].witness_map(rhs[0], whs[0], 1 << log_n)
        with group_of(devs[:2]) as g:
            got = g.witness_map(rhs, whs, 1 << log_n)
            assert g.last_wm() == 0
        assert_same(got, want, "2^%d" % log_n)


# ---------------------------------------------------------------------------------------------- proofs
@pytest.fixture(scope="module")
def circuit(devs, oracle):
    """A random satisfiable system on a 2^14 domain (eight units of the split: up to 8 witness-map ranks), its key and the
    reference proof, resident on every device."""
    rng = random.Random(515)
    nc, ni, nv = 10000, 3, 8200
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=devs[0].fixed_base)
    zm = fr_mont_vec(z)
    r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
    eproof, einf = oracle.prove(pk, r, s, r1cs, zm)
    hs = [(d.pk_load(pk, ni), d.r1cs_load(r1cs, nv), d.witness_load(zm)) for d in devs]
    proof, inf = devs[0].prove_resident(*hs[0], r, s)
    assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)
    yield dict(pk=pk, r1cs=r1cs, nv=nv, ni=ni, n_h=(1 << 14) - 1, r=r, s=s, proof=proof, inf=inf, hs=hs)
    for d, (ph, rh, wh) in zip(devs, hs):
        d.pk_free(ph)
        d.r1cs_free(rh)
        d.witness_free(wh)


@pytest.mark.parametrize("ranks,h_ranks,tables", [(1, 1, False), (3, 1, False), (3, 2, False), (6, 4, False), (2, 2, True), (5, 4, True)])
def test_prove_group_equals_single_proof(devs, circuit, ranks, h_ranks, tables):
    from zksnark_finalproject_amd.device import shard_plan
    c = circuit
    plan, k = shard_plan(ranks, c["nv"], c["n_h"], 0.0, h_ranks, window_tables=tables)
    assert k == h_ranks
    shards = []
    for i, (z_lo, z_hi, h_lo, h_hi, blind) in enumerate(plan):
        d = devs[i]
        sh = d.pk_slice(c["hs"][i][0], z_lo, z_hi, h_lo, h_hi, blind) if i % 2 == 0 else \
            d.pk_load_range(c["pk"], c["ni"], z_lo, z_hi, h_lo, h_hi, blind)
        if tables:
            d.pk_precompute(sh)
        shards.append(sh)
    try:
        with group_of(devs[:ranks]) as g:
            rhs = [c["hs"][i][1] for i in range(ranks)]
            whs = [c["hs"][i][2] for i in range(ranks)]
            for _ in range(2):                     # two group proofs in a row on the same group
                proof, inf = g.prove(shards, rhs, whs, c["r"], c["s"])
                assert np.array_equal(proof, c["proof"]) and np.array_equal(inf, c["inf"])
                assert g.last_wm() == (k if k >= 2 else 0)
        again = devs[0].prove_resident(*c["hs"][0], c["r"], c["s"])        # a member ctx on its own afterwards
        assert np.array_equal(again[0], c["proof"]) and np.array_equal(again[1], c["inf"])
    finally:
        for d, sh in zip(devs, shards):
            d.pk_free(sh)


def test_prove_group_refuses_bad_arguments(devs, circuit):
    from zksnark_finalproject_amd import DeviceGroup, Zkg16Error
    from zksnark_finalproject_amd.device import shard_plan
    c = circuit
    with pytest.raises(Zkg16Error) as e:
        DeviceGroup([devs[0], devs[1], devs[0]])                  # one ctx twice
    assert e.value.status == 1
    plan, _ = shard_plan(2, c["nv"], c["n_h"], 0.0, 2)
    shards = [devs[i].pk_slice(c["hs"][i][0], *plan[i]) for i in range(2)]
    rhs = [c["hs"][i][1] for i in range(2)]
    whs = [c["hs"][i][2] for i in range(2)]
    other, onv, oz = big_r1cs(14, 3)
    orh = devs[1].r1cs_load(other, onv)
    owh = devs[1].witness_load(oz)
    try:
        with group_of(devs[:2]) as g:
            for bad_pk, bad_rh, bad_wh, status in (
                    ([shards[0], 987654], rhs, whs, 6),                  # a missing handle
                    (shards, rhs, [whs[0], 987654], 6),
                    (shards, [rhs[0], orh], [whs[0], owh], 1),           # another system on rank 1
                    (shards, rhs, [whs[0], owh], 1),                     # an assignment of another length
                    ([c["hs"][0][0], c["hs"][1][0]], rhs, whs, 1)):      # two whole keys: the shards do not tile the key
                with pytest.raises(Zkg16Error) as e:
                    g.prove(bad_pk, bad_rh, bad_wh, c["r"], c["s"])
                assert e.value.status == status
            proof, inf = g.prove(shards, rhs, whs, c["r"], c["s"])
            assert np.array_equal(proof, c["proof"]) and np.array_equal(inf, c["inf"]) and g.last_wm() == 2
    finally:
        for d, sh in zip(devs, shards):
            d.pk_free(sh)
        devs[1].r1cs_free(orh)
        devs[1].witness_free(owh)


def test_prove_group_matrix_128(devs):
    """The reference's 128x128 MatrixCircuit (2^24: the 4096-point-tile plan) on a 4-ctx group with plain keys: every ctx builds
    the matrices on the device and the key from the same trapdoor, then slices its shard; the group proof equals the single-ctx
    proof and verifies."""
    import ctypes as C

    import bench
    from zksnark_finalproject_amd import _lib
    from zksnark_finalproject_amd.device import shard_plan, verify
    n, k = 128, 4
    rng = np.random.default_rng(128)
    a = rng.integers(0, 1 << 20, size=(n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 20, size=(n, n), dtype=np.uint64)
    trap, g1, g2 = bench.draw_key_inputs(128)
    r, s = fr_mont(31337), fr_mont(4242)
    hs, vk, pub = [], None, None
    try:
        for d in devs[:k]:
            rh = d.r1cs_matrix(n)
            wh, pub, _ = d.witness_matrix(a, b)
            ph, vk = d.setup_resident(rh, 4, trap, g1, g2)
            hs.append((ph, rh, wh))
        proof, inf = devs[0].prove_resident(*hs[0], r, s)
        assert verify(vk, pub, proof, inf)
        nc, nw = C.c_size_t(), C.c_size_t()
        assert _lib.load().zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), None) == 0
        plan, _ = shard_plan(k, 4 + nw.value, (1 << 24) - 1, 0.0, k)
        shards = [devs[i].pk_slice(hs[i][0], *plan[i]) for i in range(k)]
        try:
            with group_of(devs[:k]) as g:
                gp, gi = g.prove(shards, [h[1] for h in hs], [h[2] for h in hs], r, s)
                assert g.last_wm() == k
        finally:
            for i in range(k):
                devs[i].pk_free(shards[i])
        assert np.array_equal(gp, proof) and np.array_equal(gi, inf)
    finally:
        for d, (ph, rh, wh) in zip(devs, hs):
            d.pk_free(ph)
            d.r1cs_free(rh)
            d.witness_free(wh)
