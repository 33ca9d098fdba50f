"""The six-transform witness map (csrc/poly.hip: wm_transforms; option "wm_transforms" 6 = default, 7 = arkworks' seven): C is
only inverse-transformed, with 1/Z folded into that transform's last store, and subtracted on the store of the last transform,
whose fused load is the one product A_cos * B_cos / Z (1/Z folded into B's coset transform).  h must equal the CPU oracle's
(arkworks' seven transforms) word for word in every NTT plan and kernel variant, for a satisfied assignment and an unsatisfied one
on the same matrices (the oracle's witness map does not check satisfaction; h's top coefficient is then non-zero) — on one ctx,
twice in a row on one ctx, in a batch of proofs and on a device group."""
import contextlib
import itertools
import os
import random

import numpy as np
import pytest

import pyref as P
import synth
from helpers import fr_mont, fr_mont_vec

pytestmark = pytest.mark.gpu

R = P.R_MOD
OPT_DEFAULTS = {"ntt_radix": 1, "ntt_mode": 1, "fuse_pointwise": 1, "wm_transforms": 6}
NDEV = 4


@pytest.fixture(scope="module")
def devs():
    from zksnark_finalproject_amd import Device
    ds = [Device(0) for _ in range(NDEV)]
    yield ds
    for d in ds:
        d.close()


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    yield oracle
    oracle.set_threads(1)


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


def assert_same(got, exp, what):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(exp)).any(axis=1))
    assert bad.size == 0, "%s: %d of %d words differ, first at %d" % (what, bad.size, len(exp), bad[0])


def _mont_rows(orc, vals):
    """sequence of canonical ints -> (len, 4) Montgomery u64 words."""
    canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    return orc.fr_from_canonical(canon)


def numpy_r1cs(orc, log_n, seed, nv=1024, ni=4):
    """A satisfiable R1CS whose domain is 2^log_n (every row has two terms in A and B, random columns, coefficients from a pool
    of random residues, and C = c1 z_j + c0 z_0 with c0 chosen so that <A,z> <B,z> = <C,z>), its satisfying assignment and an
    unsatisfied one (z_0 = 1, the other variables redrawn) -> (r1cs, [z, z_bad] Montgomery, nv)."""
    nc = (1 << (log_n - 1)) + (1 << max(log_n - 3, 0)) - ni + 1
    assert max(nc + ni - 1, 0).bit_length() == log_n
    rng = np.random.default_rng(seed)
    prng = random.Random(seed)
    z = np.array([1] + [P.rand_fr(prng) for _ in range(nv - 1)], dtype=object)
    z_bad = [1] + [P.rand_fr(prng) for _ in range(nv - 1)]
    pool = np.array([P.rand_fr(prng) for _ in range(64)], dtype=object)
    pool_m = _mont_rows(orc, pool)
    cols, coefs, vals = {}, {}, {}
    for m in ("a", "b"):
        j1 = rng.integers(0, nv, size=nc)
        j2 = (j1 + rng.integers(1, nv, size=nc)) % nv            # two distinct columns
        p1, p2 = rng.integers(0, 64, size=nc), rng.integers(0, 64, size=nc)
        cols[m] = np.stack([j1, j2], axis=1)
        coefs[m] = np.stack([pool_m[p1], pool_m[p2]], axis=1)
        vals[m] = (pool[p1] * z[j1] + pool[p2] * z[j2]) % R
    jc, pc = rng.integers(1, nv, size=nc), rng.integers(0, 64, size=nc)
    c0 = (vals["a"] * vals["b"] - pool[pc] * z[jc]) % R
    cols["c"] = np.stack([jc, np.zeros(nc, dtype=np.int64)], axis=1)
    coefs["c"] = np.stack([pool_m[pc], _mont_rows(orc, c0)], axis=1)
    rp = np.arange(nc + 1, dtype=np.uint64) * np.uint64(2)
    r1cs = dict(num_inputs=ni, num_constraints=nc)
    for m in ("a", "b", "c"):
        r1cs[m] = (rp, np.ascontiguousarray(cols[m].reshape(-1), dtype=np.uint32), np.ascontiguousarray(coefs[m].reshape(-1, 4)))
    return r1cs, [_mont_rows(orc, z), _mont_rows(orc, z_bad)], nv


@pytest.fixture(scope="module")
def systems(orc):
    """log_n -> (r1cs, nv, [(name, assignment, oracle h)]) for the satisfied and the unsatisfied assignment, built once per size."""
    cache = {}

    def get(log_n):
        if log_n not in cache:
            r1cs, zs, nv = numpy_r1cs(orc, log_n, 600 + log_n)
            cases = []
            for name, zm in zip(("satisfied", "unsatisfied"), zs):
                want = orc.witness_map(r1cs, zm)
                assert want.shape[0] == 1 << log_n
                # h's top coefficient: zero when a b - c vanishes on the domain, not for the unsatisfied assignment
                assert bool(want[-1].any()) == (name == "unsatisfied"), (log_n, name)
                cases.append((name, zm, want))
            cache[log_n] = (r1cs, nv, cases)
        return cache[log_n]

    yield get
    cache.clear()


@contextlib.contextmanager
def loaded(dev, r1cs, nv, cases):
    rh = dev.r1cs_load(r1cs, nv)
    whs = [dev.witness_load(zm) for _, zm, _ in cases]
    try:
        yield rh, whs
    finally:
        dev.r1cs_free(rh)
        for wh in whs:
            dev.witness_free(wh)


# ---------------------------------------------------------------------------------------------- 1. every plan and variant
# single tile (2^4, 2^11), two-pass over 2048-point tiles (2^12, 2^17, 2^21), 4096-point tiles (2^23), three passes (2^23 with
# ntt_mode 3, and ntt_mode 0 there)
PLANS = [(4, (0, 1)), (11, (0, 1)), (12, (0, 1)), (17, (0, 1)), (21, (0, 1)), (23, (0, 1, 3))]


@pytest.mark.parametrize("log_n,modes", PLANS)
def test_witness_map_equals_oracle_in_every_variant(devs, systems, log_n, modes):
    """ntt_mode x ntt_radix {1, 2, 3, 4} x fuse_pointwise {0, 1} x wm_transforms {6, 7}, satisfied and unsatisfied."""
    dev = devs[0]
    r1cs, nv, cases = systems(log_n)
    with loaded(dev, r1cs, nv, cases) as (rh, whs):
        for mode, radix, fuse, wmt in itertools.product(modes, (1, 2, 3, 4), (0, 1), (6, 7)):
            with options([dev], {"ntt_mode": mode, "ntt_radix": radix, "fuse_pointwise": fuse, "wm_transforms": wmt}):
                for (name, _, want), wh in zip(cases, whs):
                    assert_same(dev.witness_map(rh, wh, 1 << log_n), want, (log_n, mode, radix, fuse, wmt, name))


# ---------------------------------------------------------------------------------------------- 2. stale scratch
@pytest.mark.parametrize("log_n", [11, 17, 23])
def test_back_to_back_assignments(devs, systems, log_n):
    """Witness maps in a row on one ctx with different assignments: the last store reads the subtrahend it overwrites, and no
    result may depend on what an earlier call left in the four buffers."""
    dev = devs[0]
    r1cs, nv, cases = systems(log_n)
    with loaded(dev, r1cs, nv, cases) as (rh, whs):
        for fuse in (1, 0):
            with options([dev], {"fuse_pointwise": fuse}):
                for i in (0, 1, 1, 0, 1):
                    name, _, want = cases[i]
                    assert_same(dev.witness_map(rh, whs[i], 1 << log_n), want, (log_n, fuse, name))


# ---------------------------------------------------------------------------------------------- 3. a batch of proofs
@pytest.fixture(scope="module")
def batch_setup(devs, oracle):
    """A random satisfiable R1CS on a 2^12 domain (the two-pass plan) with a host-built key; assignments: a random one (not
    satisfying), the satisfying one, another random one."""
    dev = devs[0]
    rng = random.Random(6006)
    nc, ni, nv = 3000, 3, 2500
    A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
    r1cs = synth.r1cs_arrays(A, B, C, ni)
    pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=dev.fixed_base)
    zs = [fr_mont_vec([1] + [P.rand_fr(rng) for _ in range(nv - 1)]), fr_mont_vec(z), fr_mont_vec([1] + [P.rand_fr(rng) for _ in range(nv - 1)])]
    ph, rh = dev.pk_load(pk, ni), dev.r1cs_load(r1cs, nv)
    whs = np.array([dev.witness_load(zz) for zz in zs], dtype=np.uint64)
    yield dict(pk=pk, r1cs=r1cs, zs=zs, ph=ph, rh=rh, whs=whs)
    for w in whs:
        dev.witness_free(int(w))
    dev.pk_free(ph)
    dev.r1cs_free(rh)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_prove_batch_with_an_unsatisfied_assignment(devs, oracle, batch_setup, k):
    """prove_batch of K = 1, 2, 3 (the first assignment unsatisfied): every proof equals prove_resident's and the oracle's."""
    dev, st = devs[0], batch_setup
    rng = random.Random(70 + k)
    rs = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(k)]).reshape(k, 4)
    ss = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(k)]).reshape(k, 4)
    expect = [oracle.prove(st["pk"], rs[i], ss[i], st["r1cs"], st["zs"][i]) for i in range(k)]
    for fuse in (1, 0):
        with options([dev], {"fuse_pointwise": fuse}):
            proofs, inf = dev.prove_batch(st["ph"], st["rh"], st["whs"][:k], rs, ss)
            for i in range(k):
                p, f = dev.prove_resident(st["ph"], st["rh"], int(st["whs"][i]), rs[i], ss[i])
                assert np.array_equal(proofs[i], p) and np.array_equal(inf[i], f), (fuse, i, "resident")
                assert np.array_equal(proofs[i], expect[i][0]) and np.array_equal(inf[i], expect[i][1]), (fuse, i, "oracle")


# ---------------------------------------------------------------------------------------------- 4. device groups
GROUP_VARIANTS = [{"wm_transforms": 6, "fuse_pointwise": 1}, {"wm_transforms": 6, "fuse_pointwise": 0},
                  {"wm_transforms": 6, "fuse_pointwise": 1, "ntt_mode": 0}, {"wm_transforms": 7, "fuse_pointwise": 1}]


@pytest.mark.parametrize("log_n", [16, 23])
def test_group_witness_map_equals_oracle(devs, systems, log_n):
    """zkg16_witness_map_group on 2, 3 and 4 ctxs of one GPU (the split witness map, csrc/group.hip) == the oracle, satisfied and
    unsatisfied."""
    from zksnark_finalproject_amd import DeviceGroup
    r1cs, nv, cases = systems(log_n)
    hs = [(d.r1cs_load(r1cs, nv), [d.witness_load(zm) for _, zm, _ in cases]) for d in devs]
    try:
        for k in (2, 3, 4):
            g = DeviceGroup(devs[:k])
            try:
                for opts in GROUP_VARIANTS:
                    # ntt_mode 0 runs 2^23 in three passes: no split there, the replicated map
                    split = not (log_n > 22 and opts.get("ntt_mode") == 0)
                    with options(devs[:k], opts):
                        for c, (name, _, want) in enumerate(cases):
                            got = g.witness_map([h[0] for h in hs[:k]], [h[1][c] for h in hs[:k]], 1 << log_n)
                            assert g.last_wm() == (k if split else 0), (log_n, k, opts, name)
                            assert_same(got, want, (log_n, k, opts, name))
            finally:
                g.close()
    finally:
        for d, (rh, whs) in zip(devs, hs):
            d.r1cs_free(rh)
            for wh in whs:
                d.witness_free(wh)
