"""The bucket accumulations' mixed additions without their spare carry passes on the DEVICE.

First the gfx950 build of tests/csrc/madd_lazy_shim.hip (one lane per case, one wave per block) on the case tables of
tests/madd_lazy_cases.py: every output must pass the same exact checks as in tests/test_madd_lazy_host.py AND equal the host
build's output limb for limb - code generation must not change a value.

Then the real kernels: one small MSM per group through msm_accumulate_kernel with option acc_lazy = 1 (the default: these
additions) and 0 (xyzz_madd_inline / xyzz_madd_lazy).  256 bases and 32 windows of 8 bits (128 buckets each).  Every scalar is
below 2^128 or is r - k for such a k, which the digit kernel takes as -k (scalars above (r-1)/2 are folded), so only the lower 16
windows get non-zero digits and the lists hold about 4 k terms.  Segments are kept
short, so that buckets are long and several lanes split each; repeated bases (the doubling), a base next to its negative
under the same digit (the cancellation), shared small scalars of both signs.  Both results equal each other and the CPU oracle's
sum.  These are the smallest shapes that reach every branch of the loop."""
import random

import numpy as np
import pytest

import madd_lazy_cases as MC
import pyref as P
from helpers import *

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim():
    return MC.load_shim("device")


@pytest.fixture(scope="module")
def host():
    return MC.load_shim("host")


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def both(shim, host, op, inp):
    out = MC.run(shim, op, inp)
    assert np.array_equal(out, MC.run(host, op, inp)), "device and host outputs differ"
    return out


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_madd_points_at_bounds(shim, host, group):
    inp, expected = MC.point_cases(group)
    for n in (1, 63, 64, 65, len(expected)):
        MC.check_points(group, inp[:n], expected[:n], both(shim, host, MC.OP[group + "_madd"], inp[:n]))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_madd_worst_limbs(shim, host, group):
    inp, meta = MC.worst_limb_cases(group)
    MC.check_worst(group, meta, both(shim, host, MC.OP[group + "_madd"], inp))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_madd_chains(shim, host, group):
    inp, expected = MC.chain_cases(group)
    MC.check_chain(group, inp, expected, both(shim, host, MC.OP[group + "_chain"], inp))


def test_device_build_refuses_host_only_operations(shim):
    assert shim.madd_lazy_run(MC.OP["bad_two_lazy"], 0, None, None) == -2
    assert shim.madd_lazy_run(MC.OP["bad_column"], 0, None, None) == -2


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_small_msm_acc_lazy_on_and_off(dev, oracle, group):
    rng = random.Random(8128 if group == "g1" else 8129)
    gen = oracle.point_mul(group, G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS, fr_canon(P.rand_fr(rng)))[0]
    n, distinct = 256, 40
    ks = [P.rand_fr(rng) for _ in range(distinct)]
    ks += [P.R_MOD - k for k in ks[:8]]                      # the negatives of the first eight points
    pts, pinf = oracle.fixed_base(group, gen, fr_canon_vec(ks))
    pick = [rng.randrange(len(ks)) for _ in range(n)]
    pick[:32] = [i % 8 for i in range(32)]                   # the first eight points, four times each ...
    pick[32:48] = [distinct + i % 8 for i in range(16)]      # ... and their negatives, twice each
    bases, inf = pts[np.array(pick)], pinf[np.array(pick)].copy()
    inf[200:208] = 1
    shared = rng.randrange(1, 1 << 128)
    scalars = [rng.randrange(1, 1 << 128) for _ in range(n)]
    scalars[:48] = [shared] * 48                             # one bucket per window holds P four times and -P twice
    for i in range(48, 120):
        scalars[i] = rng.choice([1, 2, 3, P.R_MOD - 1, P.R_MOD - 2, shared, P.R_MOD - shared])
    sc = fr_canon_vec(scalars)
    want, winf = oracle.msm(group, bases, sc, inf)
    assert not winf
    got = {}
    try:
        dev.set_option("window_bits", 8)
        dev.set_option("min_seg", 3)
        for lazy in (1, 0):
            dev.set_option("acc_lazy", lazy)
            got[lazy] = dev.msm(group, bases, sc, inf)
    finally:
        dev.set_option("acc_lazy", 1)
        dev.set_option("window_bits", 0)
        dev.set_option("min_seg", 0)
    assert got[1][1] == got[0][1] == winf
    assert np.array_equal(got[1][0], got[0][0])
    assert np.array_equal(got[1][0], want)
