"""Each proof's own verdict on the device: zkg16_final_exp_batch against zkg16_final_exp, zkg16_verify_each against a loop of
zkg16_verify_prepared, and the batch verifiers' switch from bisecting to the per-proof pass (option "verify_each_after").  Shapes:
below a wave, a wave, one over, many blocks — the kernels are one lane per proof, blocks of one wave, read through an index list."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as P
import verify_batch_cases as VB
from helpers import *

pytestmark = pytest.mark.gpu

NEVER = 1 << 20         # above 2K for every K here: bisecting to the end


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    d.set_option("verify_batch_min", 1)         # every batch of this module runs the kernels
    d.set_option("verify_wire_min", 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def batch1000(oracle):
    """1,000 distinct proofs, built as tests/test_verify_batch_gpu.py builds them: 40 assignments proved by the oracle, then
    re-randomised — (A, B, C) -> (t A, t^-1 B, C) is again a valid proof of the same statement"""
    return VB.rerandomised(oracle, VB.make_batch(oracle, 40), 1000, random.Random(77))


@pytest.fixture(scope="module")
def torsion():
    return VB.g2_outside_subgroup()


def tamper_every_third(oracle, b0, torsion):
    """every third proof tampered, the kinds cycled (swap_a at i exchanges A_i and A_{i+1}: both fail)"""
    b = b0
    for n, i in enumerate(range(0, b0.k, 3)):
        b = VB.tamper(oracle, b, VB.TAMPERS[n % len(VB.TAMPERS)], (i,), torsion)
    return b


@pytest.fixture(scope="module")
def dense(oracle, batch1000, torsion):
    """K = 1000 with every third proof tampered and K = 65 likewise, each with the loop's verdicts (computed once)"""
    out = {}
    for k in (65, 1000):
        b = tamper_every_third(oracle, batch1000.head(k), torsion)
        out[k] = (b, b.loop())
        assert not out[k][1][0] and out[k][1].sum() > k // 2
    return out


to_wire = VB.to_wire


def each(dev, b):
    return dev.verify_each(b.pvk, b.pubs, b.proofs, b.infs)


# ------------------------------------------------------------------------------------------------ final_exp_batch
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_final_exp_batch_vs_host(dev, oracle, n):
    """Miller values of random pairs from miller_loop_batch, with one and zero among them: each row bit-equal to zkg16_final_exp"""
    from zksnark_finalproject_amd.device import final_exp
    rng = random.Random(2000 + n)
    g1 = oracle.fixed_base("g1", G1_GEN_LIMBS, fr_canon_vec([rng.randrange(1, P.R_MOD) for _ in range(n)]))[0]
    g2 = oracle.fixed_base("g2", G2_GEN_LIMBS, fr_canon_vec([rng.randrange(1, P.R_MOD) for _ in range(n)]))[0]
    f = dev.miller_loop_batch(g1, g2)
    one = np.concatenate([fq_mont(1), np.zeros(66, dtype=np.uint64)])
    cases = [f]
    if n == 1:
        cases += [one.reshape(1, 72), np.zeros((1, 72), np.uint64)]
    else:
        f[n // 2] = one
        f[n - 1] = 0
    for x in cases:
        got = dev.final_exp_batch(x)
        check = range(n) if n <= 65 else list(range(0, n, 37)) + [n // 2, n - 2, n - 1]
        for i in check:
            assert np.array_equal(got[i], final_exp(x[i])), (n, i)
    if n == 1:
        assert dev.final_exp_batch(np.zeros((0, 72), np.uint64)).shape == (0, 72)
        assert dev.lib.zkg16_final_exp_batch(dev.ctx, None, 0, None) == 0
        assert dev.lib.zkg16_final_exp_batch(dev.ctx, None, 1, None) == 1


# ------------------------------------------------------------------------------------------------ verify_each
@pytest.mark.parametrize("k", [1, 64, 65, 1000])
def test_verify_each_all_valid(dev, batch1000, k):
    b = batch1000.head(k)
    got = each(dev, b)
    assert got.shape == (k,) and got.all()
    if k <= 65:
        assert np.array_equal(got, b.loop())


@pytest.mark.parametrize("k", [1, 65, 1000])
@pytest.mark.parametrize("kind", VB.TAMPERS)
def test_verify_each_tampered(dev, oracle, batch1000, torsion, k, kind):
    b0 = batch1000.head(k)
    for where in VB.positions(k):
        b = VB.tamper(oracle, b0, kind, where, torsion)
        got = each(dev, b)
        if k <= 65:
            want = b.loop()
        else:       # the loop's verdicts are known by construction (test_verify_batch_gpu.py checks the same at this size)
            want = np.ones(k, dtype=bool)
            want[list(where)] = False
            if kind == "swap_a":
                want[[(i + 1) % k for i in where]] = False
        assert not want.all()
        assert np.array_equal(got, want), (kind, where)


def test_verify_each_dense_failures(dev, dense):
    b, loop = dense[1000]
    assert np.array_equal(each(dev, b), loop)


def test_verify_each_zero_limbs_without_flag(dev, batch1000):
    """all-zero limbs read as the point at infinity whatever the flag says, as zkg16_verify_prepared reads them"""
    b = batch1000.head(3)
    b.proofs[1, 36:48] = 0
    assert np.array_equal(each(dev, b), b.loop())


def test_verify_each_two_passes(dev, oracle, batch1000):
    """K = 65,537: two launches of each kernel, the second of one proof; one tampered proof in each pass"""
    k = 65537
    b = batch1000.tiled(k)
    for bad in (4321, 65536):
        b.proofs[bad, 36:48] = VB.g1_add(oracle, b.proofs[bad, 36:48], G1_GEN_LIMBS)
    want = np.ones(k, dtype=bool)
    want[[4321, 65536]] = False
    assert np.array_equal(each(dev, b), want)


def test_verify_each_bad_arguments(dev, batch1000):
    b = batch1000.head(3)
    gabc = np.ascontiguousarray(b.pvk["gamma_abc_g1"], dtype=np.uint64).reshape(-1, 12)
    ab = np.ascontiguousarray(b.pvk["alpha_beta"], dtype=np.uint64)
    g = np.ascontiguousarray(b.pvk["gamma_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    d = np.ascontiguousarray(b.pvk["delta_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    p = lambda a: a.ctypes.data

    def call(**kw):
        a = dict(ctx=dev.ctx, gabc=p(gabc), ni=gabc.shape[0], ab=p(ab), g=p(g), d=p(d), nc=68, pub=p(b.pubs), proofs=p(b.proofs), inf=p(b.infs), k=3)
        a.update(kw)
        out = np.full(3, 9, dtype=np.uint8)
        rc = dev.lib.zkg16_verify_each(a["ctx"], a["gabc"], a["ni"], a["ab"], a["g"], a["d"], a["nc"], a["pub"], a["proofs"], a["inf"], a["k"],
                                       None if kw.get("out_null") else p(out))
        return rc, out
    rc, out = call()
    assert rc == 0 and (out == 1).all()
    for kw in [dict(k=0), dict(nc=67), dict(nc=69), dict(ni=0), dict(ctx=None), dict(gabc=None), dict(ab=None), dict(g=None), dict(d=None), dict(pub=None),
               dict(proofs=None), dict(inf=None), dict(out_null=True)]:
        rc, out = call(**kw)
        assert rc == 1 and (out == 9).all(), kw


# ------------------------------------------------------------------------------------------------ routing inside the batch verifiers
def run_batch(dev, b, rho, after, wire):
    dev.set_option("verify_each_after", after)
    try:
        if wire is not None:
            ok, got = dev.verify_batch_wire(b.pvk, b.pubs, wire, rho=rho, each=True)
        else:
            ok, got = dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)
        tm = dev.verify_batch_timings()
    finally:
        dev.set_option("verify_each_after", 0)
    assert tm["host_form"] == 0
    return ok, got, tm


@pytest.mark.parametrize("form", ["limbs", "wire"])
@pytest.mark.parametrize("k", [65, 1000])
@pytest.mark.parametrize("bad", ["one", "every_third"])
def test_batch_routing(dev, oracle, batch1000, dense, form, k, bad):
    """The same tampered batch with the per-proof pass after the first range test and with bisecting to the end: the same verdicts,
    the pass timed in the first run only, and no more range tests in the first run than in the second."""
    if bad == "one":
        b = VB.tamper(oracle, batch1000.head(k), "c_plus_g", (k // 3,))
        want = np.ones(k, dtype=bool)
        want[k // 3] = False
    else:
        b, want = dense[k]
    rho = VB.draw_rho(random.Random(k + len(bad)), k)
    wire = to_wire(b) if form == "wire" else None
    ok1, each1, tm1 = run_batch(dev, b, rho, 1, wire)
    ok2, each2, tm2 = run_batch(dev, b, rho, NEVER, wire)
    assert ok1 is False and ok2 is False
    assert np.array_equal(each1, want) and np.array_equal(each2, want)
    assert tm1["each_ms"] > 0 and tm2["each_ms"] == 0
    assert 1 <= tm1["range_tests"] <= tm2["range_tests"]
    assert tm1["range_tests"] == 1


def test_valid_batch_never_makes_the_pass(dev, batch1000):
    b = batch1000.head(65)
    ok, got, tm = run_batch(dev, b, VB.draw_rho(random.Random(3), 65), 1, None)
    assert ok is True and got.all() and tm["each_ms"] == 0 and tm["range_tests"] == 0
    ok, got, tm = run_batch(dev, b, VB.draw_rho(random.Random(4), 65), 1, to_wire(b))
    assert ok is True and got.all() and tm["each_ms"] == 0 and tm["range_tests"] == 0


def test_index_list_is_the_open_ranges(dev, oracle, batch1000):
    """K = 1000, bad proofs only in the last quarter, the pass after the first range test: that one test passes for the first half,
    which the pass therefore never sees; its list starts at proof 500.  A list applied as if it were 0 .. n - 1 would read the
    (valid) first half and find nothing."""
    k = 1000
    where = (760, 761, 900, 999)
    b = VB.tamper(oracle, batch1000.head(k), "c_plus_g", where)
    want = np.ones(k, dtype=bool)
    want[list(where)] = False
    ok, got, tm = run_batch(dev, b, VB.draw_rho(random.Random(11), k), 1, None)
    assert ok is False and np.array_equal(got, want)
    assert tm["range_tests"] == 1 and tm["each_ms"] > 0
    # the same through public inputs, which the pass gathers by the list too
    b = VB.tamper(oracle, batch1000.head(k), "public_input", where)
    ok, got, tm = run_batch(dev, b, VB.draw_rho(random.Random(12), k), 1, None)
    assert ok is False and np.array_equal(got, want) and tm["range_tests"] == 1


def test_default_option_and_timing_keys(dev, batch1000):
    tm = dev.verify_batch_timings()
    assert list(tm)[-2:] == ["each_ms", "range_tests"] and len(tm) == 11
    ms = (C.c_float * 9)()
    assert dev.lib.zkg16_verify_batch_timings(dev.ctx, ms, 9) == 9          # a caller with room for nine sees nine
    with pytest.raises(Exception):
        dev.set_option("verify_each_after", -1)
