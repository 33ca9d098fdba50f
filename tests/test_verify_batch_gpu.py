"""zkg16_verify_batch on the device: the Miller loops, membership tests and the product tree of csrc/verify_batch.hip against the host
pairing, and the batch verdicts against zkg16_verify_batch_host (same multipliers) and a loop of zkg16_verify_prepared."""
import random
import threading

import numpy as np
import pytest

import pyref as P
import verify_batch_cases as VB
from helpers import *

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    d.set_option("verify_batch_min", 1)         # every batch of this module runs the kernels, K = 1 included
    yield d
    d.close()


@pytest.fixture(scope="module")
def batch1000(oracle):
    """1,000 distinct proofs: 40 assignments proved by the oracle, each with 25 (r, s) — re-randomised proofs of one statement are
    distinct proofs"""
    base = VB.make_batch(oracle, 40)
    rng = random.Random(77)
    return VB.rerandomised(oracle, base, 1000, rng)


@pytest.fixture(scope="module")
def torsion():
    return VB.g2_outside_subgroup()


def random_pairs(oracle, n, seed):
    rng = random.Random(seed)
    g1 = oracle.fixed_base("g1", G1_GEN_LIMBS, fr_canon_vec([rng.randrange(1, P.R_MOD) for _ in range(n)]))[0]
    g2 = oracle.fixed_base("g2", G2_GEN_LIMBS, fr_canon_vec([rng.randrange(1, P.R_MOD) for _ in range(n)]))[0]
    i1, i2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(3, n, 17):              # never pair 0: a launch of one pair runs a Miller loop
        i1[i] = 1
    for i in range(5, n, 29):
        i2[i] = 1
    return g1, i1, g2, i2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_miller_loop_batch_vs_host_pairing(dev, oracle, n):
    """final_exp of each device Miller value == the host pairing of that pair, in the verifier's normalisation: alpha_beta of
    zkg16_pvk_prepare for a key with alpha = P, beta = Q.  A pair with a point at infinity gives one."""
    from zksnark_finalproject_amd.device import final_exp, pvk_prepare
    g1, i1, g2, i2 = random_pairs(oracle, n, 1000 + n)
    f = dev.miller_loop_batch(g1, g2, i1, i2)
    one = np.concatenate([fq_mont(1), np.zeros(66, dtype=np.uint64)])
    for i in range(n):
        if i1[i] or i2[i]:
            assert np.array_equal(f[i], one), i
            continue
        want = pvk_prepare(dict(alpha_g1=g1[i], beta_g2=g2[i], gamma_g2=G2_GEN_LIMBS, delta_g2=G2_GEN_LIMBS))["alpha_beta"]
        assert np.array_equal(final_exp(f[i]), want), i
    if n == 1:                              # and the one-pair launch with its point at infinity
        for fl in ((1, 0), (0, 1)):
            f1 = dev.miller_loop_batch(g1, g2, np.array([fl[0]], np.uint8), np.array([fl[1]], np.uint8))
            assert np.array_equal(f1[0], one), fl


def test_miller_loop_batch_limbs_equal_host_miller(dev, oracle):
    """n = 64: the device's Miller values equal the host's limb for limb (ark's line scaling on both sides; canonical limbs).  The
    host values come from the host-compiled shim tests/csrc/pairing_host_shim.hip (pairing_fast.inc's miller_loop)."""
    shim = VB.load_shim()
    g1, i1, g2, i2 = random_pairs(oracle, 64, 64064)
    f = dev.miller_loop_batch(g1, g2, i1, i2)
    for i in range(64):
        if i1[i] or i2[i]:
            continue
        od, oh = VB.host_miller(shim, g1[i], g2[i])
        assert np.array_equal(f[i], oh), i


@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_point_check_batch(dev, oracle, torsion, group, n):
    from zksnark_finalproject_amd import wire
    from zksnark_finalproject_amd.device import point_check
    rng = random.Random(n * 3 + len(group))
    w = 12 if group == "g1" else 24
    gen = G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS
    pts = oracle.fixed_base(group, gen, fr_canon_vec([rng.randrange(1, P.R_MOD) for _ in range(n)]))[0].copy()
    inf = np.zeros(n, np.uint8)
    if group == "g1":
        outside = None
        while outside is None:
            cx = rng.randrange(P.Q_MOD)
            y = wire._sqrt_fq((cx ** 3 + 4) % P.Q_MOD)
            if y is not None:
                cand = np.concatenate([fq_mont(cx), fq_mont(y)])
                if not point_check("g1", cand):
                    outside = cand
    else:
        outside = torsion
    kinds = np.zeros(n, dtype=int)                      # 0 subgroup, 1 infinity, 2 off the curve, 3 on the curve outside the subgroup
    for i in range(n):
        kinds[i] = (0, 1, 2, 3)[i % 4] if n > 1 else 0
    if n == 1:
        cases = [(0,), (1,), (2,), (3,)]
    else:
        cases = [tuple(kinds)]
    for case in cases:
        p, fl = pts.copy(), inf.copy()
        for i, kd in enumerate(case):
            if kd == 1:
                p[i] = 0
                fl[i] = 1
            elif kd == 2:
                p[i, w - 1] ^= np.uint64(1 << 9)
            elif kd == 3:
                p[i] = outside
        got = dev.point_check_batch(group, p, fl)
        for i, kd in enumerate(case):
            want = True if kd == 1 else point_check(group, p[i])
            assert want == (kd in (0, 1)), (i, kd)
            assert bool(got[i]) == want, (group, i, kd)


def both(dev, b, rho):
    from zksnark_finalproject_amd.device import verify_batch_host
    ok_d, each_d = dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)
    assert dev.verify_batch_timings()["host_form"] == 0
    ok_h, each_h = verify_batch_host(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)
    assert ok_d == ok_h and np.array_equal(each_d, each_h)
    assert dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho) == ok_h
    return ok_d, each_d


@pytest.mark.parametrize("k", [1, 64, 65, 1000])
def test_verify_batch_all_valid(dev, batch1000, k):
    b = batch1000.head(k)
    ok, each = both(dev, b, VB.draw_rho(random.Random(k), k))
    assert ok is True and each.all()
    if k <= 65:
        assert b.loop().all()
    assert dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs) is True        # multipliers from `secrets`


@pytest.mark.parametrize("k", [1, 64, 65, 1000])
@pytest.mark.parametrize("kind", VB.TAMPERS)
def test_verify_batch_tampered_sets(dev, oracle, batch1000, torsion, k, kind):
    b0 = batch1000.head(k)
    for where in VB.positions(k):
        b = VB.tamper(oracle, b0, kind, where, torsion)
        ok, each = both(dev, b, VB.draw_rho(random.Random(k * 7 + len(where)), k))
        assert ok is False, (kind, where)
        if k <= 65:
            assert np.array_equal(each, b.loop()), (kind, where)
        else:
            want = np.ones(k, dtype=bool)
            want[list(where)] = False
            if kind == "swap_a":
                want[[(i + 1) % k for i in where]] = False
            assert np.array_equal(each, want), (kind, where)


def test_verify_batch_cancelling_forgeries(dev, oracle, batch1000):
    b = batch1000.head(64)
    d = oracle.point_mul("g1", G1_GEN_LIMBS, fr_canon(987654321))[0]
    dneg = oracle.point_mul("g1", G1_GEN_LIMBS, fr_canon(P.R_MOD - 987654321))[0]
    b.proofs[10, 36:48] = VB.g1_add(oracle, b.proofs[10, 36:48], d)
    b.proofs[40, 36:48] = VB.g1_add(oracle, b.proofs[40, 36:48], dneg)
    ok, each = both(dev, b, VB.draw_rho(random.Random(9), 64))
    want = np.ones(64, dtype=bool)
    want[[10, 40]] = False
    assert ok is False and np.array_equal(each, want)


def test_verify_batch_bad_arguments(dev, batch1000):
    import ctypes as C
    b = batch1000.head(3)
    gabc = np.ascontiguousarray(b.pvk["gamma_abc_g1"], dtype=np.uint64).reshape(-1, 12)
    ab = np.ascontiguousarray(b.pvk["alpha_beta"], dtype=np.uint64)
    g = np.ascontiguousarray(b.pvk["gamma_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    d = np.ascontiguousarray(b.pvk["delta_neg_pc"], dtype=np.uint64).reshape(-1, 36)
    rho = VB.draw_rho(random.Random(1), 3)
    zero = rho.copy()
    zero[2] = 0
    p = lambda a: a.ctypes.data

    def call(**kw):
        a = dict(ctx=dev.ctx, gabc=p(gabc), ni=gabc.shape[0], ab=p(ab), g=p(g), d=p(d), nc=68, pub=p(b.pubs), proofs=p(b.proofs), inf=p(b.infs), rho=p(rho), k=3)
        a.update(kw)
        ok = C.c_int(-7)
        each = np.full(3, 9, dtype=np.uint8)
        rc = dev.lib.zkg16_verify_batch(a["ctx"], a["gabc"], a["ni"], a["ab"], a["g"], a["d"], a["nc"], a["pub"], a["proofs"], a["inf"], a["rho"], a["k"],
                                        None if kw.get("ok_null") else C.byref(ok), p(each))
        return rc, ok.value, each
    rc, ok, each = call()
    assert rc == 0 and ok == 1 and (each == 1).all()
    for kw in [dict(rho=p(zero)), dict(k=0), dict(nc=67), dict(ctx=None), dict(gabc=None), dict(ab=None), dict(g=None), dict(d=None), dict(pub=None),
               dict(proofs=None), dict(inf=None), dict(rho=None), dict(ok_null=True)]:
        rc, ok, each = call(**kw)
        assert rc == 1 and ok == -7 and (each == 9).all(), kw


def test_verify_batch_two_passes(dev, oracle, batch1000):
    """K = 70,000 (1,000 distinct proofs repeated): two passes of the kernels, one tampered proof in the second."""
    k = 70000
    b = batch1000.tiled(k)
    rho = VB.draw_rho(random.Random(70), k)
    assert dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho) is True
    bad = 65536 + 1234
    b.proofs[bad, 36:48] = VB.g1_add(oracle, b.proofs[bad, 36:48], G1_GEN_LIMBS)
    ok, each = dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)
    want = np.ones(k, dtype=bool)
    want[bad] = False
    assert ok is False and np.array_equal(each, want)


@pytest.fixture(scope="module")
def fib256(dev):
    """256 Fibonacci-1000 assignments proved in one prove_batch pass on a resident key"""
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    from zksnark_finalproject_amd.device import pvk_prepare
    import bench
    k = 256
    circs = [fibonacci_circuit(3 * i + 1, 5 * i + 2, 1000) for i in range(k)]
    rh = dev.r1cs_load(circs[0].r1cs, circs[0].num_vars)
    trap, g1, g2 = bench.draw_key_inputs(42)
    ph, vk = dev.setup_resident(rh, circs[0].num_instance, trap, g1, g2)
    whs = np.array([dev.witness_load(c.z) for c in circs], dtype=np.uint64)
    rng = random.Random(5)
    rs = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    ss = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    proofs, infs = dev.prove_batch(ph, rh, whs, rs, ss)
    pubs = np.array([c.public_inputs for c in circs], dtype=np.uint64).reshape(k, -1, 4)
    flipped = proofs.copy()
    flipped[100, 36:48].view(np.uint8)[17] ^= 0x40
    want = np.ones(k, dtype=bool)
    want[100] = False
    yield dict(k=k, ph=ph, rh=rh, whs=whs, rs=rs, ss=ss, proofs=proofs, infs=infs, pubs=pubs, pvk=pvk_prepare(vk), flipped=flipped, want=want)
    for w in whs:
        dev.witness_free(int(w))
    dev.pk_free(ph)
    dev.r1cs_free(rh)


def test_prove_batch_then_verify_batch(dev, fib256):
    """The round trip the feature exists for: what prove_batch emits, verify_batch checks; one flipped byte of one C is found."""
    st = fib256
    ok, each = dev.verify_batch(st["pvk"], st["pubs"], st["proofs"], st["infs"], each=True)
    assert ok is True and each.all()
    ok, each = dev.verify_batch(st["pvk"], st["pubs"], st["flipped"], st["infs"], each=True)
    assert ok is False and np.array_equal(each, st["want"])


def _together(jobs):
    gate = threading.Barrier(len(jobs))

    def run(fn):
        gate.wait()
        fn()
    th = [threading.Thread(target=run, args=(fn,)) for fn in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join()


def _overlapped_on_two_lanes(log):
    assert {l for l, _, _ in log} == {0, 1}, log
    (_, a0, a1), (_, b0, b1) = log
    assert a0 < b1 and b0 < a1, "the two calls did not overlap: %s" % (log,)


def test_two_verifiers_on_one_ctx(dev, fib256):
    """Two callers verifying at once: each on its own lane of the ctx, the same verdicts as alone."""
    st = fib256
    out = {}
    _together([lambda: out.__setitem__("good", dev.verify_batch(st["pvk"], st["pubs"], st["proofs"], st["infs"], each=True)),
               lambda: out.__setitem__("bad", dev.verify_batch(st["pvk"], st["pubs"], st["flipped"], st["infs"], each=True))])
    _overlapped_on_two_lanes(dev.lane_log(2))
    assert out["good"][0] is True and out["good"][1].all()
    assert out["bad"][0] is False and np.array_equal(out["bad"][1], st["want"])


def test_prove_batch_beside_verify_batch(dev, fib256):
    """A prove_batch and a verify_batch on one ctx at once: the proofs byte for byte and the verdicts as alone."""
    st = fib256
    out = {}
    _together([lambda: out.__setitem__("prove", dev.prove_batch(st["ph"], st["rh"], st["whs"][:32], st["rs"][:32], st["ss"][:32])),
               lambda: out.__setitem__("verify", dev.verify_batch(st["pvk"], st["pubs"], st["flipped"], st["infs"], each=True))])
    _overlapped_on_two_lanes(dev.lane_log(2))
    assert np.array_equal(out["prove"][0], st["proofs"][:32]) and np.array_equal(out["prove"][1], st["infs"][:32])
    assert out["verify"][0] is False and np.array_equal(out["verify"][1], st["want"])
