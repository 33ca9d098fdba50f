"""The prime form of batched verification on the device (zkg16_verify_prime_batch, zkg16_verify_prime_batch_wire, the stage entries
zkg16_prime_inputs_batch / zkg16_prime_rho_sums, handlers.verify_primes(dev=dev)): the kernels against the host entries and Python
integers byte for byte, real proofs of prove_prime_batch under the ONE extended key of their trapdoor, simulated statements whose
verdicts are known by construction (tests/prime_verify_cases.py), and the existing batch entries on an ordinary batch."""
import base64
import random

import numpy as np
import pytest

import prime_verify_cases as PV
import sim_proofs as S
import verify_batch_cases as VB
from helpers import *
from test_prime_device_host import X_J0

pytestmark = pytest.mark.gpu

M64 = PV.M64
# first-found primes (their circuits are satisfied, so the proofs verify); (2^64 - 1, 18) carries past 2^64
PROVED = [(X_J0, 0), (0, 3), (M64, 18), (12345, 9), (99, 4), (5, 19), (2**32, 3), (2**63, 5)]
BIG = 65537         # one more than a launch of the inputs kernel takes


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    d.set_option("verify_batch_min", 1)         # every batch of this module runs the kernels unless a test says otherwise
    d.set_option("verify_wire_min", 1)
    yield d
    d.close()


def thresholds(dev, batch_min, wire_min):
    dev.set_option("verify_batch_min", batch_min)
    dev.set_option("verify_wire_min", wire_min)


# ------------------------------------------------------------------------------------------------ the stage entries
@pytest.mark.parametrize("k", [1, 63, 64, 65, 300])
def test_prime_inputs_batch_equals_the_host_entries(dev, k):
    from zksnark_finalproject_amd.circuits import prime_candidate, prime_public_inputs
    pairs = PV.pairs_of(k, seed=k)
    assert k < 36 or set(PV.CARRY_PAIRS) <= set(pairs)
    dig, n, pub = dev.prime_inputs_batch([x for x, _ in pairs], [j for _, j in pairs], public_inputs=True)
    for i, (x, j) in enumerate(pairs):
        cand = prime_candidate(x, j)
        assert bytes(dig[i]) == bytes(bytearray(cand["digest"])) == PV.py_digest(x, j)[0] and int(n[i]) == int(cand["n"]), (x, j)
    for i in sorted({0, k // 2, k - 1} | set(range(min(k, 36)))):
        assert np.array_equal(pub[i], prime_public_inputs(*pairs[i])), pairs[i]


def test_prime_inputs_batch_across_a_launch_boundary(dev):
    pairs = PV.pairs_of(BIG, seed=1)
    dig, n = dev.prime_inputs_batch([x for x, _ in pairs], [j for _, j in pairs])
    want = [PV.py_digest(x, j) for x, j in pairs]
    assert bytes(dig) == b"".join(d for d, _ in want)
    assert np.array_equal(n, np.array([v for _, v in want], dtype=np.uint32))
    # k == 0: fine, nothing to write
    dig, n = dev.prime_inputs_batch([], [])
    assert dig.shape == (0, 32) and n.shape == (0,)


@pytest.mark.parametrize("case_", list(PV.sum_cases()), ids=lambda c: c[0])
def test_prime_rho_sums_equal_python_integers(dev, case_):
    name, pairs, rhos, live = case_
    got = dev.prime_rho_sums([x for x, _ in pairs], [j for _, j in pairs], S.rho_rows(rhos), live)
    assert got == PV.sums_want(name, pairs, rhos, live)


def test_prime_rho_sums_across_a_launch_boundary(dev):
    rng = random.Random(8)
    pairs = PV.pairs_of(BIG, seed=1)
    rhos = [S.RHO_EDGES[i % len(S.RHO_EDGES)] if i % 3 else rng.randrange(1, 1 << 128) for i in range(BIG)]
    live = (np.arange(BIG) % 5 != 2).astype(np.uint8)
    live[-1] = 1
    got = dev.prime_rho_sums([x for x, _ in pairs], [j for _, j in pairs], S.rho_rows(rhos), live)
    assert got == PV.py_sums_large(pairs, rhos, live)
    assert dev.prime_rho_sums([], [], np.zeros((0, 2), dtype=np.uint64)) == [0] * 260      # k == 0: nothing written


# ------------------------------------------------------------------------------------------------ real proofs
@pytest.fixture(scope="module")
def proved(dev):
    """one template key and the 8 proofs of PROVED from prove_prime_batch -> dict(key, pvk (extended, prepared), proofs, inf, g0)"""
    from zksnark_finalproject_amd import handlers
    from zksnark_finalproject_amd.device import pvk_prepare
    from zksnark_finalproject_amd.circuits import prime_search
    for x, j in PROVED:
        assert prime_search(x, 64)["j"] == j
    rng = random.Random(0x9121)
    key = handlers.prime_template_key(dev, rng)
    try:
        rs, ss = handlers._draw_rs_batch(rng, len(PROVED))
        xs, js = zip(*PROVED)
        proofs, inf, g0, _, _ = dev.prove_prime_batch(key["ph"], key["rh"], key["corr"], key["vk"]["gamma_abc_g1"][0], xs, js, rs, ss)
    finally:
        dev.pk_free(key["ph"])
        dev.r1cs_free(key["rh"])
    return dict(key=key, pvk=pvk_prepare(key["ext_vk"]), proofs=proofs, inf=inf, g0=g0)


def _tampered(proved):
    """negatives at 0, 3 and 7: (x, j + 1), (x + 1, j - 1), C dropped -> (claims, proofs, inf, the verdicts)"""
    claims = list(PROVED)
    proofs, inf = proved["proofs"].copy(), proved["inf"].copy()
    claims[0] = (PROVED[0][0], PROVED[0][1] + 1)
    x3, j3 = PROVED[3]
    claims[3] = (x3 + 1, j3 - 1)
    assert PV.py_digest(*claims[3]) == PV.py_digest(x3, j3)
    proofs[7, 36:48] = 0
    inf[7, 2] = 1
    want = np.ones(len(PROVED), dtype=bool)
    want[[0, 3, 7]] = False
    return claims, proofs, inf, want


def _wire(proofs, inf):
    return VB.to_wire(VB.Batch(None, None, proofs, inf))


def test_real_proofs_verify_under_the_one_extended_key(dev, proved):
    from zksnark_finalproject_amd import handlers, wire
    from zksnark_finalproject_amd.circuits import prime_ext_inputs, prime_public_inputs
    from zksnark_finalproject_amd.device import pvk_prepare, verify_prepared
    pvk, proofs, inf = proved["pvk"], proved["proofs"], proved["inf"]
    xs, js = zip(*PROVED)
    tvk = proved["key"]["vk"]
    for i, (x, j) in enumerate(PROVED):
        own = pvk_prepare(dict(tvk, gamma_abc_g1=np.concatenate([proved["g0"][i:i + 1], tvk["gamma_abc_g1"][1:]])))
        assert verify_prepared(own, prime_public_inputs(x, j), proofs[i], inf[i]), (x, j)
        assert verify_prepared(pvk, prime_ext_inputs(x, j), proofs[i], inf[i]), (x, j)
    rho = VB.draw_rho(random.Random(1), len(PROVED))
    ok, each = dev.verify_prime_batch(pvk, xs, js, proofs, inf, rho=rho, each=True)
    assert ok is True and each.all()
    tm = dev.verify_batch_timings(prime=True)
    assert tm["prime_inputs_ms"] > 0 and tm["prime_sums_ms"] > 0 and tm["host_form"] == 0
    assert list(tm)[:11] == list(dev.verify_batch_timings()) and len(tm) == 13
    ok, each = dev.verify_prime_batch_wire(pvk, xs, js, _wire(proofs, inf), each=True)          # rho from `secrets`
    assert ok is True and each.all()
    tm = dev.verify_batch_timings(prime=True)
    assert tm["prime_inputs_ms"] > 0 and tm["prime_sums_ms"] > 0 and tm["host_form"] == 0 and tm["decode_ms"] > 0
    requests = [(x, j, wire.encode_proof(proofs[i], inf[i])) for i, (x, j) in enumerate(PROVED)]
    out = handlers.verify_primes(proved["key"]["ext_vk"], requests, dev=dev)
    assert out["valid"] == [True] * len(PROVED)
    assert dev.verify_batch_timings(prime=True)["prime_sums_ms"] > 0
    as_sent = base64.standard_b64encode(wire.vk_serialize_compressed(proved["key"]["ext_vk"])).decode()
    assert handlers.verify_primes(as_sent, requests, dev=dev)["valid"] == [True] * len(PROVED)
    # an ordinary call afterwards: the two prime slots are zero again
    plain = VB.Batch(pvk, np.stack([prime_ext_inputs(x, j) for x, j in PROVED]), proofs, inf)
    assert dev.verify_batch(plain.pvk, plain.pubs, plain.proofs, plain.infs, rho=rho) is True
    tm = dev.verify_batch_timings(prime=True)
    assert tm["prime_inputs_ms"] == 0 and tm["prime_sums_ms"] == 0


@pytest.mark.parametrize("after", [1, 0], ids=["each_after_1", "each_after_default"])
def test_real_proofs_with_negatives(dev, proved, after):
    """after = 1: the per-proof pass takes over after the first range test and reads the z the device expanded; the default (32):
    bisecting runs to the end on inputs the host expanded from the downloaded digests"""
    from zksnark_finalproject_amd import handlers, wire
    from zksnark_finalproject_amd.circuits import prime_ext_inputs
    from zksnark_finalproject_amd.device import verify_prepared
    pvk = proved["pvk"]
    claims, proofs, inf, want = _tampered(proved)
    per_key = np.array([verify_prepared(pvk, prime_ext_inputs(x, j), proofs[i], inf[i]) for i, (x, j) in enumerate(claims)])
    assert np.array_equal(per_key, want)
    xs, js = zip(*claims)
    rho = VB.draw_rho(random.Random(2 + after), len(claims))
    dev.set_option("verify_each_after", after)
    try:
        ok, each = dev.verify_prime_batch(pvk, xs, js, proofs, inf, rho=rho, each=True)
        tm = dev.verify_batch_timings(prime=True)
        assert ok is False and np.array_equal(each, want)
        assert tm["host_form"] == 0 and tm["prime_inputs_ms"] > 0 and tm["prime_sums_ms"] > 0
        assert (tm["each_ms"] > 0 and tm["range_tests"] == 1) if after == 1 else (tm["each_ms"] == 0 and tm["range_tests"] > 1)
        ok, each, st = dev.verify_prime_batch_wire(pvk, xs, js, _wire(proofs, inf), rho=rho, each=True, status=True)
        assert ok is False and np.array_equal(each, want) and not st.any()
        tm = dev.verify_batch_timings(prime=True)
        assert (tm["each_ms"] > 0) == (after == 1) and tm["host_form"] == 0
        requests = [(x, j, wire.encode_proof(proofs[i], inf[i])) for i, (x, j) in enumerate(claims)]
        raw = bytearray(base64.standard_b64decode(requests[5][2]))
        raw[0] &= 0x7F                              # proof 5: A is not a compressed encoding
        requests[5] = requests[5][:2] + (base64.standard_b64encode(bytes(raw)).decode(),)
        exp = [bool(w) for w in want]
        exp[5] = False
        assert handlers.verify_primes(proved["key"]["ext_vk"], requests, dev=dev)["valid"] == exp
        # the undecodable proof through the wire entry itself: its status, and the others' verdicts untouched
        by = _wire(proofs, inf)
        by[5, 0] &= 0x7F
        ok, each, st = dev.verify_prime_batch_wire(pvk, xs, js, by, rho=rho, each=True, status=True)
        assert ok is False and list(each) == exp and st[5, 0] == 1 and not np.delete(st, 5, axis=0).any()
    finally:
        dev.set_option("verify_each_after", 0)
    short = dict(proved["key"]["ext_vk"], gamma_abc_g1=proved["key"]["ext_vk"]["gamma_abc_g1"][:258])
    assert handlers.verify_primes(short, requests, dev=dev)["valid"] == [False] * len(claims)


def test_host_form_below_the_default_thresholds(dev, proved):
    """8 proofs are far below both defaults: the host form answers, with the same verdicts"""
    pvk = proved["pvk"]
    claims, proofs, inf, want = _tampered(proved)
    xs, js = zip(*claims)
    rho = VB.draw_rho(random.Random(6), len(claims))
    thresholds(dev, 0, 0)                           # 0 restores the defaults
    try:
        ok, each = dev.verify_prime_batch(pvk, xs, js, proofs, inf, rho=rho, each=True)
        tm = dev.verify_batch_timings(prime=True)
        assert ok is False and np.array_equal(each, want)
        assert tm["host_form"] == 1 and tm["prime_inputs_ms"] == 0 and tm["prime_sums_ms"] == 0
        ok, each = dev.verify_prime_batch_wire(pvk, xs, js, _wire(proofs, inf), rho=rho, each=True)
        assert ok is False and np.array_equal(each, want) and dev.verify_batch_timings()["host_form"] == 1
    finally:
        thresholds(dev, 1, 1)


def test_arguments_are_checked_before_any_work(dev, proved):
    import ctypes as C
    from zksnark_finalproject_amd.device import _verify_args
    pvk, proofs, inf = proved["pvk"], proved["proofs"], proved["inf"]
    xs, js = PV.u64s(x for x, _ in PROVED), PV.u64s(j for _, j in PROVED)
    rho = VB.draw_rho(random.Random(9), len(PROVED))
    args, k = _verify_args(pvk, "prime", (xs, js), proofs, inf, rho)
    ok, each = C.c_int(7), np.full(k, 9, dtype=np.uint8)
    call = lambda a: dev.lib.zkg16_verify_prime_batch(dev.ctx, *a, C.byref(ok), each.ctypes.data)
    by = _wire(proofs, inf)
    wire_call = lambda a, raw=by.ctypes.data: dev.lib.zkg16_verify_prime_batch_wire(dev.ctx, *a[:8], raw, a[10], a[11], C.byref(ok), each.ctypes.data, None)
    for c in (call, wire_call):
        assert c(args[:1] + (258,) + args[2:]) == 1 and c(args[:1] + (261,) + args[2:]) == 1          # not the extended key
        assert c(args[:6] + (None,) + args[7:]) == 1 and c(args[:7] + (None,) + args[8:]) == 1        # xs, js
        assert c(args[:11] + (0,)) == 1
        zero = rho.copy()
        zero[2] = 0
        assert c(args[:10] + (zero.ctypes.data,) + args[11:]) == 1
    assert wire_call(tuple(args), raw=None) == 1
    assert ok.value == 7 and (each == 9).all()
    assert call(tuple(args)) == 0 and ok.value == 1 and (each == 1).all()


# ------------------------------------------------------------------------------------------------ simulated statements
@pytest.fixture(scope="module")
def sim(oracle):
    return PV.PrimeSim(oracle, 2601)


@pytest.mark.parametrize("k", [130, 1])
def test_simulated_statements(dev, sim, k):
    """K = 130: two waves and a partial third, negatives spread over them; K = 1: a negative alone, and a valid proof alone"""
    from zksnark_finalproject_amd.device import verify_prime_batch_host
    valid = [sim.valid(x, j) for x, j in PV.sim_pairs(k, seed=k)]
    claims = sim.negatives(valid, S.spread(k))
    b, xs, js, want = sim.batch(claims)
    assert not want.all() and (k == 1 or want.any())
    rho = VB.draw_rho(random.Random(k), k)
    host = verify_prime_batch_host(b.pvk, xs, js, b.proofs, b.infs, rho=rho, each=True)
    assert host[0] is False and np.array_equal(host[1], want)
    ok, each = dev.verify_prime_batch(b.pvk, xs, js, b.proofs, b.infs, rho=rho, each=True)
    assert dev.verify_batch_timings()["host_form"] == 0
    assert ok is False and np.array_equal(each, want), [(c.name, g, w) for c, g, w in zip(claims, each, want) if g != w]
    ok, each = dev.verify_prime_batch_wire(b.pvk, xs, js, VB.to_wire(b), rho=rho, each=True)
    assert ok is False and np.array_equal(each, want)
    dev.set_option("verify_each_after", 1)
    try:
        ok, each = dev.verify_prime_batch(b.pvk, xs, js, b.proofs, b.infs, rho=rho, each=True)
    finally:
        dev.set_option("verify_each_after", 0)
    assert ok is False and np.array_equal(each, want)
    v, vx, vj, vwant = sim.batch(valid)
    assert vwant.all()
    assert dev.verify_prime_batch(v.pvk, vx, vj, v.proofs, v.infs, rho=rho) is True
    assert verify_prime_batch_host(v.pvk, vx, vj, v.proofs, v.infs, rho=rho) is True


# ------------------------------------------------------------------------------------------------ the existing entries
def test_existing_entries_answer_as_before(dev, oracle):
    """vb_decide and the per-proof pass gained a second source of inputs: an ordinary batch still gets the host form's verdicts
    through zkg16_verify_batch, zkg16_verify_batch_wire and zkg16_verify_each, bisecting and the per-proof pass both"""
    from zksnark_finalproject_amd.device import verify_batch_host
    k = 6
    base = VB.make_batch(oracle, k)
    b = VB.tamper(oracle, VB.tamper(oracle, base, "public_input", (1,)), "c_plus_g", (4,))
    want = b.loop()
    assert list(want) == [True, False, True, True, False, True]
    rho = VB.draw_rho(random.Random(5), k)
    assert verify_batch_host(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)[1].tolist() == want.tolist()
    for after in (0, 1):
        dev.set_option("verify_each_after", after)
        try:
            ok, each = dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)
            assert ok is False and np.array_equal(each, want) and dev.verify_batch_timings()["host_form"] == 0
            ok, each = dev.verify_batch_wire(b.pvk, b.pubs, VB.to_wire(b), rho=rho, each=True)
            assert ok is False and np.array_equal(each, want)
        finally:
            dev.set_option("verify_each_after", 0)
    assert np.array_equal(dev.verify_each(b.pvk, b.pubs, b.proofs, b.infs), want)
    assert dev.verify_batch(base.pvk, base.pubs, base.proofs, base.infs, rho=rho) is True
    assert len(dev.verify_batch_timings()) == 11


def test_verify_prime_batch_wire_refuses_a_payload_of_no_whole_proofs(dev):
    """bytes or a uint8 array whose length is no multiple of 192: refused before the key or (x, j) are looked at"""
    for raw in (bytes(191), np.zeros(193, dtype=np.uint8)):
        with pytest.raises(ValueError) as e:
            dev.verify_prime_batch_wire(None, None, None, raw)
        assert str(e.value) == "verify_prime_batch_wire: a compressed proof is 192 bytes"
