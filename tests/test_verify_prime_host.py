"""The prime form of batched verification without a GPU: the device header of its three kernels compiled for the host
(tests/csrc/prime_inputs_host_shim.hip) against hashlib and Python integers, the host entries (zkg16_prime_vk_extend,
zkg16_prime_ext_inputs, zkg16_verify_prime_batch_host) and handlers.verify_primes(dev=None) on simulated statements whose verdicts
are known by construction (tests/prime_verify_cases.py).  Every comparison is exact."""
import base64
import ctypes as C
import random

import numpy as np
import pytest

import prime_verify_cases as PV
import pyref as P
import sim_proofs as S
import verify_batch_cases as VB
from helpers import *

K = 12
WHERE = (0, 2, 4, 6, 9)          # one negative of each kind (prime_verify_cases.PrimeSim.negatives); the exchange takes 6 and 7


@pytest.fixture(scope="module")
def shim():
    return PV.load_shim()


@pytest.fixture(scope="module")
def sim(oracle):
    return PV.PrimeSim(oracle, 2601)


@pytest.fixture(scope="module")
def case(sim):
    """K = 12 requests, negatives of every kind among them -> (claims, Batch, xs, js, want)"""
    claims = sim.negatives([sim.valid(x, j) for x, j in PV.sim_pairs(K)], WHERE)
    assert {c.name for c in claims} == {"valid", "j_plus_1", "x_plus_1", "x_plus_1_j_minus_1", "exchanged", "c_dropped"}
    b, xs, js, want = sim.batch(claims)
    assert list(np.flatnonzero(~want)) == [0, 2, 4, 6, 7, 9]
    return claims, b, xs, js, want


# ------------------------------------------------------------------------------------------------ the device header on the host
def test_lane_digest_equals_hashlib_and_prime_candidate(shim):
    from zksnark_finalproject_amd.circuits import prime_candidate
    pairs = PV.EDGE_PAIRS + PV.random_pairs(200, 11)
    assert len(PV.CARRY_PAIRS) >= 3 and set(PV.CARRY_PAIRS) <= set(pairs)
    for x, j in pairs:
        dig = np.zeros(32, dtype=np.uint8)
        n = C.c_uint32(0)
        shim.pi_digest(x, j, dig.ctypes.data, C.byref(n))
        d, want_n = PV.py_digest(x, j)
        assert bytes(dig) == d and n.value == want_n, (x, j)
        cand = prime_candidate(x, j)
        assert bytes(bytearray(cand["digest"])) == d and int(cand["n"]) == want_n, (x, j)


def test_lane_public_inputs_and_scalars(shim):
    from zksnark_finalproject_amd.circuits import prime_ext_inputs, prime_public_inputs
    for x, j in PV.CARRY_PAIRS + PV.random_pairs(6, 12) + [(0, 0)]:
        out = np.zeros((257, 4), dtype=np.uint64)
        shim.pi_public_inputs(x, j, out.ctypes.data)
        assert np.array_equal(out, prime_public_inputs(x, j)), (x, j)
        want = PV.ext_ints(x, j)
        assert [shim.pi_ext_scalar(c, x, j) for c in range(259)] == want, (x, j)
        assert fr_from_mont_vec(prime_ext_inputs(x, j)) == want, (x, j)


@pytest.mark.parametrize("case_", list(PV.sum_cases()), ids=lambda c: c[0])
def test_lane_column_sums_equal_python_integers(shim, case_):
    name, pairs, rhos, live = case_
    xs, js, rho = PV.u64s(x for x, _ in pairs), PV.u64s(j for _, j in pairs), S.rho_rows(rhos)
    sums = np.full((260, 4), 0x5A, dtype=np.uint64)
    shim.pi_rho_sums(xs.ctypes.data, js.ctypes.data, rho.ctypes.data, None if live is None else live.ctypes.data, len(pairs), sums.ctypes.data)
    want = PV.sums_want(name, pairs, rhos, live)
    assert max(want) < 1 << 224
    assert PV.sums_ints(sums) == want


def test_large_batch_reference_equals_the_plain_one():
    """prime_verify_cases.py_sums_large (what the GPU test at K = 65,537 is compared with) against py_sums"""
    for name, pairs, rhos, live in PV.sum_cases((65, 257)):
        assert PV.py_sums_large(pairs, rhos, live) == PV.sums_want(name, pairs, rhos, live), name


# ------------------------------------------------------------------------------------------------ the host entries
def test_prime_vk_extend_places_v_n_and_minus_v_j(oracle):
    from zksnark_finalproject_amd import _lib
    from zksnark_finalproject_amd.circuits import prime_vk_extend
    rng = random.Random(31)
    logs = [rng.randrange(1, P.R_MOD) for _ in range(261)]
    pts, inf = oracle.fixed_base("g1", G1_GEN_LIMBS, fr_canon_vec(logs))
    assert not inf.any()
    pts = np.asarray(pts, dtype=np.uint64).reshape(261, 12)
    gabc, corr = pts[:258], pts[258:261]
    out = prime_vk_extend(gabc, corr)
    assert out.shape == (260, 12) and np.array_equal(out[:258], gabc) and np.array_equal(out[258], corr[1])
    v_j = P.g1_from_limbs([int(v) for v in corr[2]])
    assert np.array_equal(out[259], py_g1(P.ec_neg(v_j))[0])
    assert not np.array_equal(out[259], corr[2])
    # nulls and a correction at infinity: refused, nothing written
    lib = _lib.load()
    buf = np.full((260, 12), 0x5A, dtype=np.uint64)
    g, c = np.ascontiguousarray(gabc), np.ascontiguousarray(corr)
    assert lib.zkg16_prime_vk_extend(None, c.ctypes.data, buf.ctypes.data) == 1
    assert lib.zkg16_prime_vk_extend(g.ctypes.data, None, buf.ctypes.data) == 1
    assert lib.zkg16_prime_vk_extend(g.ctypes.data, c.ctypes.data, None) == 1
    for which in range(3):
        z = c.copy()
        z[which] = 0
        assert lib.zkg16_prime_vk_extend(g.ctypes.data, z.ctypes.data, buf.ctypes.data) == 1, which
    assert (buf == 0x5A).all()


def test_prime_ext_inputs_is_public_inputs_then_n_then_j():
    from zksnark_finalproject_amd.circuits import prime_candidate, prime_ext_inputs, prime_public_inputs
    for x, j in PV.EDGE_PAIRS + PV.random_pairs(10, 13):
        got = prime_ext_inputs(x, j)
        assert got.shape == (259, 4) and np.array_equal(got[:257], prime_public_inputs(x, j)), (x, j)
        assert np.array_equal(got[257], fr_mont(int(prime_candidate(x, j)["n"]))) and np.array_equal(got[258], fr_mont(j)), (x, j)


# ------------------------------------------------------------------------------------------------ verdicts on simulated statements
def test_fixture_inputs_are_the_entries(case):
    from zksnark_finalproject_amd.circuits import prime_ext_inputs
    claims, b, xs, js, want = case
    for i, c in enumerate(claims):
        assert np.array_equal(b.pubs[i], prime_ext_inputs(c.x, c.j)), c.name


def test_verdicts_under_each_requests_own_key(sim, case):
    """the identity: under the 258-point key of the (x, j) a request claims, with prime_public_inputs, zkg16_verify_prepared says what
    the extended key says"""
    from zksnark_finalproject_amd.circuits import prime_public_inputs
    from zksnark_finalproject_amd.device import verify_prepared
    claims, b, xs, js, want = case
    got = np.array([verify_prepared(sim.own_pvk(c.x, c.j), prime_public_inputs(c.x, c.j), b.proofs[i], b.infs[i]) for i, c in enumerate(claims)])
    assert np.array_equal(got, want), [(c.name, g, w) for c, g, w in zip(claims, got, want)]
    assert np.array_equal(b.loop(), want)


def test_verify_prime_batch_host(case):
    from zksnark_finalproject_amd.device import verify_batch_host, verify_prime_batch_host
    claims, b, xs, js, want = case
    rho = VB.draw_rho(random.Random(3), K)
    ok, got = verify_prime_batch_host(b.pvk, xs, js, b.proofs, b.infs, rho=rho, each=True)
    assert ok is False and np.array_equal(got, want), [(c.name, g, w) for c, g, w in zip(claims, got, want)]
    assert (ok, list(got)) == (lambda r: (r[0], list(r[1])))(verify_batch_host(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True))
    good = np.flatnonzero(want)
    assert verify_prime_batch_host(b.pvk, xs[good], js[good], b.proofs[good], b.infs[good], rho=rho[good]) is True
    assert verify_prime_batch_host(b.pvk, xs[:1], js[:1], b.proofs[:1], b.infs[:1]) is False        # K = 1, a negative


def test_verify_prime_batch_host_checks_arguments(sim, case):
    from zksnark_finalproject_amd import _lib
    from zksnark_finalproject_amd.device import _verify_args
    claims, b, xs, js, want = case
    lib = _lib.load()
    rho = VB.draw_rho(random.Random(4), K)
    args, k = _verify_args(b.pvk, "prime", (xs, js), b.proofs, b.infs, rho)
    ok, each = C.c_int(7), np.full(K, 9, dtype=np.uint8)

    def call(a):
        return lib.zkg16_verify_prime_batch_host(*a, 0, C.byref(ok), each.ctypes.data)
    assert call(args[:1] + (258,) + args[2:]) == 1                    # a key that is not the extended one
    assert call(args[:6] + (None,) + args[7:]) == 1 and call(args[:7] + (None,) + args[8:]) == 1
    assert call(args[:11] + (0,)) == 1
    zero = rho.copy()
    zero[5] = 0
    assert call(args[:10] + (zero.ctypes.data,) + args[11:]) == 1
    assert ok.value == 7 and (each == 9).all()
    assert call(tuple(args)) == 0 and ok.value == 0 and np.array_equal(each.astype(bool), want)


def _encode(b, i):
    from zksnark_finalproject_amd import wire
    return wire.encode_proof(b.proofs[i], b.infs[i] | np.array([0, 0, not b.proofs[i, 36:48].any()], dtype=np.uint8))


def test_handler_without_device(sim, case):
    from zksnark_finalproject_amd import handlers, wire
    claims, b, xs, js, want = case
    requests = [(c.x, c.j, _encode(b, i)) for i, c in enumerate(claims)]
    ext_vk = {n: sim.key.vk[n] for n in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")}
    out = handlers.verify_primes(ext_vk, requests)
    assert out["valid"] == [bool(w) for w in want] and set(out) == {"valid", "verifying_time", "decode_time"}
    # the key as it travels, and prepared
    as_sent = base64.standard_b64encode(wire.vk_serialize_compressed(ext_vk)).decode()
    assert handlers.verify_primes(as_sent, requests)["valid"] == [bool(w) for w in want]
    assert handlers.verify_primes(b.pvk, requests)["valid"] == [bool(w) for w in want]
    # one proof that does not decode: that entry only
    bad = list(requests)
    raw = bytearray(base64.standard_b64decode(requests[1][2]))
    raw[0] &= 0x7F                                                    # A: not a compressed encoding
    bad[1] = (requests[1][0], requests[1][1], base64.standard_b64encode(bytes(raw)).decode())
    bad[3] = (requests[3][0], requests[3][1], "not base64 !")
    assert want[1] and want[3]
    exp = [bool(w) for w in want]
    exp[1] = exp[3] = False
    assert handlers.verify_primes(ext_vk, bad)["valid"] == exp
    # a key with 258 points: every entry
    short = dict(ext_vk, gamma_abc_g1=ext_vk["gamma_abc_g1"][:258])
    assert handlers.verify_primes(short, requests)["valid"] == [False] * K
    assert handlers.verify_primes("AAAA", requests)["valid"] == [False] * K


def test_prime_template_key_returns_the_extended_key():
    """the handler's key dict carries ext_vk = the template vk with prime_vk_extend's points (a stand-in device: no GPU)"""
    from test_handlers_host import FakeDevice
    from zksnark_finalproject_amd import handlers, wire
    from zksnark_finalproject_amd.circuits import prime_vk_extend
    key = handlers.prime_template_key(FakeDevice(), random.Random(1))
    ext = key["ext_vk"]
    assert np.array_equal(ext["gamma_abc_g1"], prime_vk_extend(key["vk"]["gamma_abc_g1"], key["corr"])) and ext["gamma_abc_g1"].shape == (260, 12)
    for n in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert np.array_equal(ext[n], key["vk"][n])
    back = wire.vk_deserialize_compressed(wire.vk_serialize_compressed(ext))
    assert np.array_equal(np.asarray(back["gamma_abc_g1"]).reshape(-1, 12), ext["gamma_abc_g1"])
