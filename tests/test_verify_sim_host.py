"""The verifiers on simulated statements (tests/sim_proofs.py): full-width public inputs, num_instance 1 to 257, entries of
gamma_abc_g1 at infinity, and valid proofs with A, B, C or the prepared input X at infinity, each with negative twins.  The
by-construction verdict is checked against the pure-Python pairing on a few statements, and then decides for the host verifiers
(zkg16_verify_prepared, zkg16_verify_batch_host, handlers.verify_proofs) and for the per-proof device header compiled for the CPU
with its value-bound assertions live (tests/csrc/verify_each_host_shim.hip).  No GPU."""
import random

import numpy as np
import pytest

import pyref as P
import sim_proofs as S
import verify_batch_cases as VB
from helpers import *
from test_verify_each_host import load_each_shim, verify_one

K = 20          # every edge value of S.EDGES meets the first input once


@pytest.fixture(scope="module")
def shim():
    return load_each_shim()


@pytest.fixture(scope="module")
def degenerate(oracle):
    return S.degenerate_batches(oracle)


@pytest.fixture(scope="module")
def batches(oracle, degenerate):
    """{name: (key, [Stmt], Batch, want)}: one batch per key shape with negative twins among the valid statements, and the
    degenerate batches"""
    out = {}
    for ni in (1, 2, 4, 33):
        key = S.random_key(oracle, ni, 100 + ni)
        stmts = S.with_negatives(key, S.valid_statements(key, K, 200 + ni), range(1, K, 3))
        out["ni%d" % ni] = (key, stmts) + key.batch(stmts)
    key = S.random_key(oracle, 257, 357)
    stmts = S.with_negatives(key, S.valid_statements(key, 6, 457, inputs=S.bit_inputs), (2, 3))
    out["ni257"] = (key, stmts) + key.batch(stmts)
    for name, (key, stmts) in degenerate.items():
        out["degenerate_" + name] = (key, stmts) + key.batch(stmts)
    for name, (key, stmts, b, want) in out.items():
        assert want.any() and not want.all(), name
    return out


NAMES = ["ni1", "ni2", "ni4", "ni33", "ni257", "degenerate_ni2", "degenerate_ni3", "degenerate_ni4", "degenerate_g0"]


def test_fixture_covers_what_it_says(batches):
    """the input values of the issue all occur, values >= 2^254 among them, and the degenerate families are all there"""
    for name, ni in (("ni2", 2), ("ni4", 4), ("ni33", 33)):
        seen = {v for z in S.mixed_inputs(batches[name][0], K, 200 + ni) for v in z}
        assert set(S.EDGES) <= seen and any(v >= 1 << 254 and v not in S.EDGES for v in seen), name
    names = {s.name for n in NAMES if n.startswith("degenerate") for s in batches[n][1]}
    assert {"x_zero", "x_zero_at_last_term", "infinity_mid_sum", "total_equals_term", "gamma_abc_0_zero", "gamma_abc_2_zero", "c_zero_flagged",
            "c_zero_unflagged", "a_zero", "b_zero", "c_zero_and_x_zero", "x_zero_input_changed", "c_zero_claimed"} <= names
    flips = {s.name for n in NAMES for s in batches[n][1] if s.name.startswith("flip")}
    assert flips == {"flip%d" % b for b in S.FLIP_BITS}
    assert any(s.name == "exchanged" for s in batches["ni4"][1])


# ------------------------------------------------------------------------------------------------ the fixture against Python
PY_CASES = [("ni4", "ordinary"), ("ni4", "flip130"), ("degenerate_ni2", "x_zero"), ("degenerate_ni2", "c_zero_unflagged"), ("degenerate_ni2", "a_zero"),
            ("degenerate_ni4", "gamma_abc_2_zero"), ("ni1", "ordinary"), ("degenerate_ni2", "c_zero_claimed")]


@pytest.mark.parametrize("batch,name", PY_CASES)
def test_by_construction_verdict_vs_python_pairing(batches, batch, name):
    """The limbs the fixture hands out, read back into Python points and verified by the textbook pairing (pyref_pairing): the
    verdict equals the congruence on the logs.  Independent of the product."""
    import pyref_pairing as PP
    key, stmts, b, want = batches[batch]
    i = [s.name for s in stmts].index(name)
    if name == "ordinary" and batch == "ni4":
        assert max(stmts[i].z) >= 1 << 254
    zero = lambda lo, hi: not b.proofs[i, lo:hi].any()
    vk = dict(alpha_g1=P.g1_from_limbs([int(v) for v in key.vk["alpha_g1"]]), gamma_abc_g1=[P.g1_from_limbs([int(v) for v in g], not g.any()) for g in key.vk["gamma_abc_g1"]])
    for n in ("beta_g2", "gamma_g2", "delta_g2"):
        vk[n] = P.g2_from_limbs([int(v) for v in key.vk[n]])
    proof = (P.g1_from_limbs([int(v) for v in b.proofs[i, 0:12]], zero(0, 12)), P.g2_from_limbs([int(v) for v in b.proofs[i, 12:36]], zero(12, 36)),
             P.g1_from_limbs([int(v) for v in b.proofs[i, 36:48]], zero(36, 48)))
    assert PP.groth16_verify(vk, fr_from_mont_vec(b.pubs[i]), proof) == bool(want[i]) == key.verdict(stmts[i])


# ------------------------------------------------------------------------------------------------ the host verifiers
@pytest.mark.parametrize("name", NAMES)
def test_verify_prepared(batches, name):
    key, stmts, b, want = batches[name]
    got = b.loop()
    assert np.array_equal(got, want), [(s.name, g, w) for s, g, w in zip(stmts, got, want) if g != w]


@pytest.mark.parametrize("name", NAMES)
def test_verify_batch_host(batches, name):
    from zksnark_finalproject_amd.device import verify_batch_host
    key, stmts, b, want = batches[name]
    ok, got = verify_batch_host(b.pvk, b.pubs, b.proofs, b.infs, rho=VB.draw_rho(random.Random(len(name)), b.k), each=True)
    assert ok is False and np.array_equal(got, want), [(s.name, g, w) for s, g, w in zip(stmts, got, want) if g != w]
    good = np.flatnonzero(want)
    v = VB.Batch(b.pvk, b.pubs[good], b.proofs[good], b.infs[good])
    assert verify_batch_host(v.pvk, v.pubs, v.proofs, v.infs, rho=VB.draw_rho(random.Random(5), v.k)) is True


@pytest.mark.parametrize("name", NAMES)
def test_handler_without_device(batches, name):
    """handlers.verify_proofs(dev=None): the proofs as base64 of their compressed bytes, the key as the prepared dict"""
    from zksnark_finalproject_amd import handlers, wire
    key, stmts, b, want = batches[name]
    enc = [wire.encode_proof(b.proofs[i], b.infs[i] | np.array([0, 0, not b.proofs[i, 36:48].any()], dtype=np.uint8)) for i in range(b.k)]
    out = handlers.verify_proofs(b.pvk, list(b.pubs), enc)
    assert out["valid"] == [bool(w) for w in want]


# ------------------------------------------------------------------------------------------------ the device header on the CPU
@pytest.mark.parametrize("name", NAMES)
def test_device_header_verify_one(shim, batches, name):
    """pd::verify_one behind the device header's membership tests, every bound assertion live.  The entry points hand the kernels
    flags that already say 'infinity' for all-zero limbs (zkg16_verify_each), so the shim gets them so."""
    key, stmts, b, want = batches[name]
    f = b.copy()
    f.infs[:, 2] |= (~b.proofs[:, 36:48].any(axis=1)).astype(np.uint8)
    got = np.array([verify_one(shim, f, i) for i in range(f.k)])
    assert np.array_equal(got, want), [(s.name, g, w) for s, g, w in zip(stmts, got, want) if g != w]
