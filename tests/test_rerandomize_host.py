"""Proof re-randomisation without a GPU: the device header of its kernels compiled for the host (tests/csrc/rerandomize_host_shim.hip)
and the host entry zkg16_rerandomize_batch_host against points whose logs are known (tests/rerandomize_cases.py), the compress lane
against the host encoder and the Python rules, the refusals, and the handler's host route.  Every comparison is exact."""
import base64
import ctypes as C

import numpy as np
import pytest

import pyref as P
import rerandomize_cases as RC
from helpers import *
from zksnark_finalproject_amd import _lib, device, handlers, wire

R, Q = RC.R, RC.Q
FILL = 0x5A


@pytest.fixture(scope="module")
def shim():
    return RC.load_shim()


@pytest.fixture(scope="module")
def tbl(oracle):
    return RC.table(oracle)


def ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


# ------------------------------------------------------------------------------------------------ the device header on the host
def test_case_table_holds_every_listed_case(tbl):
    names = [c.name for c in tbl.cases]
    for want in ("valid0", "r1_1", "r1_%x" % (R - 1), "r2_%x" % (2**32 - 1), "r2_%x" % 2**64, "r1_r2_product_one", "b_prime_infinity", "b_equals_delta",
                 "b_equals_minus_delta", "c_prime_infinity", "c_equals_r2_a", "a_infinity", "b_infinity", "c_infinity", "a_and_b_infinity", "c_infinity_unflagged"):
        assert want in names
    assert any(n.startswith("invalid") for n in names)
    assert tbl.verdicts.any() and not tbl.verdicts.all()
    i = names.index("c_infinity_unflagged")
    assert not tbl.batch.proofs[i, 36:].any() and not tbl.batch.infs[i, 2]          # zero limbs, no flag


def test_scalar_preparation_equals_the_integers(shim, tbl):
    out = np.zeros((4, 4), dtype=np.uint64)
    for i, c in enumerate(tbl.cases):
        shim.rr_scalars(tbl.r1[i].ctypes.data, tbl.r2[i].ctypes.data, out.ctypes.data)
        assert ints(out) == [pow(c.r1, -1, R), c.r2, c.r1, c.r1 * c.r2 % R], c.name


def test_lanes_equal_the_expected_points(shim, tbl):
    for i, c in enumerate(tbl.cases):
        out = np.full(48, FILL, dtype=np.uint64)
        inf = np.full(3, FILL, dtype=np.uint8)
        proof, fl = np.ascontiguousarray(tbl.batch.proofs[i]), np.ascontiguousarray(tbl.batch.infs[i])
        shim.rr_g1_lane(proof.ctypes.data, fl.ctypes.data, tbl.r1[i].ctypes.data, tbl.r2[i].ctypes.data, out.ctypes.data, inf.ctypes.data)
        assert np.array_equal(out[12:36], np.full(24, FILL, dtype=np.uint64)) and inf[1] == FILL, c.name          # the G1 lane leaves B' alone
        shim.rr_g2_lane(proof.ctypes.data, fl.ctypes.data, tbl.delta.ctypes.data, tbl.r1[i].ctypes.data, tbl.r2[i].ctypes.data, out.ctypes.data, inf.ctypes.data)
        assert np.array_equal(out, tbl.want[i]), c.name
        assert np.array_equal(inf, tbl.want_inf[i]), c.name


def python_compress(group, pts, inf):
    f = wire.g1_compress if group == "g1" else wire.g2_compress
    return b"".join(f(p, int(fl)) for p, fl in zip(pts, inf))


def shim_compress(shim, group, pts, inf):
    w, nb = (12, 48) if group == "g1" else (24, 96)
    pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, w)
    out = np.full(pts.shape[0] * nb, FILL, dtype=np.uint8)
    shim.rr_compress(1 if group == "g1" else 2, pts.ctypes.data, None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).ctypes.data, pts.shape[0],
                     out.ctypes.data)
    return out.tobytes()


def test_compress_lane_equals_the_host_encoder(shim, tbl):
    g1, g1_inf, g2, g2_inf = RC.points_of(tbl)
    assert g1_inf.any() and g2_inf.any() and not g1_inf.all()
    for group, pts, inf in (("g1", g1, g1_inf), ("g2", g2, g2_inf)):
        got = shim_compress(shim, group, pts, inf)
        assert got == wire.points_compress(group, pts, inf) == python_compress(group, pts, inf)
    s1, s2 = RC.sign_rule_points()
    for group, pts in (("g1", s1), ("g2", s2)):
        got = shim_compress(shim, group, pts, None)
        assert got == wire.points_compress(group, pts) == python_compress(group, pts, [0] * len(pts))
    # the rule itself, on the synthetic limbs: 0x20 exactly where y (G2: c1, then c0) is above (q - 1) / 2
    bits = [bool(shim_compress(shim, "g1", s1, None)[48 * i] & 0x20) for i in range(len(s1))]
    assert bits == [False, False, True, True] * (len(s1) // 4)
    bits = [bool(shim_compress(shim, "g2", s2, None)[96 * i] & 0x20) for i in range(len(s2))]
    assert bits == [False, True, False, True, False, False, True, True, False, True] * (len(s2) // 10)


# ------------------------------------------------------------------------------------------------ zkg16_rerandomize_batch_host
def test_host_form_equals_the_expected_points(oracle, tbl):
    for threads, t in ((1, tbl), (3, RC.table(oracle, tbl.k + 1))):
        assert threads == 1 or t.k % threads
        out, inf = device.rerandomize_batch_host(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2, threads=threads)
        assert np.array_equal(out, t.want) and np.array_equal(inf, t.want_inf)
    # a key dict in the place of the limbs, and no flags at all: the flagged points of the table are zero limbs
    out, inf = device.rerandomize_batch_host(tbl.key.vk, tbl.batch.proofs, None, tbl.r1, tbl.r2)
    assert np.array_equal(out, tbl.want) and np.array_equal(inf, tbl.want_inf)


def test_verify_prepared_agrees_after_rerandomising(tbl):
    out, inf = device.rerandomize_batch_host(tbl.delta, tbl.batch.proofs, tbl.batch.infs, tbl.r1, tbl.r2)
    names = [c.name for c in tbl.cases]
    picks = [0, 2, 3, names.index("b_prime_infinity"), names.index("c_prime_infinity"), names.index("a_and_b_infinity")]
    assert {bool(tbl.verdicts[i]) for i in picks} == {True, False}
    for i in picks:
        assert device.verify_prepared(tbl.batch.pvk, tbl.batch.pubs[i], out[i], inf[i]) == bool(tbl.verdicts[i]), names[i]
        assert device.verify_prepared(tbl.batch.pvk, tbl.batch.pubs[i], tbl.batch.proofs[i], tbl.batch.infs[i]) == bool(tbl.verdicts[i]), names[i]


def test_drawn_multipliers_give_other_proofs_with_the_same_verdicts(oracle):
    t = RC.table(oracle, 6)
    out, inf = device.rerandomize_batch_host(t.key.vk, t.batch.proofs, t.batch.infs)
    again, _ = device.rerandomize_batch_host(t.key.vk, t.batch.proofs, t.batch.infs)
    assert not np.array_equal(out, again) and not np.array_equal(out, t.batch.proofs)
    for i in range(t.k):
        assert device.verify_prepared(t.batch.pvk, t.batch.pubs[i], out[i], inf[i]) == bool(t.verdicts[i])
    r = device.draw_rerandomizers(64)
    assert all(0 < v * pow(1 << 256, -1, R) % R < R for v in ints(r)) and all(v < R for v in ints(r))


def test_host_form_refusals_leave_the_outputs_alone(oracle):
    t = RC.table(oracle, 6)
    lib = _lib.load()
    for name, (what, at, v), text in RC.refusal_calls(t):
        a = dict(delta=t.delta.copy(), proofs=t.batch.proofs.copy(), inf=t.batch.infs.copy(), r1=t.r1.copy(), r2=t.r2.copy(),
                 out=np.full((t.k, 48), FILL, dtype=np.uint64), out_inf=np.full((t.k, 3), FILL, dtype=np.uint8))
        k = t.k
        if what in ("r1", "r2"):
            a[what][at] = v
        elif what == "delta":
            a["delta"][:] = 0
        elif what == "k":
            k = 0
        p = {n: (None if what == "null" and at == n else arr.ctypes.data) for n, arr in a.items()}
        rc = lib.zkg16_rerandomize_batch_host(p["delta"], p["proofs"], p["inf"], p["r1"], p["r2"], k, 2, p["out"], p["out_inf"])
        assert rc == 1, name
        assert text.encode() in lib.zkg16_last_error(None), (name, lib.zkg16_last_error(None))
        assert (a["out"] == FILL).all() and (a["out_inf"] == FILL).all(), name
    # null flags are not a refusal
    out, oinf = np.zeros((t.k, 48), dtype=np.uint64), np.zeros((t.k, 3), dtype=np.uint8)
    assert lib.zkg16_rerandomize_batch_host(t.delta.ctypes.data, t.batch.proofs.ctypes.data, None, t.r1.ctypes.data, t.r2.ctypes.data, t.k, 0, out.ctypes.data,
                                            oinf.ctypes.data) == 0
    assert np.array_equal(out, t.want)


# ------------------------------------------------------------------------------------------------ the handler, host route
def off_curve_x():
    """the smallest x for which x^3 + 4 has no square root in Fq"""
    x = 1
    while pow((x**3 + 4) % Q, (Q - 1) // 2, Q) == 1:
        x += 1
    return x


def test_handler_round_trip_and_undecodable_proofs(oracle):
    t = RC.table(oracle, 6)
    b64 = [wire.encode_proof(t.batch.proofs[i], t.batch.infs[i]) for i in range(t.k)]
    raw = base64.standard_b64decode(b64[1])
    bad_x = bytearray(raw)
    bad_x[0:48] = off_curve_x().to_bytes(48, "big")
    bad_x[0] |= 0x80
    sent = [b64[0], base64.standard_b64encode(raw[:100]).decode(), b64[2], base64.standard_b64encode(bytes(bad_x)).decode(), b64[3], "not base64 !", b64[4]]
    src = [0, None, 2, None, 3, None, 4]
    got = handlers.rerandomize_proofs(wire.encode_vk(t.key.vk), sent)
    assert len(got) == len(sent)
    for g, s, i in zip(got, sent, src):
        if i is None:
            assert g == ""
            continue
        assert g and g != s and len(base64.standard_b64decode(g)) == 192
        proof, inf = wire.decode_proof(g)
        assert device.verify_prepared(t.batch.pvk, t.batch.pubs[i], proof, inf) == bool(t.verdicts[i])
    assert handlers.rerandomize_proofs(t.key.vk, []) == []
    with pytest.raises(KeyError):
        handlers.rerandomize_proofs({"alpha_g1": t.key.vk["alpha_g1"]}, b64[:1])          # not a decode failure: raised
