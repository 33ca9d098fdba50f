"""Proof re-randomisation on the device (csrc/verify_batch.hip: rerandomize_g1_kernel, rerandomize_g2_kernel, compress_kernel; arithmetic
csrc/rerandomize_dev.cuh): every byte against the host form zkg16_rerandomize_batch_host, which tests/test_rerandomize_host.py holds
against big-integer expectations; the wire form against the host decoders and encoder; verify_each on the results; the refusals.
The cases are tests/rerandomize_cases.py's.  A call's cost is flat in k up to one wave per SIMD, so small k is enough."""
import numpy as np
import pytest

import decompress_cases as DC
import rerandomize_cases as RC
import verify_batch_cases as VB
from helpers import *

pytestmark = pytest.mark.gpu

R = RC.R
FILL = 0x5A
KS = (None, 1, 63, 64, 65, 130)          # the whole table, then wave and block edges (padded with ordinary statements)


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    d.set_option("rerandomize_min", 1)          # every call of this module runs the kernels unless it says otherwise
    d.set_option("verify_batch_min", 1)
    yield d
    d.close()


_HOST = {}


def host_form(oracle, k):
    """(table, the host form's proofs and flags for it), computed once per k and shared"""
    from zksnark_finalproject_amd import device
    if k not in _HOST:
        t = RC.table(oracle, k)
        out, inf = device.rerandomize_batch_host(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
        assert np.array_equal(out, t.want) and np.array_equal(inf, t.want_inf)          # the host form is the expected points
        _HOST[k] = (t, out, inf)
    return _HOST[k]


def compress_proofs(proofs, infs):
    return VB.to_wire(VB.Batch(None, np.zeros((proofs.shape[0], 0, 4), np.uint64), proofs, infs))


# ------------------------------------------------------------------------------------------------ limbs
@pytest.mark.parametrize("k", KS)
def test_device_equals_host_form(dev, oracle, k):
    t, want, want_inf = host_form(oracle, k)
    out, inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
    tm = dev.rerandomize_timings()
    assert tm["host_form"] == 0 and tm["g1_ms"] > 0 and tm["g2_ms"] > 0 and tm["total_ms"] > 0
    assert out.tobytes() == want.tobytes()
    assert np.array_equal(inf, want_inf)
    if k is None:
        # no flags at all: the points at infinity of the table are zero limbs
        out, inf = dev.rerandomize_batch(t.key.vk, t.batch.proofs, None, t.r1, t.r2)
        assert out.tobytes() == want.tobytes() and np.array_equal(inf, want_inf)


def test_three_passes_equal_one(dev, oracle):
    t, want, want_inf = host_form(oracle, 130)
    dev.set_option("rerandomize_pass", 64)
    try:
        out, inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
        raw, st = dev.rerandomize_batch_wire(t.delta, VB.to_wire(t.batch), t.r1, t.r2)
    finally:
        dev.set_option("rerandomize_pass", 0)
    assert out.tobytes() == want.tobytes() and np.array_equal(inf, want_inf)
    assert not st.any() and raw.tobytes() == compress_proofs(want, want_inf).tobytes()
    for bad in (-1, 65537):
        with pytest.raises(Exception):
            dev.set_option("rerandomize_pass", bad)


def test_below_the_threshold_the_host_form_answers(dev, oracle):
    t, want, want_inf = host_form(oracle, 65)
    dev.set_option("rerandomize_min", 66)
    try:
        out, inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
        tm = dev.rerandomize_timings()
        assert tm["host_form"] == 1 and tm["g1_ms"] == 0 and tm["g2_ms"] == 0 and tm["total_ms"] > 0
        raw, st = dev.rerandomize_batch_wire(t.delta, VB.to_wire(t.batch), t.r1, t.r2)
        assert dev.rerandomize_timings()["host_form"] == 1
        dev.set_option("rerandomize_min", 65)
        again, _ = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
        assert dev.rerandomize_timings()["host_form"] == 0
    finally:
        dev.set_option("rerandomize_min", 1)
    assert out.tobytes() == want.tobytes() == again.tobytes() and np.array_equal(inf, want_inf)
    assert not st.any() and raw.tobytes() == compress_proofs(want, want_inf).tobytes()


# ------------------------------------------------------------------------------------------------ wire
def test_wire_form_equals_host_compress_of_the_host_form(dev, oracle):
    for k in (None, 65):
        t, want, want_inf = host_form(oracle, k)
        raw, st = dev.rerandomize_batch_wire(t.delta, VB.to_wire(t.batch), t.r1, t.r2)
        tm = dev.rerandomize_timings()
        assert tm["host_form"] == 0 and tm["decode_ms"] > 0 and tm["compress_ms"] > 0
        assert not st.any()
        assert raw.tobytes() == compress_proofs(want, want_inf).tobytes()
        # the flag of a point at infinity travels as 0xC0 and zeros
        i = [c.name for c in t.cases].index("b_prime_infinity")
        assert raw[i, 48] == 0xC0 and not raw[i, 49:144].any()


def test_wire_form_bad_points_leave_the_other_proofs_alone(dev, oracle):
    t, want, want_inf = host_form(oracle, 65)
    k = t.k
    good = VB.to_wire(t.batch)
    clean = compress_proofs(want, want_inf)
    where = (0, k // 2, k - 1)
    assert where[1] not in (0, k - 1)
    lib = dev.lib
    for group, lo in (("g1", 0), ("g2", 48), ("g1", 144)):
        size = DC.SIZE[group]
        bad = DC.hostile(group, good[1, lo:lo + size].tobytes())
        for name in ("not_compressed", "no_point", "outside_subgroup"):
            enc, status = bad[name]
            # what the validating host decoder says of this encoding
            assert DC.host_decode(group, enc, True)[2][0] == status and status == {"not_compressed": 1, "no_point": 4, "outside_subgroup": 5}[name]
            sent = good.copy()
            for i in where:
                sent[i, lo:lo + size] = np.frombuffer(enc, dtype=np.uint8)
            raw, st = dev.rerandomize_batch_wire(t.delta, sent, t.r1, t.r2)
            w_st = np.zeros((k, 3), dtype=np.uint8)
            w_raw = clean.copy()
            for i in where:
                w_st[i, {0: 0, 48: 1, 144: 2}[lo]] = status
                w_raw[i] = 0
            assert np.array_equal(st, w_st), (group, lo, name)
            assert raw.tobytes() == w_raw.tobytes(), (group, lo, name)
            if lo == 144:
                continue
            # status null with a failed proof: BAD_ARG; with none: OK
            out = np.zeros((k, 192), dtype=np.uint8)
            assert lib.zkg16_rerandomize_batch_wire(dev.ctx, t.delta.ctypes.data, sent.ctypes.data, t.r1.ctypes.data, t.r2.ctypes.data, k, out.ctypes.data, None) == 1, name
    out = np.zeros((k, 192), dtype=np.uint8)
    assert lib.zkg16_rerandomize_batch_wire(dev.ctx, t.delta.ctypes.data, good.ctypes.data, t.r1.ctypes.data, t.r2.ctypes.data, k, out.ctypes.data, None) == 0
    assert out.tobytes() == clean.tobytes()


# ------------------------------------------------------------------------------------------------ the compress stage
@pytest.mark.parametrize("n", [1, 64, 65, 0])
def test_points_compress_batch_equals_the_host(dev, oracle, n):
    from zksnark_finalproject_amd import wire
    t, _, _ = host_form(oracle, None)
    g1, g1_inf, g2, g2_inf = RC.points_of(t)
    s1, s2 = RC.sign_rule_points()
    for group, pts, inf in (("g1", np.concatenate([g1, s1]), np.concatenate([g1_inf, np.zeros(len(s1), np.uint8)])),
                            ("g2", np.concatenate([g2, s2]), np.concatenate([g2_inf, np.zeros(len(s2), np.uint8)]))):
        # the synthetic limbs first, then the cases' points from the last (the points at infinity) back, cut to n
        ns = len(s1) if group == "g1" else len(s2)
        order = np.concatenate([np.arange(len(pts) - ns, len(pts)), np.arange(len(pts) - ns)[::-1]])
        pick = np.resize(order, n) if n else order[:0]
        p, f = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(inf[pick])
        assert dev.points_compress_batch(group, p, f) == wire.points_compress(group, p, f)
        if n == 65:
            assert f.any()
            assert dev.points_compress_batch(group, p) == wire.points_compress(group, p)          # no flags: the limbs as they are


# ------------------------------------------------------------------------------------------------ chained on the device
def test_verify_each_gives_the_original_verdicts(dev, oracle):
    t, _, _ = host_form(oracle, 65)
    assert t.verdicts.any() and not t.verdicts.all()
    out, inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
    assert np.array_equal(dev.verify_each(t.batch.pvk, t.batch.pubs, out, inf), t.verdicts)


def test_twice_equals_once_with_the_composed_pair(dev, oracle):
    import random
    t, _, _ = host_form(oracle, None)
    rng = random.Random(7400)
    s1 = [RC.S.wide(rng) for _ in range(t.k)]
    s2 = [RC.S.wide(rng) for _ in range(t.k)]
    t1, t2 = [], []
    d = t.key.delta
    for c, u1, u2 in zip(t.cases, s1, s2):
        # the logs after the second step, from the logs after the first
        a2, b2, c2 = c.a * pow(u1, -1, R) % R, (u1 * c.b + u1 * u2 * d) % R, (c.c + u2 * c.a) % R
        v1, v2 = c.r1 * u1 % R, (c.r2 + u2 * pow(c.r1, -1, R)) % R
        once = RC.Case(t.key, c.name + "_composed", c.stmt, v1, v2) if v2 else None
        assert once is not None and (once.a, once.b, once.c) == (a2, b2, c2), c.name
        t1.append(v1)
        t2.append(v2)
    mont = lambda vs: np.array([fr_mont(v) for v in vs], dtype=np.uint64).reshape(-1, 4)
    first, first_inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
    twice, twice_inf = dev.rerandomize_batch(t.delta, first, first_inf, mont(s1), mont(s2))
    once, once_inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, mont(t1), mont(t2))
    assert twice.tobytes() == once.tobytes() and np.array_equal(twice_inf, once_inf)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(dev, oracle):
    t, want, want_inf = host_form(oracle, 65)
    lib = dev.lib
    out, inf = dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
    before = dev.rerandomize_timings()
    assert before["host_form"] == 0 and before["g2_ms"] > 0
    sent = VB.to_wire(t.batch)
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
        assert lib.zkg16_rerandomize_batch(dev.ctx, p["delta"], p["proofs"], p["inf"], p["r1"], p["r2"], k, p["out"], p["out_inf"]) == 1, name
        assert text.encode() in lib.zkg16_last_error(dev.ctx), (name, lib.zkg16_last_error(dev.ctx))
        assert (a["out"] == FILL).all() and (a["out_inf"] == FILL).all(), name
        # the wire form: the bytes in the place of the limbs, the byte output in the place of both outputs
        if what == "null" and at in ("out_inf",):
            continue
        raw = np.full((t.k, 192), FILL, dtype=np.uint8)
        st = np.full((t.k, 3), FILL, dtype=np.uint8)
        bytes_p = None if what == "null" and at == "proofs" else sent.ctypes.data
        raw_p = None if what == "null" and at == "out" else raw.ctypes.data
        assert lib.zkg16_rerandomize_batch_wire(dev.ctx, p["delta"], bytes_p, p["r1"], p["r2"], k, raw_p, st.ctypes.data) == 1, name
        assert text.encode() in lib.zkg16_last_error(dev.ctx), name
        assert (raw == FILL).all() and (st == FILL).all(), name
        assert dev.rerandomize_timings() == before, name          # no kernel ran: the entries are the last good call's
    assert lib.zkg16_rerandomize_batch(None, t.delta.ctypes.data, t.batch.proofs.ctypes.data, None, t.r1.ctypes.data, t.r2.ctypes.data, t.k, out.ctypes.data,
                                       inf.ctypes.data) == 1
    assert lib.zkg16_rerandomize_timings(dev.ctx, None, 8) == 1


def test_handler_device_route(dev, oracle):
    import base64
    from zksnark_finalproject_amd import device, handlers, wire
    t, _, _ = host_form(oracle, None)
    n = 6
    b64 = [wire.encode_proof(t.batch.proofs[i], t.batch.infs[i]) for i in range(n)]
    raw = base64.standard_b64decode(b64[1])
    outside = DC.hostile("g2", raw[48:144])["outside_subgroup"][0]
    sent = b64[:3] + [base64.standard_b64encode(raw[:48] + outside + raw[144:]).decode(), base64.standard_b64encode(raw[:191]).decode()] + b64[3:]
    src = [0, 1, 2, None, None, 3, 4, 5]
    got = handlers.rerandomize_proofs(t.key.vk, sent, dev=dev)
    for g, s, i in zip(got, sent, src):
        if i is None:
            assert g == ""
            continue
        assert g and g != s
        proof, inf = wire.decode_proof(g)
        assert device.verify_prepared(t.batch.pvk, t.batch.pubs[i], proof, inf) == bool(t.verdicts[i])
