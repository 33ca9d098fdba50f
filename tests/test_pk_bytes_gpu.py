"""zkg16_pk_read / zkg16_pk_save / zkg16_pk_load_bytes and handlers.key_to_bytes / key_from_bytes: a resident proving key to and from
ark-groth16's ProvingKey::serialize_compressed bytes, encoded and decoded on the device.  The host forms (zkg16_pk_serialize_host /
zkg16_pk_deserialize_host, tests/test_pk_bytes_host.py) are the reference for every byte and every status; every comparison here is
exact, and a handle loaded from bytes has to behave as the handle zkg16_pk_load makes from the same points."""
import ctypes as C
import random

import numpy as np
import pytest

import decompress_cases as DC
import pk_bytes_cases as PB
import pyref as P
from helpers import *

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_HANDLE, UNSUPPORTED = 1, 6, 7
SENTINEL = 0x5E4711E15E4711E1
NMAX = 257
LIN_N = 5          # the linear key: m = 86, ni = 31, n_l = 55, n_h = 63 — a wave boundary falls inside every z query


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def points(oracle):
    """NMAX valid points of each group as encodings back to back, and one encoding per decoder status (computed once, never written)"""
    enc, bad = {}, {}
    for g, group in ((1, "g1"), (2, "g2")):
        _, enc[g] = DC.valid_points(oracle, group, NMAX, 90 + g)
        h = DC.hostile(group, enc[g][:PB.SIZE[g]])
        bad[g] = {1: h["not_compressed"][0], 2: h["infinity_stray_byte"][0], 3: h["x_is_q"][0], 4: h["no_point"][0], 5: h["outside_subgroup"][0]}
    return enc, bad


def _synthetic(points, n):
    """bytes laid out as a key with m = n_h = n and one instance variable, every query the first n (n - 1 for l_query) valid points:
    not a key of any circuit — zkg16_pk_load_bytes checks points, not relations — but every decode path of a key of this size"""
    enc, _ = points
    g1, g2 = enc[1], enc[2]
    out = g1[:48] + g2[:96] + g2[96:192] + g2[192:288] + (1).to_bytes(8, "little") + g1[48:96] + g1[96:144] + g1[144:192]
    for group, cnt in ((1, n), (1, n), (2, n), (1, n), (1, n - 1)):
        out += cnt.to_bytes(8, "little") + enc[group][:PB.SIZE[group] * cnt]
    return out


def _raw_load(dev, raw, validate=0, cap_abc=None):
    """zkg16_pk_load_bytes with sentinels in every output -> (status, handle variable, outputs untouched?, error text)"""
    from zksnark_finalproject_amd import wire
    b = np.frombuffer(bytes(raw), dtype=np.uint8)
    try:
        ni = wire.pk_bytes_dims(b)[0]
    except ValueError:
        ni = 4
    outs = [np.full(w, SENTINEL, dtype=np.uint64) for w in (12, 24, 24, 24, 12 * ni)]
    h = C.c_uint64(SENTINEL)
    rc = dev.lib.zkg16_pk_load_bytes(dev.ctx, b.ctypes.data, b.size, validate, C.byref(h), *[o.ctypes.data for o in outs], ni if cap_abc is None else cap_abc)
    return rc, h.value, all((o == SENTINEL).all() for o in outs), dev.lib.zkg16_last_error(dev.ctx).decode()


def _free_bytes():
    """hipMemGetInfo's free bytes, asked of the HIP runtime the library is linked to: the copy of libamdhip64 this process has mapped
    (torch brings a runtime of its own, and the second runtime to start in a process finds no device)"""
    import re
    with open("/proc/self/maps") as f:
        libs = sorted(set(re.findall(r"(/\S*libamdhip64\.so[.\d]*)", f.read())))
    assert len(libs) == 1, libs
    hip = C.CDLL(libs[0])
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _refused(dev, raw, text, validate=0):
    rc, hv, untouched, err = _raw_load(dev, raw, validate)
    assert rc == BAD_ARG and hv == SENTINEL and untouched, (rc, err)
    assert text in err, (text, err)


# ---------------------------------------------------------------------------------------------- stage level: synthetic keys
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 257])
def test_decode_and_read_at_wave_boundaries(dev, points, n):
    """every size around a wave of 64 lanes, both groups: what the device decodes and reads back is the host form's arrays, what it
    encodes again is the bytes; one bad encoding at index 0, 63, 64 and n - 1 of a G1 and of the G2 query is named with its status"""
    from zksnark_finalproject_amd import wire
    _, bad = points
    raw = _synthetic(points, n)
    want_pk, want_vk = wire.pk_deserialize_compressed(raw, validate=False)
    ph, vk = dev.pk_load_bytes(raw)
    try:
        got = dev.pk_read(ph)
        assert PB.pk_equal(got, want_pk) and got["num_instance"] == 1
        for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1"):
            assert np.array_equal(vk[k].reshape(-1), want_vk[k].reshape(-1)), k
        assert dev.pk_save(ph, vk) == raw
        assert dev.pk_check(ph)["ok"]
    finally:
        dev.pk_free(ph)
    s = PB.sections(1, n, n)
    for k, at in enumerate(sorted({0, 63, 64, n - 1})):
        if at >= n:
            continue
        st = 1 + k % 4
        for name, g in (("h_query", 1), ("b_g2_query", 2)):
            _refused(dev, PB.with_point(raw, s[name], at, bad[g][st]), "%s[%d]: status %d" % (name, at, st))


def test_three_bad_points_in_different_waves(dev, points):
    """the smallest index and ITS status, whatever order the waves finish in; an earlier field in file order wins over a smaller index"""
    _, bad = points
    n = NMAX
    raw = _synthetic(points, n)
    s = PB.sections(1, n, n)
    for name, g in (("a_query", 1), ("b_g2_query", 2)):
        t = raw
        for at, st in ((200, 1), (70, 4), (130, 3)):
            t = PB.with_point(t, s[name], at, bad[g][st])
        _refused(dev, t, "%s[70]: status 4" % name)
        _refused(dev, PB.with_point(t, s["l_query"], 2, bad[1][2]), "%s[70]: status 4" % name)
    t = PB.with_point(PB.with_point(raw, s["b_g1_query"], 5, bad[1][3]), s["a_query"], 256, bad[1][1])
    _refused(dev, t, "a_query[256]: status 1")


# ---------------------------------------------------------------------------------------------- whole keys
class Keys:
    """the linear n = 5 key and the Fibonacci-12 key: resident (setup_resident), as host arrays of the same trapdoor (zkg16_setup),
    their bytes by the host form, and assignments to prove"""

    def __init__(self, dev):
        import bench
        from zksnark_finalproject_amd import wire
        from zksnark_finalproject_amd.circuits import fibonacci_circuit, linear_r1cs_dims
        trap, g1, g2 = bench.draw_key_inputs(55)
        self.k = {}
        d = linear_r1cs_dims(LIN_N)
        rh = dev.r1cs_linear(LIN_N)
        self._add(dev, "linear", rh, d["num_instance"], d["num_instance"] + d["num_witness"], d["num_constraints"], trap, g1, g2)
        rng = random.Random(8)
        a = np.zeros((3, LIN_N, LIN_N), dtype=np.uint64)
        for r in range(3):
            for i in range(LIN_N):
                for j in range(i + 1):
                    a[r, i, j] = rng.randrange(1, 1 << 20)
        b = np.array([[rng.randrange(1 << 20) for _ in range(LIN_N)] for _ in range(3)], dtype=np.uint64)
        self.k["linear"]["wits"] = [int(h) for h in dev.witness_linear_batch(a, b)[0]]
        circ = fibonacci_circuit(3, 5, 12)
        rh = dev.r1cs_fibonacci(12)
        self._add(dev, "fibonacci", rh, circ.num_instance, circ.num_vars, circ.num_constraints, trap, g1, g2)
        self.k["fibonacci"]["wits"] = [dev.witness_load(circ.z)]
        rng = random.Random(9)
        self.rs = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(3)]).reshape(3, 4)
        self.ss = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(3)]).reshape(3, 4)
        assert wire.pk_bytes_dims(self.k["linear"]["raw"]) == (31, 86, 63, 55)

    def _add(self, dev, name, rh, ni, nv, nc, trap, g1, g2):
        from zksnark_finalproject_amd import wire
        domain = 1 << max(nc + ni - 1, 0).bit_length()
        pk, vk = dev.setup(rh, ni, nv, domain, trap, g1, g2)
        ph, vk_r = dev.setup_resident(rh, ni, trap, g1, g2)
        raw = wire.pk_serialize_compressed(pk, vk)
        self.k[name] = dict(rh=rh, ni=ni, pk=pk, vk=vk, ph=ph, vk_r=vk_r, raw=raw)


@pytest.fixture(scope="module")
def keys(dev):
    return Keys(dev)


@pytest.mark.parametrize("name", ["linear", "fibonacci"])
def test_save_read_load_equalities(dev, keys, name):
    from zksnark_finalproject_amd import wire
    k = keys.k[name]
    assert k["pk"]["b_g1_inf"].any() and k["pk"]["b_g2_inf"].any()               # the B queries hold natural infinities
    # pk_save(setup_resident) == pk_serialize_host(zkg16_setup's arrays) for the same trapdoor
    assert dev.pk_save(k["ph"], k["vk_r"]) == k["raw"]
    tm = dev.pk_bytes_timings()
    assert tm["total_ms"] > 0 and all(tm[q] > 0 for q in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query"))
    assert PB.pk_equal(dev.pk_read(k["ph"]), k["pk"])
    # pk_read(pk_load_bytes(b)) == pk_deserialize_host(b), and pk_save(pk_load_bytes(b)) == b
    want_pk, want_vk = wire.pk_deserialize_compressed(k["raw"])
    ph, vk = dev.pk_load_bytes(k["raw"], validate=True)
    try:
        tm = dev.pk_bytes_timings()
        assert tm["check_ms"] > 0 and tm["total_ms"] >= tm["check_ms"] and all(tm[q] > 0 for q in ("a_query", "b_g2_query", "h_query"))
        assert PB.pk_equal(dev.pk_read(ph), want_pk) and PB.pk_equal(want_pk, k["pk"])
        for f in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1"):
            assert np.array_equal(vk[f].reshape(-1), np.asarray(k["vk"][f]).reshape(-1)) and np.array_equal(vk[f].reshape(-1), want_vk[f].reshape(-1)), f
        assert dev.pk_save(ph, vk) == k["raw"]
        assert dev.pk_check(ph)["ok"]
    finally:
        dev.pk_free(ph)


def _proofs(dev, keys, name, ph):
    k = keys.k[name]
    return [dev.prove_resident(ph, k["rh"], w, keys.rs[i], keys.ss[i]) for i, w in enumerate(k["wits"])]


def _same_proofs(x, y):
    return len(x) == len(y) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(x, y))


@pytest.fixture(scope="module")
def reference_proofs(dev, keys):
    """name -> proofs on a zkg16_pk_load handle of the host-decoded arrays (computed once, shared)"""
    from zksnark_finalproject_amd import wire
    out = {}
    for name, k in keys.k.items():
        ph = dev.pk_load(wire.pk_deserialize_compressed(k["raw"])[0], k["ni"])
        out[name] = _proofs(dev, keys, name, ph)
        dev.pk_free(ph)
    return out


@pytest.mark.parametrize("name", ["linear", "fibonacci"])
def test_proofs_on_a_loaded_handle_plain_batch_and_slice(dev, keys, reference_proofs, name):
    from zksnark_finalproject_amd import Zkg16Error
    k = keys.k[name]
    ph, _ = dev.pk_load_bytes(k["raw"])
    try:
        assert _same_proofs(_proofs(dev, keys, name, ph), reference_proofs[name])
        n = len(k["wits"])
        proofs, inf = dev.prove_batch(ph, k["rh"], k["wits"], keys.rs[:n], keys.ss[:n])
        assert _same_proofs([(proofs[i], inf[i]) for i in range(n)], reference_proofs[name])
        # a slice that is the whole key again: `full`, the blinding slots and l_query's placement all matter to it
        m, n_h = k["pk"]["a_query"].shape[0], k["pk"]["h_query"].shape[0]
        sh = dev.pk_slice(ph, 0, m, 0, n_h, True)
        try:
            assert _same_proofs(_proofs(dev, keys, name, sh), reference_proofs[name])
        finally:
            dev.pk_free(sh)
        part = dev.pk_slice(ph, 2, m - 1, 1, n_h, False)              # a real shard: no bytes for it
        try:
            with pytest.raises(Zkg16Error) as e:
                dev.pk_save(part, k["vk"])
            assert e.value.status == UNSUPPORTED
            with pytest.raises(Zkg16Error) as e:
                dev.pk_read(part)
            assert e.value.status == UNSUPPORTED
        finally:
            dev.pk_free(part)
    finally:
        dev.pk_free(ph)


@pytest.mark.parametrize("stride", [1, 2])
def test_window_tables_on_a_loaded_handle(dev, keys, reference_proofs, stride):
    """pk_precompute on a handle loaded from bytes: the same proofs, and level 0 of its tables at either stride saves and reads as
    the plain key does"""
    k = keys.k["linear"]
    dev.set_option("table_stride", stride)
    try:
        ph, vk = dev.pk_load_bytes(k["raw"])
        try:
            dev.pk_precompute(ph, 5, 4)
            assert dev.pk_table_bits(ph) == (5, 4)
            assert _same_proofs(_proofs(dev, keys, "linear", ph), reference_proofs["linear"])
            assert dev.pk_save(ph, vk) == k["raw"]
            assert PB.pk_equal(dev.pk_read(ph), k["pk"])
        finally:
            dev.pk_free(ph)
    finally:
        dev.set_option("table_stride", 0)


@pytest.mark.parametrize("piece", [1, 43, 64])
def test_piece_sizes(dev, keys, reference_proofs, piece):
    """one point a piece, two exact pieces of 86, one full piece and a partial one: the same bytes and the same handle"""
    from zksnark_finalproject_amd import Zkg16Error
    k = keys.k["linear"]
    dev.set_option("pk_bytes_piece", piece)
    try:
        assert dev.pk_save(k["ph"], k["vk_r"]) == k["raw"]
        assert PB.pk_equal(dev.pk_read(k["ph"]), k["pk"])
        ph, vk = dev.pk_load_bytes(k["raw"])
        try:
            assert PB.pk_equal(dev.pk_read(ph), k["pk"]) and dev.pk_save(ph, vk) == k["raw"]
            assert _same_proofs(_proofs(dev, keys, "linear", ph), reference_proofs["linear"])
        finally:
            dev.pk_free(ph)
        s = PB.sections(31, 86, 63)
        bad = DC.hostile("g1", k["raw"][s["h_query"][0]:s["h_query"][0] + 48])["no_point"][0]
        _refused(dev, PB.with_point(PB.with_point(k["raw"], s["h_query"], 62, bad), s["h_query"], 44, bad), "h_query[44]: status 4")
    finally:
        dev.set_option("pk_bytes_piece", 0)
    with pytest.raises(Zkg16Error):
        dev.set_option("pk_bytes_piece", -1)


# ---------------------------------------------------------------------------------------------- refusals
def test_tampered_byte_in_every_field(dev, keys, points):
    """one encoding replaced in each of the five queries, in gamma_abc_g1 and in each single point: the entry and its status are
    named, no handle exists, no output is written, and device memory is where it was"""
    from zksnark_finalproject_amd import wire
    _, bad = points
    k = keys.k["linear"]
    raw = k["raw"]
    s = PB.sections(31, 86, 63)
    b2_live = int(np.flatnonzero(np.asarray(k["pk"]["b_g2_inf"]) == 0)[3])
    cases = [("a_query", 64, 4), ("b_g1_query", 85, 3), ("b_g2_query", b2_live, 4), ("h_query", 62, 1), ("l_query", 54, 2), ("gamma_abc_g1", 30, 4)]
    _refused(dev, PB.with_point(raw, s["a_query"], 0, bad[1][4]), "a_query[0]: status 4")          # the ring and the cache are warm from here
    free_before = _free_bytes()
    for name, at, st in cases:
        g = 2 if s[name][1] == 96 else 1
        _refused(dev, PB.with_point(raw, s[name], at, bad[g][st]), "%s[%d]: status %d" % (name, at, st))
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "beta_g1", "delta_g1"):
        g = 2 if s[name][1] == 96 else 1
        _refused(dev, PB.with_point(raw, s[name], 0, bad[g][3]), name + ": status 3")
        _refused(dev, PB.with_point(raw, s[name], 0, bytes([0xC0]) + bytes(s[name][1] - 1)), name + ": the point at infinity")
    # a single flipped bit of an x coordinate: whatever the host form says of the bytes, the device form says, for the same entry
    flipped = bytearray(raw)
    flipped[s["l_query"][0] + 48 * 7 + 20] ^= 0x10
    try:
        wire.pk_deserialize_compressed(bytes(flipped), validate=False)
        want = None
    except ValueError as e:
        want = str(e).split("proving key: ")[1]
    rc, hv, untouched, err = _raw_load(dev, bytes(flipped))
    if want is None:
        assert rc == 0
        dev.pk_free(hv)
    else:
        assert (rc, hv, untouched, err) == (BAD_ARG, SENTINEL, True, want)
    # file order: gamma_abc_g1 lies before beta_g1
    t = PB.with_point(PB.with_point(raw, s["delta_g1"], 0, bad[1][4]), s["gamma_abc_g1"], 2, bad[1][3])
    _refused(dev, t, "gamma_abc_g1[2]: status 3")
    _refused(dev, raw[:-1], "l_query")
    _refused(dev, raw + b"\x00", "trailing")
    rc, hv, untouched, err = _raw_load(dev, raw, cap_abc=30)
    assert (rc, hv, untouched) == (BAD_ARG, SENTINEL, True) and "cap_abc" in err
    assert _free_bytes() == free_before
    ph, _ = dev.pk_load_bytes(raw)                                       # and the ctx goes on
    dev.pk_free(ph)


def test_point_outside_the_subgroup(dev, keys, points):
    """status 5 is the check's business: such a key loads without validate and pk_check names the entry; with validate, or under
    option pk_validate, it is refused before a handle exists"""
    _, bad = points
    k = keys.k["linear"]
    s = PB.sections(31, 86, 63)
    b2_live = int(np.flatnonzero(np.asarray(k["pk"]["b_g2_inf"]) == 0)[5])
    for name, at in (("h_query", 40), ("b_g2_query", b2_live), ("l_query", 54)):
        g = 2 if s[name][1] == 96 else 1
        t = PB.with_point(k["raw"], s[name], at, bad[g][5])
        ph, _ = dev.pk_load_bytes(t)
        try:
            res = dev.pk_check(ph)
            assert not res["ok"] and res["n_bad"][name] == 1 and res["first_bad"][name] == at and sum(res["n_bad"].values()) == 1
        finally:
            dev.pk_free(ph)
        _refused(dev, t, "%s[%d]" % (name, at), validate=1)
        dev.set_option("pk_validate", 1)
        try:
            _refused(dev, t, "%s[%d]" % (name, at))
        finally:
            dev.set_option("pk_validate", 0)
    t = PB.with_point(k["raw"], s["gamma_abc_g1"], 4, bad[1][5])
    ph, _ = dev.pk_load_bytes(t)
    dev.pk_free(ph)
    _refused(dev, t, "gamma_abc_g1[4]", validate=1)
    _refused(dev, PB.with_point(k["raw"], s["gamma_g2"], 0, bad[2][5]), "gamma_g2", validate=1)
    _refused(dev, PB.with_point(k["raw"], s["delta_g1"], 0, bad[1][5]), "delta_g1", validate=1)


def test_save_refusals_leave_out_untouched(dev, keys):
    k = keys.k["fibonacci"]
    out = np.full(len(k["raw"]), 0x5A, dtype=np.uint8)
    written = C.c_size_t(77)
    g2 = np.ascontiguousarray(k["vk"]["gamma_g2"], dtype=np.uint64)
    gabc = np.ascontiguousarray(k["vk"]["gamma_abc_g1"], dtype=np.uint64)
    call = lambda ph, cap, o=out.ctypes.data, g=g2.ctypes.data: dev.lib.zkg16_pk_save(dev.ctx, ph, g, gabc.ctypes.data, o, cap, C.byref(written))
    assert call(k["ph"], len(k["raw"]) - 1) == BAD_ARG
    assert call(0xDEAD, len(k["raw"])) == BAD_HANDLE
    assert call(k["ph"], len(k["raw"]), o=None) == BAD_ARG
    assert call(k["ph"], len(k["raw"]), g=None) == BAD_ARG
    assert written.value == 77 and (out == 0x5A).all()
    assert call(k["ph"], len(k["raw"])) == 0 and written.value == len(k["raw"]) and out.tobytes() == k["raw"]


# ---------------------------------------------------------------------------------------------- handlers
def test_key_to_bytes_and_back_proves_the_same(dev):
    from zksnark_finalproject_amd import handlers
    key = handlers.fibonacci_key(dev, 12, random.Random(42))
    requests = [(0, 1), (3, 5), (1 << 63, 7)]
    try:
        raw = handlers.key_to_bytes(dev, key)
        again = handlers.key_from_bytes(dev, raw, key["rh"], check_key=True)
        try:
            assert again["key_ok"] is True and again["rh"] == key["rh"] and again["ph"] != key["ph"]
            assert handlers.key_to_bytes(dev, again) == raw
            want = handlers.prove_fibonaccis(dev, requests, 12, seed=42, key=key)
            got = handlers.prove_fibonaccis(dev, requests, 12, seed=42, key=again)
            assert [r["proof"] for r in got] == [r["proof"] for r in want] and [r["vk"] for r in got] == [r["vk"] for r in want]
            claims = [(a, b, r["fib_number"]) for (a, b), r in zip(requests, got)]
            assert handlers.verify_fibonaccis(want[0]["vk"], claims, [r["proof"] for r in got])["valid"] == [True] * 3
        finally:
            dev.pk_free(again["ph"])
    finally:
        dev.pk_free(key["ph"])
        dev.r1cs_free(key["rh"])
