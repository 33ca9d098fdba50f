"""K prime requests on ONE template key (zkg16_r1cs_prime_template, zkg16_witness_prime_batch, zkg16_prove_prime_batch,
handlers.prove_primes).  The reference of every check is today's per-request path under the same trapdoor, generators, r and s:
zkg16_r1cs_prime(x, j) -> zkg16_setup_resident -> zkg16_witness_prime -> zkg16_prove_resident.  Affine points are unique, so proofs,
infinity flags and each request's gamma_abc_g1[0] must be those bytes exactly, and every other verifying-key element the template's."""
import ctypes as C
import random

import numpy as np
import pytest

from test_prime_device_host import N_ZERO, X_J0

pytestmark = pytest.mark.gpu

BAD_ARG, BAD_HANDLE, UNSUPPORTED = 1, 6, 7
# first-found primes (their circuits are satisfied, so the proofs verify): j = 0, 3, 9, 18, 4
PROVED = [(X_J0, 0), (0, 3), (12345, 9), ((1 << 64) - 1, 18), (99, 4)]
# assignments only: candidates that are not prime among them, j = 0 and j >= 1 mixed, x = 0 and 2^64 - 1
ASSIGNED = [(7, 0), (5, 1), ((1 << 64) - 1, 0), (0, 3), (12345, 3)]


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def draws():
    """one trapdoor and pair of generators, and one (r, s) per request of PROVED"""
    from zksnark_finalproject_amd.device import scalar_mul
    from zksnark_finalproject_amd.handlers import _fr_mont
    from zksnark_finalproject_amd.workloads import R_MOD, g1_generator, g2_generator
    rng = random.Random(0x9121)
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]
    rs = np.stack([_fr_mont(rng.randrange(R_MOD)) for _ in PROVED])
    ss = np.stack([_fr_mont(rng.randrange(R_MOD)) for _ in PROVED])
    return dict(trap=trap, g1=g1, g2=g2, rs=rs, ss=ss)


@pytest.fixture(scope="module")
def refs(dev, draws):
    """today's path, once per request of PROVED: (vk, proof, inf)"""
    from zksnark_finalproject_amd.circuits import prime_dims
    out = []
    for i, (x, j) in enumerate(PROVED):
        rh, wh = dev.r1cs_prime(x, j), dev.witness_prime(x, j)
        ph, vk = dev.setup_resident(rh, prime_dims(j)["num_instance"], draws["trap"], draws["g1"], draws["g2"])
        proof, inf = dev.prove_resident(ph, rh, wh, draws["rs"][i], draws["ss"][i])
        for f, h in ((dev.pk_free, ph), (dev.witness_free, wh), (dev.r1cs_free, rh)):
            f(h)
        out.append((vk, proof, inf))
    return out


def _template_key(dev, draws):
    from zksnark_finalproject_amd.circuits import prime_dims, prime_key_corrections
    rh = dev.r1cs_prime_template()
    ph, vk = dev.setup_resident(rh, prime_dims(1)["num_instance"], draws["trap"], draws["g1"], draws["g2"])
    corr, inf = prime_key_corrections(draws["trap"], draws["g1"])
    assert not inf.any()
    return dict(rh=rh, ph=ph, vk=vk, corr=corr)


@pytest.fixture(scope="module")
def key(dev, draws):
    k = _template_key(dev, draws)
    yield k
    dev.pk_free(k["ph"])
    dev.r1cs_free(k["rh"])


@pytest.fixture(scope="module")
def assigned(dev):
    """zkg16_witness_prime read back, once per candidate of ASSIGNED"""
    from zksnark_finalproject_amd.circuits import prime_dims
    nv = prime_dims(1)["num_instance"] + prime_dims(1)["num_witness"]
    out = []
    for x, j in ASSIGNED:
        wh = dev.witness_prime(x, j)
        out.append(dev.witness_read(wh, nv))
        dev.witness_free(wh)
    return nv, out


def test_template_handle_holds_the_host_template(dev, key):
    from zksnark_finalproject_amd.circuits import prime_r1cs_template_host
    want, nw, _ = prime_r1cs_template_host()
    got, nv = dev.r1cs_read(key["rh"])
    assert nv == want["num_inputs"] + nw and got["num_inputs"] == want["num_inputs"] and got["num_constraints"] == want["num_constraints"]
    for m in "abc":
        for g, w in zip(got[m], want[m]):
            assert g.shape == w.shape and np.array_equal(g, w), m


def test_witness_batch_equals_single_assignments_and_frees_in_any_order(dev, assigned):
    nv, want = assigned
    xs, js = zip(*ASSIGNED[:3])
    assert 0 in js and max(js) >= 1
    hs = dev.witness_prime_batch(xs, js)
    assert len(set(int(h) for h in hs)) == 3
    for i in range(3):
        assert np.array_equal(dev.witness_read(int(hs[i]), nv), want[i]), ASSIGNED[i]
    dev.witness_free(int(hs[1]))                # the three share one allocation: the others stay whole
    assert np.array_equal(dev.witness_read(int(hs[2]), nv), want[2])
    dev.witness_free(int(hs[2]))
    assert np.array_equal(dev.witness_read(int(hs[0]), nv), want[0])
    dev.witness_free(int(hs[0]))


@pytest.mark.parametrize("grid", [1, 2])
def test_witness_batch_grid_loops(dev, assigned, grid):
    nv, want = assigned
    xs, js = zip(*ASSIGNED)
    dev.set_option("matrix_batch_grid", grid)       # both kernels loop over requests (and the expand kernel over z) beyond the cap
    try:
        hs = dev.witness_prime_batch(xs, js)
    finally:
        dev.set_option("matrix_batch_grid", 0)
    try:
        for i in range(len(ASSIGNED)):
            assert np.array_equal(dev.witness_read(int(hs[i]), nv), want[i]), (grid, ASSIGNED[i])
    finally:
        for h in hs[::-1]:
            dev.witness_free(int(h))


def test_witness_batch_refuses_all_or_nothing(dev):
    xs = np.array([ASSIGNED[0][0], N_ZERO[0][0], ASSIGNED[1][0]], dtype=np.uint64)
    js = np.array([ASSIGNED[0][1], N_ZERO[0][1], ASSIGNED[1][1]], dtype=np.uint64)
    before = dev.witness_prime(*ASSIGNED[0])
    dev.witness_free(before)
    hs = np.full(3, 0xA5A5A5A5, dtype=np.uint64)
    assert dev.lib.zkg16_witness_prime_batch(dev.ctx, xs.ctypes.data, js.ctypes.data, 3, hs.ctypes.data) == UNSUPPORTED
    assert (hs == 0xA5A5A5A5).all()
    after = dev.witness_prime(*ASSIGNED[0])      # handles are numbered in order: the refused call took none
    dev.witness_free(after)
    assert after == before + 1
    assert dev.lib.zkg16_witness_prime_batch(dev.ctx, xs.ctypes.data, js.ctypes.data, 0, hs.ctypes.data) == BAD_ARG
    assert dev.lib.zkg16_witness_prime_batch(dev.ctx, None, js.ctypes.data, 3, hs.ctypes.data) == BAD_ARG


def _prove(dev, key, draws, idx):
    xs, js = zip(*[PROVED[i] for i in idx])
    return dev.prove_prime_batch(key["ph"], key["rh"], key["corr"], key["vk"]["gamma_abc_g1"][0], xs, js, draws["rs"][idx], draws["ss"][idx])


def _check_equal(refs, idx, proofs, inf, g0):
    for n, i in enumerate(idx):
        vk, proof, finf = refs[i]
        assert np.array_equal(proofs[n], proof), PROVED[i]
        assert np.array_equal(inf[n], finf), PROVED[i]
        assert np.array_equal(g0[n], vk["gamma_abc_g1"][0]), PROVED[i]


@pytest.mark.parametrize("k", [1, 3])
def test_prove_batch_equals_the_per_request_path(dev, key, draws, refs, k):
    from zksnark_finalproject_amd.circuits import prime_public_inputs
    from zksnark_finalproject_amd.device import verify
    idx = list(range(k)) if k > 1 else [1]
    js = [PROVED[i][1] for i in idx]
    assert k == 1 or (0 in js and max(js) >= 1)
    proofs, inf, g0, pubs, ms = _prove(dev, key, draws, idx)
    _check_equal(refs, idx, proofs, inf, g0)
    assert ms["call_ms"] > 0
    tvk = key["vk"]
    for n, i in enumerate(idx):
        vk = refs[i][0]
        for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):       # the rest of the request's key is the template's
            assert np.array_equal(np.asarray(vk[name]), np.asarray(tvk[name])), name
        assert np.array_equal(vk["gamma_abc_g1"][1:], tvk["gamma_abc_g1"][1:])
        assert not np.array_equal(vk["gamma_abc_g1"][0], tvk["gamma_abc_g1"][0])
        assert np.array_equal(pubs[n], prime_public_inputs(*PROVED[i]))
        own = dict(tvk, gamma_abc_g1=np.concatenate([g0[n:n + 1], tvk["gamma_abc_g1"][1:]]))
        assert verify(own, pubs[n], proofs[n], inf[n])
        other = refs[(i + 1) % len(PROVED)][0]["gamma_abc_g1"][0]
        assert not np.array_equal(other, g0[n])
        wrong = dict(tvk, gamma_abc_g1=np.concatenate([other[None, :], tvk["gamma_abc_g1"][1:]]))
        assert not verify(wrong, pubs[n], proofs[n], inf[n])


@pytest.mark.parametrize("variant", ["three_passes", "seven_transforms", "window_tables"])
def test_prove_batch_of_five(dev, key, draws, refs, variant):
    idx = list(range(len(PROVED)))
    mine = None
    try:
        if variant == "three_passes":
            dev.set_option("batch_max", 2)              # sub-batches of 2, 2 and 1 (the last through the one-vector witness map)
        elif variant == "seven_transforms":
            dev.set_option("wm_transforms", 7)
        else:
            mine = _template_key(dev, draws)            # the tables change the key in place: on a key of its own
            assert dev.pk_precompute(mine["ph"]) > 0
        proofs, inf, g0, _, _ = _prove(dev, mine or key, draws, idx)
    finally:
        dev.set_option("batch_max", 0)
        dev.set_option("wm_transforms", 6)
        if mine:
            dev.pk_free(mine["ph"])
            dev.r1cs_free(mine["rh"])
    _check_equal(refs, idx, proofs, inf, g0)


def test_prove_batch_checks_before_any_work_and_writes_nothing(dev, key, draws):
    from zksnark_finalproject_amd.circuits import prime_dims
    k = 3
    xs = np.array([PROVED[i][0] for i in range(k)], dtype=np.uint64)
    js = np.array([PROVED[i][1] for i in range(k)], dtype=np.uint64)
    rs, ss = np.ascontiguousarray(draws["rs"][:k]), np.ascontiguousarray(draws["ss"][:k])
    corr, g0t = np.ascontiguousarray(key["corr"]).reshape(-1), np.ascontiguousarray(key["vk"]["gamma_abc_g1"][0])
    pat = 0x5A
    outs = dict(proofs=np.full((k, 48), pat, np.uint64), inf=np.full((k, 3), pat, np.uint8), g0=np.full((k, 12), pat, np.uint64),
                pub=np.full((k, 257, 4), pat, np.uint64), ms=np.full(4, 7.0, np.float32))

    def call(ph, rh, xs=xs, js=js, kk=k, corr=corr):
        return dev.lib.zkg16_prove_prime_batch(dev.ctx, ph, rh, None if corr is None else corr.ctypes.data, g0t.ctypes.data, xs.ctypes.data,
                                               js.ctypes.data, kk, rs.ctypes.data, ss.ctypes.data, outs["proofs"].ctypes.data, outs["inf"].ctypes.data,
                                               outs["g0"].ctypes.data, outs["pub"].ctypes.data, outs["ms"].ctypes.data)
    none = 0xFFFFFFF0
    plain = dev.r1cs_prime(*PROVED[1])                  # same shape, same bytes but four coefficients: not the template
    small = dev.r1cs_matrix(2)
    trap, g1, g2 = draws["trap"], draws["g1"], draws["g2"]
    small_ph, _ = dev.setup_resident(small, 4, trap, g1, g2)
    nv = prime_dims(1)["num_instance"] + prime_dims(1)["num_witness"]
    shard = dev.pk_slice(key["ph"], 0, nv // 2, 0, 16, True)
    try:
        assert call(none, key["rh"]) == BAD_HANDLE
        assert call(key["ph"], none) == BAD_HANDLE
        assert call(none, plain) == BAD_HANDLE                  # handles before anything else
        assert call(shard, plain) == UNSUPPORTED                # a shard before any shape
        assert call(shard, key["rh"]) == UNSUPPORTED
        assert call(key["ph"], plain) == BAD_ARG                # an ordinary r1cs_prime handle
        assert call(small_ph, key["rh"]) == BAD_ARG             # a key of another circuit
        assert call(key["ph"], key["rh"], kk=0) == BAD_ARG
        assert call(key["ph"], key["rh"], corr=None) == BAD_ARG
        bad_x, bad_j = xs.copy(), js.copy()
        bad_x[k - 1], bad_j[k - 1] = N_ZERO[1]
        assert call(key["ph"], key["rh"], xs=bad_x, js=bad_j) == UNSUPPORTED      # a refused candidate, last in the batch
        assert call(key["ph"], plain, xs=bad_x, js=bad_j) == BAD_ARG                # ... is looked at after the handles' shapes
    finally:
        dev.pk_free(shard)
        dev.pk_free(small_ph)
        dev.r1cs_free(small)
        dev.r1cs_free(plain)
    for name, a in outs.items():
        assert (a == (7.0 if name == "ms" else pat)).all(), name
    assert call(key["ph"], key["rh"]) == 0                      # and the same buffers are filled by a good call
    assert not (outs["proofs"] == pat).all() and (outs["inf"] != pat).all() and not (outs["pub"] == pat).all()


def test_prove_primes_handler(dev):
    from zksnark_finalproject_amd import handlers
    from zksnark_finalproject_amd.circuits import prime_search
    missing = next(x for x in range(1, 64) if not prime_search(x, 0)["found"])
    requests = [(12345, 32), (missing, 0), (X_J0, 32), (99, 32)]
    single = handlers.prove_prime(dev, 12345, 32, seed=3)
    out = handlers.prove_primes(dev, requests, seed=3)
    assert len(out) == len(requests)
    for name in ("proof", "vk", "pvk", "j", "num_constraints", "num_variables", "prime_num", "found_prime"):
        assert out[0][name] == single[name], name
    assert out[1] == handlers.prove_prime(dev, missing, 0, seed=3) and out[1]["found_prime"] is False
    js = [o["j"] for q, o in enumerate(out) if q != 1]
    assert 0 in js and max(js) >= 1
    for q, (x, _) in enumerate(requests):
        if q == 1:
            continue
        o = out[q]
        assert o["found_prime"] and o["j"] == prime_search(x, 32)["j"]
        assert handlers.verify_prime(o["pvk"], x, o["j"], o["proof"])["valid"] is True
        assert handlers.verify_prime(o["vk"], x, o["j"], o["proof"])["valid"] is True
        assert handlers.verify_prime(o["pvk"], x + 1, o["j"], o["proof"])["valid"] is False
    assert out[2]["vk"] != out[0]["vk"] and out[2]["proof"] != out[0]["proof"]
    # a key the caller keeps: the same proofs, and the key is still there afterwards
    rng = random.Random(3)
    mine = handlers.prime_template_key(dev, rng)
    try:
        again = handlers.prove_primes(dev, requests, seed=3, key=mine)
        got, _ = dev.r1cs_read(mine["rh"])
        assert got["num_constraints"] == out[0]["num_constraints"]
    finally:
        dev.pk_free(mine["ph"])
        dev.r1cs_free(mine["rh"])
    assert [o["found_prime"] for o in again] == [o["found_prime"] for o in out]
    assert again[0]["vk"] == out[0]["vk"]                      # the same trapdoor: the same key
