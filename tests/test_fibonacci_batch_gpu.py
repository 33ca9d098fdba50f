"""zkg16_r1cs_fibonacci / zkg16_witness_fibonacci_batch / zkg16_prove_fibonacci_batch / handlers.prove_fibonaccis: K Fibonacci requests
of one round count under one key in batched device passes.  Assignment i must carry the bytes the host mirror exports for (a_i, b_i),
proof i the bytes of zkg16_prove_resident on that request's own zkg16_circuit_load handles — the batch changes how the work is laid
out, never a result."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as P
from helpers import fr_mont

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5
U64_MAX = (1 << 64) - 1
KMAX = 65           # one wave of the assignment kernel, and one lane past it


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def _requests(k=KMAX):
    """k <= 65 requests: the corners of the u64 range first, then random 64-bit pairs; the last one (lane 64) has both maxima again."""
    rng = random.Random(404)
    pairs = [(U64_MAX, U64_MAX), (0, 0), (0, 1), (U64_MAX, 0), (0, U64_MAX), (1, 1)]
    pairs += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(KMAX - len(pairs) - 1)]
    pairs.append((U64_MAX, U64_MAX - 1))
    a = np.array([p[0] for p in pairs], dtype=np.uint64)
    b = np.array([p[1] for p in pairs], dtype=np.uint64)
    return a[:k], b[:k]


def _rs(seed, k):
    rng = random.Random(seed)
    rs = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    ss = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    return rs, ss


@pytest.fixture(scope="module")
def expected():
    """steps -> the host mirror's exported assignments [65, 5, 4] of _requests(): computed once, shared, never written to."""
    cache = {}

    def get(steps):
        if steps not in cache:
            from zksnark_finalproject_amd.circuits import fibonacci_circuit
            a, b = _requests()
            zs = np.stack([fibonacci_circuit(int(a[i]), int(b[i]), steps).z for i in range(KMAX)])
            assert zs.shape == (KMAX, 5, 4)
            zs.setflags(write=False)
            cache[steps] = zs
        return cache[steps]
    return get


# ---------------------------------------------------------------------------------------------- r1cs_fibonacci
@pytest.mark.parametrize("steps", [0, 1, 12, 1000])
def test_r1cs_fibonacci_equals_host_export(dev, steps):
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    rh = dev.r1cs_fibonacci(steps)
    got, nv = dev.r1cs_read(rh)
    dev.r1cs_free(rh)
    want = fibonacci_circuit(U64_MAX, 7, steps)       # any request: the matrices are the round count's
    assert nv == 5 and got["num_inputs"] == 4 and got["num_constraints"] == steps + 1
    for m in "abc":
        for x, y in zip(got[m], want.r1cs[m]):
            assert x.tobytes() == y.tobytes(), m


# ---------------------------------------------------------------------------------------------- witness_fibonacci_batch
@pytest.mark.parametrize("k", [1, 3, 64, 65])
@pytest.mark.parametrize("steps", [0, 1, 12, 1000])
def test_witness_fibonacci_batch_equals_host_export(dev, expected, steps, k):
    zs = expected(steps)
    a, b = _requests(k)
    handles, pubs, ms = dev.witness_fibonacci_batch(steps, a, b)
    assert handles.shape == (k,) and pubs.shape == (k, 3, 4) and len(set(int(h) for h in handles)) == k
    assert ms["call_ms"] > 0
    for i in range(k):
        assert dev.witness_read(int(handles[i]), 5).tobytes() == zs[i].tobytes(), i
        assert pubs[i].tobytes() == zs[i][1:4].tobytes(), i
    for h in handles:
        dev.witness_free(int(h))


def test_witness_fibonacci_batch_grid_loop_and_shared_allocation(dev, expected):
    """With the grid capped at one block of 64 lanes the kernel loops over the 65 requests: the same bytes.  The k assignments share
    one allocation: each handle is freed on its own and the others stay whole."""
    from zksnark_finalproject_amd import Zkg16Error
    zs = expected(12)
    a, b = _requests()
    dev.set_option("matrix_batch_grid", 1)
    try:
        handles, _, _ = dev.witness_fibonacci_batch(12, a, b)
    finally:
        dev.set_option("matrix_batch_grid", 0)
    for i in range(KMAX):
        assert dev.witness_read(int(handles[i]), 5).tobytes() == zs[i].tobytes(), i
    for i in range(1, KMAX):
        dev.witness_free(int(handles[i]))
    with pytest.raises(Zkg16Error):
        dev.witness_read(int(handles[1]), 5)
    assert dev.witness_read(int(handles[0]), 5).tobytes() == zs[0].tobytes()
    dev.witness_free(int(handles[0]))


def test_witness_fibonacci_batch_errors_write_nothing(dev):
    a, b = _requests(2)
    vp = C.c_void_p

    def call(steps, pa, pb, k, with_handles=True):
        handles = np.full(2, SENTINEL, dtype=np.uint64)
        pubs = np.full((2, 3, 4), SENTINEL, dtype=np.uint64)
        rc = dev.lib.zkg16_witness_fibonacci_batch(dev.ctx, steps, pa, pb, k, handles.ctypes.data if with_handles else None, pubs.ctypes.data, None)
        assert (handles == SENTINEL).all() and (pubs == SENTINEL).all()
        return rc
    pa, pb = vp(a.ctypes.data), vp(b.ctypes.data)
    assert call(12, pa, pb, 0) == 1                 # k == 0: ZKG16_ERR_BAD_ARG
    assert call(12, None, pb, 2) == 1
    assert call(12, pa, None, 2) == 1
    assert call(12, pa, pb, 2, with_handles=False) == 1
    assert call(1 << 28, pa, pb, 2) == 1            # beyond ZKG16_FIBONACCI_STEPS_MAX
    assert call(12, pa, pb, (1 << 64) - 1) == 1     # k assignments have no size
    handles, _, _ = dev.witness_fibonacci_batch(12, a, b)       # and the ctx still works
    for h in handles:
        dev.witness_free(int(h))


# ---------------------------------------------------------------------------------------------- prove_fibonacci_batch
@pytest.fixture(scope="module")
def keys(dev):
    """steps -> the shared key on r1cs_fibonacci(steps) and, for all 65 requests, the reference: prove_resident on the request's own
    circuit_load handles with (rs[i], ss[i]).  Made once per round count, shared, never written to."""
    import bench
    from zksnark_finalproject_amd.circuits import fibonacci_circuit_handle
    cache = {}

    def get(steps):
        if steps not in cache:
            a, b = _requests()
            rs, ss = _rs(5 + steps, KMAX)
            rh = dev.r1cs_fibonacci(steps)
            trap, g1, g2 = bench.draw_key_inputs(11)
            ph, vk = dev.setup_resident(rh, 4, trap, g1, g2)
            proofs, infs = [], []
            for i in range(KMAX):
                rh_i, wh_i = dev.circuit_load(fibonacci_circuit_handle(int(a[i]), int(b[i]), steps))
                p, f = dev.prove_resident(ph, rh_i, wh_i, rs[i], ss[i])
                dev.witness_free(wh_i)
                dev.r1cs_free(rh_i)
                proofs.append(p)
                infs.append(f)
            ref = (np.stack(proofs), np.stack(infs))
            for x in ref:
                x.setflags(write=False)
            cache[steps] = dict(steps=steps, a=a, b=b, rs=rs, ss=ss, rh=rh, ph=ph, vk=vk, ref=ref)
        return cache[steps]
    yield get
    for st in cache.values():
        dev.pk_free(st["ph"])
        dev.r1cs_free(st["rh"])


def _check_prove(dev, st, zs, k, ph=None):
    proofs, inf, pubs, ms = dev.prove_fibonacci_batch(ph or st["ph"], st["rh"], st["steps"], st["a"][:k], st["b"][:k], st["rs"][:k], st["ss"][:k])
    assert proofs.shape == (k, 48) and inf.shape == (k, 3) and pubs.shape == (k, 3, 4)
    for i in range(k):
        assert np.array_equal(proofs[i], st["ref"][0][i]) and np.array_equal(inf[i], st["ref"][1][i]), i
        assert pubs[i].tobytes() == zs[i][1:4].tobytes(), i
    assert ms["call_ms"] > 0 and ms["prove_ms"] > 0
    return proofs, inf, pubs


@pytest.mark.parametrize("k", [1, 5, 65])
@pytest.mark.parametrize("steps", [12, 1000])
def test_prove_fibonacci_batch_equals_single_requests(dev, keys, expected, steps, k):
    from zksnark_finalproject_amd.device import pvk_prepare, verify_prepared
    st = keys(steps)
    proofs, inf, pubs = _check_prove(dev, st, expected(steps), k)
    pvk = pvk_prepare(st["vk"])
    for i in range(k):
        assert verify_prepared(pvk, pubs[i], proofs[i], inf[i]), i
    if k > 1:
        assert not verify_prepared(pvk, pubs[0], proofs[2], inf[2])         # request 2 is not request 0


@pytest.mark.parametrize("steps", [12, 1000])
def test_prove_fibonacci_batch_sub_batches(dev, keys, expected, steps):
    """Option batch_max = 2 at K = 5: sub-batches of 2, 2 and 1, identical bytes, and the batch described as zkg16_prove_batch's."""
    st = keys(steps)
    _check_prove(dev, st, expected(steps), 5)
    counts = dev.last_term_counts()
    dev.set_option("batch_max", 2)
    try:
        _check_prove(dev, st, expected(steps), 5)
        assert np.array_equal(dev.last_term_counts(), counts)
    finally:
        dev.set_option("batch_max", 0)
    handles, _, _ = dev.witness_fibonacci_batch(steps, st["a"][:5], st["b"][:5])
    proofs, inf = dev.prove_batch(st["ph"], st["rh"], handles, st["rs"][:5], st["ss"][:5])     # a handle of the batch is a witness handle
    assert np.array_equal(proofs, st["ref"][0][:5]) and np.array_equal(inf, st["ref"][1][:5])
    assert np.array_equal(dev.last_term_counts(), counts)
    for h in handles:
        dev.witness_free(int(h))


def test_prove_fibonacci_batch_on_a_tabled_key(dev, keys, expected):
    import bench
    st = keys(12)
    trap, g1, g2 = bench.draw_key_inputs(11)            # the same draws: the same key
    ph_tab, _ = dev.setup_resident(st["rh"], 4, trap, g1, g2)
    try:
        dev.pk_precompute(ph_tab, 0, 0)
        _check_prove(dev, st, expected(12), 5, ph=ph_tab)
    finally:
        dev.pk_free(ph_tab)


def test_prove_fibonacci_batch_errors_write_nothing(dev, keys, expected):
    st = keys(12)
    k = 5
    rh_other = dev.r1cs_fibonacci(13)
    vp = C.c_void_p
    a, b, rs, ss = st["a"][:k].copy(), st["b"][:k].copy(), st["rs"][:k].copy(), st["ss"][:k].copy()
    ptr = lambda x: vp(x.ctypes.data)

    def call(ph, rh, steps, pa, pb, kk, pr, ps, with_out=True):
        proofs = np.full((k, 48), SENTINEL, dtype=np.uint64)
        inf = np.full((k, 3), 7, dtype=np.uint8)
        pubs = np.full((k, 3, 4), SENTINEL, dtype=np.uint64)
        rc = dev.lib.zkg16_prove_fibonacci_batch(dev.ctx, ph, rh, steps, pa, pb, kk, pr, ps, ptr(proofs) if with_out else None, ptr(inf), ptr(pubs), None)
        assert (proofs == SENTINEL).all() and (inf == 7).all() and (pubs == SENTINEL).all()
        return rc
    good = (st["ph"], st["rh"], 12, ptr(a), ptr(b), k, ptr(rs), ptr(ss))
    assert call(*good[:5], 0, *good[6:]) == 1                                   # k == 0: ZKG16_ERR_BAD_ARG
    assert call(*good[:3], None, *good[4:]) == 1                                # null pointers
    assert call(*good[:4], None, *good[5:]) == 1
    assert call(*good[:6], None, good[7]) == 1
    assert call(*good[:7], None) == 1
    assert call(*good, with_out=False) == 1
    assert call(987654321, *good[1:]) == 6                                      # unknown handles: ZKG16_ERR_BAD_HANDLE
    assert call(st["ph"], 987654321, *good[2:]) == 6
    assert call(st["ph"], rh_other, 12, *good[3:]) == 1                         # the R1CS of another round count
    assert call(st["ph"], st["rh"], 13, *good[3:]) == 1                         # requests of another round count than the handle's
    assert call(st["ph"], st["rh"], 1 << 28, *good[3:]) == 1
    shard = dev.pk_slice(st["ph"], 0, 3, 0, 8, 1)
    assert call(shard, *good[1:]) == 7                                          # a shard: ZKG16_ERR_UNSUPPORTED
    dev.pk_free(shard)
    dev.r1cs_free(rh_other)
    _check_prove(dev, st, expected(12), k)                                      # and the ctx still proves


# ---------------------------------------------------------------------------------------------- handlers
def test_handlers_prove_and_verify_fibonaccis(dev):
    from zksnark_finalproject_amd import handlers
    requests = [(0, 1), (U64_MAX, U64_MAX), (3, 5), (123456789, 987654321)]
    recs = handlers.prove_fibonaccis(dev, requests, 12, seed=42)
    assert len(recs) == 4 and all("satisfied" not in r for r in recs)
    single = handlers.prove_fibonacci(dev, 0, 1, 12, seed=42)          # the same draws: request 0 is prove_fibonacci's
    assert recs[0]["proof"] == single["proof"] and recs[0]["pvk"] == single["pvk"] and recs[0]["fib_number"] == single["fib_number"]
    assert recs[0]["vk"] == single["vk"]
    assert {k for k in recs[0] if not k.startswith("_")} == {k for k in single if not k.startswith("_")}
    claims = [(a, b, r["fib_number"]) for (a, b), r in zip(requests, recs)]
    proofs = [r["proof"] for r in recs]
    for key in (recs[0]["vk"], recs[0]["pvk"]):
        assert handlers.verify_fibonaccis(key, claims, proofs, dev=dev)["valid"] == [True] * 4
    assert handlers.verify_fibonaccis(recs[0]["pvk"], claims, proofs)["valid"] == [True] * 4       # and without a device
    wrong = list(claims)
    wrong[2] = (3, 5, recs[1]["fib_number"])
    assert handlers.verify_fibonaccis(recs[0]["pvk"], wrong, proofs, dev=dev)["valid"] == [True, True, False, True]
    assert handlers.verify_fibonaccis(recs[0]["pvk"], wrong, proofs)["valid"] == [True, True, False, True]
    checked = handlers.prove_fibonaccis(dev, requests, 12, seed=42, check_on_device=True)
    assert [r["satisfied"] for r in checked] == [True] * 4
    assert [r["proof"] for r in checked] == proofs
    # a key kept by the caller serves a second batch and stays live
    key = handlers.fibonacci_key(dev, 12, random.Random(42))
    try:
        again = handlers.prove_fibonaccis(dev, requests[:2], 12, seed=1, key=key)
        assert again[0]["vk"] == recs[0]["vk"]
        assert handlers.verify_fibonaccis(again[0]["pvk"], claims[:2], [r["proof"] for r in again], dev=dev)["valid"] == [True, True]
    finally:
        dev.pk_free(key["ph"])
        dev.r1cs_free(key["rh"])
