"""zkg16_witness_matrix_batch / zkg16_prove_matrix_batch / handlers.prove_matrices: K MatrixCircuit requests of one size in batched
device passes.  Assignment i must carry the bytes of the host builder's, proof i the bytes of zkg16_prove_resident on
zkg16_witness_matrix(a_i, b_i) — the batch changes how the work is laid out, never a result."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import pyref as P
from helpers import fr_mont

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def _num_vars(dev, n):
    nc, nw = C.c_size_t(), C.c_size_t()
    assert dev.lib.zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), None) == 0
    return 4 + nw.value


def _requests(n, k=5):
    """k <= 5 requests: every entry 2^64 - 1 (c's entries need the third limb), all zero, a random one, another, the first random
    one again."""
    rng = np.random.default_rng(200 + n)
    a = rng.integers(0, 1 << 63, size=(5, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(5, n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 63, size=(5, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(5, n, n), dtype=np.uint64)
    a[0] = b[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    a[1] = b[1] = 0
    a[4], b[4] = a[2], b[2]
    return a[:k], b[:k]


def _rs(seed, k):
    rng = random.Random(seed)
    rs = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    ss = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    return rs, ss


def _matrix_key(dev, n, seed=11):
    import bench
    rh = dev.r1cs_matrix(n)
    trap, g1, g2 = bench.draw_key_inputs(seed)
    ph, vk = dev.setup_resident(rh, 4, trap, g1, g2)
    return rh, ph, vk


@pytest.fixture(scope="module")
def expected():
    """n -> the host builder's assignments of _requests(n): computed once, shared, never written to."""
    cache = {}

    def get(dev, n):
        if n not in cache:
            from zksnark_finalproject_amd.circuits import matrix_witness
            a, b = _requests(n)
            nv = _num_vars(dev, n)
            zs = [matrix_witness(a[i], b[i], nv) for i in range(5)]
            for z in zs:
                z.setflags(write=False)
            cache[n] = (nv, zs)
        return cache[n]
    return get


# ---------------------------------------------------------------------------------------------- witness_matrix_batch
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_witness_matrix_batch_equals_host_builder(dev, expected, n, k):
    from zksnark_finalproject_amd import Zkg16Error
    nv, zs = expected(dev, n)
    a, b = _requests(n, k)
    handles, pubs, ms = dev.witness_matrix_batch(a, b)
    assert handles.shape == (k,) and pubs.shape == (k, 3, 4) and len(set(int(h) for h in handles)) == k
    assert ms["call_ms"] > 0
    for i in range(k):
        assert dev.witness_read(int(handles[i]), nv).tobytes() == zs[i].tobytes(), i
        assert np.array_equal(pubs[i], zs[i][1:4]), i
        wh, pub, _ = dev.witness_matrix(a[i], b[i])
        dev.witness_free(wh)
        assert np.array_equal(pubs[i], pub), i
    # the k assignments share one allocation: each handle is freed on its own and the others stay whole
    order = [k // 2] + [i for i in range(k) if i != k // 2]
    for j, i in enumerate(order):
        dev.witness_free(int(handles[i]))
        with pytest.raises(Zkg16Error):
            dev.witness_read(int(handles[i]), nv)
        for o in order[j + 1:]:
            assert dev.witness_read(int(handles[o]), nv).tobytes() == zs[o].tobytes(), (i, o)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_witness_matrix_batch_grid_loops(dev, expected, cap):
    """With either grid dimension capped at 1..3 both kernels loop over the requests and over their elements / permutations (the
    form a batch beyond 65,535 per dimension takes): the same bytes."""
    n, k = 5, 5
    nv, zs = expected(dev, n)
    a, b = _requests(n, k)
    dev.set_option("matrix_batch_grid", cap)
    try:
        handles, pubs, _ = dev.witness_matrix_batch(a, b)
    finally:
        dev.set_option("matrix_batch_grid", 0)
    for i in range(k):
        assert dev.witness_read(int(handles[i]), nv).tobytes() == zs[i].tobytes(), i
        dev.witness_free(int(handles[i]))


def test_witness_matrix_batch_handles_work_everywhere(dev, key3):
    """A handle of the batch in prove_resident and prove_batch, and after its neighbours were freed."""
    st = key3
    handles, _, _ = dev.witness_matrix_batch(st["a"], st["b"])
    rs, ss = st["rs"], st["ss"]
    proofs, inf = dev.prove_batch(st["ph"], st["rh"], handles, rs, ss)
    assert np.array_equal(proofs, st["ref"][0]) and np.array_equal(inf, st["ref"][1])
    for i in (0, 1, 3, 4):
        dev.witness_free(int(handles[i]))
    p, f = dev.prove_resident(st["ph"], st["rh"], int(handles[2]), rs[2], ss[2])
    assert np.array_equal(p, st["ref"][0][2]) and np.array_equal(f, st["ref"][1][2])
    dev.witness_free(int(handles[2]))


def test_witness_matrix_batch_errors_write_nothing(dev):
    from zksnark_finalproject_amd import Zkg16Error
    a, b = _requests(3, 2)
    vp = C.c_void_p

    def call(n, pa, pb, k, with_handles=True):
        handles = np.full(2, SENTINEL, dtype=np.uint64)
        pubs = np.full((2, 3, 4), SENTINEL, dtype=np.uint64)
        rc = dev.lib.zkg16_witness_matrix_batch(dev.ctx, n, pa, pb, k, handles.ctypes.data if with_handles else None, pubs.ctypes.data, None)
        assert (handles == SENTINEL).all() and (pubs == SENTINEL).all()
        return rc
    pa, pb = vp(a.ctypes.data), vp(b.ctypes.data)
    assert call(3, pa, pb, 0) == 1                  # k == 0: ZKG16_ERR_BAD_ARG
    assert call(1, pa, pb, 2) == 1
    assert call(1025, pa, pb, 2) == 1
    assert call(3, None, pb, 2) == 1
    assert call(3, pa, None, 2) == 1
    assert call(3, pa, pb, 2, with_handles=False) == 1
    assert call(3, pa, pb, (1 << 64) - 1) == 1      # k assignments have no size
    for v in (-1, 17):
        with pytest.raises(Zkg16Error):
            dev.set_option("matrix_batch_threads", v)
    handles, _, _ = dev.witness_matrix_batch(a, b)  # and the ctx still works
    for h in handles:
        dev.witness_free(int(h))


# ---------------------------------------------------------------------------------------------- prove_matrix_batch
@pytest.fixture(scope="module")
def key3(dev):
    """3x3, K = 5: a plain key and the same key with window tables; the reference proofs (witness_matrix + prove_resident on the plain
    key) and public inputs, computed once."""
    n, k = 3, 5
    a, b = _requests(n, k)
    rs, ss = _rs(3, k)
    rh, ph, vk = _matrix_key(dev, n)
    rh_tab, ph_tab, _ = _matrix_key(dev, n)            # the same draws: the same key
    dev.r1cs_free(rh_tab)
    proofs, infs, pubs = [], [], []
    for i in range(k):
        wh, pub, _ms = dev.witness_matrix(a[i], b[i])
        p, f = dev.prove_resident(ph, rh, wh, rs[i], ss[i])
        dev.witness_free(wh)
        proofs.append(p)
        infs.append(f)
        pubs.append(pub)
    ref = (np.stack(proofs), np.stack(infs))
    for x in ref:
        x.setflags(write=False)
    dev.pk_precompute(ph_tab, 0, 0)
    yield dict(n=n, k=k, a=a, b=b, rs=rs, ss=ss, rh=rh, ph=ph, ph_tab=ph_tab, vk=vk, ref=ref, pubs=np.stack(pubs))
    dev.pk_free(ph)
    dev.pk_free(ph_tab)
    dev.r1cs_free(rh)


def _check_prove(dev, st, ph):
    proofs, inf, pubs, ms = dev.prove_matrix_batch(ph, st["rh"], st["a"], st["b"], st["rs"], st["ss"])
    assert proofs.shape == (st["k"], 48) and inf.shape == (st["k"], 3)
    for i in range(st["k"]):
        assert np.array_equal(proofs[i], st["ref"][0][i]) and np.array_equal(inf[i], st["ref"][1][i]), i
    assert np.array_equal(pubs, st["pubs"])
    assert ms["call_ms"] > 0 and ms["prove_ms"] > 0
    return proofs, inf, pubs


@pytest.mark.parametrize("key", ["ph", "ph_tab"])
def test_prove_matrix_batch_equals_single_requests(dev, key3, key):
    st = key3
    _check_prove(dev, st, st[key])
    counts = dev.last_term_counts()
    assert counts[0] > 0 and counts[2] > 0
    try:
        dev.set_option("batch_max", 2)              # three sub-batches
        _check_prove(dev, st, st[key])
        assert np.array_equal(dev.last_term_counts(), counts)
        dev.set_option("batch_max", 0)
        dev.set_option("matrix_batch_threads", 1)
        _check_prove(dev, st, st[key])
    finally:
        dev.set_option("batch_max", 0)
        dev.set_option("matrix_batch_threads", 0)
    # the batch is described as zkg16_prove_batch describes it
    handles, _, _ = dev.witness_matrix_batch(st["a"], st["b"])
    dev.prove_batch(st[key], st["rh"], handles, st["rs"], st["ss"])
    assert np.array_equal(dev.last_term_counts(), counts)
    for h in handles:
        dev.witness_free(int(h))


def test_prove_matrix_batch_proofs_verify(dev, key3):
    from zksnark_finalproject_amd.device import pvk_prepare, verify_prepared
    st = key3
    proofs, inf, pubs = _check_prove(dev, st, st["ph"])
    pvk = pvk_prepare(st["vk"])
    for i in range(st["k"]):
        assert verify_prepared(pvk, pubs[i], proofs[i], inf[i]), i
        assert not verify_prepared(pvk, pubs[(i + 1) % st["k"]], proofs[i], inf[i]), i      # (no two neighbours are the same request)


def test_prove_matrix_batch_errors_write_nothing(dev, key3):
    st = key3
    k = st["k"]
    rh2 = dev.r1cs_matrix(2)
    vp = C.c_void_p
    a, b, rs, ss = st["a"], st["b"], st["rs"], st["ss"]
    ptr = lambda x: vp(x.ctypes.data)

    def call(ph, rh, n, pa, pb, kk, pr, ps, with_out=True):
        proofs = np.full((k, 48), SENTINEL, dtype=np.uint64)
        inf = np.full((k, 3), 7, dtype=np.uint8)
        pubs = np.full((k, 3, 4), SENTINEL, dtype=np.uint64)
        rc = dev.lib.zkg16_prove_matrix_batch(dev.ctx, ph, rh, n, pa, pb, kk, pr, ps, ptr(proofs) if with_out else None, ptr(inf), ptr(pubs), None)
        assert (proofs == SENTINEL).all() and (inf == 7).all() and (pubs == SENTINEL).all()
        return rc
    good = (st["ph"], st["rh"], 3, ptr(a), ptr(b), k, ptr(rs), ptr(ss))
    assert call(987654321, *good[1:]) == 6                                      # unknown pk handle: ZKG16_ERR_BAD_HANDLE
    assert call(st["ph"], 987654321, *good[2:]) == 6
    assert call(st["ph"], rh2, *good[2:]) == 1                                  # the R1CS of another size: ZKG16_ERR_BAD_ARG
    assert call(st["ph"], st["rh"], 2, *good[3:]) == 1                          # requests of another size than the handles'
    assert call(*good[:5], 0, *good[6:]) == 1                                   # k == 0
    assert call(*good[:3], None, *good[4:]) == 1
    assert call(*good[:4], None, *good[5:]) == 1
    assert call(*good[:6], None, good[7]) == 1
    assert call(*good[:7], None) == 1
    assert call(*good, with_out=False) == 1
    shard = dev.pk_slice(st["ph"], 0, 100, 0, 100, 1)
    assert call(shard, *good[1:]) == 7                                          # a shard: ZKG16_ERR_UNSUPPORTED
    dev.pk_free(shard)
    dev.r1cs_free(rh2)
    _check_prove(dev, st, st["ph"])                                             # and the ctx still proves


def test_prove_matrix_batch_two_callers(dev, key3):
    """Two threads, each a batch of K = 3 on one ctx (two lanes, each with its own staging): the proofs as when run alone."""
    st = key3
    sl = (slice(0, 3), slice(2, 5))
    out, errors = {}, []

    def worker(t):
        try:
            s = sl[t]
            for _ in range(2):
                out[t] = dev.prove_matrix_batch(st["ph"], st["rh"], st["a"][s], st["b"][s], st["rs"][s], st["ss"][s])
        except Exception as e:       # pragma: no cover - reported below
            errors.append(e)
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for t in range(2):
        proofs, inf, pubs, _ = out[t]
        assert np.array_equal(proofs, st["ref"][0][sl[t]]) and np.array_equal(inf, st["ref"][1][sl[t]])
        assert np.array_equal(pubs, st["pubs"][sl[t]])


def test_handler_prove_matrices(dev):
    """handlers.prove_matrices at size 3 with three pairs: every returned proof decodes and verifies under the returned key, and
    not with its neighbour's hashes."""
    from zksnark_finalproject_amd import handlers, wire
    a, b = _requests(3, 4)
    pairs = [(a[i], b[i]) for i in (0, 2, 3)]
    res = handlers.prove_matrices(dev, 3, pairs, seed=9)
    assert len(res["requests"]) == 3
    pubs = [[wire.decode_hash(r[h]) for h in ("hash_a", "hash_b", "hash_c")] for r in res["requests"]]
    proofs = [r["proof"] for r in res["requests"]]
    for key in (res["vk"], res["pvk"]):
        assert handlers.verify_proofs(key, pubs, proofs, dev=dev)["valid"] == [True, True, True]
    assert handlers.verify_proofs(res["pvk"], pubs[1:] + pubs[:1], proofs)["valid"] == [False, False, False]
    single = handlers.prove_matrix(dev, 3, a[0], b[0], seed=9)          # the same draws: request 0 is prove_matrix's
    assert single["proof"] == proofs[0] and single["vk"] == res["vk"]
    assert (single["hash_a"], single["hash_b"], single["hash_c"]) == tuple(res["requests"][0][h] for h in ("hash_a", "hash_b", "hash_c"))
