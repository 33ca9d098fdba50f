"""The Poseidon sponge chains of a batch walked on the device (csrc/witness.hip: wit_chain_batch_kernel, option "sponge_chains_min"):
zkg16_witness_matrix_batch / zkg16_prove_matrix_batch must give the bytes of the host-chain route, zkg16_poseidon_hash_batch /
zkg16_matrix_hash_batch the bytes of their host forms — the option changes who walks a chain, never a result."""
import ctypes as C

import numpy as np
import pytest

import sponge_chain_cases as SC
from test_matrix_batch_gpu import _matrix_key, _rs

pytestmark = pytest.mark.gpu
vp = C.c_void_p


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    d.set_option("sponge_chains_min", 1)            # every test here unless it says otherwise: always the device
    yield d
    d.close()


@pytest.fixture(scope="module")
def expected():
    """n -> the host builder's assignments of SC.requests(n): computed once, shared, never written to."""
    cache = {}

    def get(n):
        if n not in cache:
            from zksnark_finalproject_amd.circuits import matrix_witness
            a, b = SC.requests(n)
            zs = [matrix_witness(a[i], b[i], SC.layout(n)["total"]) for i in range(5)]
            for z in zs:
                z.setflags(write=False)
            cache[n] = zs
        return cache[n]
    return get


def _launches(dev):
    return dev.kernel_stats("wit_chain_batch_kernel")["launches"]


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_witness_matrix_batch_equals_host_builder(dev, expected, n, k):
    zs = expected(n)
    nv = SC.layout(n)["total"]
    a, b = SC.requests(n, k)
    handles, pubs, ms = dev.witness_matrix_batch(a, b)
    assert ms["host_sponges_ms"] == 0 and ms["call_ms"] > 0
    for i in range(k):
        assert dev.witness_read(int(handles[i]), nv).tobytes() == zs[i].tobytes(), i
        assert np.array_equal(pubs[i], zs[i][1:4]), i
        dev.witness_free(int(handles[i]))


def test_three_waves_and_a_partial_one_equal_host_route(dev):
    """n = 2, k = 67: 201 chains, hash-major — the waves that straddle the a | b and b | c boundaries hold two kinds of loader."""
    n, k = 2, 67
    nv = SC.layout(n)["total"]
    a, b = SC.many_requests(n, k)
    dev.set_option("sponge_chains_min", SC.NEVER)
    try:
        h_host, pubs_host, ms_host = dev.witness_matrix_batch(a, b)
    finally:
        dev.set_option("sponge_chains_min", 1)
    h_dev, pubs_dev, ms_dev = dev.witness_matrix_batch(a, b)
    assert ms_host["host_sponges_ms"] > 0 and ms_dev["host_sponges_ms"] == 0
    assert pubs_dev.tobytes() == pubs_host.tobytes()
    for i in range(k):
        assert dev.witness_read(int(h_dev[i]), nv).tobytes() == dev.witness_read(int(h_host[i]), nv).tobytes(), i
    for h in list(h_host) + list(h_dev):
        dev.witness_free(int(h))


@pytest.mark.parametrize("seg", [1, 4])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_grid_loops_and_carried_states(dev, expected, cap, seg):
    """The grid capped at 1..3 blocks (lanes loop over chains) and a chain walked in launches of 1 and 4 permutations (13 per
    chain at n = 5: the state is carried through device memory): the same bytes."""
    n, k = 5, 5
    zs = expected(n)
    nv = SC.layout(n)["total"]
    a, b = SC.requests(n, k)
    dev.set_option("matrix_batch_grid", cap)
    dev.set_option("sponge_chain_segment", seg)
    dev.kernel_timing(True)
    dev.kernel_stats_reset()
    try:
        handles, pubs, _ = dev.witness_matrix_batch(a, b)
        launches = _launches(dev)
    finally:
        dev.kernel_timing(False)
        dev.set_option("matrix_batch_grid", 0)
        dev.set_option("sponge_chain_segment", 0)
    assert launches == (13 + seg - 1) // seg
    for i in range(k):
        assert dev.witness_read(int(handles[i]), nv).tobytes() == zs[i].tobytes(), i
        assert np.array_equal(pubs[i], zs[i][1:4]), i
        dev.witness_free(int(handles[i]))


def test_prove_matrix_batch_equals_host_route(dev):
    from zksnark_finalproject_amd.device import pvk_prepare, verify_prepared
    n, k = 3, 3
    a, b = SC.requests(n, k)
    rs, ss = _rs(3, k)
    rh, ph, vk = _matrix_key(dev, n)
    try:
        dev.set_option("sponge_chains_min", SC.NEVER)
        try:
            ref = dev.prove_matrix_batch(ph, rh, a, b, rs, ss)
        finally:
            dev.set_option("sponge_chains_min", 1)
        proofs, inf, pubs, ms = dev.prove_matrix_batch(ph, rh, a, b, rs, ss)
        assert ref[3]["host_sponges_ms"] > 0 and ms["host_sponges_ms"] == 0
        assert np.array_equal(proofs, ref[0]) and np.array_equal(inf, ref[1]) and np.array_equal(pubs, ref[2])
        dev.set_option("batch_max", 2)              # two sub-batches, each routed on its own
        try:
            sub = dev.prove_matrix_batch(ph, rh, a, b, rs, ss)
        finally:
            dev.set_option("batch_max", 0)
        assert np.array_equal(sub[0], ref[0]) and np.array_equal(sub[2], ref[2])
        pvk = pvk_prepare(vk)
        for i in range(k):
            assert verify_prepared(pvk, pubs[i], proofs[i], inf[i]), i
    finally:
        dev.pk_free(ph)
        dev.r1cs_free(rh)


@pytest.mark.parametrize("k", [1, 67, 130])
@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_poseidon_hash_batch_equals_host_form(dev, n, k):
    from zksnark_finalproject_amd.circuits import poseidon_hash, poseidon_hash_batch_host
    rng = np.random.default_rng(50 + n)
    vals = [int.from_bytes(rng.bytes(32), "little") % SC.R_MOD for _ in range(n * k)]
    vals[:n] = [SC.R_MOD - 1] * n
    elems = SC.mont_limbs(vals).reshape(k, n, 4)
    out = dev.poseidon_hash_batch(elems)
    assert out.tobytes() == poseidon_hash_batch_host(elems).tobytes()
    assert out[k - 1].tobytes() == poseidon_hash(elems[k - 1]).tobytes()


@pytest.mark.parametrize("k", [1, 67])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_matrix_hash_batch_equals_host_form(dev, n, k):
    from zksnark_finalproject_amd import handlers
    from zksnark_finalproject_amd.circuits import matrix_hash_batch_host
    m, _ = SC.many_requests(n, k)
    out = dev.matrix_hash_batch(m)
    assert out.tobytes() == matrix_hash_batch_host(m).tobytes()
    assert handlers.hash_matrices(n, list(m[:3]), dev=dev) == handlers.hash_matrices(n, list(m[:3]))


def test_routing_by_chain_count(dev):
    """With the option at 10: 9 chains (k = 3 assignments, 9 hashes) stay on the host, 12 go to the device."""
    from zksnark_finalproject_amd.circuits import matrix_hash_batch_host
    n = 2
    nv = SC.layout(n)["total"]
    a, b = SC.many_requests(n, 12)
    dev.set_option("sponge_chains_min", 10)
    dev.kernel_timing(True)
    try:
        for k, on_device in ((3, False), (4, True)):
            dev.kernel_stats_reset()
            handles, pubs, ms = dev.witness_matrix_batch(a[:k], b[:k])
            for h in handles:
                dev.witness_free(int(h))
            if on_device:
                assert ms["host_sponges_ms"] == 0 and _launches(dev) >= 1
            else:
                assert ms["host_sponges_ms"] > 0 and _launches(dev) == 0
        for k, on_device in ((9, False), (12, True)):
            dev.kernel_stats_reset()
            out = dev.matrix_hash_batch(a[:k])
            assert out.tobytes() == matrix_hash_batch_host(a[:k]).tobytes()
            assert (_launches(dev) >= 1) == on_device
    finally:
        dev.kernel_timing(False)
        dev.set_option("sponge_chains_min", 1)


def test_argument_errors_write_nothing(dev):
    from zksnark_finalproject_amd import Zkg16Error
    a, b = SC.requests(3, 2)
    elems = SC.mont_limbs(list(range(1, 7))).reshape(2, 3, 4)
    lib = dev.lib

    def witness(n, pa, pb, k, with_handles=True):
        handles = np.full(2, SC.SENTINEL, dtype=np.uint64)
        pubs = np.full((2, 3, 4), SC.SENTINEL, dtype=np.uint64)
        rc = lib.zkg16_witness_matrix_batch(dev.ctx, n, pa, pb, k, handles.ctypes.data if with_handles else None, pubs.ctypes.data, None)
        assert (handles == SC.SENTINEL).all() and (pubs == SC.SENTINEL).all()
        return rc

    def poseidon(ctx, pe, n, k, with_out=True):
        out = np.full((2, 4), SC.SENTINEL, dtype=np.uint64)
        rc = lib.zkg16_poseidon_hash_batch(ctx, pe, n, k, out.ctypes.data if with_out else None)
        assert (out == SC.SENTINEL).all()
        return rc

    def matrix(ctx, n, pm, k, with_out=True):
        out = np.full((2, 4), SC.SENTINEL, dtype=np.uint64)
        rc = lib.zkg16_matrix_hash_batch(ctx, n, pm, k, out.ctypes.data if with_out else None)
        assert (out == SC.SENTINEL).all()
        return rc

    pa, pb, pe = vp(a.ctypes.data), vp(b.ctypes.data), vp(elems.ctypes.data)
    assert witness(3, pa, pb, 0) == 1               # ZKG16_ERR_BAD_ARG on the device route as on the host route
    assert witness(1, pa, pb, 2) == 1
    assert witness(1025, pa, pb, 2) == 1
    assert witness(3, None, pb, 2) == 1
    assert witness(3, pa, pb, 2, with_handles=False) == 1
    assert witness(3, pa, pb, (1 << 64) - 1) == 1
    assert poseidon(dev.ctx, pe, 3, 0) == 1
    assert poseidon(dev.ctx, pe, 0, 2) == 1
    assert poseidon(dev.ctx, None, 3, 2) == 1
    assert poseidon(None, pe, 3, 2) == 1
    assert poseidon(dev.ctx, pe, 3, 2, with_out=False) == 1
    assert poseidon(dev.ctx, pe, 3, (1 << 64) - 1) == 1
    assert matrix(dev.ctx, 3, pa, 0) == 1
    assert matrix(dev.ctx, 0, pa, 2) == 1
    assert matrix(dev.ctx, 1, pa, 2) == 1
    assert matrix(dev.ctx, 1025, pa, 2) == 1
    assert matrix(dev.ctx, 3, None, 2) == 1
    assert matrix(None, 3, pa, 2) == 1
    assert matrix(dev.ctx, 3, pa, 2, with_out=False) == 1
    for name, v in (("sponge_chains_min", -1), ("sponge_chain_segment", -1), ("sponge_chain_segment", 65536)):
        with pytest.raises(Zkg16Error):
            dev.set_option(name, v)
    handles, _, _ = dev.witness_matrix_batch(a, b)  # and the ctx still works
    for h in handles:
        dev.witness_free(int(h))
