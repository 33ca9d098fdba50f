"""csrc/sponge_chain_dev.cuh — one Poseidon sponge chain walked by one lane, what wit_chain_batch_kernel runs — on the host
(tests/csrc/sponge_chain_host_shim.hip) against the host chains (zkg16_matrix_sponge_states_batch) and the host assignment builder, and
the host forms of the hash entries (zkg16_poseidon_hash_batch_host, zkg16_matrix_hash_batch_host, handlers.hash_matrix).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import sponge_chain_cases as SC
from zksnark_finalproject_amd import _lib
from zksnark_finalproject_amd.circuits import (matrix_hash_batch_host, matrix_sponge_states, matrix_sponge_states_batch, matrix_witness,
                                                poseidon_hash, poseidon_hash_batch_host)

NS = (2, 3, 5, 8)       # 3 and 5: n^2 odd, the last permutation absorbs one element; 8: the size the batched paths are measured at
K = 3                   # every entry 2^64 - 1, all zero, a random one
vp = C.c_void_p


@pytest.fixture(scope="module")
def shim():
    return SC.load_shim()


@pytest.fixture(scope="module")
def reference():
    """n -> (a, b, entering states [K, 3, perms, 3, 4], hashes [K, 3, 4], assignments [K]) of the host chains and the host builder:
    computed once, shared, never written to."""
    out = {}
    for n in NS:
        a, b = SC.requests(n, K)
        states, hashes = matrix_sponge_states_batch(a, b)
        zs = np.stack([matrix_witness(a[i], b[i], SC.layout(n)["total"]) for i in range(K)])
        for x in (states, hashes, zs):
            x.setflags(write=False)
        out[n] = (a, b, states, hashes, zs)
    return out


def _walk(shim, kind, use_any, elems, a, b, n, count, seg, store_words):
    """one chain in segments of `seg` permutations -> (carried states in front of every segment, hash, stored values or None)"""
    perms = (count + 1) // 2
    st = np.zeros((3, 4), dtype=np.uint64)
    out = np.full((store_words, 4), SC.SENTINEL, dtype=np.uint64) if store_words else None
    hash_ = np.zeros(4, dtype=np.uint64)
    carried = {}
    for lo in range(0, perms, seg):
        carried[lo] = st.copy()
        shim.sc_walk(kind, use_any, vp(elems.ctypes.data) if elems is not None else None, vp(a.ctypes.data), vp(b.ctypes.data), n, count, lo,
                     min(lo + seg, perms), vp(st.ctypes.data), vp(out.ctypes.data) if store_words else None, vp(hash_.ctypes.data))
    return carried, hash_, out


@pytest.mark.parametrize("seg", [1, 4, 0])              # 0: the whole chain in one call
@pytest.mark.parametrize("n", NS)
def test_lane_function_equals_host_chains(shim, reference, n, seg):
    """Every loader on every chain of every request: the state carried into a segment plus the block absorbed there is the host
    chain's entering state, the hash is the host chain's, and the stored values are the sponge segment of the host builder's z."""
    a, b, states, hashes, zs = reference[n]
    L = SC.layout(n)
    nn, perms = n * n, L["perms"]
    seg = seg or perms
    for i in range(K):
        ai, bi = np.ascontiguousarray(a[i]), np.ascontiguousarray(b[i])
        vals = SC.chain_values(ai, bi)
        for h in range(3):
            mont = SC.mont_limbs(vals[h])
            # (kind, through ChainLoadAny, elements): Montgomery Fr for all three; u64 for a and b; the product loader for c
            forms = [(0, 0, mont), (0, 1, mont)]
            forms += [(2, 0, None), (2, 1, None)] if h == 2 else [(1, 0, (ai, bi)[h].reshape(-1)), (1, 1, (ai, bi)[h].reshape(-1))]
            for kind, use_any, elems in forms:
                carried, hash_, out = _walk(shim, kind, use_any, elems, ai, bi, n, nn, seg, L["hw"])
                assert hash_.tobytes() == hashes[i, h].tobytes(), (i, h, kind, use_any)
                assert out.tobytes() == zs[i, L["off"][h]:L["off"][h] + L["hw"]].tobytes(), (i, h, kind, use_any)
                for lo, st in carried.items():
                    want = [SC.unlimbs(states[i, h, lo, j]) for j in range(3)]
                    got = [SC.unlimbs(st[j]) for j in range(3)]
                    for pos in range(2):
                        if 2 * lo + pos < nn:
                            got[1 + pos] = (got[1 + pos] + SC.unlimbs(mont[2 * lo + pos])) % SC.R_MOD
                    assert got == want, (i, h, kind, use_any, lo)
            # without the stores: the same hash, nothing written
            _, hash_, out = _walk(shim, 0, 1, mont, ai, bi, n, nn, seg, 0)
            assert out is None and hash_.tobytes() == hashes[i, h].tobytes()


def _vectors(n, k):
    rng = np.random.default_rng(40 + n)
    vals = [[int.from_bytes(rng.bytes(32), "little") % SC.R_MOD for _ in range(n)] for _ in range(k)]
    vals[0] = [SC.R_MOD - 1] * n
    if k > 1:
        vals[1] = [0] * n
    return np.stack([SC.mont_limbs(v) for v in vals])


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_poseidon_hash_batch_host(n, k, threads):
    elems = _vectors(n, k)
    out = poseidon_hash_batch_host(elems, threads=threads)
    assert out.shape == (k, 4)
    for i in range(k):
        assert out[i].tobytes() == poseidon_hash(elems[i]).tobytes(), i


@pytest.mark.parametrize("n", NS)
def test_matrix_hash_batch_host(reference, n):
    a, b, _, hashes, _ = reference[n]
    m = np.concatenate([a, b])
    for threads in (0, 1, 4):
        out = matrix_hash_batch_host(m, threads=threads)
        assert out.tobytes() == np.concatenate([hashes[:, 0], hashes[:, 1]]).tobytes()
    for i in range(K):
        assert out[i].tobytes() == matrix_sponge_states(a[i], b[i])[1][0].tobytes()


def test_handler_hash_matrix_bytes(reference):
    """handlers.hash_matrix answers the reference's OutputData: the 32 little-endian bytes of the canonical hash value."""
    from zksnark_finalproject_amd import handlers
    a, _, _, hashes, _ = reference[3]
    for i in range(K):
        res = handlers.hash_matrix(3, a[i].tolist())
        canon = SC.unlimbs(hashes[i, 0]) * pow(1 << 256, -1, SC.R_MOD) % SC.R_MOD
        assert res == {"hash": list(canon.to_bytes(32, "little"))}
    many = handlers.hash_matrices(3, [a[i] for i in range(K)])
    assert many == [handlers.hash_matrix(3, a[i]) for i in range(K)]
    with pytest.raises(ValueError):
        handlers.hash_matrices(3, [])


def test_argument_errors_leave_outputs_untouched():
    lib = _lib.load()
    elems = _vectors(3, 2)
    m, _ = SC.requests(3, 2)

    def poseidon(pe, n, k, threads, with_out=True):
        out = np.full((2, 4), SC.SENTINEL, dtype=np.uint64)
        rc = lib.zkg16_poseidon_hash_batch_host(pe, n, k, threads, out.ctypes.data if with_out else None)
        assert (out == SC.SENTINEL).all()
        return rc

    def matrix(n, pm, k, threads, with_out=True):
        out = np.full((2, 4), SC.SENTINEL, dtype=np.uint64)
        rc = lib.zkg16_matrix_hash_batch_host(n, pm, k, threads, out.ctypes.data if with_out else None)
        assert (out == SC.SENTINEL).all()
        return rc

    pe, pm = vp(elems.ctypes.data), vp(m.ctypes.data)
    assert poseidon(pe, 3, 0, 0) == 1               # k == 0: ZKG16_ERR_BAD_ARG
    assert poseidon(pe, 0, 2, 0) == 1               # n == 0
    assert poseidon(None, 3, 2, 0) == 1
    assert poseidon(pe, 3, 2, 0, with_out=False) == 1
    assert poseidon(pe, 3, 2, -1) == 1
    assert poseidon(pe, 3, (1 << 64) - 1, 0) == 1   # k vectors have no size
    assert matrix(3, pm, 0, 0) == 1
    assert matrix(0, pm, 2, 0) == 1
    assert matrix(1, pm, 2, 0) == 1                 # n outside 2..1024
    assert matrix(1025, pm, 2, 0) == 1
    assert matrix(3, None, 2, 0) == 1
    assert matrix(3, pm, 2, 0, with_out=False) == 1
    assert matrix(3, pm, 2, -1) == 1
    # and good calls fill the same buffers (threads above the cap are accepted)
    out = np.full((2, 4), SC.SENTINEL, dtype=np.uint64)
    assert lib.zkg16_poseidon_hash_batch_host(pe, 3, 2, 64, out.ctypes.data) == 0
    assert out.tobytes() == np.stack([poseidon_hash(elems[i]) for i in range(2)]).tobytes()
    assert lib.zkg16_matrix_hash_batch_host(3, pm, 2, 64, out.ctypes.data) == 0
    assert out.tobytes() == np.stack([matrix_sponge_states(m[i], m[i])[1][0] for i in range(2)]).tobytes()
