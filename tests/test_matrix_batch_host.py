"""zkg16_matrix_sponge_states_batch (csrc/witness.hip): the sponge chains of K MatrixCircuit requests on a pool of host threads.
Request i's states and hashes must be byte for byte those of zkg16_matrix_sponge_states(n, a_i, b_i) — the pool changes who walks a
chain, never a chain.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from zksnark_finalproject_amd import _lib
from zksnark_finalproject_amd.circuits import matrix_sponge_states, matrix_sponge_states_batch

NS = (2, 3, 5)          # 2: two permutations per chain, the fewest; 3 and 5: n^2 odd, the last permutation absorbs one element
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _requests(n, k=7):
    """k requests: every entry 2^64 - 1 (c's entries need the third limb), all zero, two identical ones, the rest random."""
    rng = np.random.default_rng(100 + n)
    a = rng.integers(0, 1 << 63, size=(7, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(7, n, n), dtype=np.uint64)
    b = rng.integers(0, 1 << 63, size=(7, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(7, n, n), dtype=np.uint64)
    a[0] = b[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    a[1] = b[1] = 0
    a[4], b[4] = a[2], b[2]
    return a[:k], b[:k]


@pytest.fixture(scope="module")
def singles():
    """n -> (states [7, 3, perms, 3, 4], hashes [7, 3, 4]) of seven single calls: computed once, shared, never written to."""
    out = {}
    for n in NS:
        a, b = _requests(n)
        res = [matrix_sponge_states(a[i], b[i]) for i in range(7)]
        st, hs = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        st.setflags(write=False)
        hs.setflags(write=False)
        out[n] = (st, hs)
    return out


@pytest.mark.parametrize("threads", [0, 1, 2, 8])
@pytest.mark.parametrize("k", [1, 2, 7])
@pytest.mark.parametrize("n", NS)
def test_batch_equals_single_calls(singles, n, k, threads):
    a, b = _requests(n, k)
    states, hashes = matrix_sponge_states_batch(a, b, threads=threads)
    assert states.shape == (k, 3, (n * n + 1) // 2, 3, 4) and hashes.shape == (k, 3, 4)
    assert states.tobytes() == singles[n][0][:k].tobytes()
    assert hashes.tobytes() == singles[n][1][:k].tobytes()
    if k == 7:
        assert np.array_equal(hashes[2], hashes[4]) and np.array_equal(states[2], states[4])        # the two identical requests
        assert not np.array_equal(hashes[2], hashes[3])


@pytest.mark.parametrize("n", NS)
def test_hashes_without_states(singles, n):
    a, b = _requests(n)
    states, hashes = matrix_sponge_states_batch(a, b, want_states=False)
    assert states is None
    assert hashes.tobytes() == singles[n][1].tobytes()


def test_argument_errors_leave_hashes_untouched():
    lib = _lib.load()
    a, b = _requests(3, 2)
    perms = 5
    vp = C.c_void_p

    def call(n, pa, pb, k, threads, with_hashes=True):
        states = np.full((2, 3, perms, 3, 4), SENTINEL, dtype=np.uint64)
        hashes = np.full((2, 3, 4), SENTINEL, dtype=np.uint64)
        rc = lib.zkg16_matrix_sponge_states_batch(n, pa, pb, k, threads, states.ctypes.data, hashes.ctypes.data if with_hashes else None)
        assert (hashes == SENTINEL).all() and (states == SENTINEL).all()
        return rc

    pa, pb = vp(a.ctypes.data), vp(b.ctypes.data)
    assert call(1, pa, pb, 2, 0) == 1               # n below 2: ZKG16_ERR_BAD_ARG
    assert call(0, pa, pb, 2, 0) == 1
    assert call(1025, pa, pb, 2, 0) == 1            # n above 1024
    assert call(3, pa, pb, 0, 0) == 1               # k == 0
    assert call(3, None, pb, 2, 0) == 1
    assert call(3, pa, None, 2, 0) == 1
    assert call(3, pa, pb, 2, 0, with_hashes=False) == 1
    assert call(3, pa, pb, 2, -1) == 1              # a negative pool size
    # and the same buffers are filled by a good call (threads above the cap of 16 and of 3k are accepted)
    states = np.full((2, 3, perms, 3, 4), SENTINEL, dtype=np.uint64)
    hashes = np.full((2, 3, 4), SENTINEL, dtype=np.uint64)
    assert lib.zkg16_matrix_sponge_states_batch(3, pa, pb, 2, 64, states.ctypes.data, hashes.ctypes.data) == 0
    ref = [matrix_sponge_states(a[i], b[i]) for i in range(2)]
    assert states.tobytes() == np.stack([r[0] for r in ref]).tobytes() and hashes.tobytes() == np.stack([r[1] for r in ref]).tobytes()
