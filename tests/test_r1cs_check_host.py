"""Satisfaction of an R1CS on the host: the lane function and the block reduction of r1cs_check_kernel compiled for the host
(tests/csrc/r1cs_check_host_shim.hip) and zkg16_r1cs_check_host, against Python integers (tests/r1cs_check_cases.py) and, for every
synthesized circuit, against zkg16_circuit_is_satisfied.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import r1cs_check_cases as K
from helpers import fr_mont

BAD_ARG = 1


@pytest.fixture(scope="module")
def shim():
    return K.load_shim()


# ------------------------------------------------------------------------------------------------ the lane
def test_lane_function_at_the_operand_bounds(shim):
    cases = K.lane_cases()
    assert len(cases) >= 5 * 36 + 6
    seen = set()
    for a, b, c, what in cases:
        la, lb, lc = (K.word_limbs([w]) for w in (a, b, c))
        want = K.row_fails_ref(a, b, c)
        got = shim.rck_row_fails(la.ctypes.data, lb.ctypes.data, lc.ctypes.data)
        assert got == int(want), (hex(a), hex(b), hex(c), what)
        seen.add((what, want))
    # the cases are what they claim: the product and its other representatives pass, every changed c fails
    assert ("c = ab", False) in seen and ("c = ab", True) not in seen
    assert ("a = 0, c = 0", False) in seen and ("c = ab + 1 r", False) in seen
    for what in ("c = ab + 1", "top limb", "top bit of the top limb", "lowest bit"):
        assert (what, True) in seen and (what, False) not in seen, what


# ------------------------------------------------------------------------------------------------ the blocks
def _walk(shim, a, b, c, stride, nc, nvec=1, order=0):
    res = np.full(2 * nvec, 0x1111111111111111, dtype=np.uint64)
    shim.rck_walk(a.ctypes.data, b.ctypes.data, c.ctypes.data, stride, nc, nvec, order, res.ctypes.data)
    return [(int(res[v]), int(res[nvec + v])) for v in range(nvec)]


@pytest.mark.parametrize("nc", K.WALK_NC)
def test_block_reduction_as_launched(shim, nc):
    for name, failing in K.walk_patterns(nc).items():
        a, b, c, stride = K.walk_vectors(nc, failing, seed=nc)
        want = (len(failing), failing[0] if failing else K.NONE)
        # the expectation is the reference's, not the pattern's say-so
        aw, bw, cw = K.words(a), K.words(b), K.words(c)
        assert K.verdict([K.row_fails_ref(aw[i], bw[i], cw[i]) for i in range(nc)]) == want, name
        for order in (0, 1):
            assert _walk(shim, a, b, c, stride, nc, order=order) == [want], (name, order)


def test_first_failing_row_when_a_later_block_reports_first(shim):
    nc = 513
    failing = K.walk_patterns(nc)["later_block_first"]
    assert failing[0] // K.BLOCK == 1 and failing[1] // K.BLOCK == 2          # two blocks, neither the first
    a, b, c, stride = K.walk_vectors(nc, failing, seed=9)
    assert _walk(shim, a, b, c, stride, nc, order=1) == [(2, failing[0])]
    assert _walk(shim, a, b, c, stride, nc, order=0) == [(2, failing[0])]


def test_block_reduction_keeps_vectors_apart(shim):
    """three vectors side by side, only the middle one failing: the words of the others stay (0, none)"""
    nc, nvec = 300, 3
    failing = [2, 255, 256, 299]
    a, b, c, stride = K.walk_vectors(nc, failing, seed=4, stride=320, nvec=nvec, which=1)
    for order in (0, 1):
        assert _walk(shim, a, b, c, stride, nc, nvec=nvec, order=order) == [(0, K.NONE), (4, 2), (0, K.NONE)]


# ------------------------------------------------------------------------------------------------ the host entry
def _agree(r1cs, z, nv):
    got = K.host_verdict(r1cs, z, nv)
    assert got == K.check_ref(r1cs, z)
    return got


@pytest.mark.parametrize("nc", [1, 65, 257, 600])
def test_host_entry_on_synth_systems(nc):
    r1cs, z, nv, rows = K.synth_system(nc, seed=100 + nc)
    assert _agree(r1cs, z, nv) == (0, K.NONE)
    z_bad, bad = K.spanning_redraw(r1cs, z, nc)
    assert _agree(r1cs, z_bad, nv) == (len(bad), bad[0])


def _circuit_agrees(circ):
    got = _agree(circ.r1cs, circ.z, circ.num_vars)
    assert circ.satisfied is not None and (got[0] == 0) == circ.satisfied
    return got


@pytest.mark.parametrize("steps", [1, 10])
def test_host_entry_on_fibonacci(steps):
    from zksnark_finalproject_amd.circuits import fibonacci_circuit
    circ = fibonacci_circuit(1, 1, steps)
    assert _circuit_agrees(circ) == (0, K.NONE)
    z, want = K.breaking_redraw(circ.r1cs, circ.z)
    assert K.host_verdict(circ.r1cs, z, circ.num_vars) == want and want[0] >= 1


@pytest.mark.parametrize("n", [2, 3])
def test_host_entry_on_matrix_circuit(n):
    from zksnark_finalproject_amd.circuits import matrix_circuit
    rng = np.random.default_rng(n)
    circ = matrix_circuit(rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64), rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64))
    assert _circuit_agrees(circ) == (0, K.NONE)
    z, want = K.breaking_redraw(circ.r1cs, circ.z)
    assert K.host_verdict(circ.r1cs, z, circ.num_vars) == want and want[0] >= 1


@pytest.fixture(scope="module")
def prime_circuits():
    from zksnark_finalproject_amd.circuits import prime_circuit
    return {c: prime_circuit(c[0], c[1], search=False, check_satisfied=True) for c in (K.PRIME_OK, K.PRIME_BAD)}


def test_host_entry_on_a_satisfied_prime_circuit(prime_circuits):
    assert _circuit_agrees(prime_circuits[K.PRIME_OK]) == (0, K.NONE)


def test_host_entry_on_the_unsatisfied_prime_candidate(prime_circuits):
    """(1040, 7) is a first-found candidate whose assignment does not satisfy the circuit (seen: 2 rows, the first 287435); the
    expectation is the Python reference's, computed here."""
    circ = prime_circuits[K.PRIME_BAD]
    want = K.check_ref(circ.r1cs, circ.z)
    assert want[0] >= 1 and want[1] < circ.num_constraints
    assert K.host_verdict(circ.r1cs, circ.z, circ.num_vars) == want
    assert circ.satisfied is False


# ------------------------------------------------------------------------------------------------ arguments
def test_host_entry_argument_checks():
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    r1cs, z, nv, _ = K.synth_system(40, seed=5)
    arrs = [[np.ascontiguousarray(r1cs[m][k]) for m in "abc"] for k in range(3)]
    pat = 0x5A5A5A5A5A5A5A5A

    def call(rp=None, col=None, cf=None, zz=z, n_bad=True, tabs=(True, True, True), nv_=nv):
        use = [rp or arrs[0], col or arrs[1], cf or arrs[2]]
        t = [(C.c_void_p * 3)(*[x.ctypes.data for x in u]) for u in use]
        nb, fb = C.c_uint64(pat), C.c_uint64(pat)
        rc = lib.zkg16_r1cs_check_host(C.byref(t[0]) if tabs[0] else None, C.byref(t[1]) if tabs[1] else None, C.byref(t[2]) if tabs[2] else None,
                                       r1cs["num_constraints"], nv_, None if zz is None else zz.ctypes.data,
                                       C.byref(nb) if n_bad else None, C.byref(fb))
        return rc, nb.value, fb.value

    assert call() == (0, 0, K.NONE)
    rc, nb, fb = call(zz=z)
    untouched = (BAD_ARG, pat, pat)
    assert call(zz=None) == untouched
    assert call(n_bad=False) == untouched
    for k in range(3):
        assert call(tabs=tuple(i != k for i in range(3))) == untouched, k
    # a null first_bad is fine
    nb = C.c_uint64(pat)
    t = [(C.c_void_p * 3)(*[x.ctypes.data for x in u]) for u in arrs]
    assert lib.zkg16_r1cs_check_host(C.byref(t[0]), C.byref(t[1]), C.byref(t[2]), r1cs["num_constraints"], nv, z.ctypes.data, C.byref(nb), None) == 0
    assert nb.value == 0
    # a null row pointer of one matrix
    t0 = (C.c_void_p * 3)(arrs[0][0].ctypes.data, None, arrs[0][2].ctypes.data)
    nb = C.c_uint64(pat)
    assert lib.zkg16_r1cs_check_host(C.byref(t0), C.byref(t[1]), C.byref(t[2]), r1cs["num_constraints"], nv, z.ctypes.data, C.byref(nb), None) == BAD_ARG
    assert nb.value == pat
    # a column out of range: in B, its last entry
    col = [x.copy() for x in arrs[1]]
    col[1][-1] = nv
    assert call(col=col) == untouched
    assert call(nv_=int(max(x.max() for x in arrs[1]))) == untouched          # ... or num_variables one too small for the largest column
    # a decreasing row pointer: in C, in the middle
    rp = [x.copy() for x in arrs[0]]
    mid = len(rp[2]) // 2
    rp[2][mid] = rp[2][mid + 1] + 1
    assert call(rp=rp) == untouched
    rp = [x.copy() for x in arrs[0]]
    rp[0][0] = 1                                                               # ... or one that does not start at 0
    assert call(rp=rp) == untouched


def test_strerror_and_signatures():
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    assert b"satisf" in lib.zkg16_strerror(8)
    for name in ("zkg16_r1cs_check_host", "zkg16_r1cs_check", "zkg16_r1cs_check_batch", "zkg16_prime_check_batch", "zkg16_last_check"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
