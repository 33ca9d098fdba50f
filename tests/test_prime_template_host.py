"""The PrimeCircuit's template and key corrections (zkg16_prime_r1cs_template_host, zkg16_prime_key_corrections) — host-side checks
that need no GPU.  Two candidates' R1CS differ in four coefficients of column 0 (the constant one): n three times in A, -j once in
C.  The template is the j >= 1 form with those four set to zero, so for any candidate (x, j) with assignment z (z[0] = 1)
    (A z)[r_t] = (A_T z)[r_t] + n, t = 1..3,      (C z)[r_4] = (C_T z)[r_4] - j,      every other row is the template's,
and for one trapdoor a candidate's key is the template's with a_query[0] + n U and gamma_abc_g1[0] + n V_n - j V_j, where
    U = [u] g1, V_n = [beta u / gamma] g1, V_j = [w / gamma] g1, u = L_r1(tau) + L_r2(tau) + L_r3(tau), w = L_r4(tau),
    L_i(tau) = (tau^N - 1) omega^i / (N (tau - omega^i)).
The reference of the corrections is that closed form in Python big integers (tests/golden/pyref.py)."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as P
from helpers import G1_GEN_LIMBS, fr_mont, py_g1, unlimbs
from test_prime_device_host import resolve

# a j = 0 candidate, x = 2^64 - 1 at j = 0, x = 0 at its first prime, two j >= 1 candidates
CANDIDATES = [(7, 0), ((1 << 64) - 1, 0), (0, None), (5, 1), (12345, 3)]


@pytest.fixture(scope="module")
def template():
    from zksnark_finalproject_amd.circuits import prime_r1cs_template_host
    r1cs, nw, rows = prime_r1cs_template_host()
    return r1cs, nw, [int(r) for r in rows]


def _patched_positions(r1cs, rows):
    """the positions of the four candidate-dependent coefficients: column 0 leads its row"""
    pos = [int(r1cs["a"][0][r]) for r in rows[:3]] + [int(r1cs["c"][0][rows[3]])]
    for m, p in zip("aaac", pos):
        assert r1cs[m][1][p] == 0
    return pos


def _row_dot(mat, row, z):
    rp, col, cf = mat
    lo, hi = int(rp[row]), int(rp[row + 1])
    return sum(P.fr_from_mont(unlimbs(cf[k])) * P.fr_from_mont(unlimbs(z[col[k]])) for k in range(lo, hi)) % P.R_MOD


def test_template_is_the_j1_form_with_four_zero_coefficients(template):
    from zksnark_finalproject_amd.circuits import prime_candidate, prime_dims, prime_r1cs_host
    r1cs, nw, rows = template
    x, j = 5, 1
    ref, ref_nw = prime_r1cs_host(x, j)
    d = prime_dims(1)
    assert nw == ref_nw == d["num_witness"] and r1cs["num_inputs"] == d["num_instance"] and r1cs["num_constraints"] == d["num_constraints"]
    assert tuple(len(r1cs[m][1]) for m in "abc") == tuple(d["nnz"])
    assert len(set(rows[:3])) == 3 and all(0 <= r < d["num_constraints"] for r in rows)
    pos = _patched_positions(r1cs, rows)
    n = prime_candidate(x, j)["n"]
    for m in "abc":
        assert np.array_equal(r1cs[m][0], ref[m][0]) and np.array_equal(r1cs[m][1], ref[m][1])
        mine = [p for t, p in zip("aaac", pos) if t == m]
        keep = np.ones(len(r1cs[m][1]), dtype=bool)
        keep[mine] = False
        assert np.array_equal(r1cs[m][2][keep], ref[m][2][keep])
        assert not r1cs[m][2][mine].any()                      # the four coefficients are zero ...
    for p in pos[:3]:                                          # ... where the request has n and -j
        assert np.array_equal(ref["a"][2][p], fr_mont(n))
    assert np.array_equal(ref["c"][2][pos[3]], fr_mont(-j))


@pytest.mark.parametrize("x,j", CANDIDATES)
def test_request_rows_are_the_templates_plus_n_and_minus_j(template, x, j):
    from zksnark_finalproject_amd.circuits import prime_candidate, prime_r1cs_host, prime_witness_host
    r1cs, _, rows = template
    x, j = resolve(x, j)
    ref, _ = prime_r1cs_host(x, j)
    z = prime_witness_host(x, j)
    n = prime_candidate(x, j)["n"]
    assert P.fr_from_mont(unlimbs(z[0])) == 1
    for r in rows[:3]:
        assert _row_dot(ref["a"], r, z) == (_row_dot(r1cs["a"], r, z) + n) % P.R_MOD
    assert _row_dot(ref["c"], rows[3], z) == (_row_dot(r1cs["c"], rows[3], z) - j) % P.R_MOD
    # every other row: the same non-zeros.  With the four positions taken out of both forms the arrays are identical (at j = 0
    # the request's C has no entry there at all, and its row pointers are one lower from the next row on)
    pos = _patched_positions(r1cs, rows)
    for m in "abc":
        mine = [p for t, p in zip("aaac", pos) if t == m]
        t_keep = np.ones(len(r1cs[m][1]), dtype=bool)
        t_keep[mine] = False
        r_keep = np.ones(len(ref[m][1]), dtype=bool)
        r_keep[[p for p in mine if not (m == "c" and j == 0)]] = False
        assert np.array_equal(r1cs[m][1][t_keep], ref[m][1][r_keep])
        assert np.array_equal(r1cs[m][2][t_keep], ref[m][2][r_keep])
        t_len, r_len = np.diff(r1cs[m][0].astype(np.int64)), np.diff(ref[m][0].astype(np.int64))
        if m == "c" and j == 0:
            t_len[rows[3]] -= 1
        assert np.array_equal(t_len, r_len)
        if m == "b":
            assert np.array_equal(r1cs[m][0], ref[m][0])


@pytest.mark.parametrize("seed", [1, 2])
def test_key_corrections_match_the_closed_form(template, seed):
    from zksnark_finalproject_amd.circuits import prime_key_corrections
    r1cs, _, rows = template
    rng = random.Random(0xC0 + seed)
    trap = [rng.randrange(1, P.R_MOD) for _ in range(5)]
    tau, _, beta, gamma, _ = trap
    k = rng.getrandbits(62) | 1
    g1 = P.ec_mul(P.G1_GEN, k) if seed == 2 else P.G1_GEN          # the standard generator and a random one
    g1_limbs = py_g1(g1)[0] if seed == 2 else G1_GEN_LIMBS
    log_n = (r1cs["num_constraints"] + r1cs["num_inputs"] - 1).bit_length()
    N = 1 << log_n
    omega = P.root_of_unity(log_n)
    zt = (pow(tau, N, P.R_MOD) - 1) % P.R_MOD

    def lagrange(i):
        wi = pow(omega, i, P.R_MOD)
        return zt * wi * pow(N * (tau - wi), -1, P.R_MOD) % P.R_MOD
    u = sum(lagrange(r) for r in rows[:3]) % P.R_MOD
    w = lagrange(rows[3])
    ginv = pow(gamma, -1, P.R_MOD)
    want = [P.ec_mul(g1, u), P.ec_mul(g1, beta * u * ginv % P.R_MOD), P.ec_mul(g1, w * ginv % P.R_MOD)]
    corr, inf = prime_key_corrections(np.stack([fr_mont(t) for t in trap]), g1_limbs)
    assert not inf.any()
    for got, pt in zip(corr, want):
        assert np.array_equal(got, py_g1(pt)[0])


def test_null_pointers_are_bad_arguments(template):
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    r1cs, _, _ = template
    BAD_ARG = 1              # ZKG16_ERR_BAD_ARG
    assert lib.zkg16_prime_key_corrections(None, None, None, None) == BAD_ARG
    trap = np.stack([fr_mont(t) for t in (3, 5, 7, 11, 13)]).reshape(-1)
    g1 = np.ascontiguousarray(G1_GEN_LIMBS)
    corr, inf = np.full(36, 0xA5, dtype=np.uint64), np.full(3, 0xA5, dtype=np.uint8)
    for args in ((None, g1.ctypes.data, corr.ctypes.data, inf.ctypes.data), (trap.ctypes.data, None, corr.ctypes.data, inf.ctypes.data),
                 (trap.ctypes.data, g1.ctypes.data, None, inf.ctypes.data), (trap.ctypes.data, g1.ctypes.data, corr.ctypes.data, None)):
        assert lib.zkg16_prime_key_corrections(*args) == BAD_ARG
    assert (corr == 0xA5).all() and (inf == 0xA5).all()
    rp = [np.array(r1cs[m][0]) for m in "abc"]
    col = [np.array(r1cs[m][1]) for m in "abc"]
    cf = [np.array(r1cs[m][2]) for m in "abc"]
    rows = np.zeros(4, dtype=np.uint64)
    arr = lambda xs: (C.c_void_p * 3)(*[v.ctypes.data for v in xs])
    assert lib.zkg16_prime_r1cs_template_host(None, C.byref(arr(col)), C.byref(arr(cf)), rows.ctypes.data) == BAD_ARG
    assert lib.zkg16_prime_r1cs_template_host(C.byref(arr(rp)), None, C.byref(arr(cf)), rows.ctypes.data) == BAD_ARG
    assert lib.zkg16_prime_r1cs_template_host(C.byref(arr(rp)), C.byref(arr(col)), None, rows.ctypes.data) == BAD_ARG
    assert lib.zkg16_prime_r1cs_template_host(C.byref(arr(rp)), C.byref(arr(col)), C.byref(arr(cf)), None) == BAD_ARG
    hole = (C.c_void_p * 3)(rp[0].ctypes.data, None, rp[2].ctypes.data)
    assert lib.zkg16_prime_r1cs_template_host(C.byref(hole), C.byref(arr(col)), C.byref(arr(cf)), rows.ctypes.data) == BAD_ARG
