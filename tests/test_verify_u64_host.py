"""The u64 form of batched verification without a GPU: the device header of its kernels compiled for the host
(tests/csrc/u64_inputs_host_shim.hip) against Python integers and the oracle's points, the host entry zkg16_verify_batch_u64_host on
simulated statements whose verdicts are known by construction (tests/u64_verify_cases.py), and the handler's request checks.  Every
comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import sim_proofs as S
import u64_verify_cases as U
import verify_batch_cases as VB
from helpers import *

K = 12
WHERE = (0, 2, 4, 6, 9)          # one negative of each kind (u64_verify_cases.NEGATIVE_KINDS)
X_ROWS = 6                       # rows per key on the host: the all-zero row, the rows at infinity and ordinary ones


@pytest.fixture(scope="module")
def shim():
    return U.load_shim()


@pytest.fixture(scope="module")
def sim(oracle):
    return U.U64Sim(oracle, 6, K, WHERE, 6401)


# ------------------------------------------------------------------------------------------------ the device header on the host
def test_slices_and_lane_groups(shim):
    for k in (0, 1, 127, 128, 129, 300, 32768, 32769, 65537, 2**32 - 1):
        assert shim.u6_slice_len(k) == U.slice_len(k), k
        s = shim.u6_sum_slices(k)
        assert s <= 256 and s * shim.u6_slice_len(k) >= k and (k == 0) == (s == 0), k
    # the smallest power of two >= min(m, 64)
    assert [shim.u6_group_lanes(m) for m in U.X_MS] == [1, 2, 4, 8, 16, 32, 64, 64, 64, 64, 64]
    assert [shim.u6_group_lanes(m) for m in (4, 5, 33, 1056, 4160)] == [4, 8, 64, 64, 64]


@pytest.mark.parametrize("case_", list(U.sum_cases()), ids=lambda c: c[0])
def test_lane_column_sums_equal_python_integers(shim, case_):
    name, vals, rhos, live = case_
    k, m = vals.shape
    rho = S.rho_rows(rhos)
    sums = np.full((m + 1, 4), 0x5A, dtype=np.uint64)
    shim.u6_rho_sums(vals.ctypes.data, m, rho.ctypes.data, None if live is None else live.ctypes.data, k, sums.ctypes.data)
    want = U.sums_want(name, vals, rhos, live)
    assert max(want) < 1 << 224
    if name.endswith("all_maximal"):
        assert want[1] == k * (2**128 - 1) * (2**64 - 1)
    assert U.sums_ints(sums) == want


@pytest.mark.parametrize("family", U.X_FAMILIES)
@pytest.mark.parametrize("m", U.X_MS)
def test_grouped_ladder_equals_the_oracle(shim, oracle, family, m):
    xc = U.x_case(oracle, family, m, X_ROWS)
    for p in range(X_ROWS):
        out = np.full(12, 0x5A, dtype=np.uint64)
        row = np.ascontiguousarray(xc.values[p])
        have = shim.u6_prepared_input(xc.gabc.ctypes.data, m, row.ctypes.data, 0, out.ctypes.data)
        assert have == (0 if xc.want_inf[p] else 1), (family, m, p)
        assert np.array_equal(out, xc.want[p]), (family, m, p)


def test_grouped_ladder_any_lane_count(shim, oracle):
    """the same X whatever power of two the proof is spread over, more lanes than columns included"""
    for family in ("small", "x_inf"):
        xc = U.x_case(oracle, family, 12, X_ROWS)
        for L in (1, 2, 4, 8, 16, 32, 64):
            for p in range(X_ROWS):
                out = np.zeros(12, dtype=np.uint64)
                row = np.ascontiguousarray(xc.values[p])
                have = shim.u6_prepared_input(xc.gabc.ctypes.data, 12, row.ctypes.data, L, out.ctypes.data)
                assert have == (0 if xc.want_inf[p] else 1) and np.array_equal(out, xc.want[p]), (family, L, p)


# ------------------------------------------------------------------------------------------------ the host entry
def test_fixture_values_are_the_public_inputs(sim):
    assert np.array_equal(U.expand(sim.values), sim.batch.pubs)
    assert set(sim.kinds.values()) == set(U.NEGATIVE_KINDS)


def test_verify_batch_u64_host(sim):
    from zksnark_finalproject_amd.device import verify_batch_host, verify_batch_u64_host
    b, want = sim.batch, sim.want
    rho = VB.draw_rho(random.Random(3), K)
    ok, got = verify_batch_u64_host(b.pvk, sim.values, b.proofs, b.infs, rho=rho, each=True)
    assert ok is False and np.array_equal(got, want), [(s.name, g, w) for s, g, w in zip(sim.stmts, got, want)]
    ok2, got2 = verify_batch_host(b.pvk, U.expand(sim.values), b.proofs, b.infs, rho=rho, each=True)
    assert ok2 is False and np.array_equal(got2, got)
    good = np.flatnonzero(want)
    assert verify_batch_u64_host(b.pvk, sim.values[good], b.proofs[good], b.infs[good], rho=rho[good]) is True
    assert verify_batch_u64_host(b.pvk, sim.values[good], b.proofs[good], b.infs[good]) is True          # multipliers from `secrets`
    # K = 1: a negative, and a valid one
    assert verify_batch_u64_host(b.pvk, sim.values[:1], b.proofs[:1], b.infs[:1]) is False
    assert verify_batch_u64_host(b.pvk, sim.values[1:2], b.proofs[1:2], b.infs[1:2], each=True) == (True, [True])


def test_verify_batch_u64_host_checks_arguments(sim):
    from zksnark_finalproject_amd import _lib
    from zksnark_finalproject_amd.device import _verify_args
    b = sim.batch
    lib = _lib.load()
    rho = VB.draw_rho(random.Random(4), K)
    args, k = _verify_args(b.pvk, "u64", (sim.values,), b.proofs, b.infs, rho)
    ok, each = C.c_int(7), np.full(K, 9, dtype=np.uint8)

    def call(a, threads=0):
        return lib.zkg16_verify_batch_u64_host(*a, threads, C.byref(ok), each.ctypes.data)
    assert call(args[:1] + (1,) + args[2:]) == 1 and call(args[:1] + (0,) + args[2:]) == 1        # num_instance < 2
    assert call(args[:6] + (None,) + args[7:]) == 1                                                # no values
    assert call(args[:10] + (1 << 32,)) == 1                                                       # k >= 2^32
    assert call(args[:10] + (0,)) == 1
    assert call((None,) + args[1:]) == 1 and call(args[:7] + (None,) + args[8:]) == 1 and call(args[:8] + (None,) + args[9:]) == 1
    assert call(args[:9] + (None,) + args[10:]) == 1 and call(args[:5] + (67,) + args[6:]) == 1
    assert call(tuple(args), threads=-1) == 1
    assert lib.zkg16_verify_batch_u64_host(*args, 0, None, each.ctypes.data) == 1
    zero = rho.copy()
    zero[5] = 0
    assert call(args[:9] + (zero.ctypes.data,) + args[10:]) == 1
    assert ok.value == 7 and (each == 9).all()
    assert call(tuple(args)) == 0 and ok.value == 0 and np.array_equal(each.astype(bool), sim.want)


# ------------------------------------------------------------------------------------------------ the handler's request checks
def test_linear_u64_row_is_the_row_major_matrix():
    from zksnark_finalproject_amd.handlers import _linear_public_inputs, _linear_u64_row
    rng = random.Random(8)
    a = np.array([[rng.getrandbits(64) for _ in range(3)] for _ in range(3)], dtype=np.uint64)
    b = np.array([0, 2**64 - 1, 2**63], dtype=np.uint64)
    row = _linear_u64_row(a, b)
    assert row.dtype == np.uint64 and row.shape == (12,)
    assert [int(v) for v in row] == [int(v) for v in np.concatenate([a, b[:, None]], axis=1).reshape(-1)]
    assert np.array_equal(U.expand(row), _linear_public_inputs(a, b))
    # lists of Python integers, the largest u64 among them, read the same
    assert np.array_equal(_linear_u64_row(a.tolist(), b.tolist()), row)
    assert np.array_equal(_linear_u64_row([[1, 2], [3, 4]], [5, 6]), np.array([1, 2, 5, 3, 4, 6], dtype=np.uint64))
    # what is no system of u64 values
    for bad in (([[1, 2], [3, 4]], [5]), ([[1, 2, 3], [4, 5, 6]], [7, 8]), ([[1, -2], [3, 4]], [5, 6]), ([[1, 2], [3, 4]], [5, 2**64]),
                ([[1, 2], [3]], [5, 6]), ([], []), ([[1, "x"], [3, 4]], [5, 6]), ([[1, 2], [3, 4]], [-1, 6]), ([[2**64, 2], [3, 4]], [5, 6]), (7, [1])):
        assert _linear_u64_row(*bad) is None, bad
