"""The cases of tests/sparse_cases.py are what they claim to be (so that a later change to a kernel cannot quietly disarm
tests/test_sparse_limits_gpu.py), and on small instances of every builder the CPU oracle's witness map equals one computed with
Python big integers (tests/golden/pyref.py): hash-equal coefficients, empty rows and empty matrices included.  No GPU."""
import numpy as np
import pytest

import pyref as P
import sparse_cases as S
from helpers import fr_from_mont_vec, unlimbs


# ---------------------------------------------------------------------------------------------- the dictionary's hash
def coef_hash(cf):
    """The hash of coef_dict_kernel, copied from csrc/poly.hip (uint32 arithmetic, wrapping):
        h = l[0] * 0x9E3779B1 ^ l[1] * 0x85EBCA77 ^ l[2] * 0xC2B2AE3D ^ l[5] * 0x27D4EB2F ^ l[7];  h ^= h >> 15;
    the probe sequence of the global table starts at h & (DICT_CAP - 1), the workgroup's LDS entry is (h >> 16) & (DICT_LOCAL - 1).
    If the kernel's hash changes, change it here and rebuild sparse_cases.colliding_family / near_one so that they collide again."""
    l = S.limbs32(cf)
    h = (l[:, 0] * np.uint32(0x9E3779B1)) ^ (l[:, 1] * np.uint32(0x85EBCA77)) ^ (l[:, 2] * np.uint32(0xC2B2AE3D)) \
        ^ (l[:, 5] * np.uint32(0x27D4EB2F)) ^ l[:, 7]
    h = h ^ (h >> np.uint32(15))
    return h, h & np.uint32(S.DICT_CAP - 1), (h >> np.uint32(16)) & np.uint32(S.DICT_LOCAL - 1)


def test_colliding_family_has_one_hash():
    for count in (1024, 1025):
        cf = S.colliding_family(count)
        assert S.distinct_count(cf) == count and S.below_r(cf).all()
        h, start, local = coef_hash(cf)
        assert np.unique(h).size == 1 and np.unique(start).size == 1 and np.unique(local).size == 1
        l = S.limbs32(cf)
        assert all(np.unique(l[:, k]).size == 1 for k in (0, 1, 2, 5, 7))           # the hashed limbs agree
        assert (l[:, 7] < 0x73eda753).all()
        # each of limbs 3, 4 and 6 alone tells some members apart: without it the family shrinks
        for k in (3, 4, 6):
            rest = np.delete(l, k, axis=1)
            assert np.unique(rest, axis=0).shape[0] < count, k
    assert np.array_equal(S.colliding_family(1025)[:1024], S.colliding_family(1024))


def test_near_one_limbs_and_hash():
    cf = S.near_one()
    assert cf.shape == (9, 4) and unlimbs(cf[0]) == P.FR_MONT_R and P.fr_from_mont(unlimbs(cf[0])) == 1
    l = S.limbs32(cf)
    for k in range(8):
        differs = np.flatnonzero(l[1 + k] != l[0])
        assert list(differs) == [k]                                                  # row 1 + k: limb k and nothing else
    h, start, local = coef_hash(cf)
    for k in range(8):
        same = h[1 + k] == h[0]
        assert same == (k in (3, 4, 6)), k                                           # the unhashed limbs collide with 1, the others do not
    assert np.unique(start[[0, 4, 5, 7]]).size == 1 and np.unique(local[[0, 4, 5, 7]]).size == 1


def test_random_values_do_not_collide_much():
    """the random dictionaries are the ordinary case: no probe sequence of any length, LDS entries shared by two values at most rarely"""
    h, start, _ = coef_hash(S.random_values(1024, 2024))
    assert np.unique(h).size == 1024 and np.unique(start).size > 850


# ---------------------------------------------------------------------------------------------- the case tables
def _state_by_the_rules(nc, nnz, ndistinct):
    """what spmv_run / coef_dict_build (csrc/poly.hip) do on the second use of a handle, from the constants alone"""
    perm_ok = 1 if nc >= S.PERM_MIN_ROWS else 0
    if nnz < S.DICT_MIN_NNZ or ndistinct > S.DICT_MAX:
        return (2, 0, perm_ok, 2)
    return (1, ndistinct, perm_ok, 2)


@pytest.mark.parametrize("name", list(S.DICT_CASES))
def test_dict_case_is_what_the_table_says(name):
    r1cs, nv, ndistinct, state = S.dict_case(name)
    nc = r1cs["num_constraints"]
    assert S.distinct_count(*[r1cs[m][2] for m in "abc"]) == ndistinct
    assert S.domain(r1cs) == 1 << 13
    assert state == _state_by_the_rules(nc, S.total_nnz(r1cs), ndistinct)
    assert all(r1cs[m][1].max(initial=0) < nv for m in "abc")
    if name == "tiny_nnz4095":
        assert S.total_nnz(r1cs) == 4095
    elif name == "nc4095":
        assert nc == 4095 and S.total_nnz(r1cs) >= 4096
    elif name == "empty_c":
        assert r1cs["c"][2].shape == (0, 4) and not r1cs["c"][0].any()
    if name != "tiny_nnz4095":
        # A spans two chunks of coef_dict_kernel and every value lies in both: two workgroups look it up in the global table
        cf = r1cs["a"][2]
        assert cf.shape[0] > S.DICT_CHUNK
        for part in (cf[:S.DICT_CHUNK], cf[S.DICT_CHUNK:]):
            assert S.distinct_count(part) == ndistinct


def _class_of(length):
    return min(int(length).bit_length(), S.ROW_CLASSES - 1)                          # row_class() of csrc/poly.hip


def _rows_per_class(lengths):
    uniq, inverse = np.unique(lengths, return_inverse=True)
    return list(np.bincount(np.array([_class_of(n) for n in uniq])[inverse.ravel()], minlength=S.ROW_CLASSES))


@pytest.mark.parametrize("name", list(S.ROW_CASES))
def test_row_case_is_what_the_table_says(name):
    r1cs, nv, want, hist, state = S.row_case(name)
    nc = r1cs["num_constraints"]
    by_want = _rows_per_class(want)
    if hist is not None:
        assert by_want == hist
    for m, lengths in enumerate(S.row_lengths(r1cs)):
        assert np.array_equal(lengths, np.roll(want, m))                             # the prescribed counts, three orders
        assert _rows_per_class(lengths) == by_want
    ndistinct = S.distinct_count(*[r1cs[m][2] for m in "abc"]) if S.total_nnz(r1cs) else 0
    assert ndistinct == (8 if S.total_nnz(r1cs) else 0)
    assert state == _state_by_the_rules(nc, S.total_nnz(r1cs), ndistinct)
    blocks = (nc + 255) // 256                                                       # workgroups of row_class_count_kernel
    per = ((blocks + 15) // 16 + 63) & ~63                                           # counts per wave of row_class_scan_kernel
    if name == "blocks65":
        assert blocks == 65 and per == 64                                            # wave 1 holds the 65th count: before != 0
    elif name == "blocks1026":
        assert blocks == 1026 and per == 128 and S.domain(r1cs) == 1 << 19           # two 64-element steps per wave
    elif name == "top_class":
        assert sorted(int(n).bit_length() for n in want)[-2:] == [17, 18] and by_want[17] == 2
    elif name == "class_edges":
        assert sum(1 for c in by_want if c) == 11
    elif name in ("all0", "all1", "all5"):
        assert sum(1 for c in by_want if c == 0) == 17
    elif name == "nc4159":
        assert nc % 64 == 63


@pytest.mark.parametrize("spec", [S.COLUMN_MAIN, S.COLUMN_SMALL], ids=["main", "small"])
def test_column_case_is_what_the_table_says(spec):
    r1cs, nv = S.column_case(spec)
    assert nv == len(spec["lengths"][0]) and r1cs["num_constraints"] == spec["nc"]
    for got, want in zip(S.column_lengths(r1cs, nv), spec["lengths"]):
        assert list(got) == want
    for m in "abc":                                                                  # a column at most once per row
        rp, col, _ = r1cs[m]
        rows = np.repeat(np.arange(spec["nc"]), np.diff(rp.astype(np.int64)))
        assert np.unique(rows * nv + col).size == col.size
    # the heavy queue of setup_run holds nnz / COL_HEAVY + nnz / COL_SLICE + 2 slices, nnz the largest of the three matrices
    biggest = max(int(r1cs[m][0][-1]) for m in "abc")
    slots = biggest // S.COL_HEAVY + biggest // S.COL_SLICE + 2
    heavy = [S.heavy_columns(lengths) for lengths in spec["lengths"]]
    assert all(sum(s for _, s in h) <= slots for h in heavy)
    if spec is S.COLUMN_MAIN:
        assert S.domain(r1cs) == 1 << 15
        assert heavy[0] == [(0, 3), (2, 1), (7, 2)]                                   # instance columns 0 and 2: add_inputs in the gather kernel
        assert heavy[1] == [(1, 1), (5, 2), (9, 1), (12, 3), (20, 1)]
        sizes = [spec["lengths"][1][k] for k, _ in heavy[1]]
        assert sizes != sorted(sizes) and sizes != sorted(sizes, reverse=True)
        assert heavy[2] == [(1, 2)]
        every = set(sum(spec["lengths"], []))
        assert {0, 1, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385} <= every
    else:
        assert heavy[0] == [(0, 1), (2, 1), (7, 1)] and heavy[1] == [(1, 1), (6, 1)] and heavy[2] == []
        assert max(spec["lengths"][2]) == S.COL_HEAVY


# ---------------------------------------------------------------------------------------------- oracle == big integers
def _to_int(cf):
    return [P.fr_from_mont(unlimbs(row)) for row in np.asarray(cf, dtype=np.uint64).reshape(-1, 4)]


def _bigint_witness_map(r1cs, z):
    """ark-groth16's h for ANY assignment, with pyref's transforms by definition: coset_ifft((A_cos * B_cos - C_cos) / Z)"""
    ni, nc, n = r1cs["num_inputs"], r1cs["num_constraints"], S.domain(r1cs)
    vec = []
    for m in "abc":
        rp, col, cf = r1cs[m]
        cf = _to_int(cf)
        out = [0] * n
        for i in range(nc):
            out[i] = sum(cf[k] * z[int(col[k])] for k in range(int(rp[i]), int(rp[i + 1]))) % P.R_MOD
        vec.append(out)
    for i in range(ni):
        vec[0][nc + i] = z[i]
    cos = [P.dft_naive(P.dft_naive(v, inverse=True), coset=True) for v in vec]
    zinv = pow(pow(P.FR_GEN, n, P.R_MOD) - 1, -1, P.R_MOD)
    q = [(a * b - c) * zinv % P.R_MOD for a, b, c in zip(*cos)]
    return vec, P.dft_naive(q, inverse=True, coset=True)


def _small_systems():
    hashed = np.concatenate([S.colliding_family(40), S.near_one()])
    edge = np.resize(np.array([0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32]), 200)
    yield "dict_colliding_empty_c", S.dict_system(hashed, 200, 50, seed=1, nnz=(700, 400, 0), two_chunks=False), 50
    yield "row_classes", S.row_class_system(edge, 200, 40, seed=2), 40
    yield "no_non_zeros", S.row_class_system(np.zeros(200, dtype=np.int64), 200, 40, seed=3), 40
    r1cs, nv = S.column_system([[200, 0, 1, 50, 7, 0, 199, 3], [0, 200, 0, 1, 0, 64, 2, 0], [1, 0, 0, 0, 200, 0, 0, 0]], 3, 4, 200)
    yield "columns", r1cs, nv


@pytest.mark.parametrize("name", ["dict_colliding_empty_c", "row_classes", "no_non_zeros", "columns"])
def test_oracle_witness_map_equals_big_integers(oracle, name):
    r1cs, nv = next((r, v) for n, r, v in _small_systems() if n == name)
    assert r1cs["num_constraints"] == 200 and S.domain(r1cs) == 256
    zm = S.witness(nv, seed=len(name))
    (a, b, c), want = _bigint_witness_map(r1cs, _to_int(zm))
    if name == "no_non_zeros":
        assert not any(a[:200]) and not any(b) and not any(c) and not any(want)
    else:
        assert any(a[:200]) and any(b) and any(want)
    assert fr_from_mont_vec(oracle.witness_map(r1cs, zm)) == want
