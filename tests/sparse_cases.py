"""Sparse systems at the limits of the kernels that organise an R1CS by its content: the SpMV's coefficient dictionary and
row-length order (csrc/poly.hip) and the setup's column sums with their heavy-column queue (csrc/setup.hip).  Shared by
tests/test_sparse_limits_host.py (the cases are what they claim to be, and the oracle agrees with Python big integers on them)
and tests/test_sparse_limits_gpu.py (device == oracle, and the path the case is meant to reach was taken).

Everything is built as CSR arrays in numpy, in the format of helpers.csr_from_rows: row_ptr u64, col u32, (nnz, 4) u64 Montgomery
coefficients.  Any limb pattern below r is the Montgomery form of some field element, so coefficients and assignments are drawn
as limbs; the oracle and the device read the same bytes.  Every index is in range by construction, and the builders assert it."""
import numpy as np

import pyref as P
from helpers import fr_mont

# constants of the kernels under test; tests/test_sparse_limits_host.py fails when a case no longer sits on them
DICT_CAP, DICT_MAX, DICT_CHUNK, DICT_LOCAL = 4096, 1024, 16384, 512      # poly.hip
ROW_CLASSES, PERM_MIN_ROWS, DICT_MIN_NNZ = 18, 4096, 4096                # poly.hip
COL_HEAVY, COL_SLICE = 1024, 8192                                        # setup.hip

M32 = np.uint64(0xffffffff)
R_LIMBS = [(P.R_MOD >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
ONE = fr_mont(1)


def below_r(cf):
    """per row of (n, 4) u64 limbs: value < r"""
    cf = np.asarray(cf, dtype=np.uint64).reshape(-1, 4)
    lt = np.zeros(cf.shape[0], dtype=bool)
    eq = np.ones(cf.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (cf[:, i] < np.uint64(R_LIMBS[i]))
        eq &= cf[:, i] == np.uint64(R_LIMBS[i])
    return lt


def random_fr(rng, n):
    """n field elements as limbs: three uniform limbs under a top limb below r's (all of [0, r) but its last 2^-62)"""
    cf = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    cf[:, 3] = rng.integers(0, R_LIMBS[3], size=n, dtype=np.uint64)
    assert below_r(cf).all()
    return cf


def distinct_count(*cfs):
    """distinct rows of the (n, 4) arrays together.  Exact: rows are grouped by a 64-bit mix of their limbs (one sort of n keys, not
    of n rows), and every row is compared with the first of its group; only if a group is mixed are the rows themselves sorted."""
    cf = np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1, 4) for c in cfs])
    if cf.shape[0] == 0:
        return 0
    key = cf[:, 0] * np.uint64(0x9E3779B97F4A7C15) ^ cf[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F) ^ cf[:, 2] * np.uint64(0x165667B19E3779F9) ^ cf[:, 3]
    _, first, group = np.unique(key, return_index=True, return_inverse=True)
    if (cf == cf[first[group.ravel()]]).all():
        return first.shape[0]
    return np.unique(cf, axis=0).shape[0]


def limbs32(cf):
    """(n, 4) u64 -> (n, 8) u32, the limbs the device's Fr holds"""
    cf = np.asarray(cf, dtype=np.uint64).reshape(-1, 4)
    out = np.empty((cf.shape[0], 8), dtype=np.uint32)
    out[:, 0::2] = (cf & M32).astype(np.uint32)
    out[:, 1::2] = (cf >> np.uint64(32)).astype(np.uint32)
    return out


def witness(nv, seed):
    """a full assignment of random full-range field elements, z[0] = 1"""
    z = random_fr(np.random.default_rng(seed), nv)
    z[0] = ONE
    return z


# ------------------------------------------------------------------------------------------------ coefficient families
def colliding_family(count, seed=5):
    """`count` distinct coefficients that agree in the 32-bit limbs 0, 1, 2, 5 and 7 — all that coef_dict_kernel hashes — and differ
    only in limbs 3, 4 and 6: the high half of u64 limb 1 and the low halves of u64 limbs 2 and 3.  The three limbs run through the
    digits of the index in base 11, so for each of them there are members that differ in that limb alone."""
    assert 0 < count <= 11 ** 3
    base = random_fr(np.random.default_rng(seed), 1)[0]
    base[3] = (base[3] & M32) | (np.uint64(0x3c1f5a07) << np.uint64(32))          # top 32-bit limb below r's 0x73eda753
    i = np.arange(count, dtype=np.uint64)
    digit = [i % np.uint64(11), (i // np.uint64(11)) % np.uint64(11), i // np.uint64(121)]
    mix = lambda d, k: (d * np.uint64(0x9E3779B9) + np.uint64(k)) & M32           # odd multiplier: distinct digits stay distinct
    cf = np.tile(base, (count, 1))
    cf[:, 1] = (cf[:, 1] & M32) | (mix(digit[0], 0x1234567) << np.uint64(32))     # limb 3
    cf[:, 2] = (cf[:, 2] & ~M32) | mix(digit[1], 0x89abcde)                       # limb 4
    cf[:, 3] = (cf[:, 3] & ~M32) | mix(digit[2], 0x2468ace)                       # limb 6
    assert below_r(cf).all() and distinct_count(cf) == count
    return cf


def near_one():
    """(9, 4): row 0 the Montgomery form of 1, row 1 + k the same with one bit of 32-bit limb k changed.  Rows 4, 5 and 7 (limbs 3,
    4 and 6) hash like 1."""
    cf = np.tile(ONE, (9, 1))
    for k in range(8):
        cf[1 + k, k // 2] ^= np.uint64(8) << np.uint64(32 * (k % 2))
    assert below_r(cf).all() and distinct_count(cf) == 9
    return cf


def random_values(count, seed):
    cf = random_fr(np.random.default_rng(seed), count)
    assert distinct_count(cf) == count
    return cf


# ------------------------------------------------------------------------------------------------ CSR from row lengths
def _csr_pattern(lengths, nv, rng):
    """rows of the given lengths with distinct columns: row i holds start_i + j * step_i mod nv, step_i a unit mod nv"""
    lengths = np.asarray(lengths, dtype=np.int64)
    nc = lengths.shape[0]
    assert nv >= 2 and (lengths >= 0).all() and (nc == 0 or lengths.max() <= nv)
    rp = np.zeros(nc + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(lengths)
    nnz = int(rp[-1])
    row = np.repeat(np.arange(nc, dtype=np.int64), lengths)
    pos = np.arange(nnz, dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), lengths)
    units = np.flatnonzero(np.gcd(np.arange(1, nv), nv) == 1) + 1
    start = rng.integers(0, nv, size=nc)
    step = units[rng.integers(0, units.shape[0], size=nc)]
    col = (start[row] + pos * step[row]) % nv
    assert nnz == 0 or (0 <= col.min() and col.max() < nv)
    assert np.unique(row * nv + col).shape[0] == nnz                      # distinct columns within a row
    assert rp[0] == 0 and (np.diff(rp.astype(np.int64)) == lengths).all()
    return rp, col.astype(np.uint32)


def _cyclic_picks(nnz, nvalues, rng):
    """value numbers for nnz entries that use every value: chunk by chunk (DICT_CHUNK entries, a workgroup of coef_dict_kernel) the
    values in turn, in a random order inside the chunk"""
    idx = np.empty(nnz, dtype=np.int64)
    for lo in range(0, nnz, DICT_CHUNK):
        n = min(DICT_CHUNK, nnz - lo)
        idx[lo:lo + n] = rng.permutation(np.arange(n) % nvalues)
    return idx


def _r1cs(mats, ni, nc):
    return dict(a=mats[0], b=mats[1], c=mats[2], num_inputs=ni, num_constraints=nc)


def _spread(total, nc, rng):
    """nc row lengths that add up to total, as even as they can be, in random order"""
    lengths = np.full(nc, total // nc, dtype=np.int64)
    lengths[:total % nc] += 1
    return rng.permutation(lengths)


def dict_system(values, nc, nv, seed, ni=3, nnz=None, two_chunks=True):
    """An R1CS whose three coefficient arrays together use exactly `values`.  A carries every value in turn, chunk by chunk; B and C
    draw from them at random.  nnz: non-zeros of (A, B, C), default (DICT_CHUNK + 2 * len(values) + 1000, about 2 nc, about nc);
    a 0 gives a matrix without non-zeros.  two_chunks: every value lies in at least two different DICT_CHUNK-entry chunks of A, so
    several workgroups insert it (asserted)."""
    values = np.asarray(values, dtype=np.uint64).reshape(-1, 4)
    nvalues = values.shape[0]
    assert below_r(values).all() and distinct_count(values) == nvalues
    rng = np.random.default_rng(seed)
    if nnz is None:
        nnz = (DICT_CHUNK + 2 * nvalues + 1000, 2 * nc + 17, nc - 11)
    mats = []
    for m, total in enumerate(nnz):
        rp, col = _csr_pattern(_spread(total, nc, rng), nv, rng)
        pick = _cyclic_picks(total, nvalues, rng) if m == 0 else rng.integers(0, nvalues, size=total)
        if m == 0:
            assert total >= nvalues
            if two_chunks:
                seen = np.zeros(nvalues, dtype=np.int64)
                for lo in range(0, total, DICT_CHUNK):
                    seen[np.unique(pick[lo:lo + DICT_CHUNK])] += 1
                assert (seen >= 2).all()
        mats.append((rp, col, values[pick]))
    assert distinct_count(*[cf for _, _, cf in mats]) == nvalues
    return _r1cs(mats, ni, nc)


ROW_POOL_SEED = 99


def row_pool():
    """the 8 coefficients of the row-class systems: 1, -1, 2 and five random ones"""
    return np.concatenate([np.stack([ONE, fr_mont(-1), fr_mont(2)]), random_values(5, ROW_POOL_SEED)])


def row_class_system(lengths, nc, nv, seed, ni=3):
    """Rows with the prescribed non-zero counts and distinct columns within a row: A's row i has lengths[i] entries, B's
    lengths[i - 1], C's lengths[i - 2] (the same histogram, three different orders).  Coefficients from row_pool(), each matrix with
    8 or more entries using all of it."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.shape == (nc,)
    rng = np.random.default_rng(seed)
    pool = row_pool()
    mats = []
    for m in range(3):
        rp, col = _csr_pattern(np.roll(lengths, m), nv, rng)
        mats.append((rp, col, pool[_cyclic_picks(int(rp[-1]), pool.shape[0], rng)]))
    return _r1cs(mats, ni, nc)


def column_system(col_lengths, ni, seed, nc):
    """For the setup: matrix m has exactly col_lengths[m][k] entries in column k, at most one per row, on rows drawn at random;
    coefficients are random field elements, one in eight of them 1.  -> (r1cs, num_variables)"""
    rng = np.random.default_rng(seed)
    nv = len(col_lengths[0])
    assert ni <= nv
    mats = []
    for m in range(3):
        want = np.asarray(col_lengths[m], dtype=np.int64)
        assert want.shape == (nv,) and (want >= 0).all() and want.max() <= nc
        rows = np.concatenate([rng.permutation(nc)[:n] for n in want])           # one draw per column: a row at most once in it
        cols = np.repeat(np.arange(nv, dtype=np.int64), want)
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
        rp = np.zeros(nc + 1, dtype=np.uint64)
        rp[1:] = np.cumsum(np.bincount(rows, minlength=nc))
        cf = random_fr(rng, rows.shape[0])
        cf[rng.integers(0, 8, size=rows.shape[0]) == 0] = ONE
        assert rows.shape[0] == 0 or (cols.max() < nv and rows.max() < nc)
        assert (np.bincount(cols, minlength=nv) == want).all() and np.unique(rows * nv + cols).shape[0] == rows.shape[0]
        mats.append((rp, cols.astype(np.uint32), cf))
    return _r1cs(mats, ni, nc), nv


# ------------------------------------------------------------------------------------------------ what to measure on a system
def row_lengths(r1cs):
    return [np.diff(r1cs[m][0].astype(np.int64)) for m in "abc"]


def column_lengths(r1cs, nv):
    return [np.bincount(r1cs[m][1].astype(np.int64), minlength=nv) for m in "abc"]


def total_nnz(r1cs):
    return sum(int(r1cs[m][0][-1]) for m in "abc")


def domain(r1cs):
    return 1 << max(r1cs["num_constraints"] + r1cs["num_inputs"] - 1, 0).bit_length()


# ------------------------------------------------------------------------------------------------ the case tables
# state = (dict_state, ndict, perm_ok, spmv_uses) that zkg16_r1cs_spmv_state must report after the SECOND witness map on the handle
def _dict_values(kind):
    if kind == "near_one":
        return np.concatenate([near_one(), np.stack([fr_mont(0), fr_mont(-1), fr_mont(2)])])
    name, count = kind
    return colliding_family(count) if name == "colliding" else random_values(count, 1000 + count)


DICT_CASES = {
    # name: (values, nc, nv, extra arguments of dict_system, distinct values, state)
    "random1023": (("random", 1023), 6000, 3000, {}, 1023, (1, 1023, 1, 2)),
    "random1024": (("random", 1024), 6000, 3000, {}, 1024, (1, 1024, 1, 2)),                  # 33,808 B of dynamic LDS
    "random1025": (("random", 1025), 6000, 3000, {}, 1025, (2, 0, 1, 2)),                     # plain kernel on ordered rows
    "colliding1024": (("colliding", 1024), 6000, 3000, {}, 1024, (1, 1024, 1, 2)),            # one probe sequence for all of them
    "colliding1025": (("colliding", 1025), 6000, 3000, {}, 1025, (2, 0, 1, 2)),
    "near_one": ("near_one", 6000, 3000, {}, 12, (1, 12, 1, 2)),
    "tiny_nnz4095": (("random", 600), 5000, 3000, dict(nnz=(2000, 1500, 595), two_chunks=False), 600, (2, 0, 1, 2)),      # not tried
    "nc4095": (("random", 600), 4095, 3000, {}, 600, (1, 600, 0, 2)),                         # dictionary without the row order
    "empty_c": (("random", 64), 6000, 3000, dict(nnz=(DICT_CHUNK + 1128, 12017, 0)), 64, (1, 64, 1, 2)),
}


def dict_case(name):
    """-> (r1cs, num_variables, distinct coefficients, state after the second use)"""
    kind, nc, nv, extra, ndistinct, state = DICT_CASES[name]
    return dict_system(_dict_values(kind), nc, nv, seed=len(name) + 7 * nc, **extra), nv, ndistinct, state


EDGE_LENGTHS = [0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 255, 256, 1023, 1024]      # both sides of the class edges 2^k - 1 | 2^k
SMALL_MIX = [0, 1, 2, 3, 5, 8, 1, 1]
WIDE_MIX = [0, 1, 1, 1, 2, 3, 4, 9, 17, 40]


def _cycle(pattern, nc):
    return np.resize(np.asarray(pattern, dtype=np.int64), nc)


def _drawn(pattern, nc, seed):
    return np.asarray(pattern, dtype=np.int64)[np.random.default_rng(seed).integers(0, len(pattern), size=nc)]


def _mostly_ones(nc):
    lengths = np.ones(nc, dtype=np.int64)
    lengths[::1000] = 9
    return lengths


def _two_long(nc):
    lengths = np.ones(nc, dtype=np.int64)
    lengths[1000], lengths[3000] = 70000, 131072          # bit lengths 17 and 18: both in the clamped top class
    return lengths


def _hist(pairs):
    h = [0] * ROW_CLASSES
    for c, n in pairs:
        h[c] += n
    return h


ROW_CASES = {
    # name: (lengths(nc), nc, nv, rows per length class (None: whatever the drawn lengths give), state)
    "nc4095": (lambda nc: _cycle(SMALL_MIX, nc), 4095, 512, None, (1, 8, 0, 2)),
    "nc4096": (lambda nc: _cycle(SMALL_MIX, nc), 4096, 512, _hist([(0, 512), (1, 1536), (2, 1024), (3, 512), (4, 512)]), (1, 8, 1, 2)),
    "nc4097": (lambda nc: _cycle(SMALL_MIX, nc), 4097, 512, None, (1, 8, 1, 2)),
    "nc4159": (lambda nc: _cycle(SMALL_MIX, nc), 4096 + 63, 512, None, (1, 8, 1, 2)),         # a partial last wave in row_perm_kernel
    "all0": (lambda nc: np.zeros(nc, dtype=np.int64), 6000, 512, _hist([(0, 6000)]), (2, 0, 1, 2)),      # no non-zeros at all
    "all1": (lambda nc: np.full(nc, 1, dtype=np.int64), 6000, 512, _hist([(1, 6000)]), (1, 8, 1, 2)),
    "all5": (lambda nc: np.full(nc, 5, dtype=np.int64), 6000, 512, _hist([(3, 6000)]), (1, 8, 1, 2)),
    "class_edges": (lambda nc: _cycle(EDGE_LENGTHS, nc), 6000, 1500,
                    _hist([(0, 400), (1, 400), (2, 800), (3, 800), (4, 800), (5, 800), (6, 400), (8, 400), (9, 400), (10, 400), (11, 400)]),
                    (1, 8, 1, 2)),
    "blocks65": (lambda nc: _drawn(WIDE_MIX, nc, 65), 16385 + 64, 2000, None, (1, 8, 1, 2)),           # the scan's second wave has work
    "blocks1026": (_mostly_ones, 262144 + 257, 5000, _hist([(1, 262401 - 263), (4, 263)]), (1, 8, 1, 2)),      # per = 128: a carried prefix
    "top_class": (_two_long, 4200, 140000, _hist([(1, 4198), (17, 2)]), (1, 8, 1, 2)),
}


def row_case(name):
    """-> (r1cs, num_variables, lengths asked for, rows per class or None, state after the second use)"""
    lengths, nc, nv, hist, state = ROW_CASES[name]
    want = lengths(nc)
    return row_class_system(want, nc, nv, seed=3 * nc + len(name)), nv, want, hist, state


# setup: ni = 3, nv = 24, nc = 16,400 (domain 2^15).  Heavy = more than COL_HEAVY entries; slices of COL_SLICE.
#   A: heavy at k = 0, 2 (both instance columns: the gather kernel adds L[nc + k]) and 7, with 3, 1 and 2 slices
#   B: five heavy columns in no order of length, one of them k = 1 (an instance column where nothing may be added)
#   C: one heavy column, k = 1
COLUMN_MAIN = dict(ni=3, nc=16400, lengths=[
    [16385, 1024, 1025, 0, 1, 1023, 1024, 8193, 0, 5, 1000, 1, 0, 2, 1024, 3, 0, 700, 1, 0, 64, 1023, 0, 9],
    [3, 8192, 0, 1024, 0, 16384, 1, 1023, 0, 1025, 17, 0, 16385, 1, 0, 1024, 2, 0, 0, 300, 8191, 0, 1, 1024],
    [0, 8193, 1, 0, 1024, 1023, 0, 0, 12, 1, 0, 1024, 40, 0, 1, 0, 1023, 2, 0, 1, 0, 512, 1, 0]])
# a matrix without a heavy column (C: heavy[0] stays 0) next to A and B just over the threshold, small enough for a proof
COLUMN_SMALL = dict(ni=3, nc=1100, lengths=[
    [1025, 1024, 1100, 0, 1, 1023, 1024, 1026],
    [2, 1025, 0, 1024, 1, 0, 1100, 1023],
    [0, 1024, 1, 1023, 1024, 0, 7, 1]])


def heavy_columns(lengths):
    """[(column, slices)] of the columns setup_col_sum_kernel queues"""
    return [(k, (n + COL_SLICE - 1) // COL_SLICE) for k, n in enumerate(lengths) if n > COL_HEAVY]


def column_case(spec, seed=2718):
    return column_system(spec["lengths"], spec["ni"], seed, spec["nc"])
