"""The bucket scatter, the bucket offsets and the B-side compaction on the device against the stable-sort model of
tests/sort_cases.py, through the two diagnostic entries zkg16_diag_bucket_sort (raw digit codes -> list, window totals, length) and
zkg16_diag_term_list (scalars -> the list and offsets a plan builds, masked in the digit kernel or filtered).

Every comparison is exact equality of whole arrays: the entry list (position << 1 | negate, global bucket id) in order, the
per-window totals, the length and the tb + 1 offsets.  No tolerance appears anywhere: an order inside a bucket that differs from
index order fails here, and nowhere else in the suite (a bucket's sum does not depend on it)."""
import numpy as np
import pytest

import sort_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def check_raw(dev, case, codes=None):
    codes = case.make() if codes is None else codes
    want, want_tot = S.model_sort(codes, case.c)
    got, tot, length = dev.diag_bucket_sort(codes, case.c)
    assert length == len(want), (case, length, len(want))
    assert np.array_equal(tot, want_tot), case
    assert np.array_equal(got, want), (case, first_difference(got, want))


def first_difference(got, want):
    if got.shape != want.shape:
        return got.shape, want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if not len(bad) else (int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))


def _ids(cases):
    return [c.name for c in cases]


_GEOM, _SPLIT, _WIN = S.geometry_cases(), S.split_cases(), S.window_cases()


@pytest.mark.parametrize("case", _GEOM, ids=_ids(_GEOM))
def test_chunk_geometry(dev, case):
    """n on either side of a round (64), a wave's share (1,024) and a block (4,096); one bucket (ranks carried through every round,
    wave and block), descending buckets, alternating signs, no entry at all, one whole block of ~0, one entry in the last position"""
    check_raw(dev, case)


@pytest.mark.parametrize("case", _SPLIT, ids=_ids(_SPLIT))
def test_pass_split(dev, case):
    """1+0 to 10+10 bits in two passes and 7+7+7 to 8+8+8 in three: the extreme buckets, buckets that differ in one pass's bits only"""
    check_raw(dev, case)


def test_width_above_the_build_limit_is_refused(dev):
    from zksnark_finalproject_amd import Zkg16Error
    codes = np.zeros((1, 65), dtype=np.uint32)
    with pytest.raises(Zkg16Error) as e:
        dev.diag_bucket_sort(codes, S.REFUSED_C)
    assert e.value.status == S.ERR_HIP and "above build limit" in str(e.value)
    # no output is written on an error; and the ctx goes on working
    import ctypes as C
    ent, tot, length = np.full((65, 2), 7, np.uint32), np.full(1, 7, np.uint32), C.c_uint64(7)
    rc = dev.lib.zkg16_diag_bucket_sort(dev.ctx, codes.ctypes.data, 65, 1, S.REFUSED_C, ent.ctypes.data, tot.ctypes.data, C.byref(length))
    assert rc == S.ERR_HIP and (ent == 7).all() and tot[0] == 7 and length.value == 7
    got, tot, length = dev.diag_bucket_sort(np.zeros((3, 0), dtype=np.uint32), 8)
    assert length == 0 and got.shape == (0, 2) and tot.tolist() == [0, 0, 0]
    got, tot, length = dev.diag_bucket_sort(codes, S.REFUSED_C - 1)
    assert length == 65 and np.array_equal(got[:, 0], np.arange(65, dtype=np.uint32) << 1) and not got[:, 1].any()


@pytest.mark.parametrize("case", _WIN, ids=_ids(_WIN))
def test_windows(dev, case):
    """1 to 513 windows (bases summed per block up to 32, from the prefix kernel above: one, two and three steps of 256) holding 0 to n
    entries, the first, the middle and the last none; later passes with whole trailing blocks empty"""
    check_raw(dev, case)


@pytest.mark.parametrize("nblk", [b for b in S.SCAN_BLOCKS if b < 3841])
def test_scan_waves(dev, nblk):
    """one window of 256 | 257, 769 and 3,840 blocks: 1, 2 (shares 192 + 65), 4 (the last share one block) and 15 scan waves"""
    check_raw(dev, S.scan_case(nblk))


def test_scan_sixteen_waves(dev):
    """3,841 blocks: the sixteenth wave's share is the one last block, which holds one element"""
    case = S.scan_case(3841)
    codes = case.make()
    S.assert_scan_codes(case, codes)
    check_raw(dev, case, codes)


# ------------------------------------------------------------------------------------------------ term lists
def check_terms(dev, case, modes, want=None):
    """the device's list under each mask mode == the model's"""
    ent, offs, tb = want or case.expected()
    for mode in modes:
        plan, got, goffs = dev.diag_term_list(case.limbs, case.c, case.tabled, case.mask if mode else None, mode)
        assert plan == case.plan(), (case, mode, plan)
        assert goffs[tb] == len(ent) and len(got) == len(ent), (case, mode, int(goffs[tb]), len(ent))
        assert np.array_equal(goffs, offs), (case, mode)
        assert np.array_equal(got, ent), (case, mode, first_difference(got, ent))
    return ent, offs, tb


_PLAN = S.plan_cases()


@pytest.mark.parametrize("case", _PLAN, ids=_ids(_PLAN))
def test_plan_lists(dev, case):
    """plain (batch 3 = 60 windows: the prefix path) and tabled (c = 13 and 24: two and three passes; positions w n + i) lists and
    offsets == the model; on the plain cases the rocPRIM sort (sort_mode 1) gives the same valid list"""
    want = check_terms(dev, case, (0,))
    if not case.tabled:
        try:
            dev.set_option("sort_mode", 1)
            check_terms(dev, case, (0,), want)
        finally:
            dev.set_option("sort_mode", 0)


_MASK = [(n, tabled) for n in S.MASK_N for tabled in (False, True)]


@pytest.mark.parametrize("n,tabled", _MASK, ids=["%s-n%d" % ("tabled" if t else "plain", n) for n, t in _MASK])
def test_filter_is_the_masked_sort(dev, n, tabled):
    """mask mode 2 (full list, then msm_plan_filter) == mask mode 1 (masked in the digit kernel) == the model without the masked
    scalars, for no, every, every other, the first and the last scalar masked; every digit is non-zero, so with tables idx runs through
    q n - 1, q n and q n + 1 for every q"""
    for kind in S.MASK_KINDS:
        case = S.mask_case(n, tabled, kind)
        ent, offs, tb = check_terms(dev, case, (1, 2))
        if kind == "all":
            assert len(ent) == 0 and not offs.any()
        if kind == "none":
            assert len(ent) == case.bound


_FSMALL = [S.filter_small_case(c, n) for c, n, _, _ in S.FILTER_SMALL] + [S.filter_exact_case(x) for x in S.FILTER_EXACT]


@pytest.mark.parametrize("case", _FSMALL, ids=_ids(_FSMALL))
def test_filter_chunk_edges(dev, case):
    """bounds of 2,046 | 2,048 | 2,052 entries (one chunk, one chunk exactly, two) and lists of exactly 2,047 | 2,048 | 2,049"""
    check_terms(dev, case, (1, 2))


_FLARGE = [(n, full) for n, _, _, _ in S.FILTER_LARGE for full in (False, True)]


@pytest.mark.parametrize("n,full", _FLARGE, ids=["n%d-%s" % (n, "full" if f else "u62") for n, f in _FLARGE])
def test_filter_scan_share(dev, n, full):
    """1,024 | 1,025 chunks: the scan's share per wave grows from 64 to 128 chunks.  u62: scalars below 2^62 on a plain key (a quarter
    of the chunks hold entries); full: every digit non-zero with tables, so every chunk does"""
    check_terms(dev, S.filter_large_case(n, full), (2,))
