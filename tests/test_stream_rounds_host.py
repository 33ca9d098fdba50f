"""tests/stream_cases.py without a GPU: the model's slices are the ones matrix_stream_start picks (zkg16_matrix_stream_bounds, the
function the proof itself calls), the defaults are the slices the library has always run, the layout is the circuit's, every round
case holds in the bucket it names the coincidence it names, its rounds add up to the one-round sum, and its expected point is the CPU
oracle's own MSM over the same arrays."""
import ctypes as C

import numpy as np
import pytest

import msm_limit_cases as M
import stream_cases as S

BAD_ARG = 1
SIZES = (2, 3, 4, 5, 8, 33, 46, 91, 128, 1024)
KINDS = {"skip", "into-inf", "double", "cancel", "add"}


@pytest.fixture(scope="module")
def lib():
    import zksnark_finalproject_amd as z
    return z.load()


def lib_bounds(lib, n, parts_wanted, slice_min):
    out = np.full(9, 0x5a5a5a5a, dtype=np.uint32)
    k = C.c_int(-1)
    assert lib.zkg16_matrix_stream_bounds(n, parts_wanted, slice_min, out.ctypes.data, C.byref(k)) == 0
    assert 1 <= k.value <= 8 and not out[k.value + 1:].any()
    return out[:k.value + 1].tolist()


@pytest.mark.parametrize("n", SIZES)
def test_bounds_are_the_library_s(lib, n):
    perms = (n * n + 1) // 2
    assert S.Layout(n).perms == perms
    for parts_wanted in range(9):
        for slice_min in (1, 512):
            b = S.slice_bounds(perms, parts_wanted, slice_min)
            assert b == lib_bounds(lib, n, parts_wanted, slice_min), (n, parts_wanted, slice_min)
            assert b[0] == 0 and b[-1] == perms and all(x < y for x, y in zip(b, b[1:])), (n, parts_wanted, slice_min, b)
            growing = parts_wanted == 0 and perms >= 4096
            assert growing or all(y - x >= min(slice_min, perms) for x, y in zip(b, b[1:]))
            if parts_wanted and slice_min == 1:
                assert len(b) - 1 == min(parts_wanted, perms)
        # 0 reads as the default floor
        assert lib_bounds(lib, n, parts_wanted, 0) == lib_bounds(lib, n, parts_wanted, 512)


def test_default_slices_are_pinned(lib):
    """the slices that run when no option is set: what `perms / k < 512` has always given"""
    d = lambda n: lib_bounds(lib, n, 0, 0)
    assert d(8) == [0, 32] and d(33) == [0, 545]
    assert d(46) == [0, 529, 1058]                                   # "matrix_parts = 8" at 46x46 runs these two as well
    assert lib_bounds(lib, 46, 8, 0) == [0, 529, 1058] and lib_bounds(lib, 46, 3, 0) == [0, 529, 1058]
    assert d(128) == [0, 492, 1638, 3686, 6554, 8192]                # five growing slices: 6, 20, 45, 80, 100 %
    assert d(91) == [0, 248, 828, 1863, 3313, 4141]                  # 4,141 permutations: just above the 4,096 they start at
    assert d(90) == [0, 1012, 2025, 3037, 4050]                      # 4,050: four equal ones
    assert d(1024) == [0, 31457, 104858, 235930, 419430, 524288]
    assert lib_bounds(lib, 128, 8, 0) == [1024 * i for i in range(9)] and lib_bounds(lib, 128, 1, 0) == [0, 8192]
    # the sizes the device tests run under a floor of one permutation
    assert lib_bounds(lib, 4, 8, 1) == list(range(9))                # every slice a single permutation
    assert lib_bounds(lib, 5, 8, 1) == [0, 1, 3, 4, 6, 8, 9, 11, 13]  # 13 permutations, uneven
    assert lib_bounds(lib, 3, 8, 1) == [0, 1, 2, 3, 4, 5]            # five permutations: the count is lowered to 5
    assert lib_bounds(lib, 2, 8, 1) == [0, 1, 2]


def test_bounds_argument_edges(lib):
    out = np.full(9, 7, dtype=np.uint32)
    k = C.c_int(-1)
    p = out.ctypes.data
    for args in ((1, 0, 0, p, C.byref(k)), (1025, 0, 0, p, C.byref(k)), (8, -1, 0, p, C.byref(k)), (8, 9, 0, p, C.byref(k)), (8, 0, -1, p, C.byref(k)),
                 (8, 0, (1 << 20) + 1, p, C.byref(k)), (8, 0, 0, None, C.byref(k)), (8, 0, 0, p, None)):
        assert lib.zkg16_matrix_stream_bounds(*args) == BAD_ARG, args[:3]
    assert (out == 7).all() and k.value == -1
    assert lib.zkg16_matrix_stream_bounds(8, 8, 1 << 20, p, C.byref(k)) == 0 and k.value == 1


@pytest.mark.parametrize("n", SIZES)
def test_layout_is_the_circuit_s(n):
    from zksnark_finalproject_amd.device import matrix_variables
    L = S.Layout(n)
    assert L.total == matrix_variables(n)
    assert L.total == 4 + 3 * L.nn + L.nn * (n + 1) + 3 * L.hw and L.hw == 265 * L.perms - 5


@pytest.mark.parametrize("n,parts_wanted", [(2, 8), (3, 8), (4, 8), (5, 3), (5, 8), (8, 2), (33, 0)])
def test_part_map_holds_what_it_says(n, parts_wanted):
    L = S.Layout(n)
    b = S.slice_bounds(L.perms, parts_wanted, 1 if parts_wanted else 512)
    part = S.part_map(n, b)
    slices = len(b) - 1
    assert part.shape == (L.total + 3,) and part[0] == 0 and (part[1:4] == slices).all() and not part[L.total:].any()
    assert not part[L.off_a:L.off_ha].any() and not part[L.off_mc:L.off_hc].any()
    for off in (L.off_ha, L.off_hb, L.off_hc):
        seg = part[off:off + L.hw].astype(int)
        assert seg[0] == 1 and seg[-1] == slices and (np.diff(seg) >= 0).all() and set(seg.tolist()) == set(range(1, slices + 1))
        # slice s begins where its first permutation's values begin: 265 p - 5, the first permutation being five values short
        for s in range(1, slices):
            first = int(np.argmax(seg == 1 + s))
            assert first == 265 * b[s] - 5, (n, s)
    # every part but the first holds 265 values per permutation and sponge (260 for permutation 0), the last one the hashes too
    counts = np.bincount(part[:L.total], minlength=slices + 1)
    for s in range(slices):
        assert counts[1 + s] == 3 * (265 * (b[s + 1] - b[s]) - (5 if s == 0 else 0)) + (3 if s == slices - 1 else 0)


# ------------------------------------------------------------------------------------------------ round cases
_CASES = S.round_cases("g1") + S.round_cases("g2")


def test_round_case_list_is_complete():
    names = {c.name for c in _CASES}
    assert len(names) == len(_CASES)
    for group in ("g1", "g2"):
        for what in ("equal-forms", "affine-ab", "cancel-then-add", "last-round-only", "first-round-only", "first-round-empty", "middle-round-empty",
                     "label-unused", "all-in-part-0-of-4", "all-in-part-2-of-4", "eight-rounds", "windows-c4", "windows-c8"):
            assert "%s-%s" % (group, what) in names
    assert {"g1-spill-%d-aux%d" % (n, a) for n in S.SPILL_TERMS for a in (0, 1)} <= names and not any("g2-spill" in x for x in names)
    seen = {k for c in _CASES for _, _, kinds in c.claims for k in kinds}
    assert seen == KINDS


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_round_case_sits_where_it_claims(case):
    sums = case.round_sums()
    nb = case.nb
    for w, d, kinds in case.claims:
        g = w * nb + d - 1
        assert set(kinds) <= KINDS and len(kinds) == case.parts - 1
        assert case.merge_kinds(g) == kinds, (case, w, d, case.merge_kinds(g))
        # the claimed bucket holds nothing but the terms the case put there
        placed = sum(1 for s in case.scalars if s == S.term(case.c, w, d))
        assert sum(int(case.round_counts(k)[g]) for k in range(case.parts)) == placed > 0
    if case.claims:
        # ... and every other bucket holds a single term: what the case is about happens in the buckets it names, nowhere else
        named = {w * nb + d - 1 for w, d, _ in case.claims}
        total = sum(case.round_counts(k) for k in range(case.parts))
        assert all(int(total[g]) == 1 for g in np.flatnonzero(total) if g not in named) and len(np.flatnonzero(total)) > 300
    # the coincidences as facts about the integers, for the cases the issue names
    L = M.LOGS
    if case.name.endswith("equal-forms"):
        g = 0 * nb + 76
        assert sums[0][g] == sums[1][g] == (L[M.A] + L[M.B]) % S.R != 0 and case.round_counts(0)[g] == case.round_counts(1)[g] == 2
    if case.name.endswith("affine-ab"):
        assert sums[0][76] == sums[1][76] == L[M.AB] and case.round_counts(0)[76] == 2 and case.round_counts(1)[76] == 1
        assert (sums[0][5 * nb] + sums[1][5 * nb]) % S.R == 0 != sums[0][5 * nb]
    if case.name.endswith("cancel-then-add"):
        assert (sums[0][76] + sums[1][76]) % S.R == 0 and sums[2][76] == L[M.PLAIN[1]] and sums[0][nb + 2] == 0 and case.round_counts(0)[nb + 2] == 2
    if case.name.endswith("last-round-only"):
        assert 76 not in sums[0] and 76 not in sums[1] and 76 in sums[2]
    if case.name.endswith("first-round-only"):
        assert 76 in sums[0] and 76 not in sums[1] and 76 not in sums[2] and sums[1][4 * nb + 4] == 0
    entries = case.round_entries()
    if case.name.endswith("first-round-empty"):
        assert entries[0] == 0 and min(entries[1:]) > 0
    if case.name.endswith("middle-round-empty"):
        assert entries[1] == 0 and entries[0] > 0 and entries[2] > 0
    if case.name.endswith("label-unused"):
        assert entries[3] == 0 and min(entries[:3]) > 0 and 3 not in case.part
    if "all-in-part" in case.name:
        k = int(case.name.split("-")[4])
        assert set(case.part.tolist()) == {k} and [e > 0 for e in entries] == [j == k for j in range(4)]
    if case.name.endswith("eight-rounds"):
        assert all(sums[k][76] == L[M.REP] for k in range(8)) and all(e > 0 for e in entries)
    if "windows" in case.name:
        assert all(e > 0 for e in entries) and {w for s in case.scalars for w, _, _ in M.recode(s, case.c)} == set(range(M.nwin_of(case.c)))
        # random labels meet in buckets: every kind of ordinary merge happens somewhere
        kinds = {k for g in range(case.tb) for k in case.merge_kinds(g)} if case.c == 4 else {"add"}
        assert "add" in kinds
    if case.spill:
        # round 1's list is the one bucket: at seg_len 1 (min_seg 1, far fewer entries than lanes on any device) it runs over `diff`
        # further lanes, and the fix-up queue gets the items the model of msm_limit_cases counts
        k, g, diff = case.spill["round"], case.spill["bucket"], case.spill["diff"]
        counts = case.round_counts(k)
        assert case.options["min_seg"] == 1 and k >= 1 and entries[k] == diff + 1 < 8 * 4 * 64
        assert M.seg_lens(entries[k], case.tb, 8 * 4 * 2 * 64, 8 * 4 * 64, 1) == (1, 1)
        assert M.spills(counts, 1) == [(g, 0, diff)]
        assert M.fixup_queue(counts, 1) == ((diff + M.FIXUP_ITEM - 1) // M.FIXUP_ITEM if diff > M.FIXUP_SHORT else 0, int(diff > M.FIXUP_ITEM))
        assert case.round_counts(0)[g] == 1


@pytest.mark.parametrize("case", _CASES, ids=[c.name for c in _CASES])
def test_rounds_add_up_to_the_one_round_sum(case):
    """the merged bucket array, weighted as the reduction weights it, is sum s_i k_i; so is one round over every scalar; and the
    entries of the rounds are the entries of the whole"""
    sums = case.round_sums()
    assert sum(case.weighted(s) for s in sums) % S.R == case.expected_log()
    merged = {}
    for s in sums:
        for g, v in s.items():
            merged[g] = (merged.get(g, 0) + v) % S.R
    one = S.RoundCase("one", case.group, case.c, case.scalars, case.idx, [0] * len(case.scalars), 1)
    assert merged == one.round_sums()[0] and case.weighted(merged) == case.expected_log()
    assert sum(case.round_entries()) == one.round_entries()[0] == int(M.bucket_counts(case.scalars, case.c).sum())
    assert all(M.signed_sum(s, case.c) == s for s in case.scalars)


def test_expected_points_equal_the_oracle_msm(oracle):
    ran = 0
    for case in _CASES:
        if len(case.scalars) > (4000 if case.group == "g1" else 1500):
            continue
        bases, sc = case.arrays(oracle)
        exp, einf = case.expected(oracle)
        got, ginf = oracle.msm(case.group, bases, sc)
        assert ginf == einf and (einf or np.array_equal(got, exp)), case
        ran += 1
    assert ran == len(_CASES)
