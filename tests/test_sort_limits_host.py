"""tests/sort_cases.py without a GPU: every case sits where the table says — blocks per window, scan waves and each wave's share, the
pass bit split, the window-prefix path and the compaction's chunk count, all from the constants copied out of csrc/bucket_sort.hip and
csrc/msm.hip; the model agrees with a brute-force sort of tuples; the vectorised recoding agrees with the integer one."""
import random

import numpy as np
import pytest

import msm_limit_cases as M
import sort_cases as S


def test_constants_are_the_sources():
    """the copied constants against the text of the two sources"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zksnark-finalproject_amd", "csrc")
    with open(os.path.join(csrc, "bucket_sort.hip")) as f:
        bs = f.read()
    with open(os.path.join(csrc, "msm.hip")) as f:
        ms = f.read()
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    waves, rounds = const(bs, "SORT_WAVES"), const(bs, "SORT_ROUNDS")
    assert (64, 64 * rounds, 64 * rounds * waves) == (S.SORT_ROUND, S.SORT_WCH, S.SORT_BCH)
    assert const(bs, "SORT_MAX_BITS") == S.SORT_MAX_BITS and const(bs, "SORT_PREFIX_WINDOWS") == S.SORT_PREFIX_WINDOWS
    assert "bbits > %d" % S.SORT_MAX_BUCKET_BITS in bs and "w0 += 64 * SORT_WAVES" in bs and 64 * waves == S.SORT_PREFIX_STEP
    assert "nblk <= 256 ? 1u : nblk >= 4096 ? 16u : (nblk + 255u) / 256u" in bs
    assert const(ms, "FILTER_CHUNK") == S.FILTER_CHUNK and "((nblk + 15u) / 16u + 63u) & ~63u" in ms


def test_geometry_cases_sit_on_the_chunk_edges():
    ns = set(S.GEOMETRY_N)
    for edge in (S.SORT_ROUND, S.SORT_WCH, S.SORT_BCH):
        assert {edge - 1, edge, edge + 1} <= ns
    assert {1, 2 * S.SORT_BCH + 1} <= ns and S.blocks_per_window(2 * S.SORT_BCH + 1) == 3
    cases = S.geometry_cases()
    assert {c.claims["pattern"] for c in cases} == set(S.GEOMETRY_PATTERNS)
    for case in cases:
        codes = case.make()
        valid = codes[0] != S.NONE
        p = case.claims["pattern"]
        if p == "one-bucket":
            assert valid.all() and len(set(codes[0].tolist())) == 1
        elif p == "descending":
            b = (codes[0] >> 1).astype(np.int64)
            assert valid.all() and (np.diff(b[:128]) == -1).all() and (case.n != 128 or sorted(b.tolist()) == list(range(128)))
        elif p == "alternate-neg":
            assert ((codes[0] & 1) == (np.arange(case.n) & 1)).all()
        elif p == "all-none":
            assert not valid.any()
        elif p == "none-block":
            blk = case.claims["block"]
            per_block = [int(valid[i:i + S.SORT_BCH].sum()) for i in range(0, case.n, S.SORT_BCH)]
            assert per_block[blk] == 0 and all(x > 0 for j, x in enumerate(per_block) if j != blk)
        elif p == "last-only":
            assert valid.sum() == 1 and valid[-1]
    assert {c.n for c in cases if c.claims["pattern"] == "none-block"} == {S.SORT_BCH + 1, 2 * S.SORT_BCH + 1}


def test_split_cases_cover_every_pass_width():
    assert {c: S.pass_bits(c) for c in S.SPLIT_WIDTHS} == S.SPLIT_WIDTHS
    assert S.pass_bits(S.REFUSED_C - 1) == [8, 8, 8] and S.REFUSED_C - 1 > S.SORT_MAX_BUCKET_BITS and S.REFUSED_C - 2 == S.SORT_MAX_BUCKET_BITS
    assert S.blocks_per_window(S.SPLIT_N) == 2
    cases = S.split_cases()
    for c, bits in S.SPLIT_WIDTHS.items():
        mine = [k for k in cases if k.c == c]
        assert sorted(k.claims["only_pass"] for k in mine if "only_pass" in k.claims) == [p for p, b in enumerate(bits) if b]
    for case in cases:
        codes = case.make()
        b = (codes[0][codes[0] != S.NONE] >> 1).astype(np.int64)
        assert b.max() < 1 << (case.c - 1)
        if case.name.endswith("extremes"):
            assert set(b.tolist()) == {0, (1 << (case.c - 1)) - 1}
        if "only_pass" in case.claims:
            bits, p = case.claims["bits"], case.claims["only_pass"]
            field = ((1 << bits[p]) - 1) << sum(bits[:p])
            assert len(set((b & ~field).tolist())) == 1 and len(set((b & field).tolist())) == min(1 << bits[p], len(set(b.tolist())))
            assert len(set(b.tolist())) > 1


def test_window_cases_take_both_base_paths_and_leave_blocks_empty():
    assert [S.prefix_path(nw) for nw in S.WINDOW_COUNTS] == [False, False, True, True, True, True]
    steps = [-(-nw // S.SORT_PREFIX_STEP) for nw in S.WINDOW_COUNTS]
    assert steps == [1, 1, 1, 1, 2, 3]                   # the prefix kernel's loop: one step, one step exactly full, two, three
    for case in S.window_cases():
        codes = case.make()
        kept = (codes != S.NONE).sum(axis=1)
        assert kept.tolist() == S.window_kept(case.nwin, case.n) and case.claims["prefix"] == S.prefix_path(case.nwin)
        if case.nwin >= 3:
            assert kept[0] == kept[case.nwin // 2] == kept[-1] == 0
        if case.nwin >= 9:
            assert kept.max() == case.n and len(set(kept.tolist())) >= 4
        if case.nwin >= 9:
            # later passes: a window with in_count[w] entries runs ceil(in_count / 4096) blocks, the grid has blocks_per_window(n)
            later = [S.blocks_per_window(int(k)) for k in kept]
            assert 0 in later and 1 in later and max(later) == S.blocks_per_window(case.n)
    three = [c for c in S.window_cases() if len(S.pass_bits(c.c)) == 3]
    assert {c.claims["prefix"] for c in three} == {True, False} and all(S.blocks_per_window(c.n) == 3 for c in three)


@pytest.mark.parametrize("nblk", S.SCAN_BLOCKS)
def test_scan_cases_sit_on_the_wave_counts(nblk):
    waves, sizes = S.SCAN_SHARES[nblk]
    shares, per = S.scan_shares(nblk)
    assert S.scan_waves(nblk) == waves and [hi - lo for lo, hi in shares] == sizes and per % 64 == 0
    case = S.scan_case(nblk)
    assert S.blocks_per_window(case.n) == nblk and case.n % S.SORT_BCH == 1 and S.pass_bits(case.c) == [1, 1]
    assert case.n * case.nwin > 1 << 20 or nblk <= 257
    if nblk > 769:
        return                                           # the large codes are looked at once, in the GPU test
    S.assert_scan_codes(case, case.make())


def test_scan_share_rule():
    assert S.scan_waves(256) == 1 and S.scan_waves(257) == 2 and S.scan_waves(3840) == 15 and S.scan_waves(3841) == 16
    assert S.scan_waves(4096) == 16 and S.scan_waves(49000) == 16
    for nblk in (1, 64, 65, 256, 257, 512, 513, 769, 3840, 3841, 4096, 4097, 49000):
        shares, per = S.scan_shares(nblk)
        assert shares[0][0] == 0 and shares[-1][1] == nblk and all(a[1] == b[0] for a, b in zip(shares, shares[1:]))


def test_term_cases_sit_on_their_paths():
    plans = {c.name: c for c in S.plan_cases()}
    assert plans["plain-c13-batch1"].plan() == (13, 20, 20, 20 << 12) and plans["plain-c13-batch3"].plan() == (13, 60, 20, 60 << 12)
    assert not S.prefix_path(20) and S.prefix_path(60)
    assert plans["tabled-c24-batch3"].plan() == (24, 3, 11, 3 << 23) and S.pass_bits(24) == [8, 8, 7] and S.pass_bits(13) == [6, 6]
    assert plans["tabled-c13-batch1"].plan() == (13, 1, 20, 1 << 12)
    big = 80660
    assert big in S.MASK_N and big * 13 > 1 << 20 >= (big - 1) * 13 and {3, 1000, 4097} <= set(S.MASK_N)
    for n in S.MASK_N:                                   # where filter_keep's correction is needed at all: only ever i = n, at idx = q n
        miss = S.quotient_estimate_misses(n, M.nwin_of(S.MASK_C))
        assert bool(miss) == (n in S.MASK_N_ESTIMATE_OFF) and all(i == n and idx % n == 0 for idx, i in miss.items())
    assert S.scan_waves(S.blocks_per_window(big * 20)) == 2            # tabled: one window of n * 20 terms
    for c, n, bound, chunks in S.FILTER_SMALL:
        assert n * M.nwin_of(c) == bound and S.filter_chunks(bound) == chunks
    assert [b for _, _, b, _ in S.FILTER_SMALL] == [2046, 2048, 2052]
    for c in range(2, 25):                               # no width reaches 2,047 or 2,049
        assert 2047 % M.nwin_of(c) and 2049 % M.nwin_of(c)
    for length in S.FILTER_EXACT:
        case = S.filter_exact_case(length)
        assert case.bound == 2080 and S.filter_chunks(case.bound) == 2 and sum(int((cv != S.NONE).sum()) for cv in case.codes) == length
    for n, bound, chunks, share in S.FILTER_LARGE:
        assert n * 20 == bound and S.filter_chunks(bound) == chunks and S.filter_share(chunks) == share
    assert [c for _, _, c, _ in S.FILTER_LARGE] == [1024, 1025] and S.FILTER_LARGE[0][1] <= 1 << 21 < S.FILTER_LARGE[1][1]


def test_nonzero_digit_scalars_fill_every_position():
    for n, c in ((3, 13), (1000, 13), (93, 12), (64, 8), (108, 14)):
        limbs, codes = S.nonzero_vector(n, c)
        assert codes.shape == (M.nwin_of(c), n) and (codes != S.NONE).all() and {0, 1} == set((codes & 1).ravel().tolist())
        # every position w * n + i of the tabled list is an entry, so q n - 1, q n and q n + 1 are entries for every q = 1 .. digits - 1
        ent, _, _ = S.model_term_list([codes], c, True)
        assert sorted((ent[:, 0] >> 1).tolist()) == list(range(n * M.nwin_of(c)))


def test_model_is_a_brute_force_sort():
    small = [c for c in S.geometry_cases() if c.n <= 1025] + [c for c in S.split_cases() if c.c in (2, 3, 12, 22)]
    small += [S.RawCase("win-small", 8, 5, 300, S._window_fill), S.RawCase("win-small-3pass", 22, 4, 300, S._window_fill)]
    assert len(small) > 50
    for case in small:
        codes = case.make()
        ent, tot = S.model_sort(codes, case.c)
        assert [tuple(e) for e in ent.tolist()] == S.brute_sort(codes, case.c), case
        assert tot.tolist() == (codes != S.NONE).sum(axis=1).tolist()
        tb = case.nwin << (case.c - 1)
        if tb <= 1 << 12:
            offs = S.model_offsets(ent, tb)
            assert offs.tolist() == [sum(1 for y in ent[:, 1].tolist() if y < g) for g in range(tb + 1)]


def test_model_term_list_is_the_sorted_terms_of_the_msm_model():
    """the list of a plain and of a tabled key against msm_limit_cases.sorted_terms (bucket, then index), masked scalars removed"""
    c, n = 8, 40
    rng = random.Random(8)
    s = (S.boundary_scalars() + [rng.randrange(M.R) for _ in range(n)])[:n]
    codes = S.codes_from_ints(s, c)
    mask = S.mask_of("alternate", n)
    kept = [0 if mask[i] else x for i, x in enumerate(s)]
    nb, nw = 1 << (c - 1), M.nwin_of(c)
    for m, scal in ((None, s), (mask, kept)):
        ent, offs, tb = S.model_term_list([codes], c, False, m)
        want = M.sorted_terms(scal, c)
        assert [(int(y), int(x) >> 1, bool(x & 1)) for x, y in ent.tolist()] == want and tb == nb * nw and offs[tb] == len(want)
        ent, offs, tb = S.model_term_list([codes], c, True, m)
        flat = sorted(((g % nb, (g // nb) * n + i, neg) for g, i, neg in want), key=lambda t: (t[0], t[1]))
        assert [(int(y), int(x) >> 1, bool(x & 1)) for x, y in ent.tolist()] == flat and tb == nb


def test_vectorised_recoding_is_the_integer_one():
    rng = random.Random(62)
    for c in (2, 3, 8, 12, 13, 14, 16, 20, 24):
        small = [0, 1, (1 << 62) - 1, 1 << 61] + [rng.randrange(1 << 62) for _ in range(1200)]
        wide = [(1 << 253) - 1, 1 << 252] + [rng.randrange(1 << 253) for _ in range(300)]
        want = S.codes_from_ints(small, c)
        assert np.array_equal(S.codes_from_limbs(np.asarray(small, dtype=np.uint64), c), want)
        assert np.array_equal(S.codes_from_limbs(M.canon_vec(small), c), want)
        assert np.array_equal(S.codes_from_limbs(M.canon_vec(wide), c), S.codes_from_ints(wide, c))
    for n, c in ((1000, 13), (93, 12)):
        limbs, ints = S.nonzero_digit_scalars(n, c, "check")
        assert np.array_equal(S.codes_from_limbs(limbs, c), S.codes_from_ints(ints, c))
