"""tests/msm_limit_cases.py without a GPU: the model of the signed-digit recoding agrees with integer arithmetic and with a second
implementation that reads 32-bit limbs the way msm_digits_kernel does; every case sits on the boundary it names (chain lengths, item
and chain counts, offsets modulo seg_len, entries below the lane counts of a 256-CU device); and the expected points, which come from
one scalar multiplication each, equal the CPU oracle's MSM over the same arrays wherever that is small enough to run."""
import random

import numpy as np
import pytest

import msm_limit_cases as M
import pyref as P

ORACLE_MSM_MAX = {"g1": 4000, "g2": 1500}            # terms up to which oracle.msm is run on a case

ALL_WIDTHS = sorted(set(M.DIGIT_WIDTHS) | set(M.REDUCE_WIDTHS) | {7, 9, 14, 15})


def kernel_digits(s, c):
    """msm_digits_kernel line by line on 32-bit limbs: -> per window the code (|d| - 1) << 1 | negate, or None for digit 0"""
    limb = [(s >> (32 * k)) & 0xffffffff for k in range(8)] + [0]
    rh = [(M.R_HALF >> (32 * k)) & 0xffffffff for k in range(8)]
    flip = False
    for k in range(7, -1, -1):
        if limb[k] != rh[k]:
            flip = limb[k] > rh[k]
            break
    if flip:
        borrow = 0
        for k in range(8):
            t = (((P.R_MOD >> (32 * k)) & 0xffffffff) - limb[k] - borrow) & ((1 << 64) - 1)
            limb[k] = t & 0xffffffff
            borrow = t >> 63
    out, carry, mask, half = [], 0, (1 << c) - 1, 1 << (c - 1)
    for w in range(254 // c + 1):
        bit = w * c
        v = 0
        if bit < 256:
            two = limb[bit >> 5] | (limb[(bit >> 5) + 1] << 32)
            v = (two >> (bit & 31)) & 0xffffffff & mask
        v += carry
        key, carry = 0, 0
        if v > half:
            mag = (1 << c) - v
            carry = 1
            if mag:
                key = 1 + (((mag - 1) << 1) | (1 ^ int(flip)))
        elif v:
            key = 1 + (((v - 1) << 1) | int(flip))
        out.append(key - 1 if key else None)
    return out


@pytest.mark.parametrize("c", ALL_WIDTHS)
def test_recoding_is_the_scalar(c):
    """sum digit 2^(c w) == s mod r for the boundary scalars of the digit cases and random ones, and the model == the kernel's text"""
    rng = random.Random(c)
    for s in M.digit_scalars(c, 0) + [P.rand_fr(rng) for _ in range(60)]:
        assert M.signed_sum(s, c) == s % P.R_MOD, (c, hex(s))
        model = [None] * M.nwin_of(c)
        for w, b, neg in M.recode(s, c):
            assert 0 <= b < 1 << (c - 1) and model[w] is None
            model[w] = (b << 1) | int(neg)
        assert model == kernel_digits(s, c), (c, hex(s))


def test_digit_cases_hold_what_they_name():
    for c in M.DIGIT_WIDTHS:
        s = M.digit_scalars(c)
        nw, half = M.nwin_of(c), 1 << (c - 1)
        assert 290 <= len(s) <= 420, (c, len(s))
        dig = {}
        for x in s:
            for w, b, neg in M.recode(x, c):
                dig.setdefault(w, set()).add((b + 1, neg))
        # the largest magnitude 2^(c-1) with either sign, in the lowest, a middle and the last full window; a recentred digit (negative
        # for an unflipped scalar) and a carry that makes a digit vanish (all-ones) are there too
        for w in (0, nw // 2, nw - 2):
            assert (half, False) in dig[w] and (half, True) in dig[w], (c, w)
        # every window holds the three boundary values alone in a scalar, and the model recodes them as the kernel's rule says: 2^(c-1)
        # stays, the two above it become d - 2^c with a carry of one into the next window
        have = set(s)
        for w in range(nw):
            for d in (half, half + 1, (1 << c) - 1):
                v = d << (c * w)
                assert v < P.R_MOD or w == nw - 1, (c, w, d)
                if v < P.R_MOD:
                    assert v in have, (c, w, d)
                if v <= M.R_HALF:
                    want = [(w, half - 1, False)] if d == half else [(w, (1 << c) - d - 1, True), (w + 1, 0, False)]
                    assert M.recode(v, c) == want, (c, w, d)
        assert all((d << (c * w)) <= M.R_HALF for w in range(nw - 1) for d in (half, (1 << c) - 1)), c
        ones = M.recode((1 << 253) - 1, c)
        assert ones[0] == (0, 0, True) and all(w >= 253 // c for w, _, _ in ones[1:]), c
        assert M.recode(P.R_MOD - 1, c) == [(0, 0, True)] and M.recode(M.R_HALF + 1, c) == [(w, b, not n) for w, b, n in M.recode(M.R_HALF, c)]


def test_seg_len_rule():
    assert M.seg_lens(1000, 4096, 131072, 65536, 0) == (4, 4)
    assert M.seg_lens(1000, 4096, 131072, 65536, 3) == (3, 3)
    assert M.seg_lens(131072, 64, 131072, 65536, 1) == (1, 2)
    assert M.seg_lens(131073, 64, 131072, 65536, 1) == (2, 3)
    assert M.seg_lens(1 << 20, 1 << 10, 131072, 65536, 0) == (516, 516)
    assert M.lanes("g1", 256) == 131072 and M.lanes("g2", 256) == 65536


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_fixup_cases_sit_on_their_boundaries(group):
    cases = M.fixup_cases(group)
    seen = set()
    for case in cases:
        cl, m = case.claims, case.min_seg
        assert case.entries < M.lanes("g2", M.CUS_MI355X) and case.seg_len() == m, case
        assert len(case.scalars) < 10000, case
        sp = M.spills(case.counts, m)
        longs = sorted((g // 128, g % 128 + 1, last - t) for g, t, last in sp if last - t > M.FIXUP_SHORT)
        designed = sorted(cl["chains"])
        assert longs == [x for x in designed if x[2] > M.FIXUP_SHORT], case
        offs = np.concatenate([[0], np.cumsum(case.counts)])
        for (w, d, diff), n in zip(designed, cl["lengths"]):
            g = w * 128 + d - 1
            assert case.counts[g] == n and (g, int(offs[g]) // m, int(offs[g]) // m + diff) in sp, case
        g0 = designed[0][0] * 128 + designed[0][1] - 1
        if cl["off_mod"] is not None:
            assert int(offs[g0]) % m == cl["off_mod"], case
        if cl["l_mult"] is not None:
            assert (cl["lengths"][0] % m == 0) == cl["l_mult"], case
        if cl["total_mod"] is not None:
            assert case.entries % m == cl["total_mod"], case
        assert M.fixup_queue(case.counts, m) == (cl["items"], cl["nchains"]), case
        st = case.state()
        assert st[:6] == (8, 32, case.entries, m, cl["items"], cl["nchains"]) and st[6:] == (None, None)
        if len(designed) == 1:
            seen.add((m, designed[0][2], int(offs[g0]) % m, cl["lengths"][0] % m == 0, case.entries % m != 0))
    diffs = M.FIXUP_DIFFS if group == "g1" else M.FIXUP_DIFFS_G2
    assert {(m, d) for m, d, _, _, _ in seen} >= {(1, d) for d in diffs}
    if group == "g1":
        assert {(m, d) for m, d, _, _, _ in seen} >= {(3, d) for d in diffs}
        for d in (5, 1025):
            assert {(o, mult) for m, dd, o, mult, _ in seen if m == 3 and dd == d} == {(o, mult) for o in (0, 1, 2) for mult in (True, False)}
        assert any(s[4] for s in seen if s[0] == 3)                # a list whose length is no multiple of seg_len
        multi = [c for c in cases if len(c.claims["chains"]) == 3]
        assert len(multi) == 3 and all((c.claims["items"], c.claims["nchains"]) == (6, 2) for c in multi)
    # the items of the routing rule at its edges
    by_diff = {c.claims["chains"][0][2]: c.claims for c in cases if len(c.claims["chains"]) == 1}
    want = {1: (0, 0), 4: (0, 0), 5: (1, 0), 1024: (1, 0), 1025: (2, 1), 2048: (2, 1), 2049: (3, 1), 3073: (4, 1)}
    for d, (items, chains) in want.items():
        if d in by_diff:
            assert (by_diff[d]["items"], by_diff[d]["nchains"]) == (items, chains), d


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_segment_cases_hold_every_situation(group):
    cases = M.segment_cases(group)
    for case in cases:
        assert case.entries == len(case.scalars) == 61 and case.seg_len() == case.min_seg, case
        facts = M.segment_facts(case.counts, case.min_seg)
        if case.min_seg == 3:
            assert facts == M.SEGMENT_FACTS, (case, M.SEGMENT_FACTS - facts)
        else:
            assert facts >= {"begins at a segment start", "ends at a segment end", "single entry", "short last segment",
                             "spills into a short last segment"}, case
        # the two runs lie inside one segment each, in index order, and at seg_len 6 with the terms that follow them
        terms = M.sorted_terms(case.scalars, 8)
        pos = {}
        for p, (g, i, neg) in enumerate(terms):
            assert not neg
            pos.setdefault(g, []).append((p, int(case.idx[i])))
        for g, third in ((10, M.AB), (11, M.NEG + M.AB)):
            run = pos[g]
            assert [x for _, x in run[:3]] == [M.A, M.B, third] and len(run) == 6
            assert run[0][0] % case.min_seg == 0 and run[0][0] // case.min_seg == run[2][0] // case.min_seg
            if case.min_seg == 6:
                assert run[5][0] // 6 == run[0][0] // 6
        assert M.fixup_queue(case.counts, case.min_seg) == (0, 0)
    variants = {tuple(sorted((k, v) for k, v in c.options.items() if k not in ("window_bits", "min_seg"))) for c in cases}
    need = [(), (("acc_lazy", 0),), (("g1_inline", 2),), (("acc_pipeline", 1),), (("acc_pipeline", 2),), (("acc_pipeline", 3),),
            (("g2_lazy", 2),), (("fixup_aux", 1),)]
    assert variants >= set(need)


def test_reduction_rules_and_cases():
    # mode 5 with a forced chunk: k shrunk while k > 2 and 4 k > nb; bit_sliced = log2(nb / k); no bit slicing below 8 buckets
    assert M.reduce_state(4, 5, 64) == (2, 2) and M.reduce_state(4, 5, 2) == (2, 2) and M.reduce_state(4, 5, 4) == (2, 2)
    assert M.reduce_state(5, 5, 4) == (2, 4) and M.reduce_state(5, 5, 8) == (2, 4) and M.reduce_state(6, 5, 8) == (2, 8)
    assert M.reduce_state(13, 5, 64) == (6, 64) and M.reduce_state(13, 5, 2) == (11, 2) and M.reduce_state(3, 5, 2) == (0, None)
    # mode 1: two levels exactly from 16 chunks on
    assert M.reduce_state(6, 1, 2) == (0, 2) and M.reduce_state(6, 1, 4) == (0, 0) and M.reduce_state(10, 1, 64) == (0, 0)
    assert M.reduce_state(10, 1, 16) == (0, 16) and M.reduce_state(8, 1, 8) == (0, 8) and M.reduce_state(8, 1, 16) == (0, 0)
    assert M.reduce_state(5, 1, 0) == (0, 0) and M.reduce_state(6, 1, 0) == (0, 2) and M.reduce_state(13, 1, 0) == (0, 4)
    sides = set()
    for c in M.REDUCE_WIDTHS:
        for k in M.REDUCE_CHUNKS:
            sides.add(M.reduce_state(c, 1, k)[1] != 0)
            bs, kb = M.reduce_state(c, 5, k)
            if k > 1:
                sides.add(("shrunk", kb < min(k, 64)))
    assert sides == {True, False, ("shrunk", True), ("shrunk", False)}
    for c in M.REDUCE_WIDTHS:
        nb, nw = 1 << (c - 1), M.nwin_of(c)
        for pattern in M.REDUCE_PATTERNS:
            case = M.reduce_case("g1", c, pattern, 8 if pattern == "last-chunk" else 0)
            per = case.counts.reshape(nw, nb)
            assert not per[3:nw - 1].any(), case
            for s in set(case.scalars):                  # one positive digit each: the scalar names its bucket
                (w, b, neg), = M.recode(s, c)
                assert s == (b + 1) << (c * w) and not neg, case
            full = [w for w in (0, 1, 2) if per[w].all()]
            if pattern in ("same", "signs", "two-forms", "two-forms-neg"):
                assert full == [0, 1, 2] and per[nw - 1].any() and len(set(per[0].tolist())) == 1, case
            elif pattern == "window-empty":
                assert full == [0, 2] and not per[1].any(), case
            elif pattern == "bucket0":
                assert per[:, 1:].sum() == 0 and per[0, 0] == 2, case
            elif pattern == "top-bucket":
                assert per[:, :nb - 1].sum() == 0 and per[0, nb - 1] == 2, case
            else:
                k = min(8, nb)
                assert per[:3, :nb - k].sum() == 0 and per[:3, nb - k:].all(), case
    # the two forms: (a, b) and (c, d) are different pairs with one sum
    L = M.LOGS
    assert (L[M.A] + L[M.B] - L[M.C] - L[M.D]) % P.R_MOD == 0 and len({L[M.A], L[M.B], L[M.C], L[M.D]}) == 4
    assert L[M.AB] == (L[M.A] + L[M.B]) % P.R_MOD and all((L[j] + L[M.NEG + j]) % P.R_MOD == 0 for j in range(32))


def _small_cases():
    out = []
    for group in ("g1", "g2"):
        out += [c for c in M.fixup_cases(group) if len(c.scalars) <= ORACLE_MSM_MAX[group]]
        out += M.segment_cases(group)[:2] + M.digit_cases(group)
        widths = M.REDUCE_WIDTHS if group == "g1" else (4, 8)
        out += [M.reduce_case(group, c, p, 8 if p == "last-chunk" else 0) for c in widths for p in M.REDUCE_PATTERNS
                if group == "g1" or (c, p) in M.REDUCE_G2]
    return [c for c in out if len(c.scalars) <= ORACLE_MSM_MAX[c.group]]


def test_expected_points_equal_the_oracle_msm(oracle):
    """the expected point of a case is [sum s_i k_i]G; the oracle's own MSM over the case's bases and scalars must give the same
    bytes (the points of the table really are [k]G, and the sum is the sum)"""
    cases = _small_cases()
    assert len(cases) > 100 and {c.group for c in cases} == {"g1", "g2"}
    for case in cases:
        bases, sc = case.arrays(oracle)
        exp, einf = case.expected(oracle)
        got, ginf = oracle.msm(case.group, bases, sc)
        assert ginf == einf and (einf or np.array_equal(got, exp)), case
    # cases that end on the point at infinity exist among them (P and -P in equal numbers)
    assert any(c.expected_log() == 0 for c in cases)
