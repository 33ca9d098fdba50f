"""tests/msm_tabled_cases.py without a GPU: the tabled model's term list equals a brute-force stable sort of (bucket, position); every
case sits on the boundary it names (segment facts, chain lengths, item and chain counts, bucket counts per pattern, the reduction
thresholds on both sides); the expected points, which come from one scalar multiplication each, equal the CPU oracle's MSM over the
same arrays wherever that is small enough to run; and the expected table entries are what c doublings of the level below give."""
import numpy as np
import pytest

import msm_limit_cases as M
import msm_tabled_cases as T
import pyref as P

ORACLE_MSM_MAX = {"g1": 4000, "g2": 1500}            # terms up to which oracle.msm is run on a case


def brute_terms(vectors, c):
    """every (vector, scalar, level) cell in input order, dropped where the digit is zero, then a stable sort by bucket alone: inside a
    bucket the order of the cells, level after level, index after index — the position order"""
    nb, n = 1 << (c - 1), len(vectors[0])
    cells = []
    for v, vec in enumerate(vectors):
        digits = [{w: (b, neg) for w, b, neg in M.recode(s, c)} for s in vec]
        for w in range(M.nwin_of(c)):
            for i in range(n):
                if w in digits[i]:
                    b, neg = digits[i][w]
                    cells.append((((w * n + i) << 1) | int(neg), v * nb + b))
    order = np.argsort(np.asarray([y for _, y in cells], dtype=np.int64), kind="stable")
    return [cells[k] for k in order.tolist()]


def test_term_list_is_a_stable_sort():
    cases = [T.segment_case("g1", (), 3, 1), T.digit_case("g1", 13), T.digit_case("g1", 24), T.fixup_case("g1", [(77, 5)], 3, "distinct"),
             T.reduce_case("g1", 8, "two-forms"), T.batch_cases()[2]]
    for case in cases:
        want = brute_terms(case.vectors, case.c)
        got = T.terms_tabled(case.vectors, case.c)
        assert got == want, case
        nb = 1 << (case.c - 1)
        assert np.array_equal(np.bincount([y for _, y in got], minlength=nb * case.batch), case.counts), case
        assert all(x >> 1 < M.nwin_of(case.c) * case.n for x, _ in got)
    # a batch: vector v owns the buckets [v nb, (v + 1) nb), and its list is the single vector's list shifted there
    b = T.batch_cases()[2]
    nb = 1 << (b.c - 1)
    for v, vec in enumerate(b.vectors):
        alone = [(x, y + v * nb) for x, y in T.terms_tabled([vec], b.c)]
        assert alone == [e for e in T.terms_tabled(b.vectors, b.c) if e[1] // nb == v]
    assert b.batch == 3 and not b.counts[nb:2 * nb].any() and np.array_equal(b.counts[:nb], b.counts[2 * nb:])


def test_extra_points_and_levels(oracle):
    """Q, Q-, R are what their names say, by two routes: the logs, and the oracle's scalar multiplication of P itself; level w of a
    table entry is level w - 1 multiplied by 2^c"""
    for c in (8, 13):
        lg = T.logs_ext(c)
        assert lg[T.Q] == (M.LOGS[T.TP] << c) % P.R_MOD and (lg[T.Q] + lg[T.QN]) % P.R_MOD == 0 and lg[T.RR] == (lg[T.Q] << c) % P.R_MOD
        assert len(set(lg)) == 67
        for group in ("g1", "g2"):
            pts = T.points(oracle, group, c)
            two_c = M.canon_vec([1 << c])[0]
            q, qinf = oracle.point_mul(group, pts[T.TP], two_c)
            assert not qinf and np.array_equal(q, pts[T.Q])
            r, rinf = oracle.point_mul(group, q, two_c)
            assert not rinf and np.array_equal(r, pts[T.RR])
            s, sinf = oracle.point_add(group, pts[T.Q], pts[T.QN])
            assert sinf == 1
    for group, c in (("g1", 2), ("g1", 13), ("g1", 24), ("g2", 8)):
        lv = T.level_points(oracle, group, c)
        assert lv.shape[:2] == (M.nwin_of(c), 64) and np.array_equal(lv[0], M.table(oracle, group))
        two_c = M.canon_vec([1 << c])[0]
        for w, j in ((1, 0), (1, 37), (2, T.TP), (M.nwin_of(c) - 1, 63), (M.nwin_of(c) // 2, 9)):
            up, inf = oracle.point_mul(group, lv[w - 1, j], two_c)
            assert not inf and np.array_equal(up, lv[w, j]), (group, c, w, j)
    # the expected table of a case: the input at level 0, infinity where the base is
    case = T.table_case("g1", 13, 67, 1)
    tab, tinf = T.expected_table(oracle, case)
    bases, inf, _ = case.arrays(oracle)
    assert inf.tolist().count(1) == 3 and inf[0] and inf[33] and inf[66]
    assert np.array_equal(tab[0][inf == 0], bases[inf == 0]) and not tab[:, inf != 0].any() and tinf.shape == (20, 67)
    assert T.table_case("g1", 2, 1, 1).inf.tolist() == [1] and T.table_case("g1", 2, 1, 1, with_inf=False).inf.tolist() == [0]


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_segment_cases_hold_every_situation(group):
    cases = T.segment_cases(group)
    assert {(c.stride, c.min_seg) for c in cases} == {(1, 3), (1, 6), (2, 3), (2, 6)}
    variants = {tuple(sorted((k, v) for k, v in c.options.items() if k != "min_seg")) for c in cases}
    assert variants >= {(), (("acc_lazy", 0),), (("g1_inline", 2),), (("acc_pipeline", 1),), (("acc_pipeline", 2),), (("acc_pipeline", 3),),
                        (("g2_lazy", 2),), (("fixup_aux", 1),)}
    nterms = sum(len(ts) for _, ts in T.SEGMENT_LAYOUT)
    for case in cases[:4]:
        assert case.entries == case.n == nterms == 64 and case.seg_len() == case.min_seg, case
        assert not case.counts[128:].any() and len(case.counts) == 128
        facts = M.segment_facts(case.counts, case.min_seg)
        if case.min_seg == 3:
            assert facts == M.SEGMENT_FACTS, (case, M.SEGMENT_FACTS - facts)
        else:
            assert facts >= {"begins at a segment start", "ends at a segment end", "single entry", "short last segment",
                             "spills into a short last segment"}, case
        assert M.fixup_queue(case.counts, case.min_seg) == (0, 0)
        # the sorted list holds the layout as written: bucket after bucket, the terms of a bucket by level, then in the order given
        terms = T.terms_tabled(case.vectors, 8)
        got = {}
        for x, y in terms:
            assert not x & 1
            w, i = divmod(x >> 1, case.n)
            got.setdefault(y + 1, []).append((w, int(case.idx[i])))
        assert got == dict(T.SEGMENT_LAYOUT), case
    # the runs: a bucket whose partial sum is Q in a non-trivial form when level 1 of P arrives, one that holds Q- when it does, one
    # that holds R when level 2 of P does, buckets fed from the top level alone, buckets of three and more levels
    lay = dict(T.SEGMENT_LAYOUT)
    lg = T.logs_ext(8)
    part = lambda d, k: sum(lg[pt] << (8 * w) for w, pt in lay[d][:k]) % P.R_MOD
    assert part(11, 4) == lg[T.Q] == (lg[T.TP] << 8) % P.R_MOD and lay[11][4] == (1, T.TP) and len(lay[11]) > 5
    assert all(part(11, k) not in (0, lg[T.Q]) for k in (2, 3))
    assert part(12, 1) == lg[T.QN] and lay[12][1] == (1, T.TP) and part(12, 2) == 0 and len(lay[12]) > 2
    assert part(13, 1) == lg[T.RR] == (lg[T.TP] << 16) % P.R_MOD and lay[13][1] == (2, T.TP)
    assert [d for d, ts in T.SEGMENT_LAYOUT if {w for w, _ in ts} == {31}] == [4, 9]
    assert max(len({w for w, _ in ts}) for ts in lay.values()) >= 8


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_fixup_cases_sit_on_their_boundaries(group):
    cases = T.fixup_cases(group)
    seen = set()
    for case in cases:
        cl, m = case.claims, case.min_seg
        assert case.entries < M.lanes("g2", M.CUS_MI355X) and case.seg_len() == m, case
        assert case.n < 1000 and case.batch * case.n * 32 < 1 << 25, case
        sp = M.spills(case.counts, m)
        longs = sorted((g + 1, last - t) for g, t, last in sp if last - t > M.FIXUP_SHORT)
        assert longs == [x for x in cl["chains"] if x[1] > M.FIXUP_SHORT], case
        offs = np.concatenate([[0], np.cumsum(case.counts)])
        for (d, diff), n in zip(cl["chains"], cl["lengths"]):
            assert case.counts[d - 1] == n and (d - 1, int(offs[d - 1]) // m, int(offs[d - 1]) // m + diff) in sp, case
            # deep by construction: the bucket's terms come from 31 levels, about n / 31 scalars each
            lv = np.bincount([(x >> 1) // case.n for x, y in T.terms_tabled(case.vectors, 8) if y == d - 1], minlength=32)
            assert lv[31] == 0 and (n < 31 or lv[:31].all()) and lv.max() - lv[:31].min() <= 2, case
        assert M.fixup_queue(case.counts, m) == (cl["items"], cl["nchains"]), case
        assert case.state()[:6] == (8, 1, case.entries, m, cl["items"], cl["nchains"])
        if len(cl["chains"]) == 1:
            seen.add((m, cl["chains"][0][1], case.stride))
        if case.name.endswith("-bare"):
            assert case.expected_logs() == [0] and case.entries == cl["lengths"][0]
            # P and -P in equal numbers in every level
            for w in range(31):
                ks = [T.logs_ext(8)[case.idx[i]] for i, s in enumerate(case.vectors[0]) if (s >> (8 * w)) & 255]
                assert sum(ks) % P.R_MOD == 0 and len(ks) % 2 == 0
    assert seen >= {(m, d, 1) for m in (1, 3) for d in T.FIXUP_DIFFS[group]} | {(3, d, 2) for d in T.FIXUP_STRIDE2}
    by_diff = {c.claims["chains"][0][1]: c.claims for c in cases if len(c.claims["chains"]) == 1}
    want = {4: (0, 0), 5: (1, 0), 1024: (1, 0), 1025: (2, 1), 2049: (3, 1)}
    for d, (items, chains) in want.items():
        if d in by_diff:
            assert (by_diff[d]["items"], by_diff[d]["nchains"]) == (items, chains), d
    if group == "g1":
        multi = [c for c in cases if len(c.claims["chains"]) == 3]
        assert len(multi) == 3 and all((c.claims["items"], c.claims["nchains"]) == (6, 2) for c in multi)
    assert sum(c.name.endswith("-bare") for c in cases) == 2
    # the scalar the chains are made of: one digit in 31 levels, below (r - 1) / 2, so neither folded nor recentred
    for d in T.FIXUP_DIGITS:
        s, = T.chain_scalars(d, 31)
        assert s <= M.R_HALF and M.recode(s, 8) == [(w, d - 1, False) for w in range(31)]


def test_digit_and_batch_cases():
    for group in ("g1", "g2"):
        cases = T.digit_cases(group)
        assert sorted({c.c for c in cases}) == sorted(T.DIGIT_WIDTHS[group])
        assert {c.c for c in cases if c.stride == 2} == set(T.DIGIT_STRIDE2) & set(T.DIGIT_WIDTHS[group])
        for case in cases:
            assert 290 <= case.n <= 420 and case.batch * case.n * M.nwin_of(case.c) < 1 << 25, case
            assert len(case.counts) == 1 << (case.c - 1) and case.entries == sum(len(M.recode(s, case.c)) for s in case.vectors[0])
            assert all(M.signed_sum(s, case.c) == s for s in case.vectors[0])
    for case in T.batch_cases():
        nb = 1 << (case.c - 1)
        assert case.batch in (2, 3) and len(case.counts) == nb * case.batch and case.state()[1] == case.batch
        logs = case.expected_logs()
        per = [case.counts[v * nb:(v + 1) * nb] for v in range(case.batch)]
        if "neg" in case.name:          # the negative vector: the same buckets with every sign flipped, and the opposite point
            assert (logs[0] + logs[-1]) % P.R_MOD == 0 and logs[0] != 0 and np.array_equal(per[0], per[-1])
            a, b = T.terms_tabled([case.vectors[0]], case.c), T.terms_tabled([case.vectors[-1]], case.c)
            assert [(x ^ 1, y) for x, y in a] == b
        if "zero" in case.name:
            v = case.name.split("-")[-1].split("+").index("zero")
            assert logs[v] == 0 and not per[v].any() and per[1 - v if case.batch == 2 else 0].any()
    assert {(c.batch, c.c, c.stride) for c in T.batch_cases()} == {(k, c, s) for k in (2, 3) for c in (8, 13) for s in (1, 2)}


def test_reduction_rule_and_cases():
    nbs = {c: 1 << (c - 1) for c in T.REDUCE_WIDTHS}
    assert [nbs[c] for c in T.REDUCE_WIDTHS] == [8, 128, 256, 1 << 15, 1 << 19, 1 << 20, 1 << 22, 1 << 23]
    # the default: bit-sliced exactly for 256 <= nb <= 2^19, up to 2^22 for the proof's last MSM; both sides of every threshold
    for chunk in T.REDUCE_CHUNKS:
        assert [T.reduce_rule(c, 1, 0, chunk, False)[0] for c in T.REDUCE_WIDTHS] == [False, False, True, True, True, False, False, False]
        assert [T.reduce_rule(c, 1, 0, chunk, True)[0] for c in T.REDUCE_WIDTHS] == [False, False, True, True, True, True, True, False]
        for last in (False, True):
            assert all(T.reduce_rule(c, 1, 5, chunk, last)[0] for c in T.REDUCE_WIDTHS)
            assert not any(T.reduce_rule(c, 1, m, chunk, last)[0] for c in T.REDUCE_WIDTHS for m in (1, 4))
    assert T.reduce_rule(3, 1, 5, 2, False) == (False, 0, 0)                   # four buckets: never bit-sliced
    # the forced chunk of the bit-sliced form: shrunk while k > 2 and 4 k > nb
    assert T.reduce_rule(4, 1, 5, 64, False) == (True, 2, 2) and T.reduce_rule(4, 1, 5, 2, True) == (True, 2, 2)
    assert T.reduce_rule(8, 1, 5, 64, False) == (True, 2, 32) and T.reduce_rule(8, 1, 5, 16, False) == (True, 3, 16)
    assert T.reduce_rule(9, 1, 0, 64, False) == (True, 2, 64) and T.reduce_rule(9, 1, 0, 2, False) == (True, 7, 2)
    assert T.reduce_rule(20, 1, 0, 16, False) == (True, 15, 16) and T.reduce_rule(23, 1, 0, 16, True) == (True, 18, 16)
    assert T.reduce_rule(9, 1, 0, 0, False) == (True, None, None) and T.reduce_rule(24, 1, 5, 0, True) == (True, None, None)
    # the other forms: two levels under mode 1 from 16 chunks on; under the default from 16-bit windows on unless the MSM is the last
    assert T.reduce_rule(4, 1, 1, 0, False) == (False, 0, 0) and T.reduce_rule(8, 1, 1, 0, False) == (False, 0, 2)
    assert T.reduce_rule(8, 1, 1, 16, False) == (False, 0, 0) and T.reduce_rule(8, 1, 1, 64, True) == (False, 0, 0)
    assert T.reduce_rule(9, 1, 1, 16, False) == (False, 0, 16) and T.reduce_rule(9, 1, 1, 64, False) == (False, 0, 0)
    assert T.reduce_rule(16, 1, 1, 0, True) == (False, 0, 4) and T.reduce_rule(20, 1, 1, 0, True) == (False, 0, 8)
    assert T.reduce_rule(21, 1, 0, 0, False) == (False, 0, 8) and T.reduce_rule(21, 1, 0, 2, False) == (False, 0, 2)
    assert T.reduce_rule(24, 1, 0, 0, True) == (False, 0, 0) and T.reduce_rule(24, 1, 0, 64, False) == (False, 0, 64)
    assert T.reduce_rule(8, 1, 0, 0, False) == (False, 0, 0) and T.reduce_rule(4, 1, 0, 2, False) == (False, 0, 0)
    assert all(T.reduce_rule(c, 1, 4, k, last) == (False, 0, 0) for c in T.REDUCE_WIDTHS for k in T.REDUCE_CHUNKS for last in (False, True))
    # the default without the bit-sliced form: the work-efficient rule's own threshold, 16-bit windows
    assert T.reduce_rule(15, 1, 6, 0, False) == (False, 0, 0) and T.reduce_rule(16, 1, 6, 0, False) == (False, 0, 4)
    assert T.reduce_rule(16, 1, 6, 0, True) == (False, 0, 0) and T.reduce_rule(16, 1, 6, 16, False) == (False, 0, 16)
    # a batch: the chunk default goes by the buckets of all vectors together
    assert T.reduce_rule(13, 2, 1, 0, False) == (False, 0, 2) and T.reduce_rule(13, 8, 1, 0, False) == (False, 0, 4)
    for c in T.REDUCE_WIDTHS:
        nb, hi = nbs[c], T.high_level(c)
        assert 1 < hi < M.nwin_of(c) and (nb << (c * hi)) <= M.R_HALF < (nb << (c * (hi + 1)))
        pats = T.reduce_patterns(c)
        assert {p for p, _ in pats} == set(T.REDUCE_SPARSE) | (set(T.REDUCE_DENSE) if nb <= 4096 else set())
        assert {lvl for p, lvl in pats if p in T.REDUCE_SPARSE} == {0, hi}
        for pattern, level in pats:
            case = T.reduce_case("g1", c, pattern, level)
            assert case.n <= 4096 and len(case.counts) == nb, case
            for s in set(case.vectors[0]):                  # one positive digit each: the scalar names its level and bucket
                (w, b, neg), = M.recode(s, c)
                assert s == (b + 1) << (c * w) and not neg and (w == level or pattern in T.REDUCE_DENSE), case
            cnt = case.counts
            if pattern in T.REDUCE_DENSE:
                assert cnt.all() and len(set(cnt.tolist())) == 1 and cnt[0] in (3, 6), case
            elif pattern == "bucket0":
                assert cnt[0] == 2 and cnt.sum() == 2, case
            elif pattern == "top-bucket":
                assert cnt[nb - 1] == 2 and cnt.sum() == 2, case
            elif pattern == "last-chunk":
                k = min(64, nb)
                assert cnt[nb - k:].all() and cnt.sum() == k, case
            else:
                step = max(1, nb >> 9)
                assert np.array_equal(np.nonzero(cnt)[0], np.arange(step - 1, nb, step)) and cnt[nb - 1] == 2 and cnt.sum() == 2 * min(nb, 512)
    for c, p in T.REDUCE_G2:
        assert c in T.REDUCE_WIDTHS and p in T.REDUCE_DENSE
    L = M.LOGS
    assert (L[M.A] + L[M.B] - L[M.C] - L[M.D]) % P.R_MOD == 0 and len({L[M.A], L[M.B], L[M.C], L[M.D]}) == 4


def _small_cases():
    out = []
    for group in ("g1", "g2"):
        out += T.fixup_cases(group) + T.segment_cases(group)[:4] + T.digit_cases(group)
        out += [T.table_case(group, c, n, 1) for c in T.TABLE_WIDTHS[group][:2] for n in T.TABLE_NS]
        out += [T.table_case(group, 8, 3, 1, with_inf=False)]
        if group == "g1":
            out += [T.reduce_case(group, c, p, lvl) for c in T.REDUCE_WIDTHS for p, lvl in T.reduce_patterns(c)] + T.batch_cases()
        else:
            out += [T.reduce_case(group, c, p) for c, p in T.REDUCE_G2]
    return [c for c in out if c.n <= ORACLE_MSM_MAX[c.group]]


def test_expected_points_equal_the_oracle_msm(oracle):
    """the expected point of a vector is [sum s_i k_i]G; the oracle's own MSM over the case's bases, infinity mask and scalars must give
    the same bytes (the 67 points really are [k]G, Q / Q- / R and the infinity bases included, and the sum is the sum)"""
    cases = _small_cases()
    assert len(cases) > 100 and {c.group for c in cases} == {"g1", "g2"}
    used = set()
    for case in cases:
        bases, inf, sc = case.arrays(oracle)
        for v, (exp, einf) in enumerate(case.expected(oracle)):
            got, ginf = oracle.msm(case.group, bases, sc[v], inf if inf.any() else None)
            assert ginf == einf and (einf or np.array_equal(got, exp)), (case, v)
        used |= set(case.idx.tolist())
        used |= {"inf"} if case.inf.any() else set()
    assert used >= {T.Q, T.QN, T.RR, "inf"}
    assert any(e == 0 for c in cases for e in c.expected_logs())
