"""The bucket MSM on window tables (csrc/msm.hip: tables_build, a tabled msm_plan_build, the accumulation on Affine and PadAffine
entries, the fix-ups, the one-set branch of msm_enqueue_reduce, msm_collect_part) one MSM at a time, through zkg16_diag_msm_tabled.
Shared by tests/test_msm_tabled_host.py (the model agrees with a brute-force sort, every case sits on the boundary it names, the
expected points agree with the CPU oracle's MSM) and tests/test_msm_tabled_gpu.py (device == expected point and table entry, and
zkg16_last_msm_state == the model's state).

The model reuses tests/msm_limit_cases.py (recoding, seg_len, spills, the fix-up queue) and differs where a key with tables differs:
the term of scalar i of vector v with the signed digit (w, b, neg) is x = ((w n + i) << 1) | neg on the base table[w][i], in bucket
y = v 2^(c-1) + b of the ONE set vector v has — so a scalar brings up to 254 / c + 1 terms into one set, buckets hold terms of
different levels, and the reduction sees one window per vector.

Every base is [k]G for a k out of LOGS or one of three more per width c: Q = [2^c k_P]G, Q- = -Q and R = [2^(2c) k_P]G with P = TP, so
that level 1 of P is Q (an accumulation that holds Q must double when P's level-1 term arrives), level 1 of P cancels Q-, and level 2
of P is R.  The expected value of a vector is [sum s_i k_i mod r]G: one scalar multiplication by the CPU oracle, nothing from the
device; the expected table entry of level w is [2^(c w) k_i mod r]G from the oracle's fixed-base routine."""
import random

import numpy as np

import msm_limit_cases as M
import pyref as P
from helpers import G1_GEN_LIMBS, G2_GEN_LIMBS
from msm_limit_cases import (A, AB, B, C, D, FIXUP_ITEM, FIXUP_SHORT, LOGS, NEG, PLAIN, REP, R_HALF, canon_vec, content_idx, fixup_queue,
                             nwin_of, recode, seg_lens, spills, state_matches)

R = P.R_MOD
TP = 6                                      # the point P whose multiples Q, Q-, R are bases of their own
Q, QN, RR = 64, 65, 66                      # indices behind the 64 LOGS points
_points = {}
_levels = {}


def gen(group):
    return G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS


def logs_ext(c):
    """the discrete logs of the 67 points a case of width c may use"""
    q = (LOGS[TP] << c) % R
    return LOGS + [q, R - q, (LOGS[TP] << (2 * c)) % R]


def points(oracle, group, c):
    """the 67 points of width c, affine Montgomery limbs as the C ABI takes them (the 64 of M.table, then Q, Q-, R)"""
    if (group, c) not in _points:
        pts, inf = oracle.fixed_base(group, gen(group), canon_vec(logs_ext(c)[64:]))
        assert not inf.any()
        pts = np.concatenate([M.table(oracle, group), pts])
        pts.setflags(write=False)
        _points[group, c] = pts
    return _points[group, c]


def level_points(oracle, group, c):
    """-> (levels, 64, 12 | 24): [2^(c w) LOGS[j]]G, what level w of a table holds for the base [LOGS[j]]G"""
    if (group, c) not in _levels:
        nw = nwin_of(c)
        pts, inf = oracle.fixed_base(group, gen(group), canon_vec([(k << (c * w)) % R for w in range(nw) for k in LOGS]))
        assert not inf.any()                 # r is odd: no multiple by a power of two vanishes
        pts = pts.reshape(nw, 64, -1)
        pts.setflags(write=False)
        _levels[group, c] = pts
    return _levels[group, c]


# ------------------------------------------------------------------------------------------------ the model
def terms_tabled(vectors, c):
    """the sorted term list of a batch on a tabled key: [(x, y)], by y, then by position w n + i"""
    nb, n = 1 << (c - 1), len(vectors[0])
    t = [(v * nb + b, w * n + i, neg) for v, vec in enumerate(vectors) for i, s in enumerate(vec) for w, b, neg in recode(s, c)]
    t.sort(key=lambda e: (e[0], e[1]))
    return [((pos << 1) | int(neg), y) for y, pos, neg in t]


def counts_tabled(vectors, c):
    """terms per bucket of the batch's bucket sets, vector after vector"""
    nb = 1 << (c - 1)
    return np.concatenate([M.bucket_counts(vec, c).reshape(nwin_of(c), nb).sum(0) for vec in vectors])


def reduce_rule(c, batch, mode, chunk, last):
    """msm_enqueue_reduce for one window per vector under option values reduce_mode = mode (0 = the default, 6 = the default without the
    bit-sliced form), reduce_chunk = chunk and slot.last_of_proof = last -> (does the bit-sliced form run, bit_sliced, two_level_k);
    the last two are None where the depth estimate picks the bit-sliced chunk"""
    nb = 1 << (c - 1)
    tb = nb * batch
    kk = chunk if chunk else (2 if tb <= 16384 else 4 if tb <= 131072 else 8)
    while kk > nb:
        kk //= 2
    nchunks = nb // kk
    efficient = mode == 1 or (mode in (0, 5, 6) and not last and c >= 16)
    two_level = kk if efficient and kk >= 2 and nchunks >= 16 else 0
    one_set_max = 1 << (22 if last else 19)
    if nb >= 8 and (mode == 5 or (mode == 0 and 256 <= nb <= one_set_max)):
        if chunk > 1 and chunk & (chunk - 1) == 0:
            kb = chunk
            while kb > 2 and 4 * kb > nb:
                kb //= 2
            return True, (nb // kb).bit_length() - 1, kb
        return True, None, None
    return False, 0, two_level


class TCase:
    """One call of zkg16_diag_msm_tabled: vectors (batch lists of n Python ints), idx (which of the 67 points each base is), inf (bases
    passed as the point at infinity), the stride mode, last_of_proof, the options to set, and what the model expects."""

    def __init__(self, name, group, c, vectors, idx, inf=None, stride=1, last=False, options=None, min_seg=0, claims=None):
        self.name, self.group, self.c, self.stride, self.last, self.min_seg = name, group, c, stride, last, min_seg
        self.vectors = [list(v) for v in vectors]
        self.idx = np.asarray(idx, dtype=np.int64)
        self.n, self.batch = len(self.idx), len(self.vectors)
        assert all(len(v) == self.n for v in self.vectors)
        self.inf = np.zeros(self.n, dtype=np.uint8) if inf is None else np.asarray(inf, dtype=np.uint8)
        self.options = dict(options or {})
        if min_seg:
            self.options["min_seg"] = min_seg
        self.claims = claims or {}
        self.counts = counts_tabled(self.vectors, c) if self.n else np.zeros(0, dtype=np.int64)
        self.entries = int(self.counts.sum())

    def __repr__(self):
        return self.name

    def with_(self, stride=None, last=None, options=None, suffix=""):
        """the same MSM under another stride mode / last_of_proof / option set"""
        t = TCase.__new__(TCase)
        t.__dict__.update(self.__dict__)
        t.options = dict(self.options)
        t.options.update(options or {})
        if stride is not None:
            t.stride = stride
        if last is not None:
            t.last = last
        t.name = self.name + suffix
        return t

    def arrays(self, oracle):
        """-> bases (n, 12 | 24), the infinity mask (n,), scalars (batch, n, 4)"""
        if "_arrays" not in self.__dict__:
            sc = np.stack([canon_vec(v) if self.n else np.zeros((0, 4), np.uint64) for v in self.vectors])
            sc.setflags(write=False)
            self._arrays = (points(oracle, self.group, self.c)[self.idx], self.inf, sc)
        return self._arrays

    def expected_logs(self):
        lg = logs_ext(self.c)
        k = [0 if f else lg[i] for i, f in zip(self.idx.tolist(), self.inf.tolist())]
        return [sum(s * x for s, x in zip(vec, k)) % R for vec in self.vectors]

    def expected(self, oracle):
        """-> [(affine limbs, infinity flag)] per vector; computed once"""
        if "_expected" not in self.__dict__:
            self._expected = [oracle.point_mul(self.group, gen(self.group), canon_vec([e])[0]) for e in self.expected_logs()]
        return self._expected

    def seg_len(self, cus=M.CUS_MI355X):
        terms = self.batch * self.n * nwin_of(self.c)
        s = seg_lens(self.entries, len(self.counts), M.lanes("g1", cus, terms), M.lanes("g2", cus, terms), self.min_seg)
        return s[0 if self.group == "g1" else 1]

    def state(self, cus=M.CUS_MI355X, mode=None, chunk=0):
        """what zkg16_last_msm_state must report (None = not asserted); mode: the reduce_mode option's value, None = form not asserted"""
        if self.n == 0:
            return (self.c, self.batch, 0, 0, 0, 0, 0, 0)
        seg = self.seg_len(cus)
        items, chains = fixup_queue(self.counts, seg)
        bs, k2 = reduce_rule(self.c, self.batch, mode, chunk, self.last)[1:] if mode is not None else (None, None)
        return (self.c, self.batch, self.entries, seg, items, chains, bs, k2)


# ------------------------------------------------------------------------------------------------ a. the tables themselves
TABLE_NS = (1, 3, 67, 257)
TABLE_WIDTHS = {"g1": (2, 7, 8, 13, 16, 22, 24), "g2": (8, 24)}


def table_case(group, c, n, stride, with_inf=True):
    """the 64 LOGS points in a scrambled order and, with_inf, three bases passed as infinity (first, middle, last); the scalars are small
    and large, so that the value is checked along with the table"""
    rng = random.Random("table/%s/%d/%d" % (group, c, n))
    idx = [(11 * i + 5) % 64 for i in range(n)]
    inf = np.zeros(n, dtype=np.uint8)
    if with_inf:
        inf[[0, n // 2, n - 1]] = 1
    sc = [rng.randrange(R) if i % 3 else i + 1 for i in range(n)]
    return TCase("%s-table-c%d-n%d-s%d%s" % (group, c, n, stride, "" if with_inf else "-noinf"), group, c, [sc], idx, inf=inf, stride=stride)


def expected_table(oracle, case):
    """-> (levels, n, 12 | 24) limbs and (levels, n) infinity flags: level w of base i = [2^(c w) k_i]G, infinity where the base is"""
    assert (case.idx < 64).all()
    tab = level_points(oracle, case.group, case.c)[:, case.idx].copy()
    tab[:, case.inf != 0] = 0
    return tab, np.broadcast_to(case.inf, tab.shape[:2])


# ------------------------------------------------------------------------------------------------ b. digit recoding on one set
DIGIT_WIDTHS = {"g1": (2, 3, 4, 8, 13, 16, 17, 20, 21, 22, 24), "g2": (2, 13, 22)}
DIGIT_STRIDE2 = (8, 22)


def digit_case(group, c, stride=1):
    s = M.digit_scalars(c)
    rng = random.Random(2000 + c)
    return TCase("%s-digits-c%d-s%d" % (group, c, stride), group, c, [s], [rng.randrange(64) for _ in s], stride=stride)


def digit_cases(group):
    return [digit_case(group, c, st) for c in DIGIT_WIDTHS[group] for st in ((1, 2) if c in DIGIT_STRIDE2 else (1,))]


# ------------------------------------------------------------------------------------------------ c. segment edges, mixed levels
# digit (bucket = digit - 1) -> its terms (level, point) in the order of the sorted list: by level, then by index.  Offsets at seg_len 3:
SEGMENT_LAYOUT = [
    (1, [(0, 5), (0, 6), (1, 7)]),                                        # 0..2    begins at a segment start and ends at a segment end
    (2, [(3, 8)]), (3, [(0, 9)]), (4, [(31, 10)]),                        # 3..5    single entries, one of them fed from the top level only
    (5, [(0, 11), (2, 12)]),                                              # 6..7    begins at a segment start
    (6, [(0, 13), (1, 14), (1, 15), (5, 16)]),                            # 8..11   ends at a segment end, as the head of segment 3
    (7, [(0, 17)]),                                                       # 12
    (8, [(w, 18 + j) for j, w in enumerate((0, 0, 1, 2, 2, 7, 15, 16, 30, 31))]),      # 13..22  segments 5 and 6 are whole inside it
    (9, [(31, 28), ]),                                                    # 23      the top level only
    (10, [(0, 29), (0, 30), (1, 31), (1, 5), (2, 6), (30, 7)]),           # 24..29  exactly two whole segments
    # Q + a + b - (a + b) is Q with a non-trivial ZZ; then level 1 of P, which is Q: the doubling; then more terms
    (11, [(0, Q), (0, A), (0, B), (0, NEG + AB), (1, TP), (1, 20), (2, 21)]),          # 30..36
    # Q-, then level 1 of P: the cancellation; the terms behind it start the bucket again
    (12, [(0, QN), (1, TP), (1, 23), (1, 24), (3, 25)]),                  # 37..41
    (13, [(0, RR), (2, TP), (2, 6)]),                                     # 42..44  R, then level 2 of P: a doubling of two affine points
    (14, [(0, 26)]),                                                      # 45
    (20, [(0, 8), (1, 9), (2, 10)]),                                      # 46..48
    (30, [(0, 11), (4, 12), (8, 13), (12, 14)]),                          # 49..52
    (31, [(0, C), (0, D)]),                                               # 53..54  c + d = a + b
    (127, [(0, 15), (0, NEG + 15), (1, 16)]),                             # 55..57
    (128, [(0, 17), (1, 18), (2, 19), (3, 20), (4, 21), (30, 22)]),       # 58..63  the top bucket; the last segment is short
]


def segment_case(group, variant, min_seg, stride):
    # one scalar per term, digit << (8 level); the input takes the first term of every bucket, top bucket first, then the second of
    # each, ...: the sort has something to do, and inside a bucket the scalars of one level keep the order written above
    terms = sorted(((j, -d, lvl, pt) for d, ts in SEGMENT_LAYOUT for j, (lvl, pt) in enumerate(ts)))
    assert all(ts == sorted(ts, key=lambda t: t[0]) for _, ts in SEGMENT_LAYOUT)
    scalars, idx = [-d << (8 * lvl) for _, d, lvl, _ in terms], [pt for _, _, _, pt in terms]
    name = "%s-seg%d-s%d-%s" % (group, min_seg, stride, "+".join("%s=%d" % kv for kv in variant) or "default")
    return TCase(name, group, 8, [scalars], idx, stride=stride, options=dict(variant), min_seg=min_seg)


def segment_cases(group):
    """every accumulation variant x both entry types x both kernel families (the variants of the other group's kernels are run too: they
    must change nothing)"""
    return [segment_case(group, v, m, st) for v in M.ACC_VARIANTS[group] for st in (1, 2) for m in (3, 6)]


# ------------------------------------------------------------------------------------------------ d. fix-up routing, deep buckets
FIXUP_DIFFS = {"g1": (4, 5, 1024, 1025, 2049), "g2": (5, 1025)}
FIXUP_STRIDE2 = (5, 1025)
FIXUP_DIGITS = (77, 55, 99)                  # the buckets (digit - 1) the chains are built in
CHAIN_LEVELS = 31                            # sum_{w < 31} d 2^(8 w) with d < 128 is below (r - 1) / 2: 31 terms of one bucket, no recentring


def chain_scalars(digit, nterms, pairs=False):
    """scalars that bring exactly nterms terms into bucket digit - 1 and none elsewhere: digit repeated in the levels 0 .. k - 1, k = 31
    for all but the last scalar (pairs: for all but the last two, which are equal — P and -P then meet in every level)"""
    rep = lambda k: sum(digit << (8 * w) for w in range(k))
    group = 2 if pairs else 1
    assert nterms % group == 0
    per = nterms // group
    ks = [CHAIN_LEVELS] * (per // CHAIN_LEVELS) + ([per % CHAIN_LEVELS] if per % CHAIN_LEVELS else [])
    return [rep(k) for k in ks for _ in range(group)]


def fixup_case(group, chains, min_seg, content, stride=1, nfill=150):
    """c = 8.  chains: [(digit, diff)]: bucket digit - 1 gets as many terms as make it spill over exactly `diff` further segments.  The
    other buckets get up to three single-term scalars each, from any level: they place the chains and queue nothing (with seg_len 1 a
    bucket of up to FIXUP_SHORT + 1 terms stays on the short path)."""
    c, nb, m = 8, 128, min_seg
    rng = random.Random("tfix/%s/%s/%d/%s" % (group, chains, m, content))
    assert all(d in FIXUP_DIGITS for d, _ in chains)
    scalars, idx = [], []
    free = [d for d in range(1, nb + 1) if d not in FIXUP_DIGITS]
    held = {}
    for _ in range(nfill):
        d = free[rng.randrange(len(free))]
        if held.get(d, 0) < 3:
            held[d] = held.get(d, 0) + 1
            scalars.append(d << (c * rng.randrange(30)))
            idx.append(rng.randrange(64))
    lengths = []
    for d, diff in sorted(chains):
        start = int(counts_tabled([scalars], c)[: d - 1].sum()) if scalars else 0
        lo = diff * m + 1 - start % m                       # lengths lo .. lo + m - 1 end in segment t + diff
        pairs = content == "alternate" and nfill == 0
        n = [x for x in range(lo, lo + m) if x > 0 and (not pairs or x % 2 == 0)][0]
        lengths.append(n)
        s = chain_scalars(d, n, pairs)
        scalars += s
        idx += content_idx(content, len(s)).tolist()
    name = "%s-tfix-%s-seg%d-%s-s%d%s" % (group, "+".join(str(x[1]) for x in chains), m, content, stride, "-bare" if nfill == 0 else "")
    claims = dict(chains=sorted(chains), lengths=lengths, items=sum(-(-x[1] // FIXUP_ITEM) for x in chains if x[1] > FIXUP_SHORT),
                  nchains=sum(x[1] > FIXUP_ITEM for x in chains))
    return TCase(name, group, c, [scalars], idx, stride=stride, min_seg=m, claims=claims)


def fixup_cases(group):
    out = []
    for content in M.CONTENTS:
        for diff in FIXUP_DIFFS[group]:
            for m in (1, 3):
                out.append(fixup_case(group, [(77, diff)], m, content))
            if diff in FIXUP_STRIDE2:
                out.append(fixup_case(group, [(77, diff)], 3, content, stride=2))
        if group == "g1":           # three long chains queued at once: 2, 1 and 3 items
            out.append(fixup_case(group, [(77, 1025), (55, 500), (99, 2049)], 1, content))
    # nothing but the chain, P and -P in equal numbers in every level: every partial sum, the bucket and the MSM itself are infinity
    out += [fixup_case(group, [(77, diff)], 1, "alternate", nfill=0) for diff in (5, 1025)]
    return out


# ------------------------------------------------------------------------------------------------ e. the one-set reduction
REDUCE_WIDTHS = (4, 8, 9, 16, 20, 21, 23, 24)              # 8, 128, 256, 2^15, 2^19, 2^20, 2^22, 2^23 buckets
REDUCE_DENSE = ("same", "signs", "two-forms", "two-forms-neg")        # every bucket filled: up to 2^12 buckets
REDUCE_SPARSE = ("bucket0", "top-bucket", "last-chunk", "every")      # at every width
REDUCE_MODES = (0, 1, 4, 5)
REDUCE_CHUNKS = (0, 2, 16, 64)
REDUCE_G2 = [(4, "same"), (4, "two-forms"), (9, "same"), (9, "two-forms")]
DENSE_MAX_NB = 1 << 12


def high_level(c):
    """the highest level whose every digit up to 2^(c-1) keeps the scalar at most (r - 1) / 2 (no fold, no recentring)"""
    w = nwin_of(c) - 1
    while (1 << (c - 1)) << (c * w) > R_HALF:
        w -= 1
    return w


def reduce_patterns(c):
    dense = REDUCE_DENSE if 1 << (c - 1) <= DENSE_MAX_NB else ()
    return [(p, 0) for p in dense] + [(p, lvl) for p in REDUCE_SPARSE for lvl in (0, high_level(c))]


def reduce_case(group, c, pattern, level=0):
    """Buckets filled through scalars (b + 1) << (c w): one positive digit each.  The dense patterns fill every bucket from the levels 0,
    1 and high_level(c) at once (a bucket's terms are of three levels); the sparse ones from `level` alone."""
    nb = 1 << (c - 1)
    scalars, idx = [], []
    if pattern in REDUCE_DENSE:
        for w in (0, 1, high_level(c)):
            for b in range(nb):
                if pattern == "same":
                    pts = [REP]
                elif pattern == "signs":
                    pts = [REP if b % 2 == 0 else NEG + REP]
                elif pattern == "two-forms":
                    pts = [A, B] if b % 2 == 0 else [C, D]
                else:
                    pts = [A, B] if b % 2 == 0 else [NEG + C, NEG + D]
                scalars += [(b + 1) << (c * w)] * len(pts)
                idx += pts
    else:
        w = level
        if pattern == "bucket0":
            fill = {0: [REP, PLAIN[3]]}
        elif pattern == "top-bucket":
            fill = {nb - 1: [REP, PLAIN[4]]}
        elif pattern == "last-chunk":           # the last chunk of every chunk size up to 64
            fill = {b: [PLAIN[b % 9]] for b in range(max(0, nb - 64), nb)}
        else:
            assert pattern == "every"           # every 2^(c-9)-th bucket: 512 of them (all, below 512 buckets), the last one included
            step = max(1, nb >> 9)
            fill = {b: [PLAIN[(b // step) % 11], REP] for b in range(step - 1, nb, step)}
        for b, pts in sorted(fill.items()):
            scalars += [(b + 1) << (c * w)] * len(pts)
            idx += pts
    return TCase("%s-reduce-c%d-%s-l%d" % (group, c, pattern, level), group, c, [scalars], idx)


# ------------------------------------------------------------------------------------------------ f. batches
BATCH_WIDTHS = (8, 13)


def batch_cases(group="g1"):
    out = []
    for c in BATCH_WIDTHS:
        s = M.digit_scalars(c)
        neg = [(R - x) % R for x in s]
        zero = [0] * len(s)
        rng = random.Random(3000 + c)
        idx = [rng.randrange(64) for _ in s]
        for stride in (1, 2):
            for name, vecs in (("digits+neg", [s, neg]), ("zero+digits", [zero, s]), ("digits+zero+neg", [s, zero, neg])):
                out.append(TCase("%s-batch%d-c%d-s%d-%s" % (group, len(vecs), c, stride, name), group, c, vecs, idx, stride=stride))
    return out
