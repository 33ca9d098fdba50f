"""The bucket MSM (csrc/msm.hip) at the limits of its fix-up routing, segment bookkeeping, signed-digit recoding and bucket
reductions.  Shared by tests/test_msm_limits_host.py (the model below agrees with plain integer arithmetic, every case sits on the
boundary it names, and the expected points agree with the CPU oracle's MSM) and tests/test_msm_limits_gpu.py (device == expected
point, and zkg16_last_msm_state == the model's state).

The model is Python integers plus numpy: the recoding of msm_digits_kernel, the bucket sizes of the sorted term list (by window,
then bucket, index order inside a bucket), seg_len by the rule of msm_seg_params_kernel, and from those every spilled bucket's
`last_seg - t` with the work items and chains msm_fixup_kernel must queue for it.

Every base is [k]G for a k out of LOGS (64 values: 32 and their negatives, with a + b = c + d and a + b itself among them), made on
the CPU by the oracle's fixed-base routine and indexed, so the expected value of a case is [sum s_i k_i mod r]G: one scalar
multiplication, no MSM, and nothing computed by the device."""
import random

import numpy as np

import pyref as P
from helpers import G1_GEN_LIMBS, G2_GEN_LIMBS

R = P.R_MOD
R_HALF = (R - 1) // 2
FIXUP_SHORT, FIXUP_ITEM = 4, 1024            # msm.hip
CUS_MI355X = 256


def lanes(group, cus, terms=0):
    """lanes of one resident round of accumulation waves (msm_plan_build): 4 SIMDs x waves x 64 per CU; G1 runs two waves per SIMD
    (four from 2^25 (scalar, window) terms on, far above every case here), G2 one"""
    assert terms < 1 << 25
    return 4 * cus * (2 if group == "g1" else 1) * 64


# ------------------------------------------------------------------------------------------------ the points
def _logs():
    rng = random.Random(20261019)
    k = [rng.randrange(1, R) for _ in range(32)]
    k[3] = (k[0] + k[1] - k[2]) % R          # a + b = c + d: two accumulations that end on the same point in different XYZZ forms
    k[4] = (k[0] + k[1]) % R                 # a + b as an affine base: a, b, (a + b) doubles, a, b, -(a + b) cancels
    k += [R - x for x in k]                  # LOGS[32 + j] = -LOGS[j]
    assert len(set(k)) == 64 and 0 not in k
    return k


LOGS = _logs()
A, B, C, D, AB, REP = 0, 1, 2, 3, 4, 7       # indices with a role; NEG + j is the negative of j
NEG = 32
PLAIN = list(range(5, 32))                   # random points without a relation among them
_tables = {}


def canon_vec(xs):
    """canonical scalars as (n, 4) u64 limbs"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def table(oracle, group):
    """the 64 points [LOGS[j]]G of a group, affine Montgomery limbs as the C ABI takes them"""
    if group not in _tables:
        pts, inf = oracle.fixed_base(group, G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS, canon_vec(LOGS))
        assert not inf.any()
        pts.setflags(write=False)
        _tables[group] = pts
    return _tables[group]


# ------------------------------------------------------------------------------------------------ the model
def nwin_of(c):
    return 254 // c + 1


def recode(s, c):
    """msm_digits_kernel: -> [(window, bucket, negate)] of the non-zero signed digits of s.  s above (r - 1) / 2 is replaced by r - s
    with every sign flipped; a window value above 2^(c-1) becomes value - 2^c with a carry into the next window."""
    assert 0 <= s < R
    flip = s > R_HALF
    m = R - s if flip else s
    mask, half = (1 << c) - 1, 1 << (c - 1)
    out, carry = [], 0
    for w in range(nwin_of(c)):
        v = ((m >> (w * c)) & mask) + carry
        carry = 0
        if v > half:
            carry = 1
            if v != 1 << c:
                out.append((w, (1 << c) - v - 1, not flip))
        elif v:
            out.append((w, v - 1, flip))
    assert carry == 0                        # magnitudes are below 2^254: the top window never carries out
    return out


def signed_sum(s, c):
    """sum of the signed digits times 2^(c w): must be s mod r"""
    return sum((-(b + 1) if neg else (b + 1)) << (c * w) for w, b, neg in recode(s, c)) % R


def bucket_counts(scalars, c):
    """terms per global bucket id (window * 2^(c-1) + bucket) of the sorted list"""
    nb = 1 << (c - 1)
    counts = np.zeros(nb * nwin_of(c), dtype=np.int64)
    mult = {}
    for s in scalars:
        mult[s] = mult.get(s, 0) + 1
    for s, k in mult.items():
        for w, b, _ in recode(s, c):
            counts[w * nb + b] += k
    return counts


def sorted_terms(scalars, c):
    """the sorted term list itself: [(global bucket, index, negate)], by bucket, index order inside a bucket (small cases only)"""
    nb = 1 << (c - 1)
    t = [(w * nb + b, i, neg) for i, s in enumerate(scalars) for w, b, neg in recode(s, c)]
    t.sort(key=lambda x: (x[0], x[1]))
    return t


def seg_lens(entries, total_buckets, lanes_g1, lanes_g2, min_seg):
    """msm_seg_params_kernel -> (seg_len of the G1 kernels, of the G2 kernels)"""
    if min_seg == 0:
        min_seg = entries // total_buckets // 2 + 4
    return tuple(max(-(-entries // ln), min_seg) for ln in (lanes_g1, lanes_g2))


def spills(counts, seg_len):
    """-> [(global bucket, t, last_seg)] of the buckets whose terms go on past the segment t of their first term"""
    offs = np.concatenate([[0], np.cumsum(counts)])
    g = np.nonzero(counts)[0]
    t = offs[g] // seg_len
    last = (offs[g + 1] - 1) // seg_len
    keep = last > t
    return list(zip(g[keep].tolist(), t[keep].tolist(), last[keep].tolist()))


def fixup_queue(counts, seg_len):
    """msm_fixup_kernel -> (items, chains): ceil(len / FIXUP_ITEM) items for every spilled bucket with len = last_seg - t above
    FIXUP_SHORT; a chain for each of those with more than one item"""
    items = chains = 0
    for _, t, last in spills(counts, seg_len):
        if last - t > FIXUP_SHORT:
            n = -(-(last - t) // FIXUP_ITEM)
            items += n
            chains += n > 1
    return items, chains


def reduce_state(c, mode, chunk):
    """(bit_sliced, two_level_k) msm_enqueue_reduce must choose for option values reduce_mode = mode, reduce_chunk = chunk on a plain
    key; None where the rule is not a simple one (the default mode, and the depth estimate that picks the bit-sliced chunk)"""
    nb, nw = 1 << (c - 1), nwin_of(c)
    tb = nb * nw
    if mode == 5:
        if nb < 8:
            return 0, None
        if chunk < 2:
            return None, None
        kb = chunk
        while kb > 2 and 4 * kb > nb:
            kb //= 2
        return (nb // kb).bit_length() - 1, kb
    if mode == 1:
        kk = chunk if chunk else (2 if tb <= 16384 else 4 if tb <= 131072 else 8)
        while kk > nb:
            kk //= 2
        return 0, (kk if nb // kk >= 16 else 0)
    if mode == 4:
        return 0, 0
    return None, None


class Case:
    """One MSM: scalars (Python ints), idx (which of the 64 points each base is), the options to set, and what the model expects."""

    def __init__(self, name, group, c, scalars, idx, options=None, min_seg=0, claims=None):
        assert len(scalars) == len(idx)
        self.name, self.group, self.c, self.min_seg = name, group, c, min_seg
        self.scalars, self.idx = list(scalars), np.asarray(idx, dtype=np.int64)
        self.options = dict(options or {})
        self.options["window_bits"] = c
        if min_seg:
            self.options["min_seg"] = min_seg
        self.claims = claims or {}
        self.counts = bucket_counts(self.scalars, c)
        self.entries = int(self.counts.sum())

    def __repr__(self):
        return self.name

    def arrays(self, oracle):
        return table(oracle, self.group)[self.idx], canon_vec(self.scalars)

    def expected_log(self):
        return sum(s * LOGS[i] for s, i in zip(self.scalars, self.idx.tolist())) % R

    def expected(self, oracle):
        return oracle.point_mul(self.group, G1_GEN_LIMBS if self.group == "g1" else G2_GEN_LIMBS, canon_vec([self.expected_log()])[0])

    def seg_len(self, cus=CUS_MI355X):
        terms = len(self.scalars) * nwin_of(self.c)
        s = seg_lens(self.entries, len(self.counts), lanes("g1", cus, terms), lanes("g2", cus, terms), self.min_seg)
        return s[0 if self.group == "g1" else 1]

    def state(self, cus=CUS_MI355X, mode=None, chunk=0):
        """what zkg16_last_msm_state must report; None = not asserted"""
        seg = self.seg_len(cus)
        items, chains = fixup_queue(self.counts, seg)
        bs, k2 = reduce_state(self.c, mode, chunk) if mode is not None else (None, None)
        return (self.c, nwin_of(self.c), self.entries, seg, items, chains, bs, k2)


def state_matches(got, want):
    return len(got) == len(want) and all(w is None or g == w for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ fix-up cases
CONTENTS = ("distinct", "repeat", "alternate")
FIXUP_DIFFS = (1, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
FIXUP_DIFFS_G2 = (4, 5, 1024, 1025, 2049)


def content_idx(content, n):
    """n bases of one bucket: distinct points; one point repeated (a doubling at every level of block_fold and along the chain);
    P and -P alternating (infinity, and infinity + infinity)"""
    i = np.arange(n)
    if content == "distinct":
        return np.asarray(PLAIN)[i % len(PLAIN)]
    if content == "repeat":
        return np.full(n, REP)
    assert content == "alternate"
    return np.where(i % 2 == 0, REP, NEG + REP)


_fillers = {}


def sparse_filler(c, count, limit, reserved):
    """`count` random 240-bit scalars none of whose digits lands in a `reserved` global bucket or brings any bucket above `limit`
    terms: with seg_len 1 a bucket of up to FIXUP_SHORT + 1 terms stays on the short path, so the fillers queue nothing"""
    key = (c, count, limit, tuple(sorted(reserved)))
    if key not in _fillers:
        _fillers[key] = _sparse_filler(random.Random(str(key)), c, count, limit, reserved)
    return list(_fillers[key])


def _sparse_filler(rng, c, count, limit, reserved):
    nb = 1 << (c - 1)
    counts, out = {}, []
    while len(out) < count:
        s = rng.randrange(1, 1 << 240)
        gs = [w * nb + b for w, b, _ in recode(s, c)]
        if any(g in reserved or counts.get(g, 0) >= limit for g in gs):
            continue
        for g in gs:
            counts[g] = counts.get(g, 0) + 1
        out.append(s)
    return out


FIXUP_BUCKETS = ((0, 77), (3, 55), (7, 99))      # (window, digit) of the buckets the chains are built in


def fixup_case(group, chains, min_seg, content, off_mod=None, l_mult=None, total_mod=None, nfill=None):
    """c = 8.  chains: [(window, digit, diff)]: the scalar digit << (8 window) is shared by as many bases as make the bucket of that
    digit spill over exactly `diff` further segments.  Fillers place the buckets; with off_mod, scalar-1 terms (bucket 0 of window 0,
    in front of everything) move the first chain's start to off_mod modulo seg_len, with l_mult (True / False) its length is (not) a
    multiple of seg_len, and with total_mod terms in the last window bring the list's length to total_mod modulo seg_len."""
    c, nb, m = 8, 128, min_seg
    if nfill is None:
        nfill = 200 if group == "g1" else 60
    rng = random.Random("%s/%s/%d/%s/%s/%s/%s" % (group, chains, m, content, off_mod, l_mult, total_mod))
    reserved = {w * nb + d - 1 for w, d in FIXUP_BUCKETS} | {0, 31 * nb}
    assert all((w, d) in FIXUP_BUCKETS for w, d, _ in chains)
    scalars = sparse_filler(c, nfill, FIXUP_SHORT + 1, reserved)
    idx = [rng.randrange(64) for _ in scalars]
    pads = 0
    lengths = []
    for j, (w, d, diff) in enumerate(sorted(chains)):
        assert 1 <= d <= nb and w < 31
        counts = bucket_counts(scalars, c)
        start = int(counts[: w * nb + d - 1].sum())
        if j == 0 and off_mod is not None:
            pads = (off_mod - start) % m
            scalars += [1] * pads
            idx += [PLAIN[i % len(PLAIN)] for i in range(pads)]
            start += pads
        lo = diff * m + 1 - start % m                    # lengths lo .. lo + m - 1 end in segment t + diff
        pick = [n for n in range(lo, lo + m) if n > 0 and (l_mult is None or j > 0 or (n % m == 0) == l_mult)]
        n = pick[0]
        lengths.append(n)
        scalars += [d << (c * w)] * n
        idx += content_idx(content, n).tolist()
    if total_mod is not None:
        tail = (total_mod - int(bucket_counts(scalars, c).sum())) % m
        scalars += [1 << (c * 31)] * tail                # bucket 0 of the last window: behind every chain
        idx += [PLAIN[i % len(PLAIN)] for i in range(tail)]
    name = "%s-fix-%s-seg%d-%s" % (group, "+".join(str(x[2]) for x in chains), m, content)
    if nfill == 0:
        name += "-bare"
    if off_mod is not None or l_mult is not None or total_mod is not None:
        name += "-o%s-l%s-t%s" % (off_mod, {None: "x", True: "m", False: "n"}[l_mult], total_mod)
    claims = dict(chains=sorted(chains), lengths=lengths, off_mod=off_mod, l_mult=l_mult, total_mod=total_mod,
                  items=sum(-(-x[2] // FIXUP_ITEM) for x in chains if x[2] > FIXUP_SHORT),
                  nchains=sum(x[2] > FIXUP_ITEM for x in chains))
    return Case(name, group, c, scalars, idx, min_seg=m, claims=claims)


def fixup_cases(group):
    out = []
    one = lambda diff: [(0, 77, diff)]
    if group == "g1":
        for content in CONTENTS:
            for i, diff in enumerate(FIXUP_DIFFS):
                out.append(fixup_case("g1", one(diff), 1, content))
                # seg_len 3: the start offset modulo 3, the length's divisibility and the list's remainder rotate over the boundaries ...
                out.append(fixup_case("g1", one(diff), 3, content, off_mod=i % 3, l_mult=bool(i % 2), total_mod=(i + 1) % 3))
            # ... and are crossed in full on either side of the two thresholds
            for diff in (5, 1025):
                for off in (0, 1, 2):
                    for mult in (True, False):
                        if (off, mult) != (FIXUP_DIFFS.index(diff) % 3, bool(FIXUP_DIFFS.index(diff) % 2)):
                            out.append(fixup_case("g1", one(diff), 3, content, off_mod=off, l_mult=mult, total_mod=(off + 2) % 3))
            # three long chains queued at once: 2, 1 and 3 items, in different windows
            out.append(fixup_case("g1", [(0, 77, 1025), (3, 55, 500), (7, 99, 2049)], 1, content))
    else:
        for content in CONTENTS:
            for diff in FIXUP_DIFFS_G2:
                out.append(fixup_case("g2", one(diff), 1, content))
            for diff in (5, 1025):
                out.append(fixup_case("g2", one(diff), 3, content, off_mod=2, l_mult=False, total_mod=1))
    # nothing but the chain, P and -P in equal numbers: every partial sum, the bucket and the MSM itself are the point at infinity
    out += [fixup_case(group, one(diff), 1, "alternate", nfill=0) for diff in (5, 1025)]
    return out


# ------------------------------------------------------------------------------------------------ segment-edge cases
# (option, value): every accumulation variant; all of them must give the default's bytes
ACC_VARIANTS = {
    "g1": [(), (("acc_lazy", 0),), (("g1_inline", 2),), (("acc_pipeline", 1),), (("acc_pipeline", 3),), (("fixup_aux", 1),),
           (("g1_inline", 2), ("acc_lazy", 0)), (("acc_pipeline", 2),), (("g2_lazy", 2),)],
    "g2": [(), (("acc_lazy", 0),), (("g2_lazy", 2),), (("acc_pipeline", 2),), (("acc_pipeline", 3),), (("fixup_aux", 1),),
           (("g2_lazy", 2), ("acc_lazy", 0)), (("acc_pipeline", 1),), (("g1_inline", 2),)],
}
# bucket (= scalar - 1, window 0 only: every scalar is at most 2^7) -> the points of its terms in index order.  Offsets at seg_len 3:
SEGMENT_LAYOUT = [
    (1, [5, 6, 7]),                               # 0..2    begins at a segment start and ends at a segment end
    (2, [8]), (3, [9]), (4, [10]),                # 3..5    single-entry buckets
    (5, [11, 12]),                                # 6..7    begins at a segment start
    (6, [13, 14, 15, 16]),                        # 8..11   ends at a segment end, as the head of segment 3
    (7, [17]),                                    # 12
    (8, list(range(18, 28))),                     # 13..22  segments 5 and 6 are whole inside it: head only, no tail record
    (9, [28]),                                    # 23
    (10, [29, 30, 31, 5, 6, 7]),                  # 24..29  exactly two whole segments
    (11, [A, B, AB, 20, 21, 22]),                 # 30..35  a, b, (a + b): the doubling with a non-trivial ZZ, then more terms
    (12, [A, B, NEG + AB, 23, 24, 25]),           # 36..41  a, b, -(a + b): the cancellation, then more terms
    (13, [26]), (14, [27]),                       # 42, 43
    (20, [8, 9, 10]),                             # 44..46
    (30, [11, 12, 13, 14]),                       # 47..50
    (31, [C, D]),                                 # 51..52  c + d = a + b
    (127, [15, NEG + 15, 16]),                    # 53..55
    (128, [17, 18, 19, 20, 21]),                  # 56..60  the top bucket (digit 2^(c-1): not recentred); the last segment is short
]


def segment_case(group, variant, min_seg):
    # the input takes the first term of every bucket, top bucket first, then the second of each, ...: the sort has something to do,
    # and the index order it must keep inside a bucket is the order written above
    terms = sorted(((j, -v, pt) for v, pts in SEGMENT_LAYOUT for j, pt in enumerate(pts)))
    scalars, idx = [-v for _, v, _ in terms], [pt for _, _, pt in terms]
    name = "%s-seg%d-%s" % (group, min_seg, "+".join("%s=%d" % kv for kv in variant) or "default")
    return Case(name, group, 8, scalars, idx, options=dict(variant), min_seg=min_seg)


def segment_cases(group):
    return [segment_case(group, v, m) for v in ACC_VARIANTS[group] for m in (3, 6)]


def segment_facts(counts, seg_len):
    """which of the bookkeeping situations of msm_accumulate_kernel a term list holds"""
    offs = np.concatenate([[0], np.cumsum(counts)])
    total = int(offs[-1])
    facts = set()
    for g in np.nonzero(counts)[0]:
        s, e = int(offs[g]), int(offs[g + 1])               # [s, e)
        first, last = s // seg_len, (e - 1) // seg_len
        if s % seg_len == 0:
            facts.add("begins at a segment start")
        if e % seg_len == 0:
            facts.add("ends at a segment end")
        if e - s == 1:
            facts.add("single entry")
        if last - first >= 2:
            facts.add("head and tail of one segment")        # a middle segment lies whole inside the bucket
        if s % seg_len == 0 and e % seg_len == 0 and last - first == 1:
            facts.add("two whole segments")
        if last > first and last == (total - 1) // seg_len and total % seg_len:
            facts.add("spills into a short last segment")
    if total % seg_len:
        facts.add("short last segment")
    return facts


SEGMENT_FACTS = {"begins at a segment start", "ends at a segment end", "single entry", "head and tail of one segment", "two whole segments",
                 "spills into a short last segment", "short last segment"}


# ------------------------------------------------------------------------------------------------ digit cases
DIGIT_WIDTHS = (2, 3, 4, 8, 11, 12, 13, 16, 17, 20)
DIGIT_WIDTHS_G2 = (2, 13)


def digit_scalars(c, count=300):
    nw, half, full = nwin_of(c), 1 << (c - 1), (1 << c) - 1
    top = c * (nw - 1)
    s = [0, 1, 2, R_HALF, R_HALF + 1, R - 1, R - 2, 1 << 253, ((1 << 254) - 1) % R,
         (1 << 253) - 1, R - ((1 << 253) - 1)]               # all-ones: a carry through every window, as itself and as the fold of r - s
    s += [R_HALF - j for j in (1, 2, 3)] + [R_HALF + 1 + j for j in (1, 2, 3)]
    s += [R - 1 - (j << top) for j in (1, 2, 3) if R - 1 - (j << top) > 0] + [R_HALF - (j << top) for j in (1, 2) if R_HALF > j << top]
    # every window's value 2^(c-1) (the largest digit that is not recentred), 2^(c-1) + 1 (the first that is) and 2^c - 1, alone in the
    # scalar; the top window holds what of them stays below r.  Their negatives r - x in the lowest, a middle and the last full window
    for w in range(nw):
        for d in sorted({half, half + 1, full}):
            if d << (c * w) < R:
                s.append(d << (c * w))
                if w in (0, nw // 2, nw - 2):
                    s.append(R - (d << (c * w)))
    rng = random.Random(c)
    s += [rng.randrange(R) for _ in range(max(0, count - len(s)))]
    assert all(0 <= x < R for x in s)
    return s


def digit_case(group, c):
    s = digit_scalars(c)
    rng = random.Random(1000 + c)
    return Case("%s-digits-c%d" % (group, c), group, c, s, [rng.randrange(64) for _ in s])


def digit_cases(group):
    return [digit_case(group, c) for c in (DIGIT_WIDTHS if group == "g1" else DIGIT_WIDTHS_G2)]


# ------------------------------------------------------------------------------------------------ reduction cases
REDUCE_WIDTHS = (4, 5, 6, 8, 10, 13)                        # 8 .. 4096 buckets per window
REDUCE_PATTERNS = ("same", "signs", "two-forms", "two-forms-neg", "bucket0", "top-bucket", "last-chunk", "window-empty")
REDUCE_MODES = (1, 4, 5, 0)
REDUCE_CHUNKS = (0, 2, 4, 8, 16, 64)
REDUCE_G2 = [(4, "same"), (4, "two-forms"), (8, "same"), (8, "two-forms")]


def reduce_case(group, c, pattern, chunk=0):
    """Buckets filled through scalars (b + 1) << (c w) (a digit of at most 2^(c-1) is not recentred) in the three lowest windows and in
    as much of the top one as stays at most (r - 1) / 2.  chunk: the chunk size "last-chunk" is meant for (0: 4)."""
    nb, nw = 1 << (c - 1), nwin_of(c)
    k = chunk or 4
    while k > nb:
        k //= 2
    scalars, idx = [], []
    for w in (0, 1, 2, nw - 1):
        if pattern == "window-empty" and w == 1:
            continue
        for b in range(nb):
            s = (b + 1) << (c * w)
            if s > R_HALF:
                break
            if pattern in ("same", "window-empty"):
                pts = [REP]
            elif pattern == "signs":
                pts = [REP if b % 2 == 0 else NEG + REP]
            elif pattern == "two-forms":
                pts = [A, B] if b % 2 == 0 else [C, D]
            elif pattern == "two-forms-neg":
                pts = [A, B] if b % 2 == 0 else [NEG + C, NEG + D]
            elif pattern == "bucket0":
                pts = [REP, PLAIN[w % 5]] if b == 0 else []
            elif pattern == "top-bucket":
                pts = [REP, PLAIN[w % 5]] if b == nb - 1 else []
            else:
                assert pattern == "last-chunk"
                pts = [PLAIN[b % 9]] if b >= nb - k else []
            scalars += [s] * len(pts)
            idx += pts
    return Case("%s-reduce-c%d-%s%s" % (group, c, pattern, "-k%d" % chunk if pattern == "last-chunk" else ""), group, c, scalars, idx)
