"""The streamed proof's rounds (zkg16_prove_matrix): which part of the assignment every variable arrives in, the term list of every
part, and the bucket-wise merge of the rounds' bucket arrays (msm_bucket_merge_kernel).  Shared by tests/test_stream_rounds_host.py
(the model agrees with zkg16_matrix_stream_bounds, every round case holds the coincidence it names, and its rounds add up to the one-
round sum) and tests/test_stream_rounds_gpu.py (the device's part map == what production writes in each part == the model; a
plain-key MSM fed in rounds == the expected point; whole streamed proofs at small sizes == the two-step proof).

Pure Python and numpy.  The first half restates csrc/witness.hip: MatrixWitnessLayout, the slice rule of matrix_stream_slices and
the part map, the last written from what matrix_stream_produce writes (permutation p of a sponge fills 265 values, the first one 260)
and not from wit_part_of_kernel's own arithmetic.  The second half sits on tests/msm_limit_cases.py: its 64 points with known logs and
its digit model.  A round case is (scalars, part labels, window bits); the model gives every round's bucket sums as integers mod r —
the group is cyclic of order r, so a bucket's log IS its point, and equal / opposite / infinity are read off the integers — and the
expected value is [sum s_i k_i mod r]G: one oracle scalar multiplication, nothing the device computes."""
import random

import numpy as np

import msm_limit_cases as M
from helpers import G1_GEN_LIMBS, G2_GEN_LIMBS

R = M.R

# ------------------------------------------------------------------------------------------------ the assignment's layout and parts
POSEIDON_RATE, PERM_WITNESSES, FIRST_PERM_SKIPPED = 2, 265, 5
SLICE_MIN_DEFAULT = 512
GROW = (0.06, 0.20, 0.45, 0.80, 1.0)
GROW_FROM = 4096                             # permutations from which the default is five growing slices


class Layout:
    """MatrixWitnessLayout: 1 | hash_a hash_b hash_c | a | b | sponge(a) | sponge(b) | c | products and partial sums | sponge(c)"""

    def __init__(self, n):
        self.n, self.nn, self.ni = n, n * n, 4
        self.perms = (self.nn + POSEIDON_RATE - 1) // POSEIDON_RATE
        self.hw = self.perms * PERM_WITNESSES - FIRST_PERM_SKIPPED
        self.off_a = self.ni
        self.off_b = self.off_a + self.nn
        self.off_ha = self.off_b + self.nn
        self.off_hb = self.off_ha + self.hw
        self.off_mc = self.off_hb + self.hw
        self.off_mm = self.off_mc + self.nn
        self.off_hc = self.off_mm + self.nn * (n + 1)
        self.total = self.off_hc + self.hw


def slice_bounds(perms, parts_wanted=0, slice_min=SLICE_MIN_DEFAULT):
    """-> [0, ..., perms]: the first permutation of every slice.  parts_wanted 0: five growing slices from 4096 permutations on, else
    four equal ones; k: k equal ones; either way as many fewer as it takes for a slice to hold slice_min permutations."""
    assert 0 <= parts_wanted <= 8 and slice_min >= 1
    growing = parts_wanted == 0 and perms >= GROW_FROM
    if growing:
        return [0] + [int(perms * g + 0.5) for g in GROW[:-1]] + [perms]
    k = parts_wanted or 4
    while k > 1 and perms // k < slice_min:
        k -= 1
    return [perms * i // k for i in range(k)] + [perms]


def part_map(n, bounds):
    """(total + 3,) uint8: the part in which variable i becomes valid, then the r, s, -rs slots of the z-side scalar vector.  Part 0
    is what needs only a and b: the constant, a, b, c, the products and the trailing slots.  Part 1 + s: the values of the permutations
    of slice s of each of the three sponges.  The last part also brings the three hashes (indices 1 to 3)."""
    L = Layout(n)
    slices = len(bounds) - 1
    assert bounds[0] == 0 and bounds[-1] == L.perms and all(bounds[i] < bounds[i + 1] for i in range(slices))
    slice_of_perm = np.zeros(L.perms, dtype=np.uint8)
    for s in range(slices):
        slice_of_perm[bounds[s]:bounds[s + 1]] = s
    written = np.full(L.perms, PERM_WITNESSES)          # values permutation p writes
    written[0] -= FIRST_PERM_SKIPPED
    sponge = 1 + np.repeat(slice_of_perm, written)
    assert sponge.shape == (L.hw,)
    part = np.zeros(L.total + 3, dtype=np.uint8)
    part[1:4] = slices
    for off in (L.off_ha, L.off_hb, L.off_hc):
        part[off:off + L.hw] = sponge
    return part


# ------------------------------------------------------------------------------------------------ rounds of one MSM
def _gen(group):
    return G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS


class RoundCase:
    """One plain-key MSM fed in `parts` rounds: scalars (Python ints), idx (which of the 64 points each base is), part (the round of
    each scalar), c; claims: [(window, digit, [what the merge of round 1, 2, ... meets in that bucket])] with the words of
    merge_kinds."""

    def __init__(self, name, group, c, scalars, idx, part, parts, claims=(), options=None, spill=None):
        assert len(scalars) == len(idx) == len(part) and all(0 <= p < 256 for p in part)
        self.name, self.group, self.c, self.parts = name, group, c, parts
        self.scalars, self.idx, self.part = list(scalars), np.asarray(idx, dtype=np.int64), np.asarray(part, dtype=np.uint8)
        self.claims, self.options, self.spill = list(claims), dict(options or {}), spill
        self.nb = 1 << (c - 1)
        self.tb = self.nb * M.nwin_of(c)

    def __repr__(self):
        return self.name

    def arrays(self, oracle):
        return M.table(oracle, self.group)[self.idx], M.canon_vec(self.scalars)

    def expected_log(self):
        return sum(s * M.LOGS[i] for s, i in zip(self.scalars, self.idx.tolist())) % R

    def expected(self, oracle):
        return oracle.point_mul(self.group, _gen(self.group), M.canon_vec([self.expected_log()])[0])

    def round_scalars(self, k):
        """the scalar vector round k sees: the others count as zero"""
        return [s if p == k else 0 for s, p in zip(self.scalars, self.part.tolist())]

    def round_counts(self, k):
        """terms per global bucket of round k's sorted list"""
        return M.bucket_counts(self.round_scalars(k), self.c)

    def round_entries(self):
        """offsets[tb] of every round: its non-zero digits"""
        return [int(self.round_counts(k).sum()) for k in range(self.parts)]

    def round_sums(self):
        """[round][global bucket] -> log of the bucket's sum in that round, None where the round puts no term there"""
        out = [dict() for _ in range(self.parts)]
        for s, i, p in zip(self.scalars, self.idx.tolist(), self.part.tolist()):
            if p >= self.parts:
                continue
            for w, b, neg in M.recode(s, self.c):
                g = w * self.nb + b
                out[p][g] = (out[p].get(g, 0) + (R - M.LOGS[i] if neg else M.LOGS[i])) % R
        return out

    def weighted(self, sums):
        """sum over buckets of (digit) 2^(c w) (bucket's log): what the reduction and the host Horner make of one bucket array"""
        return sum((g % self.nb + 1) * (1 << (self.c * (g // self.nb))) * v for g, v in sums.items()) % R

    def merge_kinds(self, g):
        """what msm_bucket_merge_kernel meets in bucket g when it adds round 1, 2, ... to the running sum:
        "skip"      the round's bucket is infinity (untouched, or its terms cancelled): the kernel returns early
        "into-inf"  the running sum is infinity, the round's bucket is not
        "double"    both hold the same point: the addition must take its doubling branch
        "cancel"    opposite points: the sum becomes infinity
        "add"       anything else"""
        sums = self.round_sums()
        acc = sums[0].get(g, 0)
        kinds = []
        for k in range(1, self.parts):
            b = sums[k].get(g, 0)
            kinds.append("skip" if b == 0 else "into-inf" if acc == 0 else "double" if acc == b else "cancel" if (acc + b) % R == 0 else "add")
            acc = (acc + b) % R
        return kinds


def term(c, w, d):
    """the scalar whose one digit is d in window w (bucket d - 1: a digit of at most 2^(c-1) is not recentred)"""
    s = d << (c * w)
    assert 1 <= d <= 1 << (c - 1) and s <= M.R_HALF
    return s


def _fillers(rng, c, count, reserved, labels):
    """random 240-bit scalars that stay out of the `reserved` global buckets and out of each other's (one term per bucket: a filler
    meets nothing in a merge, and no bucket of theirs crosses a lane edge), on random points, in rounds drawn from `labels`"""
    scalars = M.sparse_filler(c, count, 1, reserved)
    return scalars, [rng.randrange(64) for _ in scalars], [rng.choice(labels) for _ in scalars]


def bucket_case(group, name, parts, placed, c=8, fill_labels=None, nfill=20, options=None, spill=None):
    """placed: [(window, digit, [(point, round), ...], [kinds])]: the named buckets; fillers everywhere else, in the rounds
    fill_labels (default: every round)"""
    nb = 1 << (c - 1)
    rng = random.Random("%s/%s" % (group, name))
    reserved = {w * nb + d - 1 for w, d, _, _ in placed}
    labels = list(range(parts)) if fill_labels is None else list(fill_labels)
    scalars, idx, part = _fillers(rng, c, nfill, reserved, labels) if nfill else ([], [], [])
    for w, d, terms, _ in placed:
        for pt, k in terms:
            scalars.append(term(c, w, d))
            idx.append(pt)
            part.append(k)
    order = list(range(len(scalars)))                   # the named terms do not sit at the end of the vector
    rng.shuffle(order)
    pick = lambda xs: [xs[j] for j in order]
    claims = [(w, d, kinds) for w, d, _, kinds in placed]
    return RoundCase("%s-%s" % (group, name), group, c, pick(scalars), pick(idx), pick(part), parts, claims, options, spill)


def spread_case(group, c, parts=5, count=150):
    """full-range scalars (the digit cases' boundary values among them) over every window, in random rounds"""
    s = M.digit_scalars(c, count)
    rng = random.Random("spread/%s/%d" % (group, c))
    return RoundCase("%s-windows-c%d" % (group, c), group, c, s, [rng.randrange(64) for _ in s], [rng.randrange(parts) for _ in s], parts)


SPILL_TERMS = (2, 6, 1030)          # a bucket of this many terms at seg_len 1 goes on over 1, 5 and 1029 further segments:
#                                     the smallest spill, the first that is queued as a work item (FIXUP_SHORT + 1), and a chain of two items


def spill_case(nterms, fixup_aux):
    """G1.  Round 0 puts one point into bucket (0, 77), round 1 `nterms` distinct ones: with min_seg 1 each lane of round 1 holds one
    of them, so the bucket's value exists only once the fix-up kernels have folded the lanes' partial sums — the merge must come after
    them.  Fillers in round 0 only: round 1's list is the bucket alone."""
    pts = M.content_idx("distinct", nterms).tolist()
    placed = [(0, 77, [(M.PLAIN[3], 0)] + [(p, 1) for p in pts], ["add"])]
    return bucket_case("g1", "spill-%d-aux%d" % (nterms, fixup_aux), 2, placed, fill_labels=[0], options={"min_seg": 1, "fixup_aux": fixup_aux},
                       spill=dict(round=1, bucket=76, diff=nterms - 1))


def round_cases(group):
    A, B, C, D, AB, REP, NEG = M.A, M.B, M.C, M.D, M.AB, M.REP, M.NEG
    P, Q = M.PLAIN[0], M.PLAIN[1]
    out = [
        # a + b = c + d: the two rounds end on one point in two XYZZ forms, neither with ZZ = 1
        bucket_case(group, "equal-forms", 2, [(0, 77, [(A, 0), (B, 0), (C, 1), (D, 1)], ["double"]),
                                              (3, 55, [(C, 0), (D, 0), (B, 1), (A, 1)], ["double"])]),
        # ... and against the affine base a + b itself (ZZ = 1), either way round; -(a + b) cancels
        bucket_case(group, "affine-ab", 2, [(0, 77, [(A, 0), (B, 0), (AB, 1)], ["double"]),
                                            (2, 128, [(AB, 0), (A, 1), (B, 1)], ["double"]),
                                            (5, 1, [(A, 0), (B, 0), (NEG + AB, 1)], ["cancel"])]),
        # P, then -P: infinity; then Q is added to that infinity.  Beside it the same with the sum of two points
        bucket_case(group, "cancel-then-add", 3, [(0, 77, [(P, 0), (NEG + P, 1), (Q, 2)], ["cancel", "into-inf"]),
                                                  (7, 99, [(A, 0), (B, 0), (NEG + C, 1), (NEG + D, 1), (Q, 2)], ["cancel", "into-inf"]),
                                                  (1, 3, [(P, 0), (NEG + P, 0), (Q, 1), (Q, 2)], ["into-inf", "double"])]),
        bucket_case(group, "last-round-only", 3, [(0, 77, [(P, 2)], ["skip", "into-inf"]), (31, 9, [(P, 2), (Q, 2)], ["skip", "into-inf"])]),
        bucket_case(group, "first-round-only", 3, [(0, 77, [(P, 0)], ["skip", "skip"]), (31, 9, [(P, 0), (Q, 0)], ["skip", "skip"]),
                                                   (4, 5, [(P, 0), (Q, 1), (NEG + Q, 1)], ["skip", "skip"])]),
        bucket_case(group, "first-round-empty", 3, [(0, 77, [(P, 1), (Q, 2)], ["into-inf", "add"])], fill_labels=[1, 2]),
        bucket_case(group, "middle-round-empty", 3, [(0, 77, [(P, 0), (Q, 2)], ["skip", "add"])], fill_labels=[0, 2]),
        # a part no scalar belongs to, as the last round: parts = 4 with labels 0 .. 2
        bucket_case(group, "label-unused", 4, [(0, 77, [(P, 0), (P, 1), (Q, 2)], ["double", "add", "skip"])], fill_labels=[0, 1, 2]),
        bucket_case(group, "all-in-part-0-of-4", 4, [(0, 77, [(P, 0), (Q, 0)], ["skip"] * 3)], fill_labels=[0]),
        bucket_case(group, "all-in-part-2-of-4", 4, [(0, 77, [(P, 2), (Q, 2)], ["skip", "into-inf", "skip"])], fill_labels=[2]),
        # eight rounds: P into one bucket every time (P + P, then 2P + P, 3P + P, ...), P and -P in turns into another
        bucket_case(group, "eight-rounds", 8, [(0, 77, [(REP, k) for k in range(8)], ["double"] + ["add"] * 6),
                                               (6, 128, [(REP if k % 2 == 0 else NEG + REP, k) for k in range(8)], ["cancel", "into-inf"] * 3 + ["cancel"])]),
        spread_case(group, 4),
        spread_case(group, 8),
    ]
    if group == "g1":
        out += [spill_case(n, aux) for n in SPILL_TERMS for aux in (0, 1)]
    return out
