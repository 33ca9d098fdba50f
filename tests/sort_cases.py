"""The sorted (scalar, window) term list every MSM reads, against a stable-sort model: the bucket scatter (csrc/bucket_sort.hip), the
bucket offsets and the stable compaction of the B-side list (msm_plan_filter, csrc/msm.hip).  Shared by
tests/test_sort_limits_host.py (every case sits on the boundary it names; the model agrees with a brute-force sort; the vectorised
recoding agrees with the integer one) and tests/test_sort_limits_gpu.py (device list, window totals, length and offsets == the model,
array for array).

The model is numpy plus Python integers.  Per window: k = the positions whose code is not ~0, ordered by a STABLE argsort of
code >> 1; x = k << 1 | code & 1, y = window * 2^(c-1) + bucket; the windows follow each other; offsets = searchsorted(y, 0 .. tb).
A bucket's sum does not depend on the order of its terms, so only this comparison sees a scatter that reorders a bucket."""
import zlib

import numpy as np

import msm_limit_cases as M

NONE = np.uint32(0xffffffff)                 # the digit kernel's code for digit 0
# csrc/bucket_sort.hip
SORT_ROUND, SORT_WCH, SORT_BCH = 64, 1024, 4096          # elements per round of a wave, per wave, per workgroup
SORT_MAX_BITS, SORT_MAX_BUCKET_BITS = 10, 24
SORT_PREFIX_WINDOWS = 32                     # above: the last pass reads its window bases from sort_window_prefix_kernel
SORT_PREFIX_STEP = 256                       # windows per step of that kernel's loop
# csrc/msm.hip
FILTER_CHUNK, FILTER_WAVES = 2048, 16
ERR_HIP = 3                                  # include/zkg16.h: what the scatter's "above build limit" throw maps to


# ------------------------------------------------------------------------------------------------ what the sources compute
def blocks_per_window(n):
    return -(-n // SORT_BCH)


def pass_bits(c):
    """msm_bucket_sort: two passes of <= 10 bits up to 20 bucket bits, three of <= 8 above"""
    bbits = c - 1
    npass = 2 if bbits <= 2 * SORT_MAX_BITS else 3
    return [bbits // npass + (1 if p < bbits % npass else 0) for p in range(npass)]


def scan_waves(nblk):
    return 1 if nblk <= 256 else 16 if nblk >= 4096 else (nblk + 255) // 256


def scan_shares(nblk, waves=None):
    """sort_scan_kernel (waves = scan_waves) / filter_scan_kernel (waves = 16): [lo, hi) of blocks per wave, empty shares left out"""
    waves = waves or scan_waves(nblk)
    per = (-(-nblk // waves) + 63) & ~63
    return [(w * per, min(w * per + per, nblk)) for w in range(waves) if w * per < nblk], per


def prefix_path(nwin):
    return nwin > SORT_PREFIX_WINDOWS


def filter_chunks(bound):
    return -(-bound // FILTER_CHUNK)


def filter_share(chunks):
    return (-(-chunks // FILTER_WAVES) + 63) & ~63


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------ the model
def model_sort(codes, c):
    """codes (nwin, n) uint32 -> (entries (len, 2) uint32 of (x, y), win_totals (nwin,) uint32)"""
    codes = np.asarray(codes, dtype=np.uint32)
    nb = 1 << (c - 1)
    xs, ys, totals = [], [], []
    for w in range(codes.shape[0]):
        row = codes[w]
        k = np.nonzero(row != NONE)[0]
        kc = row[k]
        order = np.argsort(kc >> 1, kind="stable")
        k, kc = k[order], kc[order]
        xs.append((k.astype(np.uint32) << 1) | (kc & 1))
        ys.append((kc >> 1) + np.uint32(w * nb))
        totals.append(len(k))
    ent = np.stack([np.concatenate(xs), np.concatenate(ys)], axis=1).astype(np.uint32) if xs else np.zeros((0, 2), np.uint32)
    return ent, np.asarray(totals, dtype=np.uint32)


def model_offsets(entries, tb):
    """offsets[g] = first position whose bucket id is >= g, g = 0 .. tb"""
    return np.searchsorted(entries[:, 1], np.arange(tb + 1, dtype=np.uint32), side="left").astype(np.uint32)


def brute_sort(codes, c):
    """the same list by Python's sort of (window, bucket, position) tuples (small cases)"""
    nb = 1 << (c - 1)
    t = [(w, int(v) >> 1, k, int(v) & 1) for w, row in enumerate(np.asarray(codes)) for k, v in enumerate(row) if v != NONE]
    t.sort(key=lambda e: (e[0], e[1], e[2]))
    return [((k << 1) | neg, w * nb + b) for w, b, k, neg in t]


# ------------------------------------------------------------------------------------------------ scalars -> digit codes
def codes_from_ints(scalars, c):
    """(digits, n) codes by the integer recoding of msm_limit_cases (any scalar below r)"""
    out = np.full((M.nwin_of(c), len(scalars)), NONE, dtype=np.uint32)
    for i, s in enumerate(scalars):
        for w, b, neg in M.recode(int(s), c):
            out[w, i] = (b << 1) | int(neg)
    return out


def codes_from_limbs(limbs, c):
    """the same, vectorised over (n, 4) u64 limbs (or (n,) uint64 values) of scalars below 2^253: those are never folded to r - s,
    so a window's value is c bits of the scalar plus the carry of the window below"""
    limbs = np.asarray(limbs, dtype=np.uint64)
    if limbs.ndim == 1:
        limbs = np.stack([limbs] + [np.zeros_like(limbs)] * 3, axis=1)
    assert limbs.shape[1] == 4 and not (limbs[:, 3] >> np.uint64(61)).any()
    l5 = np.concatenate([limbs, np.zeros((limbs.shape[0], 1), np.uint64)], axis=1)
    nw, mask, half, full = M.nwin_of(c), np.uint64((1 << c) - 1), 1 << (c - 1), 1 << c
    out = np.full((nw, limbs.shape[0]), NONE, dtype=np.uint32)
    carry = np.zeros(limbs.shape[0], dtype=np.int64)
    for w in range(nw):
        bit = w * c
        if bit < 256:
            j, off = bit >> 6, bit & 63
            v = l5[:, j] >> np.uint64(off)
            if off:
                v = v | (l5[:, j + 1] << np.uint64(64 - off))
            v = (v & mask).astype(np.int64)
        else:
            v = np.zeros(limbs.shape[0], dtype=np.int64)
        v = v + carry
        carry = (v > half).astype(np.int64)
        neg = carry == 1
        mag = np.where(neg, full - v, v)
        code = ((mag - 1) << 1) | neg
        out[w] = np.where(mag > 0, code, int(NONE)).astype(np.uint32)
    assert not carry.any()
    return out


def term_codes(per_vector, tabled):
    """digit codes of a batch, each (digits, n) -> the scatter's input: windows v * digits + w of n positions on a plain key, one
    window per vector of digits * n positions (position w * n + i) with window tables"""
    if tabled:
        return np.stack([cv.reshape(-1) for cv in per_vector])
    return np.concatenate(per_vector, axis=0)


def model_term_list(per_vector, c, tabled, mask=None):
    """-> (entries, offsets, tb): the list of a batch of scalar vectors, scalars with mask[i] != 0 removed"""
    if mask is not None:
        per_vector = [np.where(np.asarray(mask)[None, :] != 0, NONE, cv) for cv in per_vector]
    codes = term_codes(per_vector, tabled)
    ent, _ = model_sort(codes, c)
    tb = (1 << (c - 1)) * codes.shape[0]
    return ent, model_offsets(ent, tb), tb


def nonzero_digit_scalars(n, c, name):
    """n scalars below 2^253 none of whose signed digits is zero (so every position w * n + i of a tabled list is an entry: idx =
    q n - 1, q n, q n + 1 all occur), with both signs: window values 1 .. 2^c - 2 (2^c - 1 plus a carry would be digit 0), the top
    window small enough to stay below 2^253 with its carry.  -> ((n, 4) u64 limbs, Python ints)"""
    rng = _rng(name)
    nw = M.nwin_of(c)
    top_bits = 253 - c * (nw - 1)
    assert top_bits >= 1
    vals = rng.integers(1, (1 << c) - 1, size=(nw, n), dtype=np.int64)
    vals[nw - 1] = rng.integers(1, max(2, (1 << top_bits) - 1), size=n, dtype=np.int64)
    ints = [0] * n
    for w in range(nw):
        col = vals[w].tolist()
        sh = c * w
        for i in range(n):
            ints[i] |= col[i] << sh
    return M.canon_vec(ints), ints


def boundary_scalars():
    """full-width scalars on the recoding's edges for the small term-list cases"""
    return [0, 1, 2, M.R_HALF, M.R_HALF + 1, M.R - 1, M.R - 2, 1 << 253, (1 << 253) - 1, M.R - ((1 << 253) - 1), (1 << 62) - 1]


# ------------------------------------------------------------------------------------------------ raw cases
class RawCase:
    """codes for one call of the scatter; make() builds them (deterministic), claims name the boundary the case sits on"""

    def __init__(self, name, c, nwin, n, fill, **claims):
        self.name, self.c, self.nwin, self.n, self._fill, self.claims = name, c, nwin, n, fill, claims

    def __repr__(self):
        return self.name

    def make(self):
        codes = np.full((self.nwin, self.n), NONE, dtype=np.uint32)
        self._fill(codes, _rng(self.name), 1 << (self.c - 1))
        return codes


def _code(bucket, neg):
    return ((np.asarray(bucket, dtype=np.uint64) << np.uint64(1)) | np.asarray(neg, dtype=np.uint64)).astype(np.uint32)


GEOMETRY_N = (1, 63, 64, 65, 128, 1023, 1024, 1025, 4095, 4096, 4097, 8193)       # 128: every bucket of c = 8 exactly once
GEOMETRY_PATTERNS = ("one-bucket", "descending", "alternate-neg", "all-none", "none-block", "last-only", "random")


def _geometry_fill(pattern, block=0):
    def fill(codes, rng, nb):
        n = codes.shape[1]
        i = np.arange(n)
        if pattern == "one-bucket":          # ranks carry across all 16 rounds, the 4 waves and the blocks
            codes[0] = _code(np.full(n, 77), 0)
        elif pattern == "descending":        # every bucket once per 2^(c-1) positions, top bucket first
            codes[0] = _code(nb - 1 - i % nb, 0)
        elif pattern == "alternate-neg":
            codes[0] = _code(rng.integers(0, nb, n), i & 1)
        elif pattern == "none-block":        # ~0 over exactly one whole block, random codes elsewhere
            codes[0] = _code(rng.integers(0, nb, n), rng.integers(0, 2, n))
            codes[0, block * SORT_BCH:(block + 1) * SORT_BCH] = NONE
        elif pattern == "last-only":
            codes[0, n - 1] = _code(nb - 1, 1)
        elif pattern == "random":
            codes[0] = _code(rng.integers(0, nb, n), rng.integers(0, 2, n))
            codes[0, rng.random(n) < 0.25] = NONE
        else:
            assert pattern == "all-none"
    return fill


def geometry_cases():
    out = []
    for n in GEOMETRY_N:
        for p in GEOMETRY_PATTERNS:
            if p == "none-block":
                for blk in range((n - 1) // SORT_BCH):       # whole blocks followed by at least one more element
                    out.append(RawCase("geom-n%d-none-block%d" % (n, blk), 8, 1, n, _geometry_fill(p, blk), pattern=p, block=blk))
            else:
                out.append(RawCase("geom-n%d-%s" % (n, p), 8, 1, n, _geometry_fill(p), pattern=p))
    return out


SPLIT_WIDTHS = {2: [1, 0], 3: [1, 1], 12: [6, 5], 21: [10, 10], 22: [7, 7, 7], 23: [8, 7, 7], 24: [8, 8, 7], 25: [8, 8, 8]}
SPLIT_N = 4097
REFUSED_C = 26


def _split_fill(pattern, p=0):
    def fill(codes, rng, nb):
        n = codes.shape[1]
        c = nb.bit_length()
        if pattern == "extremes":            # bucket 0 and bucket 2^(c-1) - 1
            b = np.where(rng.integers(0, 2, n) == 1, nb - 1, 0)
        elif pattern == "one-pass":          # buckets that differ only in the bits pass p sorts by
            bits = pass_bits(c)
            shift = sum(bits[:p])
            fixed = int(rng.integers(0, nb)) & ~(((1 << bits[p]) - 1) << shift)
            b = fixed | (rng.integers(0, 1 << bits[p], n) << shift)
        else:
            b = rng.integers(0, nb, n)
        codes[0] = _code(b, rng.integers(0, 2, n))
        codes[0, rng.random(n) < 0.1] = NONE
    return fill


def split_cases():
    out = []
    for c, bits in SPLIT_WIDTHS.items():
        out.append(RawCase("split-c%d-extremes" % c, c, 1, SPLIT_N, _split_fill("extremes"), bits=bits))
        for p, b in enumerate(bits):
            if b:
                out.append(RawCase("split-c%d-pass%d" % (c, p), c, 1, SPLIT_N, _split_fill("one-pass", p), bits=bits, only_pass=p))
        out.append(RawCase("split-c%d-random" % c, c, 1, SPLIT_N, _split_fill("random"), bits=bits))
    return out


WINDOW_COUNTS = (1, 32, 33, 256, 257, 513)
WINDOW_N = 4500                              # two blocks: a window that keeps at most 4096 leaves the later passes' second block empty


def window_kept(nwin, n):
    """entries each window keeps: very different counts; the first, the middle and the last window are empty (from 3 windows on)"""
    ladder = [1, n, SORT_BCH, 0, SORT_BCH + 1, 37, n - 1, SORT_ROUND, SORT_WCH + 1]
    kept = [ladder[w % len(ladder)] for w in range(nwin)]
    if nwin >= 3:
        kept[0] = kept[nwin // 2] = kept[nwin - 1] = 0
    return [min(k, n) for k in kept]


def _window_fill(codes, rng, nb):
    nwin, n = codes.shape
    for w, k in enumerate(window_kept(nwin, n)):
        pos = np.sort(rng.permutation(n)[:k])            # scattered over the window, not a prefix: the first pass compacts
        codes[w, pos] = _code(rng.integers(0, nb, k), rng.integers(0, 2, k))


def window_cases():
    out = [RawCase("win-%d-c8" % nw, 8, nw, WINDOW_N, _window_fill, prefix=prefix_path(nw)) for nw in WINDOW_COUNTS]
    # three passes: the middle pass reads in_count[w] entries of ws.keys and writes ws.stage; 8193 = three blocks, so windows that keep
    # one entry or one block leave one or two whole trailing blocks of the later passes empty
    out.append(RawCase("win-33-c22-n8193", 22, 33, 2 * SORT_BCH + 1, _window_fill, prefix=True))
    out.append(RawCase("win-9-c22-n8193", 22, 9, 2 * SORT_BCH + 1, _window_fill, prefix=False))
    return out


SCAN_BLOCKS = (256, 257, 769, 3840, 3841)
SCAN_C = 3                                   # 1 + 1 bucket bits: two rows of counts per pass
SCAN_SHARES = {256: (1, [256]), 257: (2, [192, 65]), 769: (4, [256, 256, 256, 1]), 3840: (15, [256] * 15), 3841: (16, [256] * 15 + [1])}


def _scan_fill(codes, rng, nb):
    n = codes.shape[1]
    keep = rng.random(n) < 0.1               # nine codes in ten are ~0: the model sorts a tenth of n
    keep[n - 1] = True                       # the last block holds one element
    k = int(keep.sum())
    codes[0, keep] = _code(rng.integers(0, nb, k), rng.integers(0, 2, k))


def assert_scan_codes(case, codes):
    """a tenth of the codes kept, and the first and the last block of every wave's share hold kept codes"""
    valid = codes[0] != NONE
    assert 0.09 < valid.mean() < 0.11
    shares, _ = scan_shares(case.claims["nblk"])
    for lo, hi in shares:
        for blk in (lo, hi - 1):
            assert valid[blk * SORT_BCH:(blk + 1) * SORT_BCH].any()


def scan_case(nblk):
    return RawCase("scan-%dblk" % nblk, SCAN_C, 1, (nblk - 1) * SORT_BCH + 1, _scan_fill, nblk=nblk, shares=SCAN_SHARES[nblk])


# ------------------------------------------------------------------------------------------------ term-list cases
class TermCase:
    """scalars of a batch -> the list a plan builds.  vectors: per vector (limbs (n, 4) u64, codes (digits, n))"""

    def __init__(self, name, c, tabled, vectors, mask=None, **claims):
        self.name, self.c, self.tabled, self.mask, self.claims = name, c, tabled, mask, claims
        self.limbs = np.stack([v[0] for v in vectors])
        self.codes = [v[1] for v in vectors]
        self.n, self.batch, self.digits = self.limbs.shape[1], len(vectors), M.nwin_of(c)
        self.bound = self.batch * self.n * self.digits       # MsmPlan::total_entries

    def __repr__(self):
        return self.name

    def plan(self):
        nwin = self.batch * (1 if self.tabled else self.digits)
        return (self.c, nwin, self.digits, nwin << (self.c - 1))

    def expected(self):
        return model_term_list(self.codes, self.c, self.tabled, self.mask)


_vec_cache = {}


def int_vector(n, c, seed):
    """n full-width scalars (the recoding's edges first, then random below r) by the integer recoding"""
    key = ("int", n, c, seed)
    if key not in _vec_cache:
        import random
        rng = random.Random(seed)
        s = (boundary_scalars() + [rng.randrange(M.R) for _ in range(n)])[:n]
        _vec_cache[key] = (M.canon_vec(s), codes_from_ints(s, c))
    return _vec_cache[key]


def nonzero_vector(n, c):
    key = ("nz", n, c)
    if key not in _vec_cache:
        limbs, _ = nonzero_digit_scalars(n, c, "nonzero-%d-%d" % (n, c))
        _vec_cache[key] = (limbs, codes_from_limbs(limbs, c))
    return _vec_cache[key]


def small62_vector(n, c):
    key = ("u62", n, c)
    if key not in _vec_cache:
        v = _rng("u62-%d-%d" % (n, c)).integers(0, 1 << 62, n, dtype=np.uint64)
        limbs = np.stack([v] + [np.zeros_like(v)] * 3, axis=1)
        _vec_cache[key] = (limbs, codes_from_limbs(v, c))
    return _vec_cache[key]


PLAN_N = 1000


def plan_cases():
    """plain at c = 13 (batch 3 = 60 windows: the prefix path), tabled at c = 13 and 24; batch 1 and 3"""
    out = []
    for tabled, c in ((False, 13), (True, 13), (True, 24)):
        for batch in (1, 3):
            vec = [int_vector(PLAN_N, c, 100 + v) for v in range(batch)]
            out.append(TermCase("%s-c%d-batch%d" % ("tabled" if tabled else "plain", c, batch), c, tabled, vec))
    return out


MASK_N = (3, 49, 1000, 1002, 4097, 80660, 80691)         # 80660 * 13 > 2^20 >= 80659 * 13
# filter_keep estimates q = idx / n as (uint32)(idx * (1.0 / n)) in double precision and corrects it by one.  At none of 3, 1000, 4097
# and 80660 is the estimate ever wrong for idx < 20 n (the host test computes it), so those sizes would pass without the correction;
# at these it is one too small at multiples of n (49 * (1.0 / 49) < 1), which is what the correction is for
MASK_N_ESTIMATE_OFF = (49, 1002, 80691)


def quotient_estimate_misses(n, digits):
    """-> {idx: i} for the positions idx < digits * n at which idx - (uint32)(idx * (1.0 / n)) * n is outside [0, n)"""
    idx = np.arange(n * digits, dtype=np.int64)
    q = (idx.astype(np.float64) * (np.float64(1.0) / np.float64(n))).astype(np.uint32).astype(np.int64)
    i = idx - q * n
    bad = np.nonzero((i < 0) | (i >= n))[0]
    return dict(zip(bad.tolist(), i[bad].tolist()))
MASK_KINDS = ("none", "all", "alternate", "first", "last")
MASK_C = 13


def mask_of(kind, n):
    m = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternate":
        m[0::2] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[n - 1] = 1
    else:
        assert kind == "none"
    return m


def mask_case(n, tabled, kind):
    return TermCase("mask-%s-n%d-%s" % ("tabled" if tabled else "plain", n, kind), MASK_C, tabled, [nonzero_vector(n, MASK_C)], mask_of(kind, n))


# The compaction works in chunks of 2,048 entries of the list's upper bound batch * n * digits.  No width has a digit count that divides
# 2,047 = 23 * 89 or 2,049 = 3 * 683, and 2^21 is no multiple of 20, so the bounds sit as close to the chunk edges as a width allows;
# the exact lengths 2,047 | 2,048 | 2,049 are met by the list itself (digits that are zero) under a two-chunk bound.
FILTER_SMALL = ((12, 93, 2046, 1), (8, 64, 2048, 1), (14, 108, 2052, 2))          # (c, n, bound, chunks)
FILTER_EXACT = (2047, 2048, 2049)            # list lengths under the bound 65 * 32 = 2,080 (c = 8)
FILTER_LARGE = ((104857, 2097140, 1024, 64), (104858, 2097160, 1025, 128))      # (n, bound, chunks, share) at c = 13


def filter_small_case(c, n):
    return TermCase("filter-c%d-n%d" % (c, n), c, False, [nonzero_vector(n, c)], mask_of("alternate", n))


def filter_exact_case(length):
    """65 scalars at c = 8 whose window values are 1 .. 127 (no carries: the digits are the values), but for window 3 of the first
    65 * 32 - length scalars, which is zero: the list has exactly `length` entries"""
    c, n = 8, 65
    key = ("exact", length)
    if key not in _vec_cache:
        nw = M.nwin_of(c)
        vals = _rng("exact").integers(1, 128, size=(nw, n))
        vals[nw - 1] = vals[nw - 1] % 31 + 1             # below 2^253
        drop = n * nw - length
        assert 0 <= drop <= n
        vals[3, :drop] = 0
        ints = [sum(int(vals[w, i]) << (c * w) for w in range(nw)) for i in range(n)]
        _vec_cache[key] = (M.canon_vec(ints), codes_from_ints(ints, c))
    return TermCase("filter-exact-%d" % length, c, False, [_vec_cache[key]], mask_of("alternate", n), length=length)


def filter_large_case(n, full_width):
    vec = nonzero_vector(n, MASK_C) if full_width else small62_vector(n, MASK_C)
    return TermCase("filter-n%d-%s" % (n, "full" if full_width else "u62"), MASK_C, full_width, [vec], mask_of("alternate", n))
