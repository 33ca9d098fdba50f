"""Cases for the limits tests of key generation (tests/test_setup_limits_host.py proves them on the CPU, tests/test_setup_limits_gpu.py
runs them on the device): scalars that reach the first and the last table entry of every fixed-base window, zero / non-zero masks for
the batched to-affine, small R1CS systems with empty ranges, and the key the setup has to produce for them.  Everything here is
Python integers, numpy and the CPU oracle; nothing imports the product library."""
import random

import numpy as np

import pyref as P
from helpers import G1_GEN_LIMBS, G2_GEN_LIMBS, csr_from_rows, fr_canon, fr_canon_vec, fr_mont_vec

R = P.R_MOD
WIDTHS = list(range(4, 15)) + [16, 18, 20]          # every value option "fixed_base_bits" takes, 0 (= by batch size) aside
TOP_BIT = R.bit_length() - 1                         # 254: a canonical scalar has no bit above it


# ---------------------------------------------------------------------------------------------- fixed-base digits
def two_level(w):
    """fixed_base_run builds widths >= 16 (even ones only) from two half-width levels (fixed_base_combine_kernel)"""
    return w >= 16


def nwin(w):
    return (256 + w - 1) // w


def digits(k, w):
    """fixed_base_kernel's digits of scalar k at width w: digit j = bits [j w, j w + w) of the 256-bit scalar; a digit d != 0 reads
    table entry d - 1 of window j."""
    mask = (1 << w) - 1
    return [(k >> (j * w)) & mask for j in range(nwin(w))]


def split(d, w):
    """entry d of a two-level window is half[2 j][dl] + half[2 j + 1][dh] (fixed_base_combine_kernel) -> (dl, dh)"""
    h = w // 2
    return d & ((1 << h) - 1), d >> h


def max_digit(j, w):
    """the largest digit a canonical scalar can have in window j whatever its other digits are"""
    return min((1 << w) - 1, (R - 1) >> (j * w))


def top_window(w):
    """the last window a canonical scalar reaches: the one that holds bit 254.  nwin(w) counts windows up to bit 255, so for some
    widths (5, 15, ...) one more window exists that no scalar below r has a digit in."""
    return TOP_BIT // w


def _below_r(v, j, w):
    """v (only digit: window j) with window j - 1 at its maximum too — the full digit, or what r - 1 has there where the full digit
    would pass r (the top window at its own maximum)"""
    full = v | (((1 << w) - 1) << ((j - 1) * w))
    if full < R:
        return full
    return v | ((((R - 1) >> ((j - 1) * w)) & ((1 << w) - 1)) << ((j - 1) * w))


def class_scalars(w):
    """two-level widths: {(window, class): (scalar, reachable)} for windows 0, the middle one and the top one and the classes
    "lo" (dl != 0, dh == 0), "hi" (dl == 0, dh != 0), "full" (both halves at 2^(w/2) - 1).  In the top window a class whose smallest
    digit is above max_digit cannot occur below r: reachable is False there and the scalar is the window's last reachable entry."""
    h = w // 2
    out = {}
    t = top_window(w)
    for j in (0, t // 2, t):
        for name, d in (("lo", min((1 << h) - 1, max_digit(j, w))), ("hi", 1 << h), ("full", (1 << w) - 1)):
            ok = 0 < d <= max_digit(j, w)
            out[(j, name)] = ((d if ok else max_digit(j, w)) << (j * w), ok)
    return out


def edge_scalars(w, n_random=64):
    """Canonical scalars whose digits at width w reach, in every window a scalar below r can reach, the first table entry and the
    last reachable one — alone and with the window below at its maximum, so that the entries on both sides of each window boundary of
    the table (entry 2^w - 2 of window j - 1 lies next to entry 0 of window j) are read.
    acc == +-p (the incoming table point equal to the accumulated sum or its negative, the case the mixed addition cannot take) does
    not occur for canonical scalars: the windows go upwards, the partial sum is [k mod 2^(j w)] G with k mod 2^(j w) < 2^(j w) <=
    d 2^(j w) < r, so its log is below the incoming multiple's and the two logs do not add up to r either.  Not hunted for."""
    ks = []
    t = top_window(w)
    for j in range(t + 1):
        first, last = 1 << (j * w), max_digit(j, w) << (j * w)
        ks += [first, last]
        if j:
            ks += [_below_r(first, j, w), _below_r(last, j, w)]
    ks += [0, 1, 2, R - 1, R - 2, (1 << 254) - 1, ((1 << 255) - 19) % R]          # 2^255 - 19 is above r: reduced
    if two_level(w):
        ks += [k for k, _ in class_scalars(w).values()]
    rng = random.Random(7000 + w)
    ks += [P.rand_fr(rng) for _ in range(n_random)]
    seen, out = set(), []
    for k in ks:
        if k not in seen:
            seen.add(k)
            out.append(k)
    assert all(0 <= k < R for k in out)
    return out


def random_base(oracle, group, seed):
    """a random multiple of the standard generator, as synth.make_pk draws a key's generators"""
    k = P.rand_fr(random.Random(seed))
    return oracle.point_mul(group, G1_GEN_LIMBS if group == "g1" else G2_GEN_LIMBS, fr_canon(k))[0]


# ---------------------------------------------------------------------------------------------- to-affine: infinity patterns
PATTERN_SIZES = [1, 2, 4, 5, 63, 64, 65, 256, 257, 1023]
SATURATED_SIZE = 300001          # above four points per thread of a full launch (256 CUs x 4 waves x 64 lanes): the thread count saturates


def chain_threads(n):
    """threads batch_affine_run (msm.hip) launches for n points below saturation: (n + 3) / 4 rounded up to whole blocks of 64;
    thread t owns the points t, t + T, t + 2 T, ..."""
    return 64 * (((n + 3) // 4 + 63) // 64)


def infinity_patterns(n):
    """-> [(name, mask)]: mask[i] True = scalar i is non-zero (a finite point), False = zero (the point at infinity).  Whole-chain
    patterns name every index of one thread of chain_threads(n); the random densities do not depend on the launch shape."""
    idx = np.arange(n)
    T = chain_threads(n)
    out = [("all_zero", np.zeros(n, bool)), ("only_first_nonzero", idx == 0), ("only_last_nonzero", idx == n - 1),
           ("only_first_zero", idx != 0), ("only_last_zero", idx != n - 1), ("alternating", idx % 2 == 1)]
    for t0 in (0, 1, T - 1):
        if t0 < n:
            out.append(("chain_%d_zero" % t0, idx % T != t0))
            out.append(("chain_%d_only" % t0, idx % T == t0))
    for dens in (0.1, 0.5, 0.9):
        out.append(("random_%.1f" % dens, np.random.default_rng([n, int(dens * 10)]).random(n) < dens))
    return out


def saturated_patterns():
    n = SATURATED_SIZE
    return [("random_0.5", np.random.default_rng([n, 5]).random(n) < 0.5), ("last_40000_zero", np.arange(n) < n - 40000)]


def pattern_values(mask, seed):
    """small scalars under a mask: 0 where it is False, 1..7 elsewhere -> int64 array (the expected point is entry v of eight)"""
    v = np.random.default_rng(seed).integers(1, 8, size=mask.shape[0])
    return np.where(mask, v, 0)


def small_scalars(values):
    """values < 2^63 as canonical 4-limb scalars"""
    sc = np.zeros((len(values), 4), dtype=np.uint64)
    sc[:, 0] = np.asarray(values, dtype=np.uint64)
    return sc


def small_multiples(oracle, group, base):
    """[v] base for v = 0..7 -> (points [8, w], inf [8]); entry 0 is the point at infinity"""
    return oracle.fixed_base(group, base, small_scalars(np.arange(8)))


# ---------------------------------------------------------------------------------------------- systems
def _system(name, nc, ni, nv, seed, used=None, empty=""):
    """A satisfied random system: row i is (A z)(B z) = (C z) with 1-3 terms in A and B over the columns below `used` and C made to
    fit.  empty = "b": B has no entry (so C z = 0 in every row); "c": C has no entry (so B z = 0 in every row)."""
    rng = random.Random(seed)
    used = nv if used is None else used
    z = [1] + [P.rand_fr(rng) for _ in range(nv - 1)]
    A, B, C = [], [], []

    def row():
        return [(P.rand_fr(rng) if rng.random() < .5 else rng.randrange(1, 4), rng.randrange(used)) for _ in range(rng.randrange(1, 4))]

    def zero_row():          # evaluates to 0 on z: c z_j - (c z_j) z_0
        j, c = rng.randrange(used), P.rand_fr(rng)
        return [(c, j), ((-c * z[j]) % R, 0)] if j else []

    for _ in range(nc):
        ra = row()
        rb = [] if empty == "b" else zero_row() if empty == "c" else row()
        target = sum(c * z[j] for c, j in ra) * sum(c * z[j] for c, j in rb) % R
        if empty == "c":
            rc = []
        elif empty == "b":
            rc = zero_row()
        else:
            j, c1 = rng.randrange(used), P.rand_fr(rng)
            rc = [(c1, j), ((target - c1 * z[j]) % R, 0)] if j else [(target, 0)]
        A.append(ra)
        B.append(rb)
        C.append(rc)
    return dict(name=name, A=A, B=B, C=C, ni=ni, nv=nv, nc=nc, z=z, used=used, empty=empty)


_SYSTEMS = None


def systems():
    """-> the systems by name, built once; each with its rows, dimensions and a satisfying assignment z"""
    global _SYSTEMS
    if _SYSTEMS is None:
        s = [
            # one constraint, one instance variable, one witness — by hand: 3 z1 * 1 = 3 z1
            dict(name="1-1-2", A=[[(3, 1)]], B=[[(1, 0)]], C=[[(3, 1)]], ni=1, nv=2, nc=1, z=[1, 5], used=2, empty=""),
            _system("14-2-20", 14, 2, 20, 11),                  # nc + ni = 16 exactly: N = 16
            _system("15-2-20", 15, 2, 20, 12),                  # one past: N = 32
            _system("300-257-300", 300, 257, 300, 13),          # more instance variables than a block of 256; 43 witness columns
            _system("40-3-50-b-empty", 40, 3, 50, 14, empty="b"),
            _system("40-3-50-c-empty", 40, 3, 50, 15, empty="c"),
            _system("40-3-90-unused", 40, 3, 90, 16, used=50),   # columns 50..89 in no matrix
            _system("5-4-4-no-witness", 5, 4, 4, 17),           # nv == ni: l_query is empty
            # no constraint at all, by hand: N = 1, h_query and l_query are empty
            dict(name="0-1-1", A=[], B=[], C=[], ni=1, nv=1, nc=0, z=[1], used=1, empty=""),
        ]
        _SYSTEMS = {x["name"]: x for x in s}
    return _SYSTEMS


SYSTEM_NAMES = ["1-1-2", "14-2-20", "15-2-20", "300-257-300", "40-3-50-b-empty", "40-3-50-c-empty", "40-3-90-unused", "5-4-4-no-witness",
                "0-1-1"]


def domain(s):
    return P.next_pow2(s["nc"] + s["ni"])


def satisfied(s):
    a, b, c = (P.r1cs_eval(s[m], s["z"]) for m in "ABC")
    return s["z"][0] == 1 and all(x * y % R == w for x, y, w in zip(a, b, c))


def r1cs_arrays(s):
    """the dict Device.r1cs_load and the oracle take"""
    return dict(a=csr_from_rows(s["A"]), b=csr_from_rows(s["B"]), c=csr_from_rows(s["C"]), num_inputs=s["ni"], num_constraints=s["nc"])


# ---------------------------------------------------------------------------------------------- trapdoors and keys
TRAP_ORDER = ("tau", "alpha", "beta", "gamma", "delta")
TRAP_NAMES = ["random", "bounds"]


def trapdoor(name):
    """-> dict of ints.  "bounds": every entry at an end of its range; tau = 2 lies in no radix-2 domain (its order is not a power of two)"""
    if name == "bounds":
        return dict(tau=2, alpha=1, beta=R - 1, gamma=R - 1, delta=1)
    rng = random.Random(4242)
    return {k: P.rand_fr(rng) for k in TRAP_ORDER}


def trap_mont(trap):
    return fr_mont_vec([trap[k] for k in TRAP_ORDER])


def generators(oracle):
    """(g1, g2): random multiples of the standard generators, as synth.make_pk's"""
    return random_base(oracle, "g1", 601), random_base(oracle, "g2", 602)


def setup_logs(s, trap):
    """pyref's big-integer logs of the key under the names synth.expected_proof_logs takes (a, b, l, h, gabc) + N"""
    L = P.groth16_setup_logs(s["A"], s["B"], s["C"], s["ni"], s["nv"], trap)
    return dict(a=L["a_query"], b=L["b_query"], l=L["l_query"], h=L["h_query"], gabc=L["gamma_abc"], N=L["N"])


def _points(oracle, group, base, ints):
    """[k] base for the ints -> (points, inf); the limbs of a point at infinity are zero, as the device writes them"""
    w = 12 if group == "g1" else 24
    if not len(ints):
        return np.zeros((0, w), np.uint64), np.zeros(0, np.uint8)
    pts, inf = oracle.fixed_base(group, base, fr_canon_vec(ints))
    pts[inf != 0] = 0
    return pts, inf


def expected_key(oracle, s, trap, g1, g2):
    """The key zkg16_setup has to return for system s: logs from pyref (no C in them), points from the oracle's fixed-base
    -> (pk dict as Device.setup's, flags of every query included, vk dict as Device.setup_resident's, logs)."""
    logs = setup_logs(s, trap)
    pk = {}
    pk["a_query"], pk["a_inf"] = _points(oracle, "g1", g1, logs["a"])
    pk["b_g1_query"], pk["b_g1_inf"] = _points(oracle, "g1", g1, logs["b"])
    pk["b_g2_query"], pk["b_g2_inf"] = _points(oracle, "g2", g2, logs["b"])
    pk["h_query"], pk["h_inf"] = _points(oracle, "g1", g1, logs["h"])
    pk["l_query"], pk["l_inf"] = _points(oracle, "g1", g1, logs["l"])
    single = [trap["alpha"], trap["beta"], trap["delta"], trap["gamma"]]
    p1, _ = _points(oracle, "g1", g1, single)
    p2, _ = _points(oracle, "g2", g2, single)
    pk["alpha_g1"], pk["beta_g1"], pk["delta_g1"] = p1[0], p1[1], p1[2]
    pk["beta_g2"], pk["delta_g2"] = p2[1], p2[2]
    gabc, ginf = _points(oracle, "g1", g1, logs["gabc"])
    vk = dict(alpha_g1=pk["alpha_g1"], beta_g2=pk["beta_g2"], gamma_g2=p2[3], delta_g2=pk["delta_g2"], gamma_abc_g1=gabc, gamma_abc_inf=ginf)
    return pk, vk, logs
