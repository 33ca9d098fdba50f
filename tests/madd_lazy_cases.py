"""Cases and exact checkers for tests/csrc/madd_lazy_shim.hip: the bucket accumulations' mixed additions without their spare carry
passes (csrc/ec.cuh: xyzz_madd_inline_lc for G1, xyzz_madd_lazy_lc for G2) on RAW limbs.  Shared by tests/test_madd_lazy_host.py
(CPU build, every operand assertion of csrc/ffu.cuh live) and tests/test_madd_lazy_gpu.py (gfx950 build).

Every expected value is exact: the group element from tests/golden/pyref.py's ec_add for inputs that are curve points, and the
madd-2008-s formulas evaluated in pyref's field classes for the worst-limb inputs (which are not points: all four coordinates
of an accumulator cannot have all-ones limbs and satisfy the curve equation too, but the formulas are polynomial identities and the
kernels' arithmetic does not know the difference).  Comparisons are canonical (mod q); every output limb must be normalised and
every output coordinate inside the stored bounds of DESIGN.md 2.1.  The limb packing, the group model and the point cases are
tests/prim_cases.py's."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np

import prim_cases as PC
import pyref as P

SRC = os.path.join(PC.ROOT, "tests", "csrc", "madd_lazy_shim.hip")
LIBS = {"host": os.path.join(PC.OUT_DIR, "libmadd_lazy_shim_host.so"), "device": os.path.join(PC.OUT_DIR, "libmadd_lazy_shim_dev.so")}
HEADERS = ["ff.cuh", "ffu.cuh", "ec.cuh"]
OP = {"g1_madd": 0, "g2_madd": 1, "g1_chain": 2, "g2_chain": 3, "bad_two_lazy": 4, "bad_column": 5}
CHAIN_STEPS = 32
Q = PC.Q


def build_shim(kind):
    """Compiles one build of the shim when it is stale (mtime rule of the other shims); returns the library's path."""
    out = LIBS[kind]
    deps = [SRC] + [os.path.join(PC.INC, h) for h in HEADERS] + ([PC.BUILD_PY] if kind == "device" else [])
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(PC.OUT_DIR, exist_ok=True)
        if kind == "host":
            cmd = ["hipcc", "--offload-host-only", "-O2", "-shared", "-fPIC", "-fvisibility=hidden", "-DMADD_HOST_BUILD", "-DZK_FQU_CHECK"]
        else:
            cmd = ["hipcc"] + PC.product_flags() + ["-shared"]
        subprocess.check_call(cmd + ["-I", PC.INC, "-o", out, SRC])
    return out


def load_shim(kind):
    lib = C.CDLL(build_shim(kind))
    lib.madd_lazy_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.madd_lazy_run.restype = C.c_int
    lib.madd_lazy_words.argtypes = [C.c_int, C.c_int]
    assert lib.madd_lazy_is_device_build() == (1 if kind == "device" else 0)
    return lib


def run(lib, op, inp):
    """inp: (n, in_words) uint32 -> (n, out_words) uint32"""
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    assert inp.ndim == 2 and inp.shape[1] == lib.madd_lazy_words(op, 0), (op, inp.shape, lib.madd_lazy_words(op, 0))
    out = np.zeros((inp.shape[0], lib.madd_lazy_words(op, 1)), dtype=np.uint32)
    rc = lib.madd_lazy_run(op, inp.shape[0], inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, "madd_lazy_run(op %d) returned %d" % (op, rc)
    return out


# ---------------------------------------------------------------------------------------------- single additions on curve points
def point_cases(gname):
    """tests/prim_cases.py's 640 mixed-addition records: random accumulators and bases, both signs, P + P, P - P, either or both
    operands at infinity, with every combination of accumulator coordinates at 42q / 42q / 2q (G2: 10q) or reduced and bases at 2q
    or reduced; lane 0 has everything at the top."""
    return PC.curve_inputs(gname, "madd")


def check_points(gname, inp, expected, out):
    g = PC.group(gname)
    for i, vals in enumerate(PC.u_unpack(out)):
        try:
            got, _ = g.decode(vals)
            e = expected[i]
            assert (got is None and e is None) or (got is not None and e is not None and got[0] == e[0] and got[1] == e[1]), "wrong point"
        except AssertionError as err:
            raise AssertionError("%s madd lane %d: %s" % (gname, i, err))


# ---------------------------------------------------------------------------------------------- worst limbs: the formulas themselves
def top_below(k):
    """largest top limb t with all_ones(t) < k q"""
    t = (k * Q) >> 377
    while PC.all_ones(t) >= k * Q:
        t -= 1
    return t


@functools.lru_cache(maxsize=None)
def worst_limb_cases(gname):
    """Accumulators whose coordinates have limbs 0..12 all at 2^29 - 1, under a top limb that keeps the value below q ("reduced") or
    puts it at the top of the stored bound (X, Y < 42q; ZZ, ZZZ < 2q in G1, < 10q in G2), in every subset of the four coordinates
    (the others random at the same bounds), against bases at 2q - 1, all-ones below 2q, or random, both signs.
    Returns (records, list of (coords as ints, neg))."""
    g = PC.group(gname)
    nc = g.nc
    rng = random.Random(611 if gname == "g1" else 661)
    hi = [42, 42, g.zz_hi, g.zz_hi]
    rows, meta = [], []
    for subset in range(1, 16):
        for reduced in (False, True):
            for base_kind in range(3):
                for neg in (False, True):
                    coords = []
                    for c in range(4):
                        k = 1 if reduced else hi[c]
                        for _ in range(nc):
                            coords.append(PC.all_ones(top_below(k)) if subset >> c & 1 else rng.randrange((k - 1) * Q + 1, k * Q))
                    for _ in range(2 * nc):
                        coords.append([2 * Q - 1, PC.all_ones(top_below(2)), rng.randrange(1, 2 * Q)][base_kind])
                    rows.append(coords + [0] * (2 * nc))
                    meta.append((coords, neg))
    inp = np.zeros((len(rows), 8 * 14 * nc + 1), np.uint32)
    inp[:, :-1] = PC.u_pack(rows)
    inp[:, -1] = [1 if neg else 0 for _, neg in meta]
    return inp, meta


def madd_formula(g, coords, neg):
    """madd-2008-s on field elements: (X1, Y1, ZZ1, ZZZ1) + (x2, +-y2) -> (X3, Y3, ZZ3, ZZZ3)"""
    nc = g.nc
    X1, Y1, ZZ1, ZZZ1, x2, y2 = (g.felem(coords[i * nc:(i + 1) * nc]) for i in range(6))
    if neg:
        y2 = -y2
    Pp = x2 * ZZ1 - X1
    R = y2 * ZZZ1 - Y1
    assert not Pp.is_zero()
    PP = Pp * Pp
    PPP = Pp * PP
    Qv = X1 * PP
    X3 = R * R - PPP - Qv - Qv
    return X3, R * (Qv - X3) - Y1 * PPP, ZZ1 * PP, ZZZ1 * PPP


def check_worst(gname, meta, out):
    g = PC.group(gname)
    nc = g.nc
    for i, vals in enumerate(PC.u_unpack(out)):      # u_unpack asserts normalised limbs
        coords, neg = meta[i]
        want = madd_formula(g, coords, neg)
        for c in range(4):
            got = vals[c * nc:(c + 1) * nc]
            assert max(got) < (42 if c < 2 else g.zz_hi) * Q, "%s worst-limb case %d coordinate %d at %.2f q" % (gname, i, c, max(got) / Q)
            assert g.felem(got) == want[c], "%s worst-limb case %d: coordinate %d wrong" % (gname, i, c)


# ---------------------------------------------------------------------------------------------- chains
def chain_choices(seed):
    """the lane's sequence of (base, negate), as chain_op of madd_lazy_shim.hip draws it"""
    s, out = seed, []
    for _ in range(CHAIN_STEPS):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        c = s >> 29
        out.append((0 if c < 5 else 1, c in (3, 4, 7)))
    return out


CHAIN_LANES = 70


@functools.lru_cache(maxsize=None)
def chain_cases(gname):
    """32 dependent additions per lane from an accumulator at the top of the stored bounds (every other lane: reduced) and two
    bases at 2q (reduced); a fifth of the lanes start AT the first base and a fifth at its negative, so that chains run through the
    doubling, the cancellation and a restart from infinity with either sign."""
    g = PC.group(gname)
    rng = random.Random(701 if gname == "g1" else 751)
    W = 14 * g.nc
    inp = np.zeros((CHAIN_LANES, 8 * W + 1), np.uint32)
    expected = []
    for i in range(CHAIN_LANES):
        a, b1, b2 = rng.sample(range(1, 13), 3)
        A, B1, B2 = g.mult[a], g.mult[b1], g.mult[b2]
        if i % 5 == 0:
            A = B1
        elif i % 5 == 1:
            A = P.ec_neg(B1)
        top = i % 2 == 0
        acc = g.xyzz(A, rng, [42, 42, g.zz_hi, g.zz_hi] if top else [1, 1, 1, 1])
        bases = g.affine(B1, [2, 2] if top else [1, 1])[:2 * g.nc] + g.affine(B2, [2, 2] if top else [1, 1])[:2 * g.nc]
        seed = rng.randrange(1 << 32)
        inp[i, :8 * W] = PC.u_pack([acc + bases])[0]
        inp[i, 8 * W] = seed
        pts, cur = [], A
        for which, neg in chain_choices(seed):
            b = (B1, B2)[which]
            cur = P.ec_add(cur, P.ec_neg(b) if neg else b)
            pts.append(cur)
        expected.append(pts)
    return inp, expected


def check_chain(gname, inp, expected, out):
    g = PC.group(gname)
    seen = {"inf": 0, "steps": 0}
    for i, vals in enumerate(PC.u_unpack(out)):
        for s in range(CHAIN_STEPS):
            try:
                got, _ = g.decode(vals[s * 4 * g.nc:(s + 1) * 4 * g.nc])
                e = expected[i][s]
                assert (got is None and e is None) or (got is not None and e is not None and got[0] == e[0] and got[1] == e[1]), "wrong point"
            except AssertionError as err:
                raise AssertionError("%s chain lane %d step %d: %s" % (gname, i, s, err))
            seen["inf"] += got is None
            seen["steps"] += 1
    assert seen["inf"] > 0, "no chain met the cancellation"
    return seen
