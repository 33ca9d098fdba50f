"""The streamed proof's rounds on the device, against tests/stream_cases.py.

a. The part map: zkg16_diag_matrix_stream runs the production's own start / attach / produce(k) calls on a buffer filled with 0xFF
   bytes and reports after which part every entry had been written; that, wit_part_of_kernel's array and the model's must be one array,
   entry for entry — a variable labelled a part too early would have its scalar read before wit_sponge_kernel wrote it.  Sizes at
   which every slice is a single permutation, slices are uneven, the slice count is lowered, and a slice edge sits at permutation 1
   (the first permutation is five values short).
b. The merge: a plain-key MSM fed in rounds as prove_device feeds a z-side query (zkg16_diag_msm_rounds) on buckets whose rounds
   meet as equal points in two XYZZ forms, opposite points, infinity on either side, empty rounds, and buckets that exist only after
   the fix-up kernels.  The point must be [sum s_i k_i]G from the CPU oracle's scalar multiplication, every round's term list as long
   as the model's, and one round over the same scalars must give the same bytes.
c. Whole proofs at sizes where zkg16_prove_matrix really runs 2 to 8 slices: the bytes of zkg16_witness_matrix + zkg16_prove_resident.

Every comparison is exact."""
import random

import numpy as np
import pytest

import msm_limit_cases as M
import pyref as P
import stream_cases as S
from helpers import fr_mont

pytestmark = pytest.mark.gpu

DEFAULTS = {"min_seg": 0, "fixup_aux": 0, "matrix_parts": 0, "matrix_slice_min": 0}
ONES = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def _inputs(n, kind):
    """a, b: every entry 2^64 - 1 (c's entries need the third limb), all zero, or random over the full 64 bits"""
    if kind == "ones":
        return np.full((n, n), ONES, dtype=np.uint64), np.full((n, n), ONES, dtype=np.uint64)
    if kind == "zero":
        return np.zeros((n, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)
    rng = np.random.default_rng(7000 + n)
    draw = lambda: rng.integers(0, 1 << 63, size=(n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, n), dtype=np.uint64)
    return draw(), draw()


_witness_cache = {}


def _witness(n, kind):
    """the host builder's assignment (zkg16_circuit_matrix_witness): computed once per input, shared, never written to"""
    if (n, kind) not in _witness_cache:
        from zksnark_finalproject_amd.circuits import matrix_witness
        a, b = _inputs(n, kind)
        z = matrix_witness(a, b, S.Layout(n).total)
        z.setflags(write=False)
        _witness_cache[(n, kind)] = z
    return _witness_cache[(n, kind)]


# ------------------------------------------------------------------------------------------------ a. the part map
_MAPS = [(n, parts, 1) for n in (2, 3, 4, 5, 8) for parts in range(2, 9)] + [(33, 0, 0)]


@pytest.mark.parametrize("n,parts,slice_min", _MAPS, ids=["n%d-parts%d-min%d" % x for x in _MAPS])
def test_part_map_is_what_production_writes(dev, n, parts, slice_min):
    L = S.Layout(n)
    bounds = S.slice_bounds(L.perms, parts, slice_min or S.SLICE_MIN_DEFAULT)
    want = S.part_map(n, bounds)
    if slice_min:
        assert len(bounds) - 1 == min(parts, L.perms)
    try:
        dev.set_option("matrix_parts", parts)
        dev.set_option("matrix_slice_min", slice_min)
        for kind in (("ones", "zero", "random") if n <= 8 else ("random",)):
            a, b = _inputs(n, kind)
            part_of, first, z, nparts = dev.diag_matrix_stream(a, b)
            assert nparts == len(bounds)
            assert part_of.shape == want.shape and first.shape == (L.total,)
            bad = np.flatnonzero(part_of != want)
            assert bad.size == 0, (kind, bad[:8], part_of[bad[:8]], want[bad[:8]])
            bad = np.flatnonzero(first != want[:L.total])
            assert bad.size == 0, (kind, bad[:8], first[bad[:8]], want[bad[:8]])
            assert z.tobytes() == _witness(n, kind).tobytes(), kind
    finally:
        dev.set_option("matrix_parts", 0)
        dev.set_option("matrix_slice_min", 0)


def test_matrix_stream_edges(dev):
    """matrix_parts = 1 builds no map (255 throughout) and still produces the assignment in two parts; a wrong length or a null pointer
    is refused with nothing written"""
    n = 3
    L = S.Layout(n)
    a, b = _inputs(n, "random")
    try:
        dev.set_option("matrix_parts", 1)
        part_of, first, z, nparts = dev.diag_matrix_stream(a, b)
    finally:
        dev.set_option("matrix_parts", 0)
    assert nparts == 2 and (part_of == 255).all() and z.tobytes() == _witness(n, "random").tobytes()
    assert np.array_equal(first, S.part_map(n, [0, L.perms])[:L.total])
    import ctypes as C
    po, fv, zz = np.full(L.total + 3, 7, np.uint8), np.full(L.total, 7, np.uint8), np.full((L.total, 4), 7, np.uint64)
    k = C.c_int(-1)
    p = lambda x: x.ctypes.data
    good = [dev.ctx, n, p(a), p(b), p(po), p(fv), p(zz), L.total, C.byref(k)]
    for i, v in ((0, None), (1, 1), (1, 1025), (2, None), (3, None), (4, None), (5, None), (6, None), (7, L.total - 1), (7, L.total + 3), (8, None)):
        args = list(good)
        args[i] = v
        assert dev.lib.zkg16_diag_matrix_stream(*args) == 1, i
    assert (po == 7).all() and (fv == 7).all() and (zz == 7).all() and k.value == -1


# ------------------------------------------------------------------------------------------------ b. the merge
_ROUNDS = S.round_cases("g1") + S.round_cases("g2")


@pytest.mark.parametrize("case", _ROUNDS, ids=[c.name for c in _ROUNDS])
def test_rounds_merge_to_the_expected_point(dev, oracle, case):
    bases, sc = case.arrays(oracle)
    exp, einf = case.expected(oracle)
    want_entries = case.round_entries()
    try:
        for k, v in case.options.items():
            dev.set_option(k, v)
        got, ginf, entries = dev.diag_msm_rounds(case.group, bases, sc, case.part, case.parts, case.c)
        state = dev.last_msm_state()
        # the same scalars in one round, on the same path (round 0 alone: nothing is merged) ...
        one, oinf, one_entries = dev.diag_msm_rounds(case.group, bases, sc, np.zeros(len(case.scalars), np.uint8), 1, case.c)
    finally:
        for k in case.options:
            dev.set_option(k, DEFAULTS[k])
    # ... and as the ordinary MSM entry runs them (no rounds at all)
    try:
        dev.set_option("window_bits", case.c)
        plain, pinf = dev.msm(case.group, bases, sc)
    finally:
        dev.set_option("window_bits", 0)
    assert entries.tolist() == want_entries, (case, entries.tolist(), want_entries)
    assert one_entries.tolist() == [sum(want_entries)]
    assert ginf == einf and (einf or np.array_equal(got, exp)), case
    assert oinf == ginf and one.tobytes() == got.tobytes(), case
    assert int(pinf) == ginf and plain.tobytes() == got.tobytes(), case
    assert state[:3] == (case.c, M.nwin_of(case.c), want_entries[-1])
    if case.spill:
        # the last round really was the spilled bucket: one term per lane, and the fix-up queue the model counts
        counts = case.round_counts(case.spill["round"])
        assert case.spill["round"] == case.parts - 1 and state[3] == 1 and state[4:6] == M.fixup_queue(counts, 1), (case, state)


def test_msm_rounds_argument_edges(dev, oracle):
    case = S.round_cases("g1")[0]
    bases, sc = case.arrays(oracle)
    n = len(case.scalars)
    out, oinf, ent = np.full(12, 0x5a5a, np.uint64), np.full(1, 7, np.uint8), np.full(4, 7, np.uint32)
    p = lambda x: x.ctypes.data
    part = np.ascontiguousarray(case.part)
    good = dict(ctx=dev.ctx, group=1, bases=p(bases), inf=None, sc=p(sc), n=n, part=p(part), parts=2, c=8, out=p(out), oinf=p(oinf), ent=p(ent))
    call = lambda **kw: dev.lib.zkg16_diag_msm_rounds(*[dict(good, **kw)[k] for k in good])
    for kw in (dict(ctx=None), dict(bases=None), dict(sc=None), dict(part=None), dict(out=None), dict(oinf=None), dict(ent=None), dict(group=0),
               dict(group=3), dict(parts=0), dict(parts=256), dict(c=1), dict(c=21)):
        assert call(**kw) == 1, kw
    assert call(c=2, n=1 << 24) == 3 and b"2^31" in dev.lib.zkg16_last_error(dev.ctx)        # refused before anything is read
    assert (out == 0x5a5a).all() and (oinf == 7).all() and (ent == 7).all()
    assert call() == 0
    exp, einf = case.expected(oracle)
    assert int(oinf[0]) == einf == 0 and np.array_equal(out, exp) and ent[:2].tolist() == case.round_entries() and ent[2:].tolist() == [7, 7]
    # n == 0: infinity, no terms; a label of `parts` or more takes part in no round
    got, ginf, entries = dev.diag_msm_rounds("g2", np.zeros((0, 24), np.uint64), np.zeros((0, 4), np.uint64), np.zeros(0, np.uint8), 3, 8)
    assert ginf == 1 and not got.any() and entries.tolist() == [0, 0, 0]
    got, ginf, entries = dev.diag_msm_rounds("g1", bases, sc, np.full(n, 2, np.uint8), 2, 8)
    assert ginf == 1 and not got.any() and entries.tolist() == [0, 0]
    with pytest.raises(ValueError):
        dev.diag_msm_rounds("g1", bases[:5], sc, part, 2, 8)


# ------------------------------------------------------------------------------------------------ c. whole proofs at small sizes
@pytest.fixture(scope="module")
def keys(dev):
    """(n, tables) -> (r1cs handle, key handle): one resident key per size, a second one carrying window tables"""
    import bench
    cache = {}

    def get(n, tables):
        if (n, tables) not in cache:
            rh = dev.r1cs_matrix(n)
            trap, g1, g2 = bench.draw_key_inputs(31 + n)
            ph, _ = dev.setup_resident(rh, 4, trap, g1, g2)
            if tables:
                dev.pk_precompute(ph, 8, 8)
            cache[(n, tables)] = (rh, ph)
        return cache[(n, tables)]
    yield get
    for rh, ph in cache.values():
        dev.pk_free(ph)
        dev.r1cs_free(rh)


_PROOFS = [(n, parts, tables) for n in (4, 5, 8) for parts in (2, 3, 8) for tables in (False, True)]


@pytest.mark.parametrize("n,parts,tables", _PROOFS, ids=["n%d-parts%d-%s" % (n, p, "tables" if t else "plain") for n, p, t in _PROOFS])
def test_streamed_proofs_at_small_sizes(dev, keys, n, parts, tables):
    rh, ph = keys(n, tables)
    bounds = S.slice_bounds(S.Layout(n).perms, parts, 1)
    assert len(bounds) - 1 == min(parts, S.Layout(n).perms) >= 2
    rng = random.Random(100 * n + parts)
    for kind in ("ones", "random"):
        a, b = _inputs(n, kind)
        r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
        wh, pub, _ = dev.witness_matrix(a, b)
        try:
            want = dev.prove_resident(ph, rh, wh, r, s)
            try:
                dev.set_option("matrix_parts", parts)
                dev.set_option("matrix_slice_min", 1)
                for _ in range(2):                       # twice: the second call reuses every workspace of the first
                    proof, inf, pub2, ms = dev.prove_matrix(ph, rh, a, b, r, s)
                    assert ms["parts"] == len(bounds)
                    assert np.array_equal(pub2, pub) and np.array_equal(pub2, _witness(n, kind)[1:4])
                    assert proof.tobytes() == want[0].tobytes() and inf.tobytes() == want[1].tobytes(), (kind, ms["parts"])
            finally:
                dev.set_option("matrix_parts", 0)
                dev.set_option("matrix_slice_min", 0)
            # with the floor back at its default the same request runs one slice, and gives the same bytes
            proof, inf, _, ms = dev.prove_matrix(ph, rh, a, b, r, s)
            assert ms["parts"] == 2 and proof.tobytes() == want[0].tobytes() and inf.tobytes() == want[1].tobytes()
        finally:
            dev.witness_free(wh)
