"""The bucket MSM on the device at the limits tests/msm_limit_cases.py builds: fix-up routing on either side of FIXUP_SHORT and
FIXUP_ITEM, the head / tail bookkeeping of every accumulation variant, the signed-digit recoding across window widths, and the bucket
reductions at their smallest bucket counts, fed equal, opposite and twice-represented points.

Every result is compared byte for byte (affine limbs and the infinity flag) with [sum s_i k_i]G from the CPU oracle's scalar
multiplication, and zkg16_last_msm_state must report the path the model expects: window bits and count, the length of the term
list, seg_len, the fix-up work items and chains queued, and the reduction form where its rule is a simple one.  The lane counts
behind seg_len come from the device's own CU count."""
import numpy as np
import pytest

import msm_limit_cases as M

pytestmark = pytest.mark.gpu

# the value that restores each option's default
DEFAULTS = {"window_bits": 0, "min_seg": 0, "reduce_mode": 0, "reduce_chunk": 0, "acc_lazy": 1, "g1_inline": 1, "acc_pipeline": 0,
            "g2_lazy": 1, "fixup_aux": 0}


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cus(dev):
    """compute units of device 0, asked of the HIP runtime the library is linked to: the copy of libamdhip64 this process has mapped
    since the library was loaded, whatever its version suffix.  (torch brings a HIP runtime of its own, and the second runtime
    to start in a process finds no device, so torch cannot be asked next to the library.)  The attribute's number is the one of
    hip_runtime_api.h; should it ever move, the answer is checked against the CU counts the kernel driver lists for its GPUs."""
    import ctypes as C
    import glob
    import re
    with open("/proc/self/maps") as f:
        libs = sorted(set(re.findall(r"(/\S*libamdhip64\.so[.\d]*)", f.read())))
    assert len(libs) == 1, libs
    n = C.c_int(0)
    assert C.CDLL(libs[0]).hipDeviceGetAttribute(C.byref(n), 63, 0) == 0          # hipDeviceAttributeMultiprocessorCount
    assert 8 <= n.value <= 1024, n.value
    listed = set()
    for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            with open(path) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            if int(props.get("simd_count", 0)) and int(props.get("simd_per_cu", 0)):
                listed.add(int(props["simd_count"]) // int(props["simd_per_cu"]))
        except (OSError, ValueError):
            pass
    assert not listed or n.value in listed, (n.value, listed)
    return n.value


def run(dev, oracle, cus, case, extra=None, mode=None, chunk=0):
    """one MSM under the case's options: value == expected point, state == model"""
    opts = dict(case.options)
    opts.update(extra or {})
    bases, sc = case.arrays(oracle)
    exp, einf = case.expected(oracle)
    try:
        for k, v in opts.items():
            dev.set_option(k, v)
        got, ginf = dev.msm(case.group, bases, sc)
        state = dev.last_msm_state()
    finally:
        for k in opts:
            dev.set_option(k, DEFAULTS[k])
    want = case.state(cus, mode, chunk)
    assert ginf == einf and (einf or np.array_equal(got, exp)), (case, extra)
    assert M.state_matches(state, want), (case, extra, state, want)
    return state


def _ids(cases):
    return [c.name for c in cases]


_FIX1, _FIX2 = M.fixup_cases("g1"), M.fixup_cases("g2")


@pytest.mark.parametrize("case", _FIX1, ids=_ids(_FIX1))
def test_fixup_routing_g1(dev, oracle, cus, case):
    st = run(dev, oracle, cus, case)
    assert st[4:6] == (case.claims["items"], case.claims["nchains"])           # the state assertion is live: both counters are pinned


@pytest.mark.parametrize("case", _FIX2, ids=_ids(_FIX2))
def test_fixup_routing_g2(dev, oracle, cus, case):
    st = run(dev, oracle, cus, case)
    assert st[4:6] == (case.claims["items"], case.claims["nchains"])


_SEG = M.segment_cases("g1") + M.segment_cases("g2")


@pytest.mark.parametrize("case", _SEG, ids=_ids(_SEG))
def test_segment_edges_per_accumulation_variant(dev, oracle, cus, case):
    """the same 61-entry list through every accumulation loop (default, acc_lazy 0, g1_inline 2, acc_pipeline 1 / 2 / 3, g2_lazy 2,
    fixup_aux 1): each gives the expected point's bytes, hence the default's"""
    run(dev, oracle, cus, case)


_DIG = M.digit_cases("g1") + M.digit_cases("g2")


@pytest.mark.parametrize("case", _DIG, ids=_ids(_DIG))
def test_digit_recoding_across_widths(dev, oracle, cus, case):
    run(dev, oracle, cus, case)
    if case.c < 4:          # fewer than 8 buckets per window: the bit-sliced form must step aside even when it is asked for
        assert M.reduce_state(case.c, 5, 0)[0] == 0
        for chunk in (0, 2):
            assert run(dev, oracle, cus, case, {"reduce_mode": 5, "reduce_chunk": chunk}, 5, chunk)[6] == 0


_RED = [("g1", c, p) for c in M.REDUCE_WIDTHS for p in M.REDUCE_PATTERNS] + [("g2", c, p) for c, p in M.REDUCE_G2]


@pytest.mark.parametrize("group,c,pattern", _RED, ids=["%s-c%d-%s" % x for x in _RED])
def test_reduction_forms_at_small_bucket_counts(dev, oracle, cus, group, c, pattern):
    """reduce_mode 1 (two-level), 4 (classic), 5 (bit-sliced), 0 (default) x reduce_chunk 0 .. 64 on buckets that hold equal points,
    opposite points, and one point in two XYZZ forms; the form that ran is asserted for the forced modes"""
    shared = None if pattern == "last-chunk" else M.reduce_case(group, c, pattern)
    forced = 0
    for mode in M.REDUCE_MODES:
        for chunk in M.REDUCE_CHUNKS:
            case = shared or M.reduce_case(group, c, pattern, chunk)
            st = run(dev, oracle, cus, case, {"reduce_mode": mode, "reduce_chunk": chunk}, mode, chunk)
            want = M.reduce_state(c, mode, chunk)
            forced += want[0] is not None and want[1] is not None and st[6:] == want
    assert forced >= 12 + 5          # modes 1 and 4 at every chunk size, mode 5 at every forced one


def test_state_accessor_edges(dev, oracle):
    """a null output is refused; a ctx that has run no MSM reports zeros; an empty MSM reports its plan and no list; a proof on the
    ctx takes over the workspace the words live in, and the state reads zeros again rather than a mix of the two"""
    import random
    import pyref as P
    import synth
    from helpers import fr_mont, fr_mont_vec
    assert dev.lib.zkg16_last_msm_state(dev.ctx, None) == 1
    from zksnark_finalproject_amd import Device
    d = Device(0)
    try:
        assert d.last_msm_state() == (0,) * 8
        d.set_option("window_bits", 8)
        got, ginf = d.msm("g1", np.zeros((0, 12), np.uint64), np.zeros((0, 4), np.uint64))
        assert ginf == 1 and d.last_msm_state() == (8, 32, 0, 0, 0, 0, 0, 0)
        d.msm("g1", M.table(oracle, "g1")[:8], M.canon_vec(range(1, 9)))
        assert d.last_msm_state()[:6] == (8, 32, 8, 4, 0, 0)
        d.set_option("window_bits", 0)
        rng = random.Random(5)
        nc, ni, nv = 27, 3, 14
        A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
        r1cs = synth.r1cs_arrays(A, B, C, ni)
        pk, _ = synth.make_pk(oracle, r1cs, nv, rng, point_gen=d.fixed_base)
        r, s = fr_mont(P.rand_fr(rng)), fr_mont(P.rand_fr(rng))
        proof, inf = d.prove(d.pk_load(pk, ni), r, s, r1cs, fr_mont_vec(z))
        eproof, einf = oracle.prove(pk, r, s, r1cs, fr_mont_vec(z))
        assert np.array_equal(proof, eproof) and np.array_equal(inf, einf)
        assert d.last_msm_state() == (0,) * 8
    finally:
        d.close()
