"""The bucket MSM on window tables, one MSM at a time (zkg16_diag_msm_tabled), at the limits tests/msm_tabled_cases.py builds: the
table entries themselves at both strides, the recoding on one bucket set up to 24-bit windows, every accumulation loop on packed and
on padded entries with buckets that mix levels, fix-up routing on buckets that are deep by construction, the one-set branch of the
reduction on both sides of its thresholds, batches whose vectors are one window each, and the entry's argument edges.

Every result is compared byte for byte (affine limbs and the infinity flag) with [sum s_i k_i]G from the CPU oracle's scalar
multiplication, every table entry with [2^(c w) k_i]G from its fixed-base routine, and zkg16_last_msm_state must report the path the
model expects.  There is no tolerance anywhere.  The lane counts behind seg_len come from the device's own CU count."""
import numpy as np
import pytest

import msm_limit_cases as M
import msm_tabled_cases as T
from test_msm_limits_gpu import DEFAULTS, cus, dev      # noqa: F401  (the option defaults and the two module fixtures)

pytestmark = pytest.mark.gpu

BAD_ARG, ERR_HIP = 1, 3


def run(dev, oracle, cus, case, extra=None, mode=None, chunk=0, want_table=False):
    """one MSM on tables under the case's options: value == expected point per vector, state == model"""
    opts = dict(case.options)
    opts.update(extra or {})
    bases, inf, sc = case.arrays(oracle)
    exp = case.expected(oracle)
    try:
        for k, v in opts.items():
            dev.set_option(k, v)
        res = dev.diag_msm_tabled(case.group, bases, sc, case.c, case.stride, case.last, inf if inf.any() else None, want_table)
        state = dev.last_msm_state()
    finally:
        for k in opts:
            dev.set_option(k, DEFAULTS[k])
    got, ginf = res[0], res[1]
    assert got.shape[0] == case.batch == len(exp)
    for v, (e, einf) in enumerate(exp):
        assert int(ginf[v]) == einf and (einf or np.array_equal(got[v], e)), (case, extra, v)
    want = case.state(cus, mode, chunk)
    assert M.state_matches(state, want), (case, extra, state, want)
    return state, res


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ a. the tables themselves
_TAB = [(g, c, n) for g in ("g1", "g2") for c in T.TABLE_WIDTHS[g] for n in T.TABLE_NS]


@pytest.mark.parametrize("group,c,n", _TAB, ids=["%s-c%d-n%d" % x for x in _TAB])
def test_table_entries(dev, oracle, cus, group, c, n):
    """every entry of every level == [2^(c w) k]G, infinity stays infinity, level 0 is the input; both strides.  n = 1 and 3 are all
    infinity under the mask (first, middle, last), so they run without it as well"""
    for stride in (1, 2):
        for with_inf in ((True, False) if n <= 3 else (True,)):
            case = T.table_case(group, c, n, stride, with_inf)
            _, (_, _, tab, tinf) = run(dev, oracle, cus, case, want_table=True)
            etab, einf = T.expected_table(oracle, case)
            assert tab.shape == etab.shape == (M.nwin_of(c), n, 12 if group == "g1" else 24)
            assert np.array_equal(tinf, einf), (case, np.argwhere(tinf != einf)[:4])
            assert np.array_equal(tab, etab), (case, np.argwhere((tab != etab).any(axis=2))[:4])
            bases, inf, _ = case.arrays(oracle)
            assert np.array_equal(tab[0][inf == 0], bases[inf == 0]) and not tab[:, inf != 0].any()


# ------------------------------------------------------------------------------------------------ b. digit recoding on one set
_DIG = T.digit_cases("g1") + T.digit_cases("g2")


@pytest.mark.parametrize("case", _DIG, ids=_ids(_DIG))
def test_digit_recoding_on_one_set(dev, oracle, cus, case):
    run(dev, oracle, cus, case)


# ------------------------------------------------------------------------------------------------ c. accumulation loops, both entry types
_SEG = T.segment_cases("g1") + T.segment_cases("g2")


@pytest.mark.parametrize("case", _SEG, ids=_ids(_SEG))
def test_segment_edges_per_accumulation_variant_and_stride(dev, oracle, cus, case):
    """the same 64-entry list, its buckets fed from up to ten levels, through every accumulation loop on Affine and on PadAffine
    entries: each gives the expected point's bytes"""
    run(dev, oracle, cus, case)


# ------------------------------------------------------------------------------------------------ d. fix-up routing, deep buckets
_FIX1, _FIX2 = T.fixup_cases("g1"), T.fixup_cases("g2")


@pytest.mark.parametrize("case", _FIX1, ids=_ids(_FIX1))
def test_fixup_routing_deep_buckets_g1(dev, oracle, cus, case):
    st, _ = run(dev, oracle, cus, case)
    assert st[4:6] == (case.claims["items"], case.claims["nchains"])


@pytest.mark.parametrize("case", _FIX2, ids=_ids(_FIX2))
def test_fixup_routing_deep_buckets_g2(dev, oracle, cus, case):
    st, _ = run(dev, oracle, cus, case)
    assert st[4:6] == (case.claims["items"], case.claims["nchains"])


# ------------------------------------------------------------------------------------------------ e. the one-set reduction
_RED = [("g1", c, p, lvl) for c in T.REDUCE_WIDTHS for p, lvl in T.reduce_patterns(c)] + [("g2", c, p, 0) for c, p in T.REDUCE_G2]


@pytest.mark.parametrize("group,c,pattern,level", _RED, ids=["%s-c%d-%s-l%d" % x for x in _RED])
def test_one_set_reduction_at_its_thresholds(dev, oracle, cus, group, c, pattern, level):
    """last_of_proof x reduce_mode (default, 1 two-level, 4 classic, 5 bit-sliced) x reduce_chunk on one bucket set of 8 .. 2^23 buckets:
    under the default the bit-sliced form runs exactly for 256 <= nb <= 2^19, up to 2^22 for the proof's last MSM; the forced modes
    run the exact form the rule gives"""
    base = T.reduce_case(group, c, pattern, level)
    base.arrays(oracle), base.expected(oracle)
    nb = 1 << (c - 1)
    exact = 0
    for last in (False, True):
        case = base.with_(last=last)
        for mode in T.REDUCE_MODES:
            for chunk in T.REDUCE_CHUNKS:
                st, _ = run(dev, oracle, cus, case, {"reduce_mode": mode, "reduce_chunk": chunk}, mode, chunk)
                runs, bits, k = T.reduce_rule(c, 1, mode, chunk, last)
                assert (st[6] > 0) == runs, (case, last, mode, chunk, st)
                if mode == 0:
                    assert runs == (256 <= nb <= (1 << 22 if last else 1 << 19))
                exact += bits is not None and st[6:] == (bits, k)
    assert exact >= 2 * (4 + 4 + 3 + 3)          # modes 1 and 4 at every chunk size; 5, and the default whichever form it is, at every forced one


@pytest.mark.parametrize("c", [15, 16])
def test_work_efficient_form_from_16_bit_windows(dev, oracle, cus, c):
    """where the default's bit-sliced form steps aside the work-efficient one is chosen by !last_of_proof && c >= 16.  On one set the
    widths around 16 bits are bit-sliced under the default, so reduce_mode 6 (the default without that form) shows the rule's own
    threshold: two levels at 16 bits unless the MSM is the proof's last, the classic form at 15 bits"""
    base = T.reduce_case("g1", c, "every", 0)
    for last in (False, True):
        for chunk in (0, 16):
            st, _ = run(dev, oracle, cus, base.with_(last=last), {"reduce_mode": 6, "reduce_chunk": chunk}, 6, chunk)
            assert st[6:] == (0, (chunk or 4) if c == 16 and not last else 0), (c, last, chunk, st)


# ------------------------------------------------------------------------------------------------ f. batches
_BAT = T.batch_cases()


@pytest.mark.parametrize("case", _BAT, ids=_ids(_BAT))
def test_batches_one_window_per_vector(dev, oracle, cus, case):
    st, (got, ginf) = run(dev, oracle, cus, case)
    assert st[1] == case.batch
    if "zero" in case.name:
        assert int(ginf[case.name.split("-")[-1].split("+").index("zero")]) == 1


# ------------------------------------------------------------------------------------------------ g. argument edges
def test_argument_edges(dev, oracle, cus):
    case = T.digit_case("g1", 8)
    bases, inf, sc = case.arrays(oracle)
    run(dev, oracle, cus, case)
    before = dev.last_msm_state()
    n, fn = case.n, dev.lib.zkg16_diag_msm_tabled
    out = np.full((1, 12), 0x5a5a, dtype=np.uint64)
    oinf = np.full(1, 7, dtype=np.uint8)
    tab, tinf = np.full((32, n, 12), 0x5a5a, dtype=np.uint64), np.full((32, n), 7, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    good = dict(ctx=dev.ctx, group=1, bases=p(bases), inf=None, sc=p(sc), n=n, batch=1, c=8, stride=1, last=0, out=p(out), oinf=p(oinf), tab=None, tinf=None)
    call = lambda **kw: fn(*[dict(good, **kw)[k] for k in good])
    refused = [dict(ctx=None), dict(bases=None), dict(sc=None), dict(out=None), dict(oinf=None), dict(tab=p(tab)), dict(tinf=p(tinf)), dict(batch=0),
               dict(batch=-1), dict(stride=0), dict(stride=3), dict(c=1), dict(c=25), dict(c=0), dict(group=0), dict(group=3), dict(last=2),
               dict(last=-1), dict(c=24, batch=512)]
    for kw in refused:
        assert call(**kw) == BAD_ARG, kw
    # as many (scalar, window) terms as the plan refuses: nothing is read (the vectors are 2^20 times 16 scalars that nobody touches)
    big = np.zeros((1 << 20, 16, 4), dtype=np.uint64)
    assert call(c=2, n=16, batch=1 << 20, sc=p(big), tab=p(tab), tinf=p(tinf)) == ERR_HIP
    assert b"2^31" in dev.lib.zkg16_last_error(dev.ctx)
    del big
    # on any error nothing is written, and the state still is the last good call's
    assert (out == 0x5a5a).all() and (oinf == 7).all() and (tab == 0x5a5a).all() and (tinf == 7).all()
    assert dev.last_msm_state() == before
    # the infinity mask is optional, the table too; the call that succeeds writes all of it
    assert call(tab=p(tab), tinf=p(tinf)) == 0
    exp, einf = case.expected(oracle)[0]
    assert int(oinf[0]) == einf == 0 and np.array_equal(out[0], exp) and not (tinf != 0).any() and np.array_equal(tab[0], bases)
    assert dev.last_msm_state() == before
    # n == 0: every vector's value is the point at infinity, the state is the plan's alone, no table is written
    for group, w in (("g1", 12), ("g2", 24)):
        for batch in (1, 3):
            got, ginf, t, ti = dev.diag_msm_tabled(group, np.zeros((0, w), np.uint64), np.zeros((batch, 0, 4), np.uint64), 13, 2, True, want_table=True)
            assert ginf.tolist() == [1] * batch and not got.any() and t.shape == (20, 0, w) and ti.shape == (20, 0)
            assert dev.last_msm_state() == (13, batch, 0, 0, 0, 0, 0, 0)
    assert call(n=0, bases=None, sc=None) == 0 and int(oinf[0]) == 1 and not out.any()
    # a proof-sized call afterwards finds the slot's last_of_proof as it was, and zkg16_msm_g1 its own path
    got, ginf = dev.msm("g1", M.table(oracle, "g1")[:8], M.canon_vec(range(1, 9)))
    assert dev.last_msm_state()[:3] == (4, 64, 8)
    with pytest.raises(ValueError):
        dev.diag_msm_tabled("g1", bases[:5], sc, 8)
