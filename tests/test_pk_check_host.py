"""The lane functions of pk_check_g1_kernel / pk_check_g2_kernel (csrc/pk_check_dev.cuh) run on the CPU through
tests/csrc/pk_check_host_shim.hip, built with ZK_FQU_CHECK: every operand bound of the unsaturated field is asserted while the
cases run.  Every case's lane verdict equals zkg16_point_check's, by the endomorphism route and by the ladder by r, at the packed
entry stride and at the padded one with non-zero filler behind every entry.  Plus what needs no device: the ABI's argument checks,
the option's range, and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import pk_check_cases as K
from helpers import *


@pytest.fixture(scope="module")
def shim():
    return K.load_shim()


@pytest.mark.parametrize("fast", [True, False], ids=["endomorphism", "ladder_by_r"])
@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("group", K.GROUPS)
def test_lane_verdicts_equal_point_check(oracle, shim, group, layout, fast):
    if fast:
        assert shim.pkc_fast_available(1 if group == "g1" else 2) == 1         # the calibration found the constants: the fast route is the one tested
    pts, inf, names = K.case_arrays(oracle, group)
    want = K.expected(group, pts, inf)
    assert want.any() and not want.all()
    stride, filler = (K.PACKED[group], 0) if layout == "packed" else (K.PADDED[group], 0xA5)
    got = K.shim_verdicts(shim, group, pts, inf, stride, fast, filler)
    for name, g, w in zip(names, got, want):
        assert g == w, (name, layout, fast)


@pytest.mark.parametrize("group", K.GROUPS)
def test_padding_is_never_read(oracle, shim, group):
    """the same points at the padded stride under two different fillers, and at a stride with a whole entry of filler in between:
    the verdicts are the packed layout's"""
    pts, inf, _ = K.case_arrays(oracle, group)
    base = K.shim_verdicts(shim, group, pts, inf, K.PACKED[group], True)
    for stride, filler in ((K.PADDED[group], 0xFF), (K.PADDED[group], 0x01), (2 * K.PACKED[group], 0x5A)):
        assert np.array_equal(K.shim_verdicts(shim, group, pts, inf, stride, True, filler), base), (stride, filler)


def test_shim_refuses_a_stride_below_the_entry(shim):
    good = np.zeros(1, dtype=np.uint8)
    pts = np.zeros(24, dtype=np.uint64)
    assert shim.pkc_lanes(1, pts.ctypes.data, None, 1, 108, 1, 0, good.ctypes.data) == -1
    assert shim.pkc_lanes(2, pts.ctypes.data, None, 1, 112, 1, 0, good.ctypes.data) == -1


def test_abi_argument_checks():
    """what the two entries refuse before they touch a ctx"""
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    BAD_ARG = 1
    assert lib.zkg16_strerror(BAD_ARG).decode()          # the status the refusals below return is a named one
    n_bad, first_bad = np.zeros(5, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    mask, ok = C.c_uint32(0), C.c_int(0)
    nb, fb = C.c_uint64(0), C.c_uint64(0)
    pts = np.zeros(12, dtype=np.uint64)
    assert lib.zkg16_pk_check(None, 1, n_bad.ctypes.data, first_bad.ctypes.data, C.byref(mask), C.byref(ok)) == BAD_ARG
    assert lib.zkg16_points_check_bulk(None, 1, pts.ctypes.data, None, 1, C.byref(nb), C.byref(fb)) == BAD_ARG


def test_python_surface():
    from zksnark_finalproject_amd import Device, handlers
    from zksnark_finalproject_amd.device import PK_QUERIES, PK_SINGLES
    import inspect
    assert PK_QUERIES == ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
    assert PK_SINGLES == ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2")
    assert callable(Device.pk_check) and callable(Device.points_check_bulk)
    for fn in (handlers.fibonacci_key, handlers.linear_key, handlers.prime_template_key):
        assert inspect.signature(fn).parameters["check_key"].default is False
