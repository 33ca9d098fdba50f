"""Field and curve primitives one operation at a time on the DEVICE, on raw limbs at the top of their operand bounds: the gfx950
build of tests/csrc/prim_shim.hip, one kernel per operation variant, one lane per case, 64 lanes per block (cases and exact
checkers: tests/prim_cases.py; tests/test_prim_host.py runs them on the CPU).

The device runs what a host compile cannot reach: `fp_mul_inline` behind the `fq_mul_call` wrapper, `fqu_mul_call` /
`fqu_sqr_call`, `fq2u_mul_lazy` with its LDS parking, `xyzz_madd_lazy`, `xyzz_madd_inline` / `xyzz_dbl_affine_inline`.  Every
operation that exists in both builds must also give the host build's raw output limbs exactly: code generation must not change a
value.

Scope: this tests the headers as compiled for gfx950 in small kernels, with the product's flags.  It does not test the exact
instruction stream of `msm_accumulate_kernel`, whose register pressure and scheduling differ."""
import numpy as np
import pytest

import prim_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return PC.load_shim("device")


@pytest.fixture(scope="module")
def host():
    return PC.load_shim("host")


def both(dev, host, batches):
    return PC.run_batches(dev, batches, host=host, include_device_only=True)


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_saturated_field_edges(dev, host, field):
    """fp_mul on the device is fp_mul_inline (Fr) / fq_mul_call (Fq); the host build's fp_mul is fp_mul_host64: equal outputs"""
    assert both(dev, host, PC.sat_batches(field)) == 10


def test_fqu_products_at_bounds(dev, host):
    both(dev, host, PC.fqu_product_batches())


def test_fqu_linear_at_bounds(dev, host):
    both(dev, host, PC.fqu_linear_batches())


def test_fqu_is_zero_mod_and_tidy(dev, host):
    both(dev, host, PC.fqu_zero_batches())


def test_fqu_conversions_and_inverse(dev, host):
    both(dev, host, PC.fqu_conversion_batches())


def test_fq2u_at_bounds(dev, host):
    """with fq2u_mul_lazy (device only): components up to 127q in, below 2q out"""
    names = [b.name for b in PC.fq2u_batches() if b.device_only]
    assert names == ["fq2u_mul_lazy"]
    both(dev, host, PC.fq2u_batches())


def test_fru_ops(dev, host):
    both(dev, host, PC.fru_batches())


@pytest.mark.parametrize("variant", ["madd", "madd_split", "madd_device", "add", "dbl", "dbl_affine"])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_curve_ops_at_bounds(dev, host, group, variant):
    """madd_device is xyzz_madd_inline in G1 and xyzz_madd_lazy in G2"""
    assert both(dev, host, PC.curve_batches(group, variant)) == len(PC.LANE_COUNTS)


def test_g1_madd_inline_equals_madd(dev):
    """ec.cuh: "the same formulas, in the same order, as xyzz_madd (bit-identical sums)" - limb for limb, every case"""
    inp, _ = PC.curve_inputs("g1", "madd")
    assert np.array_equal(PC.run(dev, PC.OP["g1_madd_device"], inp), PC.run(dev, PC.OP["g1_madd"], inp))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_curve_chain(dev, host, group):
    both(dev, host, PC.chain_batches(group))
    print("\n".join(PC.report(group, "device build")))
