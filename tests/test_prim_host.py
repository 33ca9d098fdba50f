"""Field and curve primitives one operation at a time, on raw limbs at the top of their operand bounds, through the HOST build of
tests/csrc/prim_shim.hip (cases and exact checkers: tests/prim_cases.py).  No GPU needed.

What this adds to tests/test_ff_host.py: `fp_mul_inline` - the 32-bit-limb CIOS the kernels run, which a host compile otherwise
never reaches because `fp_mul` routes to `fp_mul_host64` there - on every ordered pair of the edge patterns; U-form operands fed
as raw limbs, so products meet operands up to 2^12 q - 1, subtractions meet subtrahends of exactly (L - 1) q, and the curve
formulas meet accumulators at 42q / 42q / 10q / 10q with bases at 2q.  The shim is compiled with ZK_FQU_CHECK (csrc/ffu.cuh), so
every intermediate subtrahend and product operand inside the formulas is asserted against its stated condition while the cases
run, not only the outputs.  tests/test_prim_gpu.py runs the same cases through the gfx950 build."""
import pytest

import prim_cases as PC


@pytest.fixture(scope="module")
def shim():
    return PC.load_shim("host")


def test_checked_build(shim):
    """the host build carries the operand assertions, and refuses the operations that only a device pass has"""
    assert shim.prim_fqu_check_active() == 1
    for name in ("fq2u_mul_lazy", "g1_madd_device", "g2_madd_device"):
        assert shim.prim_run(PC.OP[name], 0, None, None) == -2
    assert shim.prim_run(99, 0, None, None) == -1


@pytest.mark.parametrize("field", ["fr", "fq"])
def test_saturated_field_edges(shim, field):
    """add, sub, neg, dbl, fp_mul, fp_mul_inline (called directly), sqr, to_mont, from_mont on all ordered pairs of the edge
    patterns, inv on 64 of them"""
    assert PC.run_batches(shim, PC.sat_batches(field)) == 10


def test_fqu_products_at_bounds(shim):
    """fqu_mul, fqu_sqr, fqu_mul_impl<false|true>, fqu_mul2 with every operand at bound 1, 2, 4095 or 4096: congruent, < 2q"""
    PC.run_batches(shim, PC.fqu_product_batches())


def test_fqu_linear_at_bounds(shim):
    """fqu_add, fqu_dbl, fqu_sub<8|32|64|128> with the subtrahend at (L - 1) q, fqu_neg, and the constants against their definitions"""
    PC.run_batches(shim, PC.fqu_linear_batches())


def test_fqu_is_zero_mod_and_tidy(shim):
    """k q, k q + 1, k q - 1 for every k = 0 .. 4096"""
    PC.run_batches(shim, PC.fqu_zero_batches())


def test_fqu_conversions_and_inverse(shim):
    PC.run_batches(shim, PC.fqu_conversion_batches())


def test_fq2u_at_bounds(shim):
    """f_mul, fq2u_mul_inline, f_sqr, f_sub, f_sub2, f_neg, f_inv against pyref.Fq2, outputs inside the commented bounds"""
    PC.run_batches(shim, PC.fq2u_batches())


def test_fru_ops(shim):
    PC.run_batches(shim, PC.fru_batches())


@pytest.mark.parametrize("variant", ["madd", "madd_split", "add", "dbl", "dbl_affine"])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_curve_ops_at_bounds(shim, group, variant):
    """the group element equals ec_add, infinity is an exact-zero ZZ, ZZ^3 == ZZZ^2, and the outputs are again inside the
    stored bounds, at n = 1, 63, 64, 65, 640 cases"""
    assert PC.run_batches(shim, PC.curve_batches(group, variant)) == len(PC.LANE_COUNTS)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_curve_chain(shim, group):
    """32 dependent steps per lane; prints the largest stored coordinates met (DESIGN.md 2.1 records them)"""
    PC.run_batches(shim, PC.chain_batches(group))
    print("\n".join(PC.report(group, "host build")))
