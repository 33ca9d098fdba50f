"""The bucket accumulations' mixed additions without their spare carry passes (csrc/ec.cuh: xyzz_madd_inline_lc, xyzz_madd_lazy_lc)
through the HOST build of tests/csrc/madd_lazy_shim.hip, against Python big integers (cases and checkers:
tests/madd_lazy_cases.py).  No GPU needed.

The shim is compiled with ZK_FQU_CHECK (csrc/ffu.cuh): while the cases run, every subtrahend and product operand is asserted
against its value bound, every operand that skipped its carry pass against the limb bound it was declared with (2^30 or 2^31), and
every product column is accumulated a second time in 128 bits and must equal the 64-bit accumulator.  An assertion aborts the
process, so a passing test means they all stayed silent; the last two tests show, in a child process, that they can fire."""
import subprocess
import sys

import numpy as np
import pytest

import madd_lazy_cases as MC
import prim_cases as PC


@pytest.fixture(scope="module")
def shim():
    return MC.load_shim("host")


def test_checked_build(shim):
    assert shim.madd_lazy_check_active() == 1
    assert shim.madd_lazy_run(99, 0, None, None) == -1


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_madd_points_at_bounds(shim, group):
    """random accumulators and bases of both signs, P + P, P - P, either operand at infinity, accumulators at 42q / 42q / 2q (G2:
    10q) and bases at 2q: the group element equals ec_add, ZZ^3 == ZZZ^2, outputs normalised and inside the stored bounds"""
    inp, expected = MC.point_cases(group)
    assert inp[:, -1].any() and not inp[:, -1].all()
    MC.check_points(group, inp, expected, MC.run(shim, MC.OP[group + "_madd"], inp))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_madd_worst_limbs(shim, group):
    """accumulator coordinates with limbs 0..12 all at 2^29 - 1, reduced or at the stored bound: the four output coordinates equal
    the formulas evaluated in Python, normalised and inside the stored bounds"""
    inp, meta = MC.worst_limb_cases(group)
    assert len(meta) == 15 * 2 * 3 * 2
    assert (inp[0, :13] == PC.M29).all()
    MC.check_worst(group, meta, MC.run(shim, MC.OP[group + "_madd"], inp))


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_madd_chains(shim, group):
    """32 dependent additions per lane, the point after every step checked; some chains pass through the doubling, the cancellation
    and a restart from infinity"""
    inp, expected = MC.chain_cases(group)
    seen = MC.check_chain(group, inp, expected, MC.run(shim, MC.OP[group + "_chain"], inp))
    assert seen["steps"] == MC.CHAIN_LANES * MC.CHAIN_STEPS


CHILD = """
import sys
sys.path[:0] = %r
import numpy as np
import madd_lazy_cases as MC
lib = MC.load_shim("host")
inp = np.full((1, 28), %d, np.uint32)
inp[0, 13] = inp[0, 27] = 1
print("before", flush=True)
MC.run(lib, MC.OP[%r], inp)
print("after", flush=True)
"""


@pytest.mark.parametrize("op,limb,message", [("bad_two_lazy", (1 << 29) + (1 << 30) - 1, "fqu_mul_impl a: a limb of the operand is not below 2^29"),
                                             ("bad_column", (1 << 31) - 1, "overflows its 64-bit accumulator")])
def test_forbidden_operands_abort(shim, op, limb, message):
    """a product of two operands that both skipped their carry pass (limbs at 2^30.58) trips the operand check of fqu_mul_impl; a
    column of products of 2^31-sized limbs trips the 128-bit column check.  Host aborts in a CPU child process."""
    r = subprocess.run([sys.executable, "-c", CHILD % ([p for p in sys.path if p], limb, op)], capture_output=True, text=True, timeout=120)
    assert r.returncode == -6, (r.returncode, r.stdout, r.stderr)
    assert "before" in r.stdout and "after" not in r.stdout
    assert message in r.stderr, r.stderr
