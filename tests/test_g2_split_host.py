"""The pair-split G2 mixed addition (csrc/g2split.cuh: what msm_accumulate_split_kernel runs, option "g2_split") on the CPU: the lane
pair is emulated by a two-element array (H2Pair), the shim tests/csrc/g2_split_host_shim.hip is compiled with ZK_FQU_CHECK, and the
cases run in a child process (tests/g2_split_cases.py: check_all).  No GPU needed, no sanitizer, nothing preloaded.

While the cases run, every subtrahend and product operand is asserted against its value bound, every operand that skipped its carry
pass against the limb bound it was declared with, and every product column is accumulated a second time in 128 bits and must equal
the 64-bit accumulator.  An assertion aborts the child, so "ok" means they all stayed silent; the last test shows that they can fire."""
import subprocess
import sys

import pytest

import g2_split_cases as GC

CHILD = """
import sys
sys.path[:0] = %r
import g2_split_cases as GC
print("before", flush=True)
print(GC.check_all(%d), flush=True)
"""

CHILD_BAD = """
import sys
sys.path[:0] = %r
import numpy as np
import g2_split_cases as GC
import madd_lazy_cases as MC
import prim_cases as PC
lib = GC.load_shim()
inp, _ = MC.chain_cases("g2")
rec = inp[2:3].copy()                       # the accumulator of one chain; its Y.c1 is raised to 64q + 1: above what the addition may subtract
rec[0, 3 * 14:4 * 14] = PC.u_pack([[64 * PC.Q + 1]])[0]
print("before", flush=True)
GC.run(lib, GC.OP["madd"] + %d, rec)
print("after", flush=True)
"""


@pytest.fixture(scope="module")
def built():
    return GC.build_shim()


def _child(code):
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("lc", [0, 1], ids=["carry-passes", "lazy-carries"])
def test_split_addition_against_points_formulas_and_one_lane(built, lc):
    """640 single additions (both signs, P + P, P - P, operands at infinity, coordinates at 42q / 42q / 10q), 180 worst-limb
    accumulators against the formulas, 70 chains of 32 additions from accumulators at the stored maxima through the doubling, the
    cancellation and the restart, each step equal to ec_add's point and, coordinate by coordinate as residues, to the one-lane
    xyzz_madd_lazy (lc: xyzz_madd_lazy_lc)"""
    r = _child(CHILD % ([p for p in sys.path if p], lc))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok points=640 "), r.stdout
    assert "chain_steps=2240" in last and "worst=180" in last


@pytest.mark.parametrize("lc,message", [(0, "fqu_sub subtrahend"), (1, "fqu_rsub_raw")])
def test_operand_assertions_fire(built, lc, message):
    """an accumulator whose Y is above 63q trips the subtrahend bound of R = S2 - Y1 in either form: the checks are live in the text the
    split addition runs.  Host abort in a CPU child process."""
    r = _child(CHILD_BAD % ([p for p in sys.path if p], lc))
    assert r.returncode == -6, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "before" in r.stdout and "after" not in r.stdout
    assert message in r.stderr, r.stderr[-2000:]
