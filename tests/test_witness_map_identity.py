"""The identity behind the six-transform witness map (csrc/poly.hip: wm_transforms), checked in Python big integers with the
ark-poly transforms by definition (pyref.dft_naive):

    coset_ifft((A_cos * B_cos - C_cos) / Z) == coset_ifft(A_cos * B_cos / Z) - ifft(c) / Z,   X_cos = coset_fft(ifft(x)),

Z = g^N - 1 (Z(X) = X^N - 1 is one constant on the coset g H).  coset_ifft is linear and coset_ifft(coset_fft(y)) = y, so C needs
only its inverse transform.  Exact in Fr for any a, b, c: satisfied (a * b = c on the domain) or not."""
import random

import pytest

import pyref as P

R = P.R_MOD


def seven(a, b, c):
    """arkworks' LibsnarkReduction::witness_map_from_matrices: seven transforms."""
    n = len(a)
    zinv = pow((pow(P.FR_GEN, n, R) - 1) % R, -1, R)
    cos = [P.dft_naive(P.dft_naive(x, inverse=True), coset=True) for x in (a, b, c)]
    return P.dft_naive([(x * y - w) * zinv % R for x, y, w in zip(*cos)], inverse=True, coset=True)


def six(a, b, c):
    """the device's six: A and B to the coset, C only inverse-transformed and subtracted after the last transform."""
    n = len(a)
    zinv = pow((pow(P.FR_GEN, n, R) - 1) % R, -1, R)
    ac, bc = (P.dft_naive(P.dft_naive(x, inverse=True), coset=True) for x in (a, b))
    h = P.dft_naive([x * y * zinv % R for x, y in zip(ac, bc)], inverse=True, coset=True)
    ci = P.dft_naive(c, inverse=True)
    return [(v - zinv * w) % R for v, w in zip(h, ci)]


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
@pytest.mark.parametrize("satisfied", [True, False])
def test_six_transforms_equal_seven(log_n, satisfied):
    n = 1 << log_n
    rng = random.Random(1000 * log_n + satisfied)
    a = [P.rand_fr(rng) for _ in range(n)]
    b = [P.rand_fr(rng) for _ in range(n)]
    c = [x * y % R for x, y in zip(a, b)] if satisfied else [P.rand_fr(rng) for _ in range(n)]
    want = seven(a, b, c)
    assert six(a, b, c) == want
    # satisfied: a b - c vanishes on the domain, so h has degree <= N - 2; an unsatisfied vector reaches the top coefficient
    assert (want[-1] == 0) == satisfied
