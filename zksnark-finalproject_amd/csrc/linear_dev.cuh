// The per-request arithmetic of the linear-equations assignment (witness.hip: wit_linear_solve_kernel, one 64-lane wave per
// request, and wit_linear_fill_kernel, one lane per element), written __host__ __device__ so that
// tests/csrc/linear_host_shim.hip can drive the same code lane by lane on a machine without a GPU.
//
// The handler's solver (backend/linear_equations.rs:20-41) is a forward substitution on the lower triangle of a:
//   x_i = (b_i - sum_{j < i} a_ij x_j) / a_ii,  i = 0 .. n-1.
// Row i needs every earlier x_j, so the rows are sequential; inside a row the i products are independent.  A wave shares them: lane l
// takes the j = l, l + 64, ... below i, the 64 partial sums are folded by a butterfly of limb exchanges (linear_fold_step, partner =
// lane ^ 32, 16, .. 1, after which every lane holds the sum), and lane 0 forms x_i.  The n inversions are taken first, lane l the
// rows i = l, l + 64, ...
//
// Value bounds: every function takes and returns fully reduced residues (fp_add, fp_sub and fp_mul all end on a value below r).  Field
// addition is exact, so the folded sum is the canonical residue whatever order the butterfly adds in, and every stored element is
// byte for byte the host solver's.  The inputs are u64 and enter the products as they are: the Montgomery product of a canonical a
// with y = x R^2 (x in Montgomery form taken to Montgomery form once more) is a x R, the Montgomery form of a x — one product per
// term where converting a first would cost two.  y_j is what a wave keeps of x_j.
//
// Include after ff.cuh inside namespace zk (or after `using namespace zk`).
#pragma once

constexpr int LINEAR_LANES = 64;

ZK_HD Fr linear_canon(uint64_t v) {             // v as a canonical (non-Montgomery) residue: below 2^64 < r
    Fr c = Fr::zero();
    c.l[0] = (uint32_t)v;
    c.l[1] = (uint32_t)(v >> 32);
    return c;
}
ZK_HD Fr linear_mont(uint64_t v) { return fp_to_mont(linear_canon(v)); }

// 1 / a_ii in Montgomery form.  a_ii != 0: every entry refuses a zero diagonal before any device work.
ZK_HD Fr linear_diag_inv(uint64_t aii) { return fp_inv(linear_mont(aii)); }

// lane's share of row i: sum of a_ij x_j over j < i with j = lane mod 64, in Montgomery form.  arow = a + i n; y[j] = x_j R^2.
ZK_HD Fr linear_partial(const uint64_t *arow, const Fr *y, size_t i, int lane) {
    Fr acc = Fr::zero();
    for (size_t j = (size_t)lane; j < i; j += LINEAR_LANES) acc = fp_add(acc, fp_mul(linear_canon(arow[j]), y[j]));
    return acc;
}

// one step of the butterfly: a lane's value after it has seen its partner's
ZK_HD Fr linear_fold_step(const Fr &mine, const Fr &partner) { return fp_add(mine, partner); }

// x_i from the folded sum, and what the wave keeps of it
ZK_HD Fr linear_finish(uint64_t bi, const Fr &sum, const Fr &inv) { return fp_mul(fp_sub(linear_mont(bi), sum), inv); }
ZK_HD Fr linear_keep(const Fr &x) { return fp_to_mont(x); }

// Element t of a request's assignment z (t < 3 n^2 + 2 n + 1; the layout is in zkg16.h): 1 | per row i: a_i0 .. a_i,n-1, b_i | per row
// i: 0, then x_j, a_ij x_j for j < n.  x: the request's solution in Montgomery form.
ZK_HD Fr linear_fill_value(size_t n, const uint64_t *a, const uint64_t *b, const Fr *x, size_t t) {
    const size_t ni = 1 + n * (n + 1);
    if (t == 0) return Fr::one();
    if (t < ni) {
        const size_t i = (t - 1) / (n + 1), j = (t - 1) % (n + 1);
        return linear_mont(j < n ? a[i * n + j] : b[i]);
    }
    const size_t w = t - ni, i = w / (2 * n + 1), q = w % (2 * n + 1);
    if (q == 0) return Fr::zero();
    const size_t j = (q - 1) / 2;
    return (q & 1) ? x[j] : fp_mul(linear_mont(a[i * n + j]), x[j]);
}
