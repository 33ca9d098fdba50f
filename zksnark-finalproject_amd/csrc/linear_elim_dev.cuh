// The second solver of the linear-equations route (option "linear_solver" = 1; witness.hip: wit_linear_elim_kernel, one workgroup of
// LINEAR_ELIM_LANES lanes per request): Gaussian elimination over Fr with row pivoting, for any square a.  Written __host__ __device__
// as what ONE lane of `lanes` does between two barriers, so that the host solver (circuits.hip: lanes = 1) and
// tests/csrc/linear_general_host_shim.hip (64 and 256 simulated lanes, phase by phase) run the kernel's own code.
//
// Working set of a request: M, the n x (n + 1) augmented matrix [a | b] in Montgomery form, row-major; order[n], a permutation of
// the rows — order[0 .. c) are the pivot rows of columns 0 .. c-1, order[c .. n) the rows still to be reduced; inv[n], the
// inverted pivots, later x.
//
// Forward elimination, column c = 0 .. n-1, division-free.  Pivot: the smallest k >= c with M[order[k]][c] != 0 (every lane offers
// the smallest of its k = c + lane, c + lane + lanes, ..; the least offer wins and order[c], order[k] swap — any non-zero entry would
// do, the solution does not depend on it).  Then every row i = order[k], k > c, with f = M[i][c] != 0 becomes p row_i - f row_p over
// the columns j > c (p = M[order[c]][c]; column c of row i is not written: nothing reads it again).  p != 0, so the rank is kept;
// a row with f = 0 stays as it is.  No inversion happens here: a lone lane's fp_inv per column would be ~380 serial products n times.
// Then the n pivots are inverted at once (lane l the columns l, l + lanes, ..), and the back substitution runs by columns,
// c = n-1 .. 0: x_c = M[order[c]][n] inv_c, which every lane forms for itself, and row order[r], r < c, takes M[.][c] x_c off its
// right-hand side M[.][n] — one barrier per column and no exchange between lanes, where the forward solver's row-wise fold needs six.
//
// Singular systems: a column c without a pivot is the smallest c for which columns 0 .. c of a are linearly dependent mod r (the rows
// left have zeros in columns 0 .. c-1, which the c pivots span, so column c adds nothing to the rank) — whatever pivots were taken
// before.  The status of the request is 1 + c, 0 for a solved one.  From there on the kernel skips the arithmetic of that request
// but passes every barrier, so the barrier counts depend on n alone; the host solver returns at once.
//
// Value bounds: every function takes and returns fully reduced residues (fp_to_mont, fp_mul, fp_sub and fp_inv all end below r), so
// whatever is stored in M, inv or x is the canonical Montgomery form.  The solution of a non-singular system is unique in Fr, so x is
// byte for byte the same for every lane count, pivot choice and summation order.  n <= ZKG16_LINEAR_N_MAX = 1024: the indices
// i (n + 1) + j stay below 2^21.
//
// Include after ff.cuh and linear_dev.cuh inside namespace zk (or after `using namespace zk`).
#pragma once

constexpr int LINEAR_ELIM_LANES = 256;
constexpr int LINEAR_ELIM_LDS_N = 64;           // the largest n whose working set a workgroup keeps in LDS by default (M: 133,120 bytes)

// phase 0: M from the request, order = identity
ZK_HD void linear_elim_load(size_t n, const uint64_t *a, const uint64_t *b, Fr *M, uint32_t *order, int lane, int lanes) {
    const size_t w = n + 1;
    for (size_t e = (size_t)lane; e < n * w; e += (size_t)lanes) {
        const size_t i = e / w, j = e % w;
        M[e] = linear_mont(j < n ? a[i * n + j] : b[i]);
    }
    for (size_t i = (size_t)lane; i < n; i += (size_t)lanes) order[i] = (uint32_t)i;
}

// column c, phase 1: the lane's offer for the pivot, the smallest of its k in [c, n) with a non-zero entry in column c, or n
ZK_HD uint32_t linear_elim_offer(size_t n, const Fr *M, const uint32_t *order, size_t c, int lane, int lanes) {
    for (size_t k = c + (size_t)lane; k < n; k += (size_t)lanes)
        if (!M[(size_t)order[k] * (n + 1) + c].is_zero()) return (uint32_t)k;
    return (uint32_t)n;
}

// column c, phase 2 (one lane): the least offer k < n takes place c
ZK_HD void linear_elim_swap(uint32_t *order, size_t c, uint32_t k) {
    const uint32_t t = order[c];
    order[c] = order[k];
    order[k] = t;
}

// column c, phase 3: the lane's share of the (n - c - 1) x (n - c) entries below and right of the pivot
ZK_HD void linear_elim_reduce(size_t n, Fr *M, const uint32_t *order, size_t c, int lane, int lanes) {
    const size_t w = n + 1, cols = n - c, total = (n - c - 1) * cols;
    const Fr *prow = M + (size_t)order[c] * w;
    const Fr p = prow[c];
    for (size_t e = (size_t)lane; e < total; e += (size_t)lanes) {
        Fr *row = M + (size_t)order[c + 1 + e / cols] * w;
        const size_t j = c + 1 + e % cols;
        const Fr f = row[c];
        if (!f.is_zero()) row[j] = fp_sub(fp_mul(p, row[j]), fp_mul(f, prow[j]));
    }
}

// after the last column: 1 / pivot of the lane's columns
ZK_HD void linear_elim_invert(size_t n, const Fr *M, const uint32_t *order, Fr *inv, int lane, int lanes) {
    for (size_t c = (size_t)lane; c < n; c += (size_t)lanes) inv[c] = fp_inv(M[(size_t)order[c] * (n + 1) + c]);
}

// back substitution, column c: -> x_c (the same in every lane); the lane's rows r < c take their term in x_c off the right-hand side
ZK_HD Fr linear_elim_back(size_t n, Fr *M, const uint32_t *order, const Fr *inv, size_t c, int lane, int lanes) {
    const size_t w = n + 1;
    const Fr xc = fp_mul(M[(size_t)order[c] * w + n], inv[c]);
    for (size_t r = (size_t)lane; r < c; r += (size_t)lanes) {
        Fr *row = M + (size_t)order[r] * w;
        if (!row[c].is_zero()) row[n] = fp_sub(row[n], fp_mul(row[c], xc));
    }
    return xc;
}

// The whole schedule on one lane: the host solver.  M: n (n + 1), inv: n, order: n.  -> the status; x (n, Montgomery) is written only
// for 0.
inline uint32_t linear_elim_solve_host(size_t n, const uint64_t *a, const uint64_t *b, Fr *M, Fr *inv, uint32_t *order, Fr *x) {
    linear_elim_load(n, a, b, M, order, 0, 1);
    for (size_t c = 0; c < n; c++) {
        const uint32_t k = linear_elim_offer(n, M, order, c, 0, 1);
        if (k == n) return (uint32_t)(1 + c);
        linear_elim_swap(order, c, k);
        linear_elim_reduce(n, M, order, c, 0, 1);
    }
    linear_elim_invert(n, M, order, inv, 0, 1);
    for (size_t c = n; c-- > 0;) x[c] = linear_elim_back(n, M, order, inv, c, 0, 1);
    return 0;
}
