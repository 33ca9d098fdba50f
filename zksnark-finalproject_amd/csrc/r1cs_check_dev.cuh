// Does an assignment satisfy its R1CS?  (A z)_i (B z)_i == (C z)_i for every constraint row i: the lane function and the block
// reduction of r1cs_check_kernel (poly.hip), which reads the three vectors the witness map's SpMV has just written.  All of it is
// integer arithmetic on u32 / u64, ZK_HD, so tests/csrc/r1cs_check_host_shim.hip runs the same functions on the host.
//
//   row_fails     the Montgomery product of a and b against c, as fully reduced residues.  What the SpMV leaves behind is already
//                 below r when the coefficients and the assignment are (fp_mul and fp_add both end in fp_reduce_once, and so does
//                 wm_patch_kernel's sum) — but an assignment is the caller's bytes, a row of the dictionary kernel whose
//                 coefficient is one adds z[col] without a product, and 2^256 < 3 r: two conditional subtractions make any 256-bit
//                 word the residue it stands for, so the verdict never depends on which representative a row arrived as.
//   block_fold    the verdicts of a 256-lane block, four 64-bit wave ballots, as (failing rows, smallest failing row)
//   result_init   what the result words hold before the first block reports: no failing row, first = all ones
//   result_merge  how a block with a failing row reports (the kernel: atomicAdd + atomicMin — any order of blocks gives the same words)
#pragma once
#include <stddef.h>

#include "ff.cuh"

namespace zk {
namespace rck {

constexpr unsigned BLOCK = 256, WAVES = BLOCK / 64;
constexpr uint64_t NONE = ~(uint64_t)0;

ZK_HD Fr canonical(Fr v) {
    fp_reduce_once(v);
    fp_reduce_once(v);
    return v;
}
ZK_HD bool row_fails(const Fr &a, const Fr &b, const Fr &c) { return canonical(fp_mul(a, b)) != canonical(c); }

ZK_HD unsigned popcount64(uint64_t m) { return (unsigned)__builtin_popcountll(m); }
ZK_HD unsigned lowest_bit64(uint64_t m) { return (unsigned)__builtin_ctzll(m); }      // m != 0
// ballots[w]: bit l set = lane 64 w + l of the block found its row failing; row0 = the block's first row.  -> any failing row
ZK_HD bool block_fold(const uint64_t ballots[WAVES], uint64_t row0, uint64_t &count, uint64_t &first) {
    count = 0;
    first = NONE;
    for (unsigned w = 0; w < WAVES; w++) {
        const uint64_t m = ballots[w];
        if (!m) continue;
        if (first == NONE) first = row0 + 64u * w + lowest_bit64(m);
        count += popcount64(m);
    }
    return count != 0;
}
// res: n_bad[nvec] | first_bad[nvec]; word t < 2 nvec
ZK_HD uint64_t result_init(unsigned t, unsigned nvec) { return t < nvec ? 0 : NONE; }
ZK_HD void result_merge(uint64_t &n_bad, uint64_t &first_bad, uint64_t count, uint64_t first) {
    n_bad += count;
    if (first < first_bad) first_bad = first;
}

}  // namespace rck
}  // namespace zk
