// The front of batched verification for statements whose public inputs are plain 64-bit values (verify_batch.hpp: the u64 form):
// proof k of a key with num_instance points has the m = num_instance - 1 inputs values[k][0 .. m), 8 bytes each, row-major.  Here:
// the lane functions of the three kernels of verify_batch.hip that take the multiplier sums of the batch equation and each listed
// proof's prepared input X_k on the device from those rows.  ZK_HD throughout, so tests/csrc/u64_inputs_host_shim.hip runs the same
// functions on the host.
//
//   column_sum       what one lane of a 256-lane block adds up over a slice of proofs: column 0 is sum rho_k, column 1 + c is
//                    sum rho_k values[k][c] — plain integers in 4 u64: rho < 2^128, values < 2^64, K < 2^32, so every sum stays
//                    below 2^224 < r and nothing is reduced on the device.  A lane owns a column: the reads of a row are contiguous
//                    across the lanes of a wave, and rho_k is one address for all of them
//   ladder           one lane's share of X_k = gamma_abc[0] + sum_c values[k][c] gamma_abc[1 + c]: a proof is spread over L lanes,
//                    lane l owning the columns c = l (mod L), and a lane runs ONE doubling chain for all its columns — for
//                    b = 63 .. 0: acc = 2 acc, then acc += gamma_abc[1 + c] for every owned column whose bit b is set.  64
//                    doublings and 64 ceil(m / L) guarded mixed additions per lane, where one scalar multiplication per input
//                    costs up to 63 of each per column on a single lane
//   finish           the group's sum (the L partial sums met by xyzz_add in log2 L rounds, verify_batch.hip) plus gamma_abc[0],
//                    to affine: what pd::prepared_input returns for the same inputs, limb for limb once in canonical limbs
#pragma once
#include <stddef.h>

#include "pairing_dev.cuh"
#include "prime_inputs_dev.cuh"

namespace zk {
namespace u6 {

constexpr size_t SUM_SLICE = 128;        // proofs per slice, at least
constexpr size_t SUM_SLICES_MAX = 256;   // ... and at most this many slices: the partial sums of m = 4,160 stay at 34 MB
constexpr unsigned SUM_LANES = 256;

// the slices a batch of k proofs is cut into, and the proofs of one slice (the last slice may be shorter or empty)
ZK_HD size_t sum_slices(size_t k) {
    const size_t s = (k + SUM_SLICE - 1) / SUM_SLICE;
    return s < SUM_SLICES_MAX ? s : SUM_SLICES_MAX;
}
ZK_HD size_t slice_len(size_t k) {
    const size_t s = sum_slices(k);
    return s ? (k + s - 1) / s : 0;
}

// column col (<= m) over the proofs [lo, hi): acc = sum rho_k (col == 0) or sum rho_k values[k][col - 1], live proofs only
// (live nullable: all).  values: k x m; rho: 2 u64 per proof
ZK_HD void column_sum(size_t col, const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t lo, size_t hi, uint64_t acc[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = 0;
    for (size_t k = lo; k < hi; k++) {
        if (live && !live[k]) continue;
        const uint64_t v = col ? values[k * m + (col - 1)] : 1;
        pi::add_mul(acc, rho[2 * k], rho[2 * k + 1], v);
    }
}

// the lanes a proof of m inputs is spread over: the smallest power of two >= min(m, 64)
ZK_HD unsigned group_lanes(size_t m) {
    unsigned l = 1;
    while (l < 64 && l < m) l <<= 1;
    return l;
}

// lane `lane` of the L that share a proof: sum over its columns c = lane, lane + L, ... < m of row[c] gamma_abc[1 + c].
// gamma_abc: 1 + m affine points in U-form (tidy; exact zeros = the point at infinity); row: the proof's m values.
// xyzz_madd meets equal, opposite and infinite operands (the accumulator is a sum of multiples of the very bases it adds)
ZK_HD XYZZ<FqU> ladder(const Affine<FqU> *gamma_abc, size_t m, const uint64_t *row, unsigned lane, unsigned L) {
    XYZZ<FqU> acc = XYZZ<FqU>::inf();
#pragma unroll 1
    for (int b = 63; b >= 0; b--) {
        acc = xyzz_dbl(acc);
#pragma unroll 1
        for (size_t c = lane; c < m; c += L)
            if ((row[c] >> b) & 1) xyzz_madd(acc, gamma_abc[1 + c], false);
    }
    return acc;
}

// sum (the group's total) + gamma_abc[0], to affine as pd::prepared_input does.  false: the point at infinity (ox, oy untouched)
ZK_HD bool finish(XYZZ<FqU> sum, const Affine<FqU> &g0, FqU &ox, FqU &oy) {
    xyzz_madd(sum, g0, false);
    if (sum.is_inf()) return false;
    // stored coordinates are < 42q (ec.cuh); fqu_inv takes anything below 2^12 q and returns a product
    const FqU iv = fqu_inv(pd::mulq(sum.zz, sum.zzz));
    ox = pd::mulq(sum.x, pd::mulq(iv, sum.zzz));
    oy = pd::mulq(sum.y, pd::mulq(iv, sum.zz));
    return true;
}

}  // namespace u6
}  // namespace zk
