// TEST-ONLY: the device decompression header (csrc/decompress_dev.cuh — what verify_batch.hip's decompress_kernel runs, one GPU lane
// per point) compiled for the host, so that its square roots and whole-point decoding can be compared with the library's host
// decoders on a machine without a GPU.  Built by tests/test_decompress_dev.py with `hipcc --offload-host-only`; ZK_PD_CHECK turns on
// the value-bound assertions of pairing_dev.cuh, which the header's operations go through.  Field values cross this interface in
// saturated Montgomery limbs (u64), points as wire bytes.
#define ZK_PD_CHECK 1
#include "ff.cuh"
#include "ec.cuh"
#include "decompress_dev.cuh"
#include "hostff.hpp"
#include <string.h>
#include <vector>
using namespace zk;

namespace {
#include "final_exp.inc"
const uint64_t Z_ABS = 0xd201000000010000ULL;
struct Fq12 { Fq2 c[6]; };
#include "pairing_fast.inc"
}  // namespace

extern "C" {

// the header's constants against the ones pairing_dev.cuh derives (2^-1, 4) and against their definitions (R^2: to_mont(1) == one;
// (q - 1) / 2: the largest value that is not "largest").  0 = all hold; otherwise the number of the first that fails
int dc_consts_check() {
    const pd::Consts k = pd::consts();
    if (!(fqu_to_sat(dc::k_two_inv()) == fqu_to_sat(k.two_inv))) return 1;
    if (!(fqu_to_sat(dc::k_four()) == fqu_to_sat(k.twist_b.c0))) return 2;
    FqU one = FqU::zero();
    one.l[0] = 1;
    if (!(fqu_to_sat(dc::to_mont(one)) == Fq::one())) return 3;
    FqU half;
    for (int i = 0; i < 14; i++) half.l[i] = dc::DcP::half(i);
    FqU next = half;
    next.l[0] += 1;                     // the low limb of (q - 1) / 2 is not all ones
    if (dc::gt_half(half) || !dc::gt_half(next)) return 4;
    const FqU twice = dc::from_mont(fqu_add(dc::to_mont(half), dc::to_mont(half)));          // q - 1
    for (int i = 0; i < 14; i++)
        if (twice.l[i] != FqUP::mod(i) - (i == 0 ? 1u : 0u)) return 5;
    return 0;
}
// r = a^((q + 1) / 4) (6 u64 each, Montgomery); returns whether r^2 == a
int dc_fq_sqrt(const uint64_t *a, uint64_t *r) {
    Fq s; memcpy(&s, a, sizeof s);
    FqU root;
    const bool ok = dc::fq_sqrt(fqu_from_sat(s), root);
    const Fq o = fqu_to_sat(root);
    memcpy(r, &o, sizeof o);
    return ok ? 1 : 0;
}
// a root of a in Fq2 (12 u64 each: c0, c1); returns whether one exists (r zero otherwise)
int dc_fq2_sqrt(const uint64_t *a, uint64_t *r) {
    Fq2 s; memcpy(&s, a, sizeof s);
    pd::F2 root;
    const bool ok = dc::fq2_sqrt(fq2u_from_sat(s), root);
    const Fq2 o = fq2u_to_sat(root);
    memcpy(r, &o, sizeof o);
    return ok ? 1 : 0;
}
// zkg16_g1_decompress / zkg16_g2_decompress (group 1 / 2) by the device header: out n x 12 / 24 u64, inf n, status n ints; the
// endomorphism constants are the host's calibration, as the kernel receives them.  Returns the number of points with a status != 0
int dc_decompress(int group, const uint8_t *bytes, size_t n, uint64_t *out, uint8_t *inf, int validate, int *status) {
    const pf::Endo &en = pf::endo();
    const Fq beta = en.beta.to();
    const Fq2 cx = pf::to_sat(en.cx), cy = pf::to_sat(en.cy);
    int bad = 0;
    for (size_t i = 0; i < n; i++) {
        if (group == 1) {
            G1Affine p;
            status[i] = dc::g1_decompress(bytes + 48 * i, validate != 0, beta, en.fast_g1, p, inf[i]);
            memcpy(out + 12 * i, &p, sizeof p);
        } else {
            G2Affine p;
            status[i] = dc::g2_decompress(bytes + 96 * i, validate != 0, cx, cy, en.fast_g2, p, inf[i]);
            memcpy(out + 24 * i, &p, sizeof p);
        }
        if (status[i]) bad++;
    }
    return bad;
}

}  // extern "C"
