// TEST-ONLY: the lane functions of csrc/pk_bytes_dev.cuh (what pk_bytes.hip's kernels run, one GPU lane per point of a proving key)
// compiled for the host, so that its decoding, its stored U-form words, its encoding and its inversion-free Fq2 square root can be
// compared with the library's host code on a machine without a GPU.  Built by tests/pk_bytes_cases.py with `hipcc
// --offload-host-only`; ZK_PD_CHECK turns on the value-bound assertions of pairing_dev.cuh.  Points cross this interface as wire
// bytes, as saturated Montgomery limbs (u64) or as the raw words of a U-form entry (28 / 56 u32, as they lie in a resident key).
#define ZK_PD_CHECK 1
#define ZK_PKB_LANES_ONLY 1
#include "ff.cuh"
#include "ec.cuh"
#include "pk_bytes_dev.cuh"
#include <string.h>
using namespace zk;

extern "C" {

// n encodings of one group (1 / 2) -> status[i], limbs (12 / 24 u64, the host decoders' output), inf[i], words (28 / 56 u32: the stored entry)
void pkb_decode(int group, const uint8_t *bytes, size_t n, uint64_t *limbs, uint8_t *inf, int *status, uint32_t *words) {
    for (size_t i = 0; i < n; i++) {
        if (group == 1) {
            Affine<FqU> u;
            G1Affine s;
            status[i] = pkb::g1_decode(bytes + 48 * i, u, &s);
            memcpy(limbs + 12 * i, &s, sizeof s);
            memcpy(words + 28 * i, &u, sizeof u);
            inf[i] = status[i] == 0 && u.is_inf();
        } else {
            Affine<Fq2U> u;
            G2Affine s;
            status[i] = pkb::g2_decode(bytes + 96 * i, u, &s);
            memcpy(limbs + 24 * i, &s, sizeof s);
            memcpy(words + 56 * i, &u, sizeof u);
            inf[i] = status[i] == 0 && u.is_inf();
        }
    }
}
// what zkg16_pk_load stores for these limbs: convert_g1_bases / convert_g2_bases' conversion (to_u per coordinate), a flagged point as (0, 0)
void pkb_convert(int group, const uint64_t *limbs, const uint8_t *inf, size_t n, uint32_t *words) {
    for (size_t i = 0; i < n; i++) {
        if (group == 1) {
            G1Affine p;
            memcpy(&p, limbs + 12 * i, sizeof p);
            if (inf[i]) p = G1Affine::inf();
            const Affine<FqU> u{to_u(p.x), to_u(p.y)};
            memcpy(words + 28 * i, &u, sizeof u);
        } else {
            G2Affine p;
            memcpy(&p, limbs + 24 * i, sizeof p);
            if (inf[i]) p = G2Affine::inf();
            const Affine<Fq2U> u{to_u(p.x), to_u(p.y)};
            memcpy(words + 56 * i, &u, sizeof u);
        }
    }
}
// stored entries -> wire bytes / -> limbs and flags
void pkb_encode(int group, const uint32_t *words, size_t n, uint8_t *bytes) {
    for (size_t i = 0; i < n; i++) {
        if (group == 1) {
            Affine<FqU> u;
            memcpy(&u, words + 28 * i, sizeof u);
            pkb::g1_encode(u, bytes + 48 * i);
        } else {
            Affine<Fq2U> u;
            memcpy(&u, words + 56 * i, sizeof u);
            pkb::g2_encode(u, bytes + 96 * i);
        }
    }
}
void pkb_read(int group, const uint32_t *words, size_t n, uint64_t *limbs, uint8_t *inf) {
    for (size_t i = 0; i < n; i++) {
        if (group == 1) {
            Affine<FqU> u;
            memcpy(&u, words + 28 * i, sizeof u);
            G1Affine s;
            pkb::g1_read(u, s, inf[i]);
            memcpy(limbs + 12 * i, &s, sizeof s);
        } else {
            Affine<Fq2U> u;
            memcpy(&u, words + 56 * i, sizeof u);
            G2Affine s;
            pkb::g2_read(u, s, inf[i]);
            memcpy(limbs + 24 * i, &s, sizeof s);
        }
    }
}
// a root of a in Fq2 (12 u64 each: c0, c1) by the inversion-free form (which = 0) or by dc::fq2_sqrt (which = 1); returns whether
// one exists (r zero otherwise)
int pkb_fq2_sqrt(int which, const uint64_t *a, uint64_t *r) {
    Fq2 s;
    memcpy(&s, a, sizeof s);
    pd::F2 root;
    const bool ok = which == 0 ? pkb::fq2_sqrt(fq2u_from_sat(s), root) : dc::fq2_sqrt(fq2u_from_sat(s), root);
    const Fq2 o = fq2u_to_sat(root);
    memcpy(r, &o, sizeof o);
    return ok ? 1 : 0;
}

}  // extern "C"
