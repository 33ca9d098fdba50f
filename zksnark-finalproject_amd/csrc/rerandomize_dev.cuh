// Re-randomising a Groth16 proof (ark-groth16 0.4 rerandomize_proof) on one GPU lane per (proof, group), and the compressed
// encoding of a point on one lane (verify_batch.hip: rerandomize_g1_kernel, rerandomize_g2_kernel, compress_kernel).  For non-zero
// r1, r2 and the key's delta in G2
//
//     A' = r1^-1 A        B' = r1 B + (r1 r2) delta        C' = C + r2 A
//
// __host__ __device__ throughout: zkg16_rerandomize_batch_host runs this header on host threads, so every byte the kernels write
// is the host form's by construction, and tests/csrc/rerandomize_host_shim.hip runs it against big-integer expectations with the
// bound assertions of pairing_dev.cuh live.
//
// Value bounds (ffu.cuh, ec.cuh): the curve formulas are ec.cuh's xyzz_dbl / xyzz_add / xyzz_madd, chained as pd::mul_z chains them
// for the membership tests, and the bounds are theirs: a coordinate they store is one level-32 subtraction away from a product,
// X, Y < 42q in G1 (a product is < 2q) and < 42q per component in G2 (a Karatsuba product is < 10q), ZZ, ZZZ products; every
// subtrahend inside them is a product, a sum of three products (< 30q per G2 component, level 32) or a stored coordinate (level 64).
// What this header adds multiplies only: table entries and accumulators enter xyzz_add as they were stored (< 42q << 2^12 q), the
// denominators ZZ ZZZ are products, fqu_inv takes anything below 2^12 q and returns a product (0 for 0), and pd::inv(F2) takes
// components <= 63q.  Outputs leave through fqu_to_sat, which is canonical for any value below 2^12 q.
// Nothing here branches on data in a way that could fail to end: the ladders walk all 255 bits of a scalar below r, the
// inversion's exponents are constants, and no input traps (pairing_each_dev.cuh's rule).
#pragma once
#include "pairing_each_dev.cuh"

namespace zk {
namespace rr {

using pd::F2;
using pd::mulq;

constexpr int SCALAR_BITS = 255;      // r < 2^255

// ------------------------------------------------------------------------------------------------ scalars
// a^(r - 2) on saturated Montgomery limbs; a != 0 (the entry points refuse a zero multiplier); 0 gives 0
ZK_HD Fr fr_inv(const Fr &a) {
    uint32_t e[8];
    uint32_t borrow = 2;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)FrP::mod(i) - borrow;
        e[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    Fr acc = a;                             // bit 254 of r - 2 is set
#pragma unroll 1
    for (int i = SCALAR_BITS - 2; i >= 0; i--) {
        acc = fp_sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = fp_mul(acc, a);
    }
    return acc;
}
// Montgomery -> the canonical 8 x u32 a ladder walks
ZK_HD void fr_canonical(const Fr &m, uint32_t k[8]) {
    const Fr c = fp_from_mont(m);
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = c.l[i];
}
ZK_HD uint32_t bit_of(const uint32_t k[8], int i) { return (k[i >> 5] >> (i & 31)) & 1u; }
// the G1 lane's pair (r1^-1, r2) and the G2 lane's pair (r1, r1 r2), canonical
ZK_HD void g1_scalars(const Fr &r1, const Fr &r2, uint32_t ka[8], uint32_t kc[8]) {
    fr_canonical(fr_inv(r1), ka);
    fr_canonical(r2, kc);
}
ZK_HD void g2_scalars(const Fr &r1, const Fr &r2, uint32_t kb[8], uint32_t kd[8]) {
    fr_canonical(r1, kb);
    fr_canonical(fp_mul(r1, r2), kd);
}

// ------------------------------------------------------------------------------------------------ the G1 lane
// A' = ka A and C' = C + kc A.  One doubling chain for both products: the base walks A, 2A, 4A, .. and each accumulator takes the
// base where its scalar has a bit (255 doublings and about 255 complete additions, against 510 doublings and 255 mixed additions
// for two ladders: DESIGN 2.7.6 has the instruction and scratch figures of both).  xyzz_add is complete: an accumulator that equals
// the base (ka = 2^j: the first addition of the next bit is a doubling), its opposite and either at infinity come out right.
// Then C + kc A by the complete mixed addition, and both results to affine with one fqu_inv over the product of the two
// denominators (Montgomery's trick; a result at infinity contributes the denominator one).
// a, c: saturated Montgomery limbs; a_inf / c_inf: load_pt's rule already applied (flag set or all limbs zero).
// Outputs: canonical saturated limbs, zero limbs with the flag set for the point at infinity
ZK_HD void g1_lane(const G1Affine &a, bool a_inf, const G1Affine &c, bool c_inf, const uint32_t ka[8], const uint32_t kc[8], G1Affine &oa, uint8_t &oa_inf,
                   G1Affine &oc, uint8_t &oc_inf) {
    XYZZ<FqU> base = XYZZ<FqU>::inf(), ra = XYZZ<FqU>::inf(), rc = XYZZ<FqU>::inf();
    if (!a_inf) base = XYZZ<FqU>{fqu_from_sat(a.x), fqu_from_sat(a.y), FqU::one(), FqU::one()};
#pragma unroll 1
    for (int i = 0; i < SCALAR_BITS; i++) {
        if (bit_of(ka, i)) xyzz_add(ra, base);
        if (bit_of(kc, i)) xyzz_add(rc, base);
        base = xyzz_dbl(base);
    }
    if (!c_inf) xyzz_madd(rc, Affine<FqU>{fqu_from_sat(c.x), fqu_from_sat(c.y)}, false);
    const bool ia = ra.is_inf(), ic = rc.is_inf();
    const FqU da = ia ? FqU::one() : mulq(ra.zz, ra.zzz), dc = ic ? FqU::one() : mulq(rc.zz, rc.zzz);
    const FqU iv = fqu_inv(mulq(da, dc));
    const FqU iva = mulq(iv, dc), ivc = mulq(iv, da);
    oa = G1Affine::inf();
    oc = G1Affine::inf();
    if (!ia) oa = G1Affine{fqu_to_sat(mulq(ra.x, mulq(iva, ra.zzz))), fqu_to_sat(mulq(ra.y, mulq(iva, ra.zz)))};
    if (!ic) oc = G1Affine{fqu_to_sat(mulq(rc.x, mulq(ivc, rc.zzz))), fqu_to_sat(mulq(rc.y, mulq(ivc, rc.zz)))};
    oa_inf = ia ? 1 : 0;
    oc_inf = ic ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ the G2 lane
// B' = kb B + kd delta as one interleaved ladder over the table {B, delta, B + delta}: one doubling per bit and one complete
// addition where either scalar has a bit.  The three entries are kept in one form (XYZZ) and added at ONE call site selected by the
// bit pair: the lanes of a wave hold different bit pairs, and three call sites (two mixed additions and a full one) would run one
// after the other for the wave.  B + delta is made here by the complete addition: B = delta is a doubling, B = -delta and B = O
// leave the entry at infinity or at delta, and adding an entry at infinity changes nothing.
// b, delta: saturated Montgomery limbs; b_inf: load_pt's rule already applied; delta is never at infinity (refused by the entries)
ZK_HD void g2_lane(const G2Affine &b, bool b_inf, const G2Affine &delta, const uint32_t kb[8], const uint32_t kd[8], G2Affine &ob, uint8_t &ob_inf) {
    XYZZ<F2> tbl[3];
    tbl[0] = XYZZ<F2>::inf();
    if (!b_inf) tbl[0] = XYZZ<F2>{fq2u_from_sat(b.x), fq2u_from_sat(b.y), F2::one(), F2::one()};
    tbl[1] = XYZZ<F2>{fq2u_from_sat(delta.x), fq2u_from_sat(delta.y), F2::one(), F2::one()};
    tbl[2] = tbl[0];
    xyzz_add(tbl[2], tbl[1]);
    XYZZ<F2> acc = XYZZ<F2>::inf();
#pragma unroll 1
    for (int i = SCALAR_BITS - 1; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        const uint32_t d = bit_of(kb, i) | (bit_of(kd, i) << 1);
        if (d) xyzz_add(acc, tbl[d - 1]);
    }
    ob = G2Affine::inf();
    ob_inf = 1;
    if (acc.is_inf()) return;
    // stored ZZ, ZZZ are products (< 10q per component); their product's components (< 10q) are inside pd::inv's 63q
    const F2 iv = pd::inv(pd::mul(acc.zz, acc.zzz));
    ob = G2Affine{fq2u_to_sat(pd::mul(acc.x, pd::mul(iv, acc.zzz))), fq2u_to_sat(pd::mul(acc.y, pd::mul(iv, acc.zz)))};
    ob_inf = 0;
}

// ------------------------------------------------------------------------------------------------ one proof
// load_pt's rule (pairing_each_dev.cuh: miller_one; api_verify.hip: vb_flags): the flag decides, and so do all-zero limbs
ZK_HD bool limbs_zero(const uint64_t *p, int n) {
    uint64_t any = 0;
    for (int i = 0; i < n; i++) any |= p[i];
    return any == 0;
}
ZK_HD Fr fr_load(const uint64_t *p) {
    Fr v;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        v.l[2 * i] = (uint32_t)p[i];
        v.l[2 * i + 1] = (uint32_t)(p[i] >> 32);
    }
    return v;
}
// proof / out: 48 u64 (A 12 | B 24 | C 12), inf / out_inf: 3 flags (nullable inf: none set); r1, r2: 4 u64 each, Montgomery
ZK_HD void proof_g1(const uint64_t *proof, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2, uint64_t *out, uint8_t *out_inf) {
    const G1Affine a = *reinterpret_cast<const G1Affine *>(proof), c = *reinterpret_cast<const G1Affine *>(proof + 36);
    const bool a_inf = (inf && inf[0]) || limbs_zero(proof, 12), c_inf = (inf && inf[2]) || limbs_zero(proof + 36, 12);
    uint32_t ka[8], kc[8];
    g1_scalars(fr_load(r1), fr_load(r2), ka, kc);
    G1Affine oa, oc;
    uint8_t fa, fc;
    g1_lane(a, a_inf, c, c_inf, ka, kc, oa, fa, oc, fc);
    *reinterpret_cast<G1Affine *>(out) = oa;
    *reinterpret_cast<G1Affine *>(out + 36) = oc;
    out_inf[0] = fa;
    out_inf[2] = fc;
}
ZK_HD void proof_g2(const uint64_t *proof, const uint8_t *inf, const G2Affine &delta, const uint64_t *r1, const uint64_t *r2, uint64_t *out, uint8_t *out_inf) {
    const G2Affine b = *reinterpret_cast<const G2Affine *>(proof + 12);
    const bool b_inf = (inf && inf[1]) || limbs_zero(proof + 12, 24);
    uint32_t kb[8], kd[8];
    g2_scalars(fr_load(r1), fr_load(r2), kb, kd);
    G2Affine ob;
    uint8_t fb;
    g2_lane(b, b_inf, delta, kb, kd, ob, fb);
    *reinterpret_cast<G2Affine *>(out + 12) = ob;
    out_inf[1] = fb;
}

// ------------------------------------------------------------------------------------------------ the compress lane
// wire.g1_compress / g2_compress and zkg16_points_compress: Montgomery limbs -> canonical, big-endian bytes, 0x80 always, 0x40
// for the point at infinity (the flag alone decides, as on the host; the rest zero), 0x20 when y is the larger of y and -y.
// Limbs are taken as they come (any value below q; what limbs not below q give is unspecified, as on the host)
ZK_HD void fq_be(const Fq &canon, uint8_t *b) {
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const uint32_t w = canon.l[j];
        b[47 - 4 * j] = (uint8_t)w;
        b[46 - 4 * j] = (uint8_t)(w >> 8);
        b[45 - 4 * j] = (uint8_t)(w >> 16);
        b[44 - 4 * j] = (uint8_t)(w >> 24);
    }
}
// y > q - y on a canonical value  <=>  y > (q - 1) / 2 = q >> 1; scanned from the low word up, the highest differing word decides
ZK_HD bool gt_half(const Fq &c) {
    bool gt = false;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const uint32_t h = (FqP::mod(j) >> 1) | (j < 11 ? FqP::mod(j + 1) << 31 : 0u);
        gt = c.l[j] > h || (c.l[j] == h && gt);
    }
    return gt;
}
ZK_HD void g1_compress(const uint64_t *p, bool inf, uint8_t *b) {
    if (inf) {
        for (int i = 0; i < 48; i++) b[i] = 0;
        b[0] = 0xC0;
        return;
    }
    const G1Affine a = *reinterpret_cast<const G1Affine *>(p);
    fq_be(fp_from_mont(a.x), b);
    b[0] |= 0x80 | (gt_half(fp_from_mont(a.y)) ? 0x20 : 0);
}
// x.c1 || x.c0; (y.c1, y.c0) compared: c1 decides unless it is zero
ZK_HD void g2_compress(const uint64_t *p, bool inf, uint8_t *b) {
    if (inf) {
        for (int i = 0; i < 96; i++) b[i] = 0;
        b[0] = 0xC0;
        return;
    }
    const G2Affine a = *reinterpret_cast<const G2Affine *>(p);
    fq_be(fp_from_mont(a.x.c1), b);
    fq_be(fp_from_mont(a.x.c0), b + 48);
    const Fq y1 = fp_from_mont(a.y.c1);
    const bool largest = y1.is_zero() ? gt_half(fp_from_mont(a.y.c0)) : gt_half(y1);
    b[0] |= 0x80 | (largest ? 0x20 : 0);
}

}  // namespace rr
}  // namespace zk
