// One proof's own Groth16 verdict on one GPU lane (verify_batch.hip: each_x_kernel, each_miller_kernel, final_exp_kernel): what
// pairing_dev.cuh lacks for it — inversion up the tower, the cyclotomic squaring, the Frobenius maps, the final exponentiation by
// the Hayashida-Hayasaka-Teruya chain, the Miller loop on a key's prepared line coefficients beside the unprepared loop on (A, B),
// and the prepared public input X = gamma_abc[0] + sum_i z_i gamma_abc[i].  A restatement of pairing_fast.inc, operation for
// operation, so that every value equals the host's limb for limb once it is back in canonical limbs.  __host__ __device__
// throughout: tests/csrc/verify_each_host_shim.hip runs this header on the CPU against pairing_fast.inc with ZK_PD_CHECK on.
//
// Value bounds as in pairing_dev.cuh: what lives across operations is tidy (< 2q per Fq component); inside an operation the bound
// of every subtrahend is written beside the subtraction, as multiples of q.  Nothing here branches on data in a way that could
// fail to end: every loop count is a constant or the bit length of a 256-bit scalar, and fqu_inv(0) is 0.
#pragma once
#include "pairing_dev.cuh"

// The tower operations below are calls on the device, as the Fq products under them are: one lane runs ~80 Fq12 products and
// ~320 cyclotomic squarings per final exponentiation, and inlining them all buys nothing but code (the call passes 12 Fq through
// scratch, against the 54 Fq products of an Fq12 product)
#if defined(__HIP_DEVICE_COMPILE__)
#define ZK_PD_CALL __device__ __noinline__
#else
#define ZK_PD_CALL inline
#endif

namespace zk {
namespace pd {

ZK_PD_CALL F12 mul_call(const F12 &a, const F12 &b) { return mul(a, b); }

ZK_HD FqU sqrq(const FqU &a) {
    ZK_PD_BOUND(a, 4096);
    return fqu_sqr(a);
}

// ------------------------------------------------------------------------------------------------ inversion: one fqu_inv each
// conj(a) / (c0^2 + c1^2); components of a <= 63q.  Output < 2q; inv(0) = 0
ZK_HD F2 inv(const F2 &a) {
    const FqU n = fqu_inv(fqu_add(sqrq(a.c0), sqrq(a.c1)));                                      // the norm: < 4q
    return F2{mulq(a.c0, n), mulq(sub<64>(FqU::zero(), a.c1), n)};
}
// x tidy.  Output tidy
ZK_HD F6 inv(const F6 &x) {
    const F2 t0 = sub<64>(sqr<8>(x.a0), mul_xi<32>(mul(x.a1, x.a2)));                            // 4 + 64 (subtrahend 10 + 32, 20)
    const F2 t1 = sub<32>(mul_xi<8>(sqr<8>(x.a2)), mul(x.a0, x.a1));                             // (4 + 8, 8) + 32 (subtrahend 10)
    const F2 t2 = sub<32>(sqr<8>(x.a1), mul(x.a0, x.a2));                                        // 4 + 32
    const F2 d = add(mul(x.a0, t0), mul_xi<32>(add(mul(x.a2, t1), mul(x.a1, t2))));              // 10 + (20 + 32, 40)
    const F2 di = inv(d);                                                                        // d <= 62q
    return F6{tidy(mul(t0, di)), tidy(mul(t1, di)), tidy(mul(t2, di))};
}
// a tidy.  Output tidy: (c0 - c1 w) / (c0^2 - v c1^2)
ZK_PD_CALL F12 inv(const F12 &a) {
    const F6 s0 = mul(a.c0, a.c0), s1 = mul(a.c1, a.c1);                                         // 116, 84, 52
    const F6 d = inv(tidy(sub<128>(s0, mul_v<64>(s1))));                                         // 116 + 128 (subtrahend (116, 104), 116, 84)
    return F12{tidy(mul(a.c0, d)), tidy(sub<128>(F6{F2::zero(), F2::zero(), F2::zero()}, mul(a.c1, d)))};
}

// ------------------------------------------------------------------------------------------------ the cyclotomic subgroup
// (a + b y)^2 = (a^2 + xi b^2) + 2ab y over Fq4 = Fq2[y]/(y^2 - xi); a, b tidy.  Output: r0 < 74q, r1 < 20q
ZK_HD void fq4_sqr(const F2 &a, const F2 &b, F2 &r0, F2 &r1) {
    const F2 t = mul(a, b);                                                                      // 10
    const F2 m = mul(add(a, b), add(a, mul_xi<8>(b)));                                           // inputs 4; 2 + (2 + 8, 4)
    r0 = sub<64>(m, add(t, mul_xi<32>(t)));                                                      // 10 + 64 (subtrahend 10 + (42, 20))
    r1 = dbl(t);
}
// Granger-Scott squaring (pf::cyclotomic_sqr); f tidy.  Output tidy
ZK_PD_CALL F12 cyclotomic_sqr(const F12 &f) {
    const F2 &z0 = f.c0.a0, &z4 = f.c0.a1, &z3 = f.c0.a2, &z2 = f.c1.a0, &z1 = f.c1.a1, &z5 = f.c1.a2;
    F2 t0, t1, t2, t3, t4, t5;
    fq4_sqr(z0, z1, t0, t1);
    fq4_sqr(z2, z3, t2, t3);
    fq4_sqr(z4, z5, t4, t5);
    F12 r;
    // 3t - 2z: d = t - z < 74 + 8, 2d + t < 238.  3t + 2z: < 3 bound(t) + 4
    r.c0.a0 = tidy(add(dbl(sub<8>(t0, z0)), t0));
    r.c0.a1 = tidy(add(dbl(sub<8>(t2, z4)), t2));
    r.c0.a2 = tidy(add(dbl(sub<8>(t4, z3)), t4));
    const F2 x5 = mul_xi<32>(t5);                                                                // (20 + 32, 40)
    r.c1.a0 = tidy(add(dbl(add(x5, z2)), x5));                                                   // 160
    r.c1.a1 = tidy(add(dbl(add(t1, z1)), t1));                                                   // 64
    r.c1.a2 = tidy(add(dbl(add(t3, z5)), t3));
    return r;
}

// The Frobenius constants gamma_i = xi^(i (q-1)/6), i = 1..5, as the host computed them (pf::frob_coeffs), U-form, tidy
struct Frob { F2 g[5]; };
// conj(a) g for a tidy: conj < (2, 10), the product < 10q
ZK_HD F2 frob_coeff(const F2 &a, const F2 &g) { return tidy(mul(F2{a.c0, sub<8>(FqU::zero(), a.c1)}, g)); }
// a^(q^times), times = 1 or 2; a tidy.  Output tidy.  Tower slot (c, k) holds the coefficient of w^(2k + c)
ZK_PD_CALL F12 frob(const F12 &a, int times, const Frob &fr) {
    F12 r = a;
    for (int t = 0; t < times; t++) {
        r.c0.a0 = tidy(F2{r.c0.a0.c0, sub<8>(FqU::zero(), r.c0.a0.c1)});
        r.c1.a0 = frob_coeff(r.c1.a0, fr.g[0]);
        r.c0.a1 = frob_coeff(r.c0.a1, fr.g[1]);
        r.c1.a1 = frob_coeff(r.c1.a1, fr.g[2]);
        r.c0.a2 = frob_coeff(r.c0.a2, fr.g[3]);
        r.c1.a2 = frob_coeff(r.c1.a2, fr.g[4]);
    }
    return r;
}
// a^z for a in the cyclotomic subgroup, z = -|z|
ZK_PD_CALL F12 pow_z(const F12 &a) {
    F12 acc = a;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        acc = cyclotomic_sqr(acc);
        if ((Z_ABS >> i) & 1) acc = mul_call(acc, a);
    }
    return conj(acc);
}
// f^(3 (q^12 - 1)/r) by pf::final_exp's chain, step for step; f tidy, any value (zero gives zero)
ZK_HD F12 final_exp(const F12 &f, const Frob &fr) {
    const F12 f1 = mul_call(conj(f), inv(f));                                         // f^(q^6 - 1)
    const F12 g = mul_call(frob(f1, 2, fr), f1);                                      // ^(q^2 + 1): now in the cyclotomic subgroup
    const F12 t0 = mul_call(pow_z(g), conj(g));                                       // g^(z - 1)
    const F12 t1 = mul_call(pow_z(t0), conj(t0));                                     // g^((z - 1)^2)
    const F12 t2 = mul_call(pow_z(t1), frob(t1, 1, fr));                              // ^(z + q)
    const F12 t3 = mul_call(mul_call(pow_z(pow_z(t2)), frob(t2, 2, fr)), conj(t2));   // ^(z^2 + q^2 - 1)
    return mul_call(t3, mul_call(cyclotomic_sqr(g), g));                              // * g^3
}
// a == b as field elements (both tidy): on canonical limbs
ZK_HD bool f12_eq_sat(const F12 &a, const Fq2 b[6]) {
    Fq2 s[6];
    f12_to_sat(a, s);
    bool same = true;
#pragma unroll
    for (int t = 0; t < 6; t++) {
#pragma unroll
        for (int i = 0; i < 12; i++) same = same && s[t].c0.l[i] == b[t].c0.l[i] && s[t].c1.l[i] == b[t].c1.l[i];
    }
    return same;
}

// ------------------------------------------------------------------------------------------------ Miller loops with prepared pairs
// A prepared pair: a G1 point (U-form, tidy) and the 68 line triples of its G2 point in loop order (U-form, tidy; null = the pair
// is left out, as a pair with a point at infinity is)
struct PreparedPair { FqU px, py; const Ell *ell; };
// Bls12::multi_miller_loop over an optional unprepared pair (P, Q) (have_pq; its lines are made as they are used, as
// pd::miller_loop does) and np prepared pairs: one squaring of f per bit for all of them, one mul_by_014 per pair and line —
// pf::miller_loop's formula.  np <= 2
ZK_HD F12 multi_miller_loop(bool have_pq, const FqU &px, const FqU &py, const F2 &qx, const F2 &qy, const PreparedPair *pairs, int np) {
    const Consts k = consts();
    P2 t{qx, qy, F2::one()};
    F12 f = f12_one();
    int line = 0;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        if (i != 62) f = sqr(f);
        if (have_pq) ell(f, ark_double(t, k), px, py);
        for (int j = 0; j < np; j++)
            if (pairs[j].ell) ell(f, pairs[j].ell[line], pairs[j].px, pairs[j].py);
        line++;
        if ((Z_ABS >> i) & 1) {
            if (have_pq) ell(f, ark_add(t, qx, qy), px, py);
            for (int j = 0; j < np; j++)
                if (pairs[j].ell) ell(f, pairs[j].ell[line], pairs[j].px, pairs[j].py);
            line++;
        }
    }
    return conj(f);
}

// ------------------------------------------------------------------------------------------------ the prepared public input
// gamma_abc[0] + sum_{i >= 1} z_i gamma_abc[i], to affine.  gamma_abc: num_instance affine points in U-form (tidy; exact zeros =
// the point at infinity); z: (num_instance - 1) x 4 u64, canonical (the host converts from Montgomery form before upload).  A
// zero scalar is skipped and each multiplication walks from its scalar's top set bit, as pf::pt_mul does: a bit-valued input
// costs one addition.  false: the point at infinity (that pair is left out)
ZK_HD bool prepared_input(const Affine<FqU> *gamma_abc, size_t num_instance, const uint64_t *z, FqU &ox, FqU &oy) {
    XYZZ<FqU> total = XYZZ<FqU>::from_affine(gamma_abc[0]);
    for (size_t i = 1; i < num_instance; i++) {
        const uint64_t *k = z + 4 * (i - 1);
        int top = 255;
        while (top >= 0 && !((k[top / 64] >> (top % 64)) & 1)) top--;
        if (top < 0) continue;
        const Affine<FqU> p = gamma_abc[i];
        XYZZ<FqU> acc = XYZZ<FqU>::from_affine(p);       // the top bit
#pragma unroll 1
        for (int b = top - 1; b >= 0; b--) {
            acc = xyzz_dbl(acc);
            if ((k[b / 64] >> (b % 64)) & 1) xyzz_madd(acc, p, false);
        }
        xyzz_add(total, acc);
    }
    if (total.is_inf()) return false;
    // stored coordinates are < 42q (ec.cuh); fqu_inv takes anything below 2^12 q and returns a product
    const FqU iv = fqu_inv(mulq(total.zz, total.zzz));
    ox = mulq(total.x, mulq(iv, total.zzz));
    oy = mulq(total.y, mulq(iv, total.zz));
    return true;
}

// ------------------------------------------------------------------------------------------------ one proof
// The key as a lane sees it: everything in U-form except e(alpha, beta), which is compared on canonical limbs
struct EachKey {
    const Ell *gamma_neg, *delta_neg;       // 68 triples each
    const Fq2 *alpha_beta;                  // 6 Fq2, ark's tower order, as zkg16_pvk_prepare wrote them
};
// ML(A, B) ML(X, -gamma) ML(C, -delta) for a proof whose points passed membership; a pair with a point at infinity contributes
// one (zkg16_verify_prepared's rule).  proof: 48 u64 (A 12 | B 24 | C 12), saturated Montgomery limbs; inf: the three flags;
// have_x / xx / xy: prepared_input's result
ZK_HD F12 miller_one(const uint64_t *proof, const uint8_t *inf, bool have_x, const FqU &xx, const FqU &xy, const EachKey &key) {
    const G1Affine a = *reinterpret_cast<const G1Affine *>(proof), c = *reinterpret_cast<const G1Affine *>(proof + 36);
    const G2Affine b = *reinterpret_cast<const G2Affine *>(proof + 12);
    // load_pt's rule: the flag decides, and so do all-zero limbs
    const bool a_inf = inf[0] || a.is_inf(), b_inf = inf[1] || b.is_inf(), c_inf = inf[2] || c.is_inf();
    const bool have_ab = !a_inf && !b_inf;
    FqU ax = FqU::zero(), ay = FqU::zero();
    F2 bx = F2::zero(), by = F2::zero();
    if (have_ab) {
        ax = fqu_from_sat(a.x); ay = fqu_from_sat(a.y);
        bx = fq2u_from_sat(b.x); by = fq2u_from_sat(b.y);
    }
    PreparedPair pr[2];
    pr[0] = PreparedPair{xx, xy, have_x ? key.gamma_neg : nullptr};
    pr[1] = PreparedPair{FqU::zero(), FqU::zero(), nullptr};
    if (!c_inf) pr[1] = PreparedPair{fqu_from_sat(c.x), fqu_from_sat(c.y), key.delta_neg};
    return multi_miller_loop(have_ab, ax, ay, bx, by, pr, 2);
}
// what zkg16_verify_prepared says of a proof whose points passed membership: FE(miller_one) == e(alpha, beta).  The unscaled A and
// no multiplier: the verdict is exact
ZK_HD bool verify_one(const uint64_t *proof, const uint8_t *inf, const Affine<FqU> *gamma_abc, size_t num_instance, const uint64_t *z, const EachKey &key,
                      const Frob &fr) {
    FqU xx = FqU::zero(), xy = FqU::zero();
    const bool have_x = prepared_input(gamma_abc, num_instance, z, xx, xy);
    return f12_eq_sat(final_exp(miller_one(proof, inf, have_x, xx, xy, key), fr), key.alpha_beta);
}

}  // namespace pd
}  // namespace zk
