// The pairing's arithmetic over the device field FqU (ffu.cuh): the tower Fq2 -> Fq6 -> Fq12, the Miller loop of one pair on
// an unprepared G2 point, and the subgroup tests — a restatement of pairing_fast.inc (the host verifier) for one GPU lane per
// pair / per point (verify_batch.hip).  __host__ __device__ throughout: tests/csrc/pairing_host_shim.hip runs this header on
// the CPU against pairing_fast.inc, limb for limb.
//
//   Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = 1 + u        (ark's tower and order)
//
// Value bounds.  FqU values are not kept below q (ffu.cuh): a product is < 2q, an addition adds bounds, a subtraction at level L
// adds L q and needs a subtrahend <= (L-1) q, and a product's inputs must stay below 2^12 q.  The rule here: every value that
// lives ACROSS operations of this header — the running Miller value f, the G2 point T, the line coefficients — is "tidy",
// < 2q per Fq component (pd::tidy: one multiply-subtract pass over the 14 limbs, ~1/10 of a product), so each operation's
// bounds can be read off its own body; they are written beside every subtraction (as multiples of q, per Fq component).  The
// host shim compiles with ZK_PD_CHECK and asserts every one of them while the tests run.
#pragma once
#include "ec.cuh"
#include "ffu.cuh"

#ifdef ZK_PD_CHECK
#include <stdio.h>
#include <stdlib.h>
// b <= (L-1) q is implied by its top limb: q = 13.002 * 2^377 and b < (l13 + 1) 2^377
#define ZK_PD_BOUND(v, mult) do { if ((v).l[13] + 1u > 13u * (unsigned)(mult)) { fprintf(stderr, "pairing_dev.cuh:%d: bound %d q exceeded (top limb %u)\n", __LINE__, (int)(mult), (v).l[13]); abort(); } } while (0)
#else
#define ZK_PD_BOUND(v, mult) do { } while (0)
#endif

namespace zk {
namespace pd {

constexpr uint64_t Z_ABS = 0xd201000000010000ULL;      // |z| of BLS12-381; z < 0

// a - k q with k = floor(a / q) or one less: < 2q for every normalised a < 2^12 q.  20160 / 2^18 is just below 2^377 / q, so k
// never exceeds a / q (the result stays non-negative) and falls short of it by less than 1.42.  Exact zero stays exact zero.
ZK_HD FqU tidy(const FqU &a) {
    ZK_PD_BOUND(a, 4096);
    const uint32_t k = (a.l[13] * 20160u) >> 18;
    FqU r;
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const int64_t v = (int64_t)a.l[i] - (int64_t)((uint64_t)k * FqUP::mod(i)) + carry;
        r.l[i] = (uint32_t)v & FqU::MASK;
        carry = v >> 29;
    }
    r.l[13] = (uint32_t)((int64_t)a.l[13] - (int64_t)((uint64_t)k * FqUP::mod(13)) + carry);
    return r;
}
template <int L>
ZK_HD FqU sub(const FqU &a, const FqU &b) {
    ZK_PD_BOUND(b, L - 1);
    return fqu_sub<L>(a, b);
}
ZK_HD FqU mulq(const FqU &a, const FqU &b) {
    ZK_PD_BOUND(a, 4096);
    ZK_PD_BOUND(b, 4096);
    return fqu_mul(a, b);
}

// ------------------------------------------------------------------------------------------------ Fq2
using F2 = Fq2U;
ZK_HD F2 add(const F2 &a, const F2 &b) { return F2{fqu_add(a.c0, b.c0), fqu_add(a.c1, b.c1)}; }
ZK_HD F2 dbl(const F2 &a) { return add(a, a); }
template <int L>
ZK_HD F2 sub(const F2 &a, const F2 &b) { return F2{sub<L>(a.c0, b.c0), sub<L>(a.c1, b.c1)}; }
template <int L>
ZK_HD F2 neg(const F2 &a) { return sub<L>(F2::zero(), a); }
ZK_HD F2 tidy(const F2 &a) { return F2{tidy(a.c0), tidy(a.c1)}; }
// Karatsuba; inputs: c0 + c1 < 4096 q.  Output < 10q
ZK_HD F2 mul(const F2 &a, const F2 &b) {
    const FqU v0 = mulq(a.c0, b.c0), v1 = mulq(a.c1, b.c1);
    const FqU s = mulq(fqu_add(a.c0, a.c1), fqu_add(b.c0, b.c1));
    return F2{sub<8>(v0, v1), sub<8>(s, fqu_add(v0, v1))};          // 2 + 8, 2 + 8
}
// (c0 + c1)(c0 - c1) + 2 c0 c1 u; c1 <= (L-1) q.  Output < 4q
template <int L>
ZK_HD F2 sqr(const F2 &a) {
    const FqU p = mulq(a.c0, a.c1);
    return F2{mulq(fqu_add(a.c0, a.c1), sub<L>(a.c0, a.c1)), fqu_dbl(p)};
}
// a (1 + u); a <= (L-1) q.  Output <= (bound + L, 2 bound)
template <int L>
ZK_HD F2 mul_xi(const F2 &a) { return F2{sub<L>(a.c0, a.c1), fqu_add(a.c0, a.c1)}; }
ZK_HD F2 scale(const F2 &a, const FqU &k) { return F2{mulq(a.c0, k), mulq(a.c1, k)}; }      // < 2q

// ------------------------------------------------------------------------------------------------ Fq6
struct F6 { F2 a0, a1, a2; };
ZK_HD F6 add(const F6 &x, const F6 &y) { return F6{add(x.a0, y.a0), add(x.a1, y.a1), add(x.a2, y.a2)}; }
template <int L>
ZK_HD F6 sub(const F6 &x, const F6 &y) { return F6{sub<L>(x.a0, y.a0), sub<L>(x.a1, y.a1), sub<L>(x.a2, y.a2)}; }
// v (a0, a1, a2) = (xi a2, a0, a1); a2 <= (L-1) q
template <int L>
ZK_HD F6 mul_v(const F6 &x) { return F6{mul_xi<L>(x.a2), x.a0, x.a1}; }
// Karatsuba, six Fq2 products; inputs < 500 q.  Output: a0 < 116q, a1 < 84q, a2 < 52q
ZK_HD F6 mul(const F6 &x, const F6 &y) {
    const F2 t0 = mul(x.a0, y.a0), t1 = mul(x.a1, y.a1), t2 = mul(x.a2, y.a2);                     // 10
    const F2 m12 = sub<32>(mul(add(x.a1, x.a2), add(y.a1, y.a2)), add(t1, t2));                  // 10 + 32 = 42 (subtrahend 20)
    const F2 m01 = sub<32>(mul(add(x.a0, x.a1), add(y.a0, y.a1)), add(t0, t1));
    const F2 m02 = sub<32>(mul(add(x.a0, x.a2), add(y.a0, y.a2)), add(t0, t2));
    return F6{add(t0, mul_xi<64>(m12)),              // 10 + (42 + 64, 84)
              add(m01, mul_xi<32>(t2)),              // 42 + (10 + 32, 20)
              add(m02, t1)};                         // 42 + 10
}
// x (b0 + b1 v), five Fq2 products.  Output: a0 < 52q, a1 < 42q, a2 < 20q
ZK_HD F6 mul_by_01(const F6 &x, const F2 &b0, const F2 &b1) {
    const F2 t0 = mul(x.a0, b0), t1 = mul(x.a1, b1);
    const F2 m01 = sub<32>(mul(add(x.a0, x.a1), add(b0, b1)), add(t0, t1));                      // 42
    return F6{add(t0, mul_xi<32>(mul(x.a2, b1))), m01, add(mul(x.a2, b0), t1)};                  // 10 + 42, 42, 20
}
// x (b1 v), three Fq2 products.  Output: a0 < 42q, a1, a2 < 10q
ZK_HD F6 mul_by_1(const F6 &x, const F2 &b1) { return F6{mul_xi<32>(mul(x.a2, b1)), mul(x.a0, b1), mul(x.a1, b1)}; }
ZK_HD F6 tidy(const F6 &x) { return F6{tidy(x.a0), tidy(x.a1), tidy(x.a2)}; }

// ------------------------------------------------------------------------------------------------ Fq12 (inputs and outputs tidy)
struct F12 { F6 c0, c1; };
ZK_HD F12 f12_one() { return F12{F6{F2::one(), F2::zero(), F2::zero()}, F6{F2::zero(), F2::zero(), F2::zero()}}; }
ZK_HD F12 mul(const F12 &a, const F12 &b) {
    const F6 t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);                                         // 116, 84, 52
    const F6 m = sub<128>(sub<128>(mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1);             // 116 + 256
    return F12{tidy(add(t0, mul_v<64>(t1))), tidy(m)};                                           // 116 + 116
}
// complex squaring: (c0 + c1 w)^2 = (c0 + c1)(c0 + v c1) - t - v t + 2 t w, t = c0 c1
ZK_HD F12 sqr(const F12 &a) {
    const F6 t = mul(a.c0, a.c1);
    const F6 s = mul(add(a.c0, a.c1), add(a.c0, mul_v<8>(a.c1)));                                // inputs 4, 2 + 10
    return F12{tidy(sub<128>(sub<128>(s, t), mul_v<64>(t))), tidy(add(t, t))};                   // 116 + 256; 232
}
// a (l0 + l1 v + l4 v w): 13 Fq2 products; l0, l1, l4 tidy
ZK_HD F12 mul_by_014(const F12 &a, const F2 &l0, const F2 &l1, const F2 &l4) {
    const F6 aa = mul_by_01(a.c0, l0, l1);                                                       // 52, 42, 20
    const F6 bb = mul_by_1(a.c1, l4);                                                            // 42, 10, 10
    const F6 m = mul_by_01(add(a.c0, a.c1), l0, add(l1, l4));
    return F12{tidy(add(aa, mul_v<32>(bb))), tidy(sub<64>(sub<64>(m, aa), bb))};                 // 52 + 42; 52 + 128
}
ZK_HD F12 conj(const F12 &a) { return F12{a.c0, tidy(sub<8>(F6{F2::zero(), F2::zero(), F2::zero()}, a.c1))}; }

// ---- ABI: 72 u64 = 6 Fq2 in ark's tower order, saturated Montgomery limbs (the layout of alpha_beta in zkg16_pvk_prepare)
ZK_HD void f12_to_sat(const F12 &a, Fq2 out[6]) {
    out[0] = fq2u_to_sat(a.c0.a0); out[1] = fq2u_to_sat(a.c0.a1); out[2] = fq2u_to_sat(a.c0.a2);
    out[3] = fq2u_to_sat(a.c1.a0); out[4] = fq2u_to_sat(a.c1.a1); out[5] = fq2u_to_sat(a.c1.a2);
}
ZK_HD F12 f12_from_sat(const Fq2 in[6]) {
    // fqu_from_sat keeps exact zeros exact, which tidy values may be; everything else is a product (< 2q)
    return F12{F6{fq2u_from_sat(in[0]), fq2u_from_sat(in[1]), fq2u_from_sat(in[2])}, F6{fq2u_from_sat(in[3]), fq2u_from_sat(in[4]), fq2u_from_sat(in[5])}};
}

// ------------------------------------------------------------------------------------------------ line steps, ark's scaling
// G2 in homogeneous projective coordinates (ark-ec G2HomProjective), M twist; the constants: 2^-1 and b' = 4 (1 + u)
struct P2 { F2 x, y, z; };            // tidy
struct Ell { F2 c0, c1, c2; };        // c0 tidy; c1, c2 are multiplied by the G1 point's coordinates before use
struct Consts { FqU two_inv; F2 twist_b; };
ZK_HD Consts consts() {
    // the U-form of 2^-1 = (q + 1) / 2 and of 4: from the saturated constants through the conversion product
    Consts k;
    Fq four = Fq::zero();
    four.l[0] = 4;
    const FqU four_u = fqu_from_sat(fp_to_mont(four));
    k.twist_b = F2{four_u, four_u};
    // 2^-1 = 4 * 8^-1 would need an inverse; (q + 1) / 2 in canonical saturated limbs instead
    Fq h;
    uint32_t carry = 1;
    uint32_t t[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint64_t v = (uint64_t)FqP::mod(i) + carry;
        t[i] = (uint32_t)v;
        carry = (uint32_t)(v >> 32);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) h.l[i] = (t[i] >> 1) | (i < 11 ? t[i + 1] << 31 : 0u);
    k.two_inv = fqu_from_sat(fp_to_mont(h));
    return k;
}
// T <- 2T; returns (i, 3j, -h) of G2HomProjective::double_in_place
ZK_HD Ell ark_double(P2 &r, const Consts &k) {
    const F2 a = scale(mul(r.x, r.y), k.two_inv);                      // 2
    const F2 b = sqr<8>(r.y);                                          // 4
    const F2 c = sqr<8>(r.z);                                          // 4
    const F2 e = mul(k.twist_b, add(dbl(c), c));                       // 10
    const F2 f = add(dbl(e), e);                                       // 30
    const F2 g = scale(add(b, f), k.two_inv);                          // 2
    const F2 hh = sub<32>(sqr<8>(add(r.y, r.z)), add(b, c));           // 4 + 32 (subtrahend 8)
    const F2 i = sub<8>(e, b);                                         // 10 + 8
    const F2 j = sqr<8>(r.x);                                          // 4
    const F2 e2 = sqr<32>(e);                                          // 4
    r.x = tidy(mul(a, sub<32>(b, f)));                                 // inputs 2, 4 + 32
    r.y = tidy(sub<32>(sqr<8>(g), add(dbl(e2), e2)));                  // 4 + 32 (subtrahend 12)
    r.z = tidy(mul(b, hh));
    return Ell{tidy(i), add(dbl(j), j), neg<64>(hh)};                  // 2; 12; 64
}
// T <- T + Q; returns (j, -theta, lambda) of G2HomProjective::add_in_place.  qx, qy tidy
ZK_HD Ell ark_add(P2 &r, const F2 &qx, const F2 &qy) {
    const F2 theta = sub<32>(r.y, mul(qy, r.z));                       // 2 + 32 (subtrahend 10)
    const F2 lambda = sub<32>(r.x, mul(qx, r.z));                      // 34
    const F2 c = sqr<64>(theta), d = sqr<64>(lambda);                  // 4
    const F2 e = mul(lambda, d), f = mul(r.z, c), g = mul(r.x, d);     // 10
    const F2 hh = sub<32>(add(e, f), dbl(g));                          // 20 + 32 (subtrahend 20)
    const F2 ry = r.y;
    r.x = tidy(mul(lambda, hh));
    r.y = tidy(sub<32>(mul(theta, sub<64>(g, hh)), mul(e, ry)));       // inner 10 + 64 (subtrahend 52); 10 + 32
    r.z = tidy(mul(r.z, e));
    const F2 j = sub<32>(mul(theta, qx), mul(lambda, qy));             // 42
    return Ell{tidy(j), neg<64>(theta), lambda};                       // 2; 64; 34
}
// f <- f * line(P): Bls12::ell — c1 *= p.x, c2 *= p.y, mul_by_014
ZK_HD void ell(F12 &f, const Ell &c, const FqU &px, const FqU &py) { f = mul_by_014(f, c.c0, scale(c.c1, px), scale(c.c2, py)); }

// The Miller loop of one pair (P affine in G1, Q affine in G2, neither at infinity; U-form, tidy): 63 doublings and 5 additions,
// the value conjugated for the negative z — pf::miller_loop(pf::prepare(Q)) with the lines used as they are made.
ZK_HD F12 miller_loop(const FqU &px, const FqU &py, const F2 &qx, const F2 &qy) {
    const Consts k = consts();
    P2 t{qx, qy, F2::one()};
    F12 f = f12_one();
    for (int i = 62; i >= 0; i--) {
        if (i != 62) f = sqr(f);
        ell(f, ark_double(t, k), px, py);
        if ((Z_ABS >> i) & 1) ell(f, ark_add(t, qx, qy), px, py);
    }
    return conj(f);
}

// ------------------------------------------------------------------------------------------------ membership
// Curve equation and the endomorphism tests of pairing_fast.inc on ec.cuh's XYZZ formulas.  beta, cx, cy: the constants the host
// calibrated (pf::endo()), in U-form.
template <class F>
ZK_HD XYZZ<F> mul_z(const XYZZ<F> &p) {             // [|z|] p
    XYZZ<F> acc = p;                                // bit 63 is set
    for (int i = 62; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        if ((Z_ABS >> i) & 1) xyzz_add(acc, p);
    }
    return acc;
}
// a == b as group elements (coordinates of both: results of xyzz_* or affine inputs, <= 42 q)
// -p for stored coordinates (<= 63 q): ec.cuh's xyzz_neg is for values <= 7 q
ZK_HD XYZZ<FqU> neg_pt(const XYZZ<FqU> &p) { return XYZZ<FqU>{p.x, fqu_sub<64>(FqU::zero(), p.y), p.zz, p.zzz}; }
ZK_HD XYZZ<F2> neg_pt(const XYZZ<F2> &p) { return XYZZ<F2>{p.x, neg<64>(p.y), p.zz, p.zzz}; }
template <class F>
ZK_HD bool xyzz_eq(const XYZZ<F> &a, const XYZZ<F> &b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    return f_is_zero_mod(f_sub(f_mul(a.x, b.zz), f_mul(b.x, a.zz))) && f_is_zero_mod(f_sub(f_mul(a.y, b.zzz), f_mul(b.y, a.zzz)));
}
ZK_HD bool g1_on_curve(const FqU &x, const FqU &y) {
    Fq four = Fq::zero();
    four.l[0] = 4;
    const FqU rhs = fqu_add(fqu_mul(fqu_sqr(x), x), fqu_from_sat(fp_to_mont(four)));           // < 4q
    return fqu_is_zero_mod(fqu_sub<8>(fqu_sqr(y), rhs));
}
ZK_HD bool g2_on_curve(const F2 &x, const F2 &y) {
    const F2 rhs = add(mul(sqr<8>(x), x), consts().twist_b);                                   // < 12q
    return f_is_zero_mod(sub<32>(sqr<8>(y), rhs));
}
// r as 8 x u32 for the plain ladder (where the start-up calibration of the endomorphism constants fell back)
ZK_HD void r_limbs(uint32_t l[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) l[i] = FrP::mod(i);
}
// phi(P) = (beta x, y) == -[z^2] P
ZK_HD bool g1_subgroup(const FqU &x, const FqU &y, const FqU &beta, bool fast) {
    const XYZZ<FqU> p{x, y, FqU::one(), FqU::one()};
    if (!fast) {
        uint32_t r[8];
        r_limbs(r);
        return xyzz_mul(p, r).is_inf();
    }
    const XYZZ<FqU> z2p = mul_z(mul_z(p));
    const XYZZ<FqU> phi{fqu_mul(x, beta), y, FqU::one(), FqU::one()};
    return xyzz_eq(neg_pt(z2p), phi);
}
// psi(P) = (conj(x) cx, conj(y) cy) == -[|z|] P
ZK_HD bool g2_subgroup(const F2 &x, const F2 &y, const F2 &cx, const F2 &cy, bool fast) {
    const XYZZ<F2> p{x, y, F2::one(), F2::one()};
    if (!fast) {
        uint32_t r[8];
        r_limbs(r);
        return xyzz_mul(p, r).is_inf();
    }
    const XYZZ<F2> zp = neg_pt(mul_z(p));
    const XYZZ<F2> psi{mul(F2{x.c0, fqu_neg(x.c1)}, cx), mul(F2{y.c0, fqu_neg(y.c1)}, cy), F2::one(), F2::one()};
    return xyzz_eq(zp, psi);
}
// what zkg16_point_check says of an affine point given in saturated limbs (not at infinity)
ZK_HD bool g1_valid(const G1Affine &p, const FqU &beta, bool fast) {
    const FqU x = fqu_from_sat(p.x), y = fqu_from_sat(p.y);
    return g1_on_curve(x, y) && g1_subgroup(x, y, beta, fast);
}
ZK_HD bool g2_valid(const G2Affine &p, const F2 &cx, const F2 &cy, bool fast) {
    const F2 x = fq2u_from_sat(p.x), y = fq2u_from_sat(p.y);
    return g2_on_curve(x, y) && g2_subgroup(x, y, cx, cy, fast);
}

// [k] P for a 128-bit k (4 x u32, non-zero), back to affine: the rho_k A_k of the batch equation.  false: the point at infinity
ZK_HD bool g1_scale128(const FqU &x, const FqU &y, const uint32_t k[4], FqU &ox, FqU &oy) {
    const XYZZ<FqU> p{x, y, FqU::one(), FqU::one()};
    XYZZ<FqU> acc = XYZZ<FqU>::inf();
    for (int i = 127; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        if ((k[i / 32] >> (i % 32)) & 1) xyzz_add(acc, p);
    }
    if (acc.is_inf()) return false;
    const Affine<FqU> a = xyzz_to_affine(acc);      // products: < 2q
    ox = a.x;
    oy = a.y;
    return true;
}

}  // namespace pd
}  // namespace zk
