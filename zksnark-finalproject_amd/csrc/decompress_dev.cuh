// Point decompression over the device field FqU (ffu.cuh): the ark-serialize / zcash BLS12-381 encoding of G1 (48 bytes) and G2 (96
// bytes) back to affine Montgomery limbs, for one GPU lane per point (verify_batch.hip: decompress_kernel) — a restatement of
// zkg16_g1_decompress / zkg16_g2_decompress (verify.hip, host arithmetic) with the same statuses decided in the same order.
// __host__ __device__ throughout: tests/csrc/decompress_host_shim.hip runs this header on the CPU against the host decoders, byte for
// byte, with pairing_dev.cuh's bound assertions live.
//
// Values follow pairing_dev.cuh's discipline: what lives across operations is a product (< 2q) or tidy, every Fq product is a call
// (fqu_mul / fqu_sqr), and the bound of each subtrahend is written beside it.  The arithmetic is total: a non-residue gives
// `false` and nothing else, fqu_inv(0) is 0 (a power), no input traps.
//
// Cost per point, in Fq products: one power by (q + 1) / 4 is 376 squarings + 14 table products + 91 window products.
// G1: one power.  G2: two powers and one inversion (fqu_inv, a^(q-2) bit by bit: 380 squarings + 228 products) — the complex method
// with the second candidate's root taken from the first power instead of a third (fq2_sqrt below).
#pragma once
#include "pairing_dev.cuh"

namespace zk {
namespace dc {

using pd::F2;
using pd::mulq;

struct DcP {
    ZK_HD static constexpr uint32_t r2(int i) {         // 2^812 mod q: plain value -> U-form by one product
        constexpr uint32_t M[14] = {0x15bef7aeu, 0x1031cd0eu, 0x02dd93e8u, 0x09226323u, 0x0e6e2cd2u, 0x11684daau, 0x1170e5dbu,
                                    0x088e25b1u, 0x1b366399u, 0x1c536f47u, 0x0d1f9cbcu, 0x0278b67fu, 0x1ea66a2bu, 0x0000000cu};
        return M[i];
    }
    ZK_HD static constexpr uint32_t two_inv(int i) {    // 2^405 mod q: the U-form of 2^-1
        constexpr uint32_t M[14] = {0x01d4fdc2u, 0x15d00348u, 0x13894478u, 0x07acde62u, 0x09365b0au, 0x12c2df9bu, 0x0dc2d61eu,
                                    0x1e7c2b7du, 0x1c48f65eu, 0x0d3f7602u, 0x1aad4478u, 0x13a0d636u, 0x198be187u, 0x00000004u};
        return M[i];
    }
    ZK_HD static constexpr uint32_t four(int i) {       // 4 * 2^406 mod q: the U-form of 4 (b of G1; both components of b' of G2)
        constexpr uint32_t M[14] = {0x0ea898bau, 0x0e901a40u, 0x124a23e8u, 0x0d66f84fu, 0x0aee547cu, 0x03760629u, 0x181b776eu,
                                    0x12a47aa6u, 0x137ec460u, 0x05c6f549u, 0x0fdc4fe8u, 0x1707174du, 0x0c3ccef5u, 0x0000000cu};
        return M[i];
    }
    ZK_HD static constexpr uint32_t half(int i) {       // (q - 1) / 2, plain
        constexpr uint32_t M[14] = {0x1fffd555u, 0x07fbffffu, 0x0a7ffff7u, 0x0bfffeb1u, 0x07b120f5u, 0x14a83dacu, 0x057ece61u,
                                    0x184f3851u, 0x0bb23ba5u, 0x190d2eb3u, 0x096374f6u, 0x197fe69au, 0x10088f51u, 0x00000006u};
        return M[i];
    }
};
#define ZK_DC_CONST(name)                                        \
    ZK_HD FqU k_##name() {                                       \
        FqU r;                                                   \
        _Pragma("unroll") for (int i = 0; i < 14; i++) r.l[i] = DcP::name(i); \
        return r;                                                \
    }
ZK_DC_CONST(r2)
ZK_DC_CONST(two_inv)
ZK_DC_CONST(four)
#undef ZK_DC_CONST

ZK_HD FqU sqrq(const FqU &a) {
    ZK_PD_BOUND(a, 4096);
    return fqu_sqr(a);
}

// ------------------------------------------------------------------------------------------------ bytes and plain values
// 48 big-endian bytes (the top three bits of byte 0 masked off when `flags`: only the first byte of an encoding carries them) ->
// the plain value in base 2^29; false: the value is >= q (the limbs are then meaningless to the caller)
ZK_HD bool fq_parse(const uint8_t *b, bool flags, FqU &plain) {
    uint32_t w[12];
#pragma unroll
    for (int j = 0; j < 12; j++)
        w[j] = (uint32_t)b[47 - 4 * j] | (uint32_t)b[46 - 4 * j] << 8 | (uint32_t)b[45 - 4 * j] << 16 | (uint32_t)b[44 - 4 * j] << 24;
    if (flags) w[11] &= 0x1FFFFFFFu;
    bool less = false;              // scanned from the low word up: the highest differing word decides
#pragma unroll
    for (int j = 0; j < 12; j++) less = w[j] < FqP::mod(j) || (w[j] == FqP::mod(j) && less);
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const int bit = 29 * i;
        const int k = bit >> 5, off = bit & 31;
        uint64_t two = w[k];
        if (k + 1 < 12) two |= (uint64_t)w[k + 1] << 32;
        plain.l[i] = (uint32_t)(two >> off) & FqU::MASK;
    }
    return less;
}
// plain value < q -> U-form (< 2q; exact zero stays exact zero: a product by zero has no reduction digits)
ZK_HD FqU to_mont(const FqU &plain) { return mulq(plain, k_r2()); }
// U-form (< 4096 q) -> the canonical plain value: one product by the integer 1, then at most one subtraction of q
ZK_HD FqU from_mont(const FqU &a) {
    FqU one = FqU::zero();
    one.l[0] = 1;
    const FqU v = mulq(a, one);                                   // < 2q
    FqU d;
    int32_t carry = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const int32_t t = (int32_t)v.l[i] - (int32_t)FqUP::mod(i) + carry;
        d.l[i] = (uint32_t)t & FqU::MASK;
        carry = t >> 29;                                          // arithmetic shift = floor
    }
    const int32_t top = (int32_t)v.l[13] - (int32_t)FqUP::mod(13) + carry;
    d.l[13] = (uint32_t)top;
    return top < 0 ? v : d;
}
// "lexicographically largest" of (y, -y) on a canonical plain value: y > q - y  <=>  y > (q - 1) / 2
ZK_HD bool gt_half(const FqU &c) {
    bool gt = false;
#pragma unroll
    for (int i = 0; i < 14; i++) gt = c.l[i] > DcP::half(i) || (c.l[i] == DcP::half(i) && gt);
    return gt;
}

// ------------------------------------------------------------------------------------------------ square roots
// a^((q + 1) / 4), fixed windows of four bits: the exponent is a constant, so every lane of a wave takes the same path.
// a < 4096 q; result < 2q (zero for zero)
ZK_HD FqU pow_q1_4(const FqU &a) {
    uint32_t e[12];
    {
        uint32_t t[12], carry = 1;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const uint64_t v = (uint64_t)FqP::mod(i) + carry;
            t[i] = (uint32_t)v;
            carry = (uint32_t)(v >> 32);
        }
#pragma unroll
        for (int i = 0; i < 12; i++) e[i] = (t[i] >> 2) | (i < 11 ? t[i + 1] << 30 : 0u);
    }
    FqU tbl[16];
    tbl[0] = FqU::one();
    tbl[1] = a;
    for (int i = 2; i < 16; i++) tbl[i] = mulq(tbl[i - 1], a);
    // 379 bits = the window at bit 376 (non-zero: bit 378 is set) and 94 windows below it
    FqU acc = tbl[(e[11] >> 24) & 15u];
    for (int w = 93; w >= 0; w--) {
        acc = sqrq(sqrq(sqrq(sqrq(acc))));
        const uint32_t nib = (e[w >> 3] >> (4 * (w & 7))) & 15u;
        if (nib) acc = mulq(acc, tbl[nib]);
    }
    return acc;
}
// r = a^((q + 1) / 4) and whether r^2 == a (q = 3 mod 4).  a <= 7q
ZK_HD bool fq_sqrt(const FqU &a, FqU &r) {
    r = pow_q1_4(a);
    return fqu_is_zero_mod(pd::sub<8>(sqrq(r), a));              // 2 + 8
}
// Square root in Fq[u] / (u^2 + 1), the complex method of the host decoder in one straight line.  With n = sqrt(a0^2 + a1^2),
// exactly one of cand = (a0 + n) / 2 and cand' = (a0 - n) / 2 is a residue when a1 != 0, and cand cand' = -a1^2 / 4.  One power
// c = cand^((q + 1) / 4) decides: c^2 == cand gives the root (c, a1 / 2c); otherwise c^2 == -cand, so a1 / 2c is the root of
// cand' and the root is (a1 / 2c, c).  a1 == 0: cand = a0, and the same power gives (c, 0) for a residue and (0, c) for a
// non-residue (c^2 == -a0).  c == 0 only when a == 0 (cand = 0 means n = -a0, a1 = 0); fqu_inv(0) = 0 then and is not used.
// The result is checked by squaring, so `false` is exact: a has no root (its norm is a non-residue).  Either root may come out.
// a tidy (< 2q per component); r < 2q per component
ZK_HD bool fq2_sqrt(const F2 &a, F2 &r) {
    r = F2::zero();
    const bool real = fqu_is_zero_mod(a.c1);
    FqU n;
    if (!fq_sqrt(fqu_add(sqrq(a.c0), sqrq(a.c1)), n)) return false;                            // a0^2 for a real a: a residue
    const FqU cand = real ? a.c0 : mulq(fqu_add(a.c0, n), k_two_inv());
    const FqU c = pow_q1_4(cand);
    const bool first = fqu_is_zero_mod(pd::sub<8>(sqrq(c), cand));                              // 2 + 8
    const FqU t = real ? FqU::zero() : mulq(a.c1, fqu_inv(fqu_dbl(c)));
    const F2 root = first ? F2{c, t} : F2{t, c};
    if (!f_is_zero_mod(pd::sub<8>(pd::sqr<8>(root), a))) return false;                         // 4 + 8
    r = root;
    return true;
}

// ------------------------------------------------------------------------------------------------ whole points
// Statuses of zkg16_g1_decompress / zkg16_g2_decompress, decided in their order: 0 ok, 1 not compressed, 2 non-canonical infinity,
// 3 x not reduced, 4 not on the curve, 5 not in the subgroup (only with validate).  out: saturated Montgomery limbs; zero for
// statuses 1 to 4 and for the point at infinity (*inf = 1, status 0).  A point of status 5 keeps its limbs, as the host decoders
// leave them.  beta / cx, cy, fast: the endomorphism constants of the membership test (pairing_dev.cuh), read only with validate.
ZK_HD bool inf_is_clean(const uint8_t *b, int nb) {
    uint32_t rest = 0;
    for (int i = 1; i < nb; i++) rest |= b[i];
    return b[0] == 0xC0 && rest == 0;
}
ZK_HD int g1_decompress(const uint8_t *b, bool validate, const Fq &beta, bool fast, G1Affine &out, uint8_t &inf) {
    out = G1Affine::inf();
    inf = 0;
    if (!(b[0] & 0x80)) return 1;
    if (b[0] & 0x40) {
        if (!inf_is_clean(b, 48)) return 2;
        inf = 1;
        return 0;
    }
    FqU xp;
    if (!fq_parse(b, true, xp)) return 3;
    const FqU x = to_mont(xp);
    FqU y;
    if (!fq_sqrt(fqu_add(mulq(sqrq(x), x), k_four()), y)) return 4;                             // < 4q
    if (gt_half(from_mont(y)) != ((b[0] & 0x20) != 0)) y = pd::sub<8>(FqU::zero(), y);          // 8q - y
    out.x = fqu_to_sat(x);
    out.y = fqu_to_sat(y);
    if (validate && !pd::g1_subgroup(x, pd::tidy(y), fqu_from_sat(beta), fast)) return 5;
    return 0;
}
ZK_HD int g2_decompress(const uint8_t *b, bool validate, const Fq2 &cx, const Fq2 &cy, bool fast, G2Affine &out, uint8_t &inf) {
    out = G2Affine::inf();
    inf = 0;
    if (!(b[0] & 0x80)) return 1;
    if (b[0] & 0x40) {
        if (!inf_is_clean(b, 96)) return 2;
        inf = 1;
        return 0;
    }
    FqU x1p, x0p;
    const bool r1 = fq_parse(b, true, x1p), r0 = fq_parse(b + 48, false, x0p);
    if (!r1 || !r0) return 3;
    const F2 x{to_mont(x0p), to_mont(x1p)};
    // x^3 + 4 (1 + u)
    const F2 rhs = pd::tidy(pd::add(pd::mul(pd::sqr<8>(x), x), F2{k_four(), k_four()}));        // 10 + 2
    F2 y;
    if (!fq2_sqrt(rhs, y)) return 4;
    // (y1, y0) > (-y1, -y0) on canonical values: y1 decides unless it is zero
    const FqU y1p = from_mont(y.c1);
    const bool largest = y1p.is_zero() ? gt_half(from_mont(y.c0)) : gt_half(y1p);
    if (largest != ((b[0] & 0x20) != 0)) y = pd::tidy(pd::neg<8>(y));
    out.x = fq2u_to_sat(x);
    out.y = fq2u_to_sat(y);
    if (validate && !pd::g2_subgroup(x, y, fq2u_from_sat(cx), fq2u_from_sat(cy), fast)) return 5;
    return 0;
}

}  // namespace dc
}  // namespace zk
