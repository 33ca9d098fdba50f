// G2 arithmetic with every Fq2 value SPLIT OVER A PAIR OF LANES: lane 2j holds c0, lane 2j + 1 holds c1 (h = lane & 1).
//
// Why: one lane holding whole Fq2 coordinates needs 478 registers for the bucket accumulation (msm_accumulate_kernel<Fq2U>: 112 for the
// running sum, 56 for the base, the temporaries of the formula and four 14-limb operands per fused product), so a SIMD holds ONE such
// wave and nothing covers its waits (profiles/rocprofv3_pmc_r3_sq.txt).  With the halves on two lanes every lane carries half the
// state (G1-sized: under 256 registers, two waves per SIMD) and does exactly half the multiplications:
//   product   c0 = a0 b0 - a1 b1 (even lane),  c1 = a0 b1 + a1 b0 (odd lane): each ONE fqu_mul2 (two half-products, one reduction) of
//             the lane's own halves and its partner's;
//   square    c0 = (a0 + a1)(a0 - a1),  c1 = 2 a0 a1: ONE fqu_mul per lane;
//   add / sub / double / negate: limb-wise on the lane's own half.
// Value bounds are those of the one-lane lazy form (ffu.cuh fq2u_mul_lazy, ec.cuh xyzz_madd_lazy): products < 2q per component,
// squares < 2q / < 4q, everything multiplied <= 127 q.
//
// The formulas are written ONCE over a lane model M with three primitives:
//   m.partner(v)          the other lane's value of v
//   m.by_parity(o, e)     o on the odd lane, e on the even one
//   m.both(p)             p holds on both lanes of the pair (one bool for the pair)
// and m.each(f, v...) / m.test(f, v...) for the limb-wise work and the predicates of a lane's own half.
//   H2Lane<INL> (device)  V = FqU, the lane's own half.  partner = DPP quad_perm [1, 0, 3, 2] (a VALU move, no LDS).  DPP reads the
//                         partner's REGISTERS, so both lanes of a pair must take every branch together: every branch below is
//                         decided by m.both() on the combined test, or by values equal on both lanes (the sign, the parity-free flags).
//   H2Pair (host)         V = both halves in a two-element array, so that a ZK_FQU_CHECK build runs the same text with every operand
//                         assertion of ffu.cuh live (tests/csrc/g2_split_host_shim.hip).
// LC (h2_madd<LC = true>): the carry passes the one-lane xyzz_madd_lazy_lc skips, where the limb rule of ffu.cuh ("Skipped carry
// passes") admits them in this form: the sign folded into R, X3 as one expression, the bare 128q - b1 sent to the partner (it
// meets a normalised operand beside a normalised pair: fqu_mul2_lc<30>) and the bare sum a0 + a1 of a squaring (fqu_mul_impl<30, 29>).
#pragma once
#include "ec.cuh"

namespace zk {

template <bool INL>
struct H2Lane {
    using V = FqU;
    using B = bool;
    static constexpr bool INLINE = INL;      // products inlined (scheduling barriers around each, as G1's loop) instead of called
    int h;
    ZK_HD static uint32_t swap_u32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
#else
        return v;      // host pass of a kernel: parsed, never run
#endif
    }
    ZK_HD V partner(const V &a) const {
        V r;
#pragma unroll
        for (int i = 0; i < 14; i++) r.l[i] = swap_u32(a.l[i]);
        return r;
    }
    ZK_HD V by_parity(const V &odd, const V &even) const {
        V r;
#pragma unroll
        for (int i = 0; i < 14; i++) r.l[i] = h ? odd.l[i] : even.l[i];
        return r;
    }
    ZK_HD bool both(bool mine) const { return mine && swap_u32(mine ? 1u : 0u) != 0u; }
    template <class Fn, class... A> ZK_HD V each(Fn f, const A &...a) const { return f(a...); }
    template <class Fn, class... A> ZK_HD B test(Fn f, const A &...a) const { return f(a...); }
    ZK_HD V one() const {      // Fq2 one = (1, 0)
        V r;
#pragma unroll
        for (int i = 0; i < 14; i++) r.l[i] = h ? 0u : FqUP::one(i);
        return r;
    }
};

#if !defined(__HIP_DEVICE_COMPILE__)
struct H2PairV { FqU c[2]; };
struct H2PairB { bool c[2]; };
struct H2Pair {
    using V = H2PairV;
    using B = H2PairB;
    static constexpr bool INLINE = true;
    V partner(const V &a) const { return V{{a.c[1], a.c[0]}}; }
    V by_parity(const V &odd, const V &even) const { return V{{even.c[0], odd.c[1]}}; }
    bool both(const B &p) const { return p.c[0] && p.c[1]; }
    template <class Fn, class... A> V each(Fn f, const A &...a) const { return V{{f(a.c[0]...), f(a.c[1]...)}}; }
    template <class Fn, class... A> B test(Fn f, const A &...a) const { return B{{f(a.c[0]...), f(a.c[1]...)}}; }
    V one() const { return V{{FqU::one(), FqU::zero()}}; }
};
#endif

// ---- limb-wise work on a lane's own half
template <class M> ZK_HD typename M::V h2_zero(const M &m) { return m.each([]() { return FqU::zero(); }); }
template <class M> ZK_HD typename M::V h2_add(const M &m, const typename M::V &a, const typename M::V &b) {
    return m.each([](const FqU &x, const FqU &y) { return fqu_add(x, y); }, a, b);
}
template <class M> ZK_HD typename M::V h2_dbl(const M &m, const typename M::V &a) { return h2_add(m, a, a); }
template <int L, class M> ZK_HD typename M::V h2_sub(const M &m, const typename M::V &a, const typename M::V &b) {
    return m.each([](const FqU &x, const FqU &y) { return fqu_sub<L>(x, y); }, a, b);
}
template <class M> ZK_HD typename M::V h2_neg(const M &m, const typename M::V &a) {
    return m.each([](const FqU &x) { return fqu_neg(x); }, a);
}
template <class M> ZK_HD bool h2_is_zero(const M &m, const typename M::V &a) {      // exact zero (flags)
    return m.both(m.test([](const FqU &x) { return x.is_zero(); }, a));
}
template <class M> ZK_HD bool h2_is_zero_mod(const M &m, const typename M::V &a) {      // 0 mod q in both components
    return m.both(m.test([](const FqU &x) { return fqu_is_zero_mod(x); }, a));
}

// ---- products.  a, b: halves normalised, <= 127 q
// even lane: a0 b0 + a1 (128q - b1);  odd lane: a1 b0 + a0 b1.  The odd lane sends 128q - b1 (bare limb differences with LC), the
// even lane b0; the received half is fqu_mul2_lc's third operand, the one that may carry 30-bit limbs.
template <bool LC, class M> ZK_HD typename M::V h2_mul_body(const M &m, const typename M::V &a, const typename M::V &b) {
    using V = typename M::V;
    const V nb = m.each([](const FqU &x) { return LC ? fqu_rsub_raw<128>(x) : fqu_sub<128>(FqU::zero(), x); }, b);
    const V pb = m.partner(m.by_parity(nb, b)), pa = m.partner(a);
    const V mine = m.by_parity(pa, a), theirs = m.by_parity(a, pa);      // even: a0, a1; odd: a0 (partner's), a1 (own)
    return m.each([](const FqU &x, const FqU &y, const FqU &z, const FqU &w) { return fqu_mul2_lc<LC ? 30 : 29>(x, y, z, w); }, mine, b, pb, theirs);
}
// own component of a^2: even (a0 + a1)(a0 - a1) < 2q, odd 2 a0 a1 < 4q.  One product per lane: the even lane multiplies the sum
// (bare with LC: limbs < 2^30) by the difference, the odd lane a0 by a1 and doubles the result.
template <bool LC, class M> ZK_HD typename M::V h2_sqr_operand_x(const M &m, const typename M::V &a, const typename M::V &pa) {
    return m.by_parity(pa, m.each([](const FqU &x, const FqU &y) { return LC ? fqu_add_raw(x, y) : fqu_add(x, y); }, a, pa));
}
template <class M> ZK_HD typename M::V h2_sqr_operand_y(const M &m, const typename M::V &a, const typename M::V &pa) {
    return m.by_parity(a, h2_sub<128>(m, a, pa));
}
template <class M> ZK_HD typename M::V h2_sqr_finish(const M &m, const typename M::V &r) {
    return h2_add(m, r, m.by_parity(r, h2_zero(m)));
}

#if defined(__HIP_DEVICE_COMPILE__)
// the product as a device-function call: 28 argument registers + the parity; one copy of the body per code object
template <bool LC>
__device__ __noinline__ FqURet h2_mul_call(zk_v4u a0, zk_v4u a1, zk_v4u a2, zk_v2u a3, zk_v4u b0, zk_v4u b1, zk_v4u b2, zk_v2u b3, int h) {
    FqU a, b;
    a.l[0] = a0.x; a.l[1] = a0.y; a.l[2] = a0.z; a.l[3] = a0.w; a.l[4] = a1.x; a.l[5] = a1.y; a.l[6] = a1.z; a.l[7] = a1.w;
    a.l[8] = a2.x; a.l[9] = a2.y; a.l[10] = a2.z; a.l[11] = a2.w; a.l[12] = a3.x; a.l[13] = a3.y;
    b.l[0] = b0.x; b.l[1] = b0.y; b.l[2] = b0.z; b.l[3] = b0.w; b.l[4] = b1.x; b.l[5] = b1.y; b.l[6] = b1.z; b.l[7] = b1.w;
    b.l[8] = b2.x; b.l[9] = b2.y; b.l[10] = b2.z; b.l[11] = b2.w; b.l[12] = b3.x; b.l[13] = b3.y;
    const FqU r = h2_mul_body<LC>(H2Lane<false>{h}, a, b);
    FqURet o;
#pragma unroll
    for (int i = 0; i < 14; i++) o.l[i] = r.l[i];
    return o;
}
#endif

template <bool LC, class M> ZK_HD typename M::V h2_mul(const M &m, const typename M::V &a, const typename M::V &b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (!M::INLINE) {
        zk_v4u a0 = {a.l[0], a.l[1], a.l[2], a.l[3]}, a1 = {a.l[4], a.l[5], a.l[6], a.l[7]}, a2 = {a.l[8], a.l[9], a.l[10], a.l[11]};
        zk_v2u a3 = {a.l[12], a.l[13]};
        zk_v4u b0 = {b.l[0], b.l[1], b.l[2], b.l[3]}, b1 = {b.l[4], b.l[5], b.l[6], b.l[7]}, b2 = {b.l[8], b.l[9], b.l[10], b.l[11]};
        zk_v2u b3 = {b.l[12], b.l[13]};
        const FqURet r = h2_mul_call<LC>(a0, a1, a2, a3, b0, b1, b2, b3, m.h);
        FqU o;
#pragma unroll
        for (int i = 0; i < 14; i++) o.l[i] = r.l[i];
        return o;
    } else {
        __builtin_amdgcn_sched_barrier(0);      // products are not interleaved: one working set at a time (ec.cuh: fqu_mul_il)
        const typename M::V r = h2_mul_body<LC>(m, a, b);
        __builtin_amdgcn_sched_barrier(0);
        return r;
    }
#else
    return h2_mul_body<LC>(m, a, b);
#endif
}
template <bool LC, class M> ZK_HD typename M::V h2_sqr(const M &m, const typename M::V &a) {
    using V = typename M::V;
    const V pa = m.partner(a);
    const V x = h2_sqr_operand_x<LC>(m, a, pa), y = h2_sqr_operand_y(m, a, pa);
    V r;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (!M::INLINE) r = fqu_mul(x, y);      // the shared product body (fqu_mul_call): device code carries no operand checks
    else r = fqu_mul_il(x, y);
#else
    r = m.each([](const FqU &s, const FqU &t) { return fqu_mul_impl<false, LC ? 30 : 29, 29>(s, t); }, x, y);
#endif
    return h2_sqr_finish(m, r);
}

// ---- points: one half of an affine / XYZZ G2 point per lane
template <class M> struct H2Affine { typename M::V x, y; };
template <class M> struct H2XYZZ { typename M::V x, y, zz, zzz; };

template <class M> ZK_HD H2XYZZ<M> h2_inf(const M &m) { return H2XYZZ<M>{h2_zero(m), h2_zero(m), h2_zero(m), h2_zero(m)}; }
template <class M> ZK_HD bool h2_is_inf(const M &m, const H2XYZZ<M> &p) { return h2_is_zero(m, p.zz); }
template <class M> ZK_HD bool h2_is_inf(const M &m, const H2Affine<M> &p) {
    return m.both(m.test([](const FqU &x, const FqU &y) { return x.is_zero() && y.is_zero(); }, p.x, p.y));
}

// 2 * (affine q), q != inf  (ec.cuh xyzz_dbl_affine)
template <class M> ZK_HD H2XYZZ<M> h2_dbl_affine(const M &m, const H2Affine<M> &q) {
    using V = typename M::V;
    const V U = h2_dbl(m, q.y);
    const V Vv = h2_sqr<false>(m, U);
    const V W = h2_mul<false>(m, U, Vv);
    const V S = h2_mul<false>(m, q.x, Vv);
    const V X2 = h2_sqr<false>(m, q.x);
    const V Mm = h2_add(m, h2_dbl(m, X2), X2);
    H2XYZZ<M> r;
    r.x = h2_sub<32>(m, h2_sqr<false>(m, Mm), h2_dbl(m, S));
    r.y = h2_sub<32>(m, h2_mul<false>(m, Mm, h2_sub<64>(m, S, r.x)), h2_mul<false>(m, W, q.y));
    r.zz = Vv;
    r.zzz = W;
    return r;
}

// acc += (neg ? -q : q): ec.cuh xyzz_madd_lazy (LC: xyzz_madd_lazy_lc), the same formula, bounds and exceptional cases: base at
// infinity, start of a run, P = -Q to infinity, and P = Q, which h2_madd_nd only REPORTS (it returns false and leaves acc as it
// was): the doubling needs the base, and a caller that can fetch it again (the accumulation kernel re-gathers it) does not keep its
// 28 registers alive across the products of every ordinary addition.  h2_madd does the doubling itself.
// `neg` is the same on both lanes (one term per pair).  The products are ordered as G1's (ec.cuh: xyzz_madd_front): at most six
// values are live across any of them, which is what the callee-saved half of 256 registers holds beside the loop's own state.
template <bool LC, class M> ZK_HD bool h2_madd_nd(const M &m, H2XYZZ<M> &acc, const H2Affine<M> &q, bool neg) {
    using V = typename M::V;
    if (h2_is_inf(m, q)) return true;
    if (h2_is_inf(m, acc)) {
        acc = H2XYZZ<M>{q.x, neg ? h2_neg(m, q.y) : q.y, m.one(), m.one()};
        return true;
    }
    const V U2 = h2_mul<LC>(m, q.x, acc.zz);
    V R;
    if constexpr (LC) {
        // the sign folded into R: (neg ? 8q - S2 : S2) + (64q - Y1) as one expression with one pass; -q is formed only where it is needed
        const V S2 = h2_mul<LC>(m, q.y, acc.zzz);
        R = m.each([neg](const FqU &s, const FqU &y) { return fqu_addsub_sel(s, fqu_rsub_raw<64>(y), neg); }, S2, acc.y);
    } else {
        const V S2 = h2_mul<LC>(m, neg ? h2_neg(m, q.y) : q.y, acc.zzz);
        R = h2_sub<64>(m, S2, acc.y);
    }
    const V Pp = h2_sub<64>(m, U2, acc.x);
    if (h2_is_zero_mod(m, Pp)) {
        if (h2_is_zero_mod(m, R)) return false;
        acc = h2_inf(m);
        return true;
    }
    const V PP = h2_sqr<LC>(m, Pp);
    const V PPP = h2_mul<LC>(m, Pp, PP);
    acc.zz = h2_mul<LC>(m, acc.zz, PP);
    acc.zzz = h2_mul<LC>(m, acc.zzz, PPP);
    const V Q = h2_mul<LC>(m, acc.x, PP);
    const V RR = h2_sqr<LC>(m, R);
    V X3;
    if constexpr (LC) X3 = m.each([](const FqU &rr, const FqU &b, const FqU &c) { return fqu_sub_b_2c(rr, b, c); }, RR, PPP, Q);
    else X3 = h2_sub<32>(m, RR, h2_add(m, PPP, h2_dbl(m, Q)));
    const V T = h2_mul<LC>(m, R, h2_sub<64>(m, Q, X3));
    acc.y = h2_sub<32>(m, T, h2_mul<LC>(m, acc.y, PPP));
    acc.x = X3;
    return true;
}
template <class M> ZK_HD H2XYZZ<M> h2_dbl_term(const M &m, const H2Affine<M> &q, bool neg) {
    return h2_dbl_affine(m, H2Affine<M>{q.x, neg ? h2_neg(m, q.y) : q.y});
}
template <bool LC, class M> ZK_HD void h2_madd(const M &m, H2XYZZ<M> &acc, const H2Affine<M> &q, bool neg) {
    if (!h2_madd_nd<LC>(m, acc, q, neg)) acc = h2_dbl_term(m, q, neg);
}

// ---- memory.  The layout is Affine<Fq2U> / XYZZ<Fq2U> (x.c0 x.c1 y.c0 y.c1 ...; 56 bytes per component): lane h reads / writes
// component h of each coordinate.  Component 1 starts at a multiple of 8 bytes, not 16: 8-byte accesses.
__device__ __forceinline__ FqU h2_ld(const FqU *p) {
    const uint2 *q = reinterpret_cast<const uint2 *>(p);
    FqU v;
#pragma unroll
    for (int i = 0; i < 7; i++) { const uint2 w = q[i]; v.l[2 * i] = w.x; v.l[2 * i + 1] = w.y; }
    return v;
}
__device__ __forceinline__ void h2_st(FqU *p, const FqU &v) {
    uint2 *q = reinterpret_cast<uint2 *>(p);
#pragma unroll
    for (int i = 0; i < 7; i++) q[i] = make_uint2(v.l[2 * i], v.l[2 * i + 1]);
}
template <class M> __device__ __forceinline__ H2Affine<M> h2_ld_affine(const M &m, const Affine<Fq2U> *p) {
    const FqU *f = reinterpret_cast<const FqU *>(p);
    return H2Affine<M>{h2_ld(f + m.h), h2_ld(f + 2 + m.h)};
}
template <class M> __device__ __forceinline__ H2XYZZ<M> h2_ld_xyzz(const M &m, const XYZZ<Fq2U> *p) {
    const FqU *f = reinterpret_cast<const FqU *>(p);
    return H2XYZZ<M>{h2_ld(f + m.h), h2_ld(f + 2 + m.h), h2_ld(f + 4 + m.h), h2_ld(f + 6 + m.h)};
}
template <class M> __device__ __forceinline__ void h2_st_xyzz(const M &m, XYZZ<Fq2U> *p, const H2XYZZ<M> &v) {
    FqU *f = reinterpret_cast<FqU *>(p);
    h2_st(f + m.h, v.x); h2_st(f + 2 + m.h, v.y); h2_st(f + 4 + m.h, v.zz); h2_st(f + 6 + m.h, v.zzz);
}

}  // namespace zk
