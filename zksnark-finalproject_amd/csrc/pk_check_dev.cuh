// Curve and prime-order-subgroup membership of the points of a RESIDENT query (zkg16_pk_check, zkg16_points_check_bulk): one lane
// per point of a device array of U-form affine entries, addressed as base + i * stride (112 / 224 bytes for a plain query, 128 / 256
// for level 0 of a padded window table; a lane reads the two coordinates at the front of its entry and nothing behind them).
//
// The verdict is zkg16_point_check's: (0, 0) is the point at infinity and passes; any other point is good iff it satisfies the curve
// equation and the endomorphism test of pairing_dev.cuh,
//     G1:  phi(P) = (beta x, y)                 == -[z^2] P      one ladder by z^2: 127 doublings, 16 mixed additions
//     G2:  psi(P) = (conj(x) cx, conj(y) cy)    == -[|z|] P      one ladder by |z|:  63 doublings,  5 mixed additions
// or, where the start-up calibration of the constants fell back (VbEndo::fast_g1 / fast_g2 == 0), [r] P == O by the plain ladder.
// The formulas are ec.cuh's (xyzz_dbl, xyzz_madd: the same value bounds), restated with every field product INLINED
// (fqu_mul_ilc / fqu_sqr_ilc / fqu_mul2): membership_kernel calls its products, so what is live across a call has to sit in the
// callee-saved half of the register file or in scratch (1,232 B a lane); here the XYZZ accumulator and the affine addend stay in
// registers for the whole ladder.  G1 walks z^2 in ONE ladder with the affine addend, not |z| twice (pairing_dev.cuh: mul_z(mul_z(p))):
// the second of those adds an XYZZ point (14 products against 10, and 56 more registers held for 63 doublings, which spilled at two
// waves per SIMD); the single ladder is 1,303 products against 1,254 and holds 84 registers of state.  A ladder's scalar is read from the kernel arguments (lane-uniform bits: scalar loads and scalar
// branches), never from a per-lane array.  No lane leaves early on a bad point: an off-curve point walks the same ladder (the
// a = 0 formulas never use b), so a wave's time does not depend on its data.
//
// __host__ __device__ throughout: tests/csrc/pk_check_host_shim.hip runs the lane functions on the CPU with ZK_FQU_CHECK, which
// asserts every operand bound while the tests run.
#pragma once
#include "ec.cuh"
#include "ffu.cuh"

namespace zk {
namespace pkc {

// a ladder's scalar: bit `top` is set and is the accumulator's start; the bits below it are walked
struct Scalar {
    uint32_t w[8];
    int top;
};
// everything a launch of one group needs beside the array (kernel arguments; made on the host by pkc::params_*)
struct ParamsG1 {
    FqU b;              // 4
    FqU beta;           // phi's cube root of unity
    Scalar k;           // z^2 (fast) or r
    int fast;
};
struct ParamsG2 {
    Fq2U b;             // 4 (1 + u)
    Fq2U cx, cy;        // psi's constants
    Scalar k;
    int fast;
};
constexpr uint64_t Z_ABS = 0xd201000000010000ULL;      // |z| of BLS12-381
ZK_HD Scalar scalar_z() {
    Scalar s;
#pragma unroll
    for (int i = 0; i < 8; i++) s.w[i] = 0;
    s.w[0] = (uint32_t)Z_ABS;
    s.w[1] = (uint32_t)(Z_ABS >> 32);
    s.top = 63;
    return s;
}
ZK_HD Scalar scalar_z2() {                              // z^2 = 0xac45a401 0001a402 00000001 00000000: 128 bits, 17 of them set
    static_assert((uint32_t)(Z_ABS * Z_ABS) == 0u && (uint32_t)((Z_ABS * Z_ABS) >> 32) == 1u, "low half of z^2");
    Scalar s;
#pragma unroll
    for (int i = 0; i < 8; i++) s.w[i] = 0;
    s.w[1] = 0x00000001u;
    s.w[2] = 0x0001a402u;
    s.w[3] = 0xac45a401u;
    s.top = 127;
    return s;
}
ZK_HD Scalar scalar_r() {
    Scalar s;
#pragma unroll
    for (int i = 0; i < 8; i++) s.w[i] = FrP::mod(i);
    s.top = 254;
    return s;
}
ZK_HD FqU four_u() {
    Fq four = Fq::zero();
    four.l[0] = 4;
    return fqu_from_sat(fp_to_mont(four));
}
// beta, cx, cy: the calibrated constants in saturated limbs (VbEndo)
ZK_HD ParamsG1 params_g1(const Fq &beta, bool fast) {
    return ParamsG1{four_u(), fqu_from_sat(beta), fast ? scalar_z2() : scalar_r(), fast ? 1 : 0};
}
ZK_HD ParamsG2 params_g2(const Fq2 &cx, const Fq2 &cy, bool fast) {
    const FqU f = four_u();
    return ParamsG2{Fq2U{f, f}, fq2u_from_sat(cx), fq2u_from_sat(cy), fast ? scalar_z() : scalar_r(), fast ? 1 : 0};
}

// ------------------------------------------------------------------------------------------------ inlined products, by overload
ZK_HD FqU pm(const FqU &a, const FqU &b) { return fqu_mul_ilc(a, b); }
ZK_HD FqU ps(const FqU &a) { return fqu_sqr_ilc(a); }
// a b - c d, c a stored coordinate (<= 63 q): one reduction (f_mul_sub)
ZK_HD FqU pmsub(const FqU &a, const FqU &b, const FqU &c, const FqU &d) {
    const FqU nc = fqu_sub<64>(FqU::zero(), c);
#if defined(__HIP_DEVICE_COMPILE__)
    return fqu_mul2_il(a, b, nc, d);
#else
    return fqu_mul2(a, b, nc, d);
#endif
}
// Karatsuba (f_mul of Fq2U); components < 10 q
ZK_HD Fq2U pm(const Fq2U &a, const Fq2U &b) {
    const FqU v0 = pm(a.c0, b.c0), v1 = pm(a.c1, b.c1);
    const FqU s = pm(fqu_add(a.c0, a.c1), fqu_add(b.c0, b.c1));
    return Fq2U{fqu_sub<8>(v0, v1), fqu_sub<8>(s, fqu_add(v0, v1))};
}
// f_sqr of Fq2U: components <= 127 q; result (< 2q, < 4q)
ZK_HD Fq2U ps(const Fq2U &a) {
    const FqU p = pm(a.c0, a.c1);
    const FqU r0 = pm(fqu_add(a.c0, a.c1), fqu_sub<128>(a.c0, a.c1));
    return Fq2U{r0, fqu_dbl(p)};
}
ZK_HD Fq2U pmsub(const Fq2U &a, const Fq2U &b, const Fq2U &c, const Fq2U &d) { return f_sub(pm(a, b), pm(c, d)); }

// ------------------------------------------------------------------------------------------------ ec.cuh's formulas on them
template <class F>
ZK_HD XYZZ<F> dbl_affine(const Affine<F> &p) {             // xyzz_dbl_affine
    const F U = f_dbl(p.y);
    const F V = ps(U);
    const F W = pm(U, V);
    const F S = pm(p.x, V);
    const F X2 = ps(p.x);
    const F M = f_add(f_dbl(X2), X2);
    XYZZ<F> r;
    r.x = f_sub(ps(M), f_dbl(S));
    r.y = pmsub(M, f_sub2(S, r.x), p.y, W);
    r.zz = V;
    r.zzz = W;
    return r;
}
template <class F>
ZK_HD void dbl(XYZZ<F> &p) {                               // xyzz_dbl
    if (p.is_inf()) return;
    const F U = f_dbl(p.y);
    const F V = ps(U);
    const F W = pm(U, V);
    const F S = pm(p.x, V);
    const F X2 = ps(p.x);
    const F M = f_add(f_dbl(X2), X2);
    const F X3 = f_sub(ps(M), f_dbl(S));
    p.y = pmsub(M, f_sub2(S, X3), p.y, W);
    p.x = X3;
    p.zz = pm(V, p.zz);
    p.zzz = pm(W, p.zzz);
}
template <class F>
ZK_HD void madd(XYZZ<F> &acc, const Affine<F> &q) {        // xyzz_madd, q not at infinity
    if (acc.is_inf()) {
        acc = XYZZ<F>{q.x, q.y, F::one(), F::one()};
        return;
    }
    const F U2 = pm(q.x, acc.zz);
    const F S2 = pm(q.y, acc.zzz);
    const F Pp = f_sub2(U2, acc.x);
    const F R = f_sub2(S2, acc.y);
    if (f_is_zero_mod(Pp)) {
        if (f_is_zero_mod(R)) acc = dbl_affine(q);
        else acc = XYZZ<F>::inf();
        return;
    }
    const F PP = ps(Pp);
    const F PPP = pm(Pp, PP);
    const F Q = pm(acc.x, PP);
    const F X3 = f_sub(ps(R), f_add(PPP, f_dbl(Q)));
    acc.y = pmsub(R, f_sub2(Q, X3), acc.y, PPP);
    acc.x = X3;
    acc.zz = pm(acc.zz, PP);
    acc.zzz = pm(acc.zzz, PPP);
}
ZK_HD bool bit(const Scalar &k, int i) { return (k.w[i >> 5] >> (i & 31)) & 1u; }
// [k] p for an affine p that is not at infinity: the mixed addition all the way
template <class F>
ZK_HD XYZZ<F> ladder(const Affine<F> &p, const Scalar &k) {
    XYZZ<F> acc{p.x, p.y, F::one(), F::one()};
    for (int i = k.top - 1; i >= 0; i--) {
        dbl(acc);
        if (bit(k, i)) madd(acc, p);
    }
    return acc;
}
// ------------------------------------------------------------------------------------------------ one lane
// coordinates as they are stored: products (< 2q per Fq component), (0, 0) = infinity
ZK_HD bool g1_good(const Affine<FqU> &p, const ParamsG1 &prm) {
    if (p.is_inf()) return true;
    const FqU rhs = fqu_add(pm(ps(p.x), p.x), prm.b);                                       // < 4q
    const bool curve = fqu_is_zero_mod(fqu_sub<8>(ps(p.y), rhs));
    const XYZZ<FqU> acc = ladder(p, prm.k);                                                 // [z^2] P, or [r] P
    if (!prm.fast) return curve && acc.is_inf();
    if (acc.is_inf()) return false;
    // -[z^2] P == (beta x, y):  X == beta x ZZ  and  Y + y ZZZ == 0
    const bool same_x = fqu_is_zero_mod(fqu_sub<64>(pm(pm(p.x, prm.beta), acc.zz), acc.x));
    const bool opp_y = fqu_is_zero_mod(fqu_add(acc.y, pm(p.y, acc.zzz)));
    return curve && same_x && opp_y;
}
ZK_HD bool g2_good(const Affine<Fq2U> &p, const ParamsG2 &prm) {
    if (p.is_inf()) return true;
    const Fq2U rhs = f_add(pm(ps(p.x), p.x), prm.b);                                        // < 12q
    const bool curve = f_is_zero_mod(f_sub(ps(p.y), rhs));
    const XYZZ<Fq2U> acc = ladder(p, prm.k);
    if (!prm.fast) return curve && acc.is_inf();
    if (acc.is_inf()) return false;
    // -[|z|] P == (conj(x) cx, conj(y) cy)
    const Fq2U psi_x = pm(Fq2U{p.x.c0, fqu_neg(p.x.c1)}, prm.cx), psi_y = pm(Fq2U{p.y.c0, fqu_neg(p.y.c1)}, prm.cy);
    const bool same_x = f_is_zero_mod(f_sub2(pm(psi_x, acc.zz), acc.x));
    const bool opp_y = f_is_zero_mod(f_add(acc.y, pm(psi_y, acc.zzz)));
    return curve && same_x && opp_y;
}
// the entry of point i: two coordinates at the front of base + i * stride
ZK_HD bool g1_lane(const unsigned char *base, size_t stride, size_t i, const ParamsG1 &prm) {
    return g1_good(*reinterpret_cast<const Affine<FqU> *>(base + i * stride), prm);
}
ZK_HD bool g2_lane(const unsigned char *base, size_t stride, size_t i, const ParamsG2 &prm) {
    return g2_good(*reinterpret_cast<const Affine<Fq2U> *>(base + i * stride), prm);
}

// ------------------------------------------------------------------------------------------------ kernels
// (left out of a host-only build of the lane functions: ZK_PKC_LANES_ONLY, tests/csrc/pk_check_host_shim.hip)
#if defined(__HIPCC__) && !defined(ZK_PKC_LANES_ONLY)
// minimum waves per SIMD the two kernels are compiled for (pk_check.hip states the choice)
#ifndef ZK_PKC_G1_WAVES
#define ZK_PKC_G1_WAVES 2
#endif
#ifndef ZK_PKC_G2_WAVES
#define ZK_PKC_G2_WAVES 1
#endif
// the result slot of one array: res[0] = number of bad points, res[1] = smallest bad index (UINT64_MAX: none)
__global__ void pk_check_init_kernel(unsigned long long *res, int slots) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < slots) {
        res[2 * t] = 0ull;
        res[2 * t + 1] = ~0ull;
    }
}
// One wave per block, one point per lane.  The wave's bad lanes are counted by a ballot; the lowest of them adds the count and
// offers its index (an integer sum and a minimum: the same whatever the order), a wave without a bad point writes nothing.
__device__ __forceinline__ void report(bool bad, size_t i, unsigned long long *res) {
    const unsigned long long m = __ballot(bad);
    if (bad && (threadIdx.x & 63u) == (unsigned)(__ffsll(m) - 1)) {
        atomicAdd(res, (unsigned long long)__popcll(m));
        atomicMin(res + 1, (unsigned long long)i);
    }
}
__global__ __launch_bounds__(64, ZK_PKC_G1_WAVES) void pk_check_g1_kernel(const unsigned char *base, size_t stride, size_t n, ParamsG1 prm, unsigned long long *res) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool bad = i < n && !g1_lane(base, stride, i, prm);
    report(bad, i, res);
}
__global__ __launch_bounds__(64, ZK_PKC_G2_WAVES) void pk_check_g2_kernel(const unsigned char *base, size_t stride, size_t n, ParamsG2 prm, unsigned long long *res) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool bad = i < n && !g2_lane(base, stride, i, prm);
    report(bad, i, res);
}
#endif

}  // namespace pkc
}  // namespace zk
