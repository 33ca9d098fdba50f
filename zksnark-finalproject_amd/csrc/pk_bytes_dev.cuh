// A proving key's points between arkworks' compressed bytes and the RESIDENT form (zkg16_pk_load_bytes, zkg16_pk_save, zkg16_pk_read;
// launches: pk_bytes.hip), one lane per point:
//   decode   48 / 96 wire bytes at a byte stride -> the U-form affine entry at base + i * stride, (0, 0) for the point at infinity,
//            with the statuses of zkg16_g1_decompress / zkg16_g2_decompress decided in their order (0 ok, 1 not compressed,
//            2 non-canonical infinity, 3 x not reduced, 4 not on the curve; the subgroup is zkg16_pk_check's business);
//   encode   the U-form entry -> the bytes of zkg16_points_compress;
//   read     the U-form entry -> saturated Montgomery limbs and an infinity flag (zkg16_pk_load's arrays).
//
// What a decode lane stores.  The MSM kernels' operand bounds assume the words convert_g1_bases / convert_g2_bases write for a
// key's limbs (fqu_from_sat: one product by a constant, < 2q, exact zero for zero), and a handle loaded from bytes has to be the
// handle zkg16_pk_load makes from the host-decoded limbs, word for word.  So a lane ENDS with that very conversion: the decoded
// coordinates leave through fqu_to_sat (canonical limbs, the host decoders' output) and come back through fqu_from_sat.
//
// The square roots.  The exponents are constants, so every lane of a wave takes the same path; the products of the two power
// loops are inlined (fqu_mul_ilc / fqu_sqr_ilc, as pk_check_dev.cuh) and the 16-entry window table is indexed by a lane-uniform
// digit (it lies in scratch: profiles/kernel_resource_usage_pk_bytes.txt).  G1 is one power by (q + 1) / 4: 376 squarings, 14 table
// products, at most 94 window products.  G2 is the complex method of decompress_dev.cuh WITHOUT its inversion.  There the root of
// a = a0 + a1 u is (c, a1 / 2c) or (a1 / 2c, c) with c = cand^((q + 1) / 4), and 1 / 2c came from fqu_inv (608 products).  Here
//     t = cand^((q - 3) / 4),     c = t cand,     1 / c = t^3 cand:
// t^3 cand = cand^((3q - 5) / 4), and (3q - 5) / 4 + (q + 1) / 4 = q - 1, so c t^3 cand = cand^(q - 1) = 1 for every cand != 0
// (cand == 0 only for a == 0, whose root is zero and is not divided).  Five products instead of 608: two powers and ~10 products
// a point, against two powers and the inversion (1,570 -> 975).  The root is still checked by squaring, so `false` is exact.
//
// __host__ __device__ throughout: tests/csrc/pk_bytes_host_shim.hip runs the lane functions on the CPU against the host decoders,
// zkg16_points_compress and dc::fq2_sqrt, with the bound assertions of pairing_dev.cuh live.
#pragma once
#include "decompress_dev.cuh"

namespace zk {
namespace pkb {

using pd::F2;

ZK_HD FqU pm(const FqU &a, const FqU &b) {
    ZK_PD_BOUND(a, 4096);
    ZK_PD_BOUND(b, 4096);
    return fqu_mul_ilc(a, b);
}
ZK_HD FqU ps(const FqU &a) {
    ZK_PD_BOUND(a, 4096);
    return fqu_sqr_ilc(a);
}

// a^((q + ADD) / 4) for ADD = 1 or -3 (q = 3 mod 4: both are whole), fixed windows of four bits.  a < 4096 q; result < 2q, zero
// for zero.  Both exponents have 379 bits: the window at bit 376 is not zero and starts the accumulator, 94 windows follow
template <int ADD>
ZK_HD FqU pow_q4(const FqU &a) {
    static_assert(ADD == 1 || ADD == -3, "exponent");
    uint32_t e[12];
    {
        uint32_t t[12];
        int64_t carry = ADD;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const int64_t v = (int64_t)FqP::mod(i) + carry;
            t[i] = (uint32_t)v;
            carry = v >> 32;                                      // arithmetic shift = floor
        }
#pragma unroll
        for (int i = 0; i < 12; i++) e[i] = (t[i] >> 2) | (i < 11 ? t[i + 1] << 30 : 0u);
    }
    FqU tbl[16];
    tbl[0] = FqU::one();
    tbl[1] = a;
#pragma unroll 1
    for (int i = 2; i < 16; i++) tbl[i] = pm(tbl[i - 1], a);
    FqU acc = tbl[(e[11] >> 24) & 15u];
#pragma unroll 1
    for (int w = 93; w >= 0; w--) {
        acc = ps(ps(ps(ps(acc))));
        const uint32_t nib = (e[w >> 3] >> (4 * (w & 7))) & 15u;
        if (nib) acc = pm(acc, tbl[nib]);
    }
    return acc;
}
// r = a^((q + 1) / 4) and whether r^2 == a.  a <= 7q
ZK_HD bool fq_sqrt(const FqU &a, FqU &r) {
    r = pow_q4<1>(a);
    return fqu_is_zero_mod(pd::sub<8>(ps(r), a));                 // 2 + 8
}
// A root of a in Fq[u] / (u^2 + 1) without an inversion (the header's first comment).  Branches as dc::fq2_sqrt: a1 == 0 gives
// (c, 0) for a residue a0 and (0, c) for a non-residue; a == 0 gives zero.  Either root of a may come out; false: a has none
// (r = 0).  a tidy (< 2q per component); r < 2q per component
ZK_HD bool fq2_sqrt(const F2 &a, F2 &r) {
    r = F2::zero();
    const bool real = fqu_is_zero_mod(a.c1);
    const FqU norm = fqu_add(ps(a.c0), ps(a.c1));                 // < 4q
    FqU n;
    if (!fq_sqrt(norm, n)) return false;                          // a0^2 for a real a: a residue
    const FqU cand = real ? a.c0 : pm(fqu_add(a.c0, n), dc::k_two_inv());
    const FqU t = pow_q4<-3>(cand);
    const FqU c = pm(t, cand);                                    // cand^((q + 1) / 4)
    const bool first = fqu_is_zero_mod(pd::sub<8>(ps(c), cand));  // 2 + 8
    const FqU half_inv = pm(pm(pm(ps(t), t), cand), dc::k_two_inv());      // 1 / 2c (0 for cand == 0)
    const FqU im = real ? FqU::zero() : pm(a.c1, half_inv);
    const F2 root = first ? F2{c, im} : F2{im, c};
    if (!f_is_zero_mod(pd::sub<8>(pd::sqr<8>(root), a))) return false;     // 4 + 8
    r = root;
    return true;
}

// ------------------------------------------------------------------------------------------------ decode
// the stored entry of decoded coordinates: through the host decoders' limbs (sat, nullable: where a caller wants them too)
ZK_HD Affine<FqU> store_g1(const FqU &x, const FqU &y, G1Affine *sat) {
    const G1Affine s{fqu_to_sat(x), fqu_to_sat(y)};
    if (sat) *sat = s;
    return Affine<FqU>{fqu_from_sat(s.x), fqu_from_sat(s.y)};
}
ZK_HD Affine<Fq2U> store_g2(const F2 &x, const F2 &y, G2Affine *sat) {
    const G2Affine s{fq2u_to_sat(x), fq2u_to_sat(y)};
    if (sat) *sat = s;
    return Affine<Fq2U>{fq2u_from_sat(s.x), fq2u_from_sat(s.y)};
}
// b: 48 bytes.  u: the entry, (0, 0) for infinity and for statuses 1 to 4.  Returns the status
ZK_HD int g1_decode(const uint8_t *b, Affine<FqU> &u, G1Affine *sat = nullptr) {
    u = Affine<FqU>{FqU::zero(), FqU::zero()};
    if (sat) *sat = G1Affine::inf();
    if (!(b[0] & 0x80)) return 1;
    if (b[0] & 0x40) return dc::inf_is_clean(b, 48) ? 0 : 2;
    FqU xp;
    if (!dc::fq_parse(b, true, xp)) return 3;
    const FqU x = pm(xp, dc::k_r2());
    FqU y;
    if (!fq_sqrt(fqu_add(pm(ps(x), x), dc::k_four()), y)) return 4;                             // < 4q
    if (dc::gt_half(dc::from_mont(y)) != ((b[0] & 0x20) != 0)) y = pd::sub<8>(FqU::zero(), y);  // 8q - y
    u = store_g1(x, y, sat);
    return 0;
}
// b: 96 bytes, x.c1 || x.c0
ZK_HD int g2_decode(const uint8_t *b, Affine<Fq2U> &u, G2Affine *sat = nullptr) {
    u = Affine<Fq2U>{Fq2U::zero(), Fq2U::zero()};
    if (sat) *sat = G2Affine::inf();
    if (!(b[0] & 0x80)) return 1;
    if (b[0] & 0x40) return dc::inf_is_clean(b, 96) ? 0 : 2;
    FqU x1p, x0p;
    const bool r1 = dc::fq_parse(b, true, x1p), r0 = dc::fq_parse(b + 48, false, x0p);
    if (!r1 || !r0) return 3;
    const F2 x{pm(x0p, dc::k_r2()), pm(x1p, dc::k_r2())};
    const F2 rhs = pd::tidy(pd::add(pd::mul(pd::sqr<8>(x), x), F2{dc::k_four(), dc::k_four()}));       // x^3 + 4 (1 + u): 10 + 2
    F2 y;
    if (!fq2_sqrt(rhs, y)) return 4;
    const FqU y1p = dc::from_mont(y.c1);
    const bool largest = y1p.is_zero() ? dc::gt_half(dc::from_mont(y.c0)) : dc::gt_half(y1p);
    if (largest != ((b[0] & 0x20) != 0)) y = pd::tidy(pd::neg<8>(y));
    u = store_g2(x, y, sat);
    return 0;
}

// ------------------------------------------------------------------------------------------------ encode and read
// a canonical plain value in base 2^29 -> 48 big-endian bytes
ZK_HD void fq_bytes(const FqU &v, uint8_t *b) {
#pragma unroll
    for (int w = 0; w < 12; w++) {
        const int bit = 32 * w;
        const int i = bit / 29, off = bit % 29;
        uint64_t acc = (uint64_t)v.l[i] >> off;
        if (i + 1 < 14) acc |= (uint64_t)v.l[i + 1] << (29 - off);
        if (i + 2 < 14) acc |= (uint64_t)v.l[i + 2] << (58 - off);
        const uint32_t word = (uint32_t)acc;
        b[47 - 4 * w] = (uint8_t)word;
        b[46 - 4 * w] = (uint8_t)(word >> 8);
        b[45 - 4 * w] = (uint8_t)(word >> 16);
        b[44 - 4 * w] = (uint8_t)(word >> 24);
    }
}
// stored coordinates (< 2q per Fq component; anything below 4096 q would do)
ZK_HD void g1_encode(const Affine<FqU> &p, uint8_t *b) {
    if (p.is_inf()) {
        for (int i = 0; i < 48; i++) b[i] = 0;
        b[0] = 0xC0;
        return;
    }
    fq_bytes(dc::from_mont(p.x), b);
    b[0] |= 0x80 | (dc::gt_half(dc::from_mont(p.y)) ? 0x20 : 0);
}
// x.c1 || x.c0; (y.c1, y.c0) compared: c1 decides unless it is zero
ZK_HD void g2_encode(const Affine<Fq2U> &p, uint8_t *b) {
    if (p.is_inf()) {
        for (int i = 0; i < 96; i++) b[i] = 0;
        b[0] = 0xC0;
        return;
    }
    fq_bytes(dc::from_mont(p.x.c1), b);
    fq_bytes(dc::from_mont(p.x.c0), b + 48);
    const FqU y1 = dc::from_mont(p.y.c1);
    const bool largest = y1.is_zero() ? dc::gt_half(dc::from_mont(p.y.c0)) : dc::gt_half(y1);
    b[0] |= 0x80 | (largest ? 0x20 : 0);
}
// the limbs zkg16_pk_load takes: zero limbs and the flag for the point at infinity
ZK_HD void g1_read(const Affine<FqU> &p, G1Affine &out, uint8_t &inf) {
    inf = p.is_inf() ? 1 : 0;
    out = G1Affine::inf();
    if (!inf) out = G1Affine{fqu_to_sat(p.x), fqu_to_sat(p.y)};
}
ZK_HD void g2_read(const Affine<Fq2U> &p, G2Affine &out, uint8_t &inf) {
    inf = p.is_inf() ? 1 : 0;
    out = G2Affine::inf();
    if (!inf) out = G2Affine{fq2u_to_sat(p.x), fq2u_to_sat(p.y)};
}

// ------------------------------------------------------------------------------------------------ kernels
// (left out of a host-only build of the lane functions: ZK_PKB_LANES_ONLY, tests/csrc/pk_bytes_host_shim.hip)
#if defined(__HIPCC__) && !defined(ZK_PKB_LANES_ONLY)
// minimum waves per SIMD the two decode kernels are compiled for (pk_bytes.hip states the choice)
#ifndef ZK_PKB_G1_WAVES
#define ZK_PKB_G1_WAVES 2
#endif
#ifndef ZK_PKB_G2_WAVES
#define ZK_PKB_G2_WAVES 2
#endif
// the result slot of one array: res[0] = points with a status, res[1] = the smallest (index << 3 | status) (UINT64_MAX: none)
__global__ void pkb_init_kernel(unsigned long long *res, int slots) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < slots) {
        res[2 * t] = 0ull;
        res[2 * t + 1] = ~0ull;
    }
}
// One wave per block, one point per lane; indices grow with the lane, so the lowest failing lane holds the wave's smallest key.
// A sum and a minimum: the same whatever the order; a wave without a failure writes nothing
__device__ __forceinline__ void pkb_report(int status, size_t index, unsigned long long *res) {
    const bool bad = status != 0;
    const unsigned long long m = __ballot(bad);
    if (bad && (threadIdx.x & 63u) == (unsigned)(__ffsll(m) - 1)) {
        atomicAdd(res, (unsigned long long)__popcll(m));
        atomicMin(res + 1, ((unsigned long long)index << 3) | (unsigned long long)status);
    }
}
// bytes: n encodings back to back; out + i * stride: the entries; first: the index of point 0 in its query (what a failure names)
__global__ __launch_bounds__(64, ZK_PKB_G1_WAVES) void pkb_decode_g1_kernel(const uint8_t *bytes, size_t n, unsigned char *out, size_t stride, size_t first,
                                                                            unsigned long long *res) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    int st = 0;
    if (i < n) {
        Affine<FqU> u;
        st = g1_decode(bytes + 48 * i, u);
        *reinterpret_cast<Affine<FqU> *>(out + i * stride) = u;
    }
    pkb_report(st, first + i, res);
}
__global__ __launch_bounds__(64, ZK_PKB_G2_WAVES) void pkb_decode_g2_kernel(const uint8_t *bytes, size_t n, unsigned char *out, size_t stride, size_t first,
                                                                            unsigned long long *res) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    int st = 0;
    if (i < n) {
        Affine<Fq2U> u;
        st = g2_decode(bytes + 96 * i, u);
        *reinterpret_cast<Affine<Fq2U> *>(out + i * stride) = u;
    }
    pkb_report(st, first + i, res);
}
// One kernel for both groups: three or six products a point behind 112 / 224 bytes in and 48 / 96 out
__global__ __launch_bounds__(256) void pkb_encode_kernel(int group, const unsigned char *base, size_t stride, size_t n, uint8_t *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (group == 1) g1_encode(*reinterpret_cast<const Affine<FqU> *>(base + i * stride), out + 48 * i);
    else g2_encode(*reinterpret_cast<const Affine<Fq2U> *>(base + i * stride), out + 96 * i);
}
__global__ __launch_bounds__(256) void pkb_read_kernel(int group, const unsigned char *base, size_t stride, size_t n, uint64_t *limbs, uint8_t *inf) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (group == 1) g1_read(*reinterpret_cast<const Affine<FqU> *>(base + i * stride), reinterpret_cast<G1Affine *>(limbs)[i], inf[i]);
    else g2_read(*reinterpret_cast<const Affine<Fq2U> *>(base + i * stride), reinterpret_cast<G2Affine *>(limbs)[i], inf[i]);
}
#endif

}  // namespace pkb
}  // namespace zk
