// TEST-ONLY: the device pairing header (csrc/pairing_dev.cuh — what verify_batch.hip's kernels run, one GPU lane per pair) compiled
// for the host beside the host verifier's arithmetic (csrc/pairing_fast.inc), so that each operation can be compared limb for limb
// on a machine without a GPU.  Built by tests/test_verify_batch.py with `hipcc --offload-host-only`; ZK_PD_CHECK turns on the
// header's value-bound assertions.  Every value crosses this interface in saturated Montgomery limbs (u64, ark's order).
#define ZK_PD_CHECK 1
#include "ff.cuh"
#include "ec.cuh"
#include "pairing_dev.cuh"
#include "hostff.hpp"
#include <string.h>
#include <vector>
using namespace zk;

namespace {
#include "final_exp.inc"
const uint64_t Z_ABS = 0xd201000000010000ULL;
struct Fq12 { Fq2 c[6]; };
#include "pairing_fast.inc"

pf::F2 h2(const uint64_t *p) { Fq2 s; memcpy(&s, p, sizeof s); return pf::from_sat(s); }
void h2_st(uint64_t *p, const pf::F2 &v) { const Fq2 s = pf::to_sat(v); memcpy(p, &s, sizeof s); }
pd::F2 d2(const uint64_t *p) { Fq2 s; memcpy(&s, p, sizeof s); return fq2u_from_sat(s); }
void d2_st(uint64_t *p, const pd::F2 &v) { const Fq2 s = fq2u_to_sat(v); memcpy(p, &s, sizeof s); }
pf::F12 h12(const uint64_t *p) {
    pf::F12 r;
    r.c0.a0 = h2(p); r.c0.a1 = h2(p + 12); r.c0.a2 = h2(p + 24); r.c1.a0 = h2(p + 36); r.c1.a1 = h2(p + 48); r.c1.a2 = h2(p + 60);
    return r;
}
void h12_st(uint64_t *p, const pf::F12 &r) {
    h2_st(p, r.c0.a0); h2_st(p + 12, r.c0.a1); h2_st(p + 24, r.c0.a2); h2_st(p + 36, r.c1.a0); h2_st(p + 48, r.c1.a1); h2_st(p + 60, r.c1.a2);
}
pd::F12 d12(const uint64_t *p) { Fq2 s[6]; memcpy(s, p, sizeof s); return pd::f12_from_sat(s); }
void d12_st(uint64_t *p, const pd::F12 &r) { Fq2 s[6]; pd::f12_to_sat(r, s); memcpy(p, s, sizeof s); }
}  // namespace

extern "C" {

// op 0: a b, 1: a^2, 2: a (l0 + l1 v + l4 v w) with (l0, l1, l4) = the first three Fq2 of b, 3: conj(a)
void pd_f12_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out_dev, uint64_t *out_host) {
    const pd::F12 x = d12(a), y = d12(b);
    const pf::F12 hx = h12(a), hy = h12(b);
    switch (op) {
        case 0: d12_st(out_dev, pd::mul(x, y)); h12_st(out_host, pf::mul(hx, hy)); break;
        case 1: d12_st(out_dev, pd::sqr(x)); h12_st(out_host, pf::sqr(hx)); break;
        case 2: d12_st(out_dev, pd::mul_by_014(x, d2(b), d2(b + 12), d2(b + 24))); h12_st(out_host, pf::mul_by_014(hx, h2(b), h2(b + 12), h2(b + 24))); break;
        default: d12_st(out_dev, pd::conj(x)); h12_st(out_host, pf::conj(hx)); break;
    }
}
// one line step on T = (x, y, z) (36 u64), add = 0: the doubling, 1: the addition of q (24 u64).  Outputs: T' (36) and the three
// line coefficients (36), device header and pairing_fast.inc
void pd_line_step(int add, const uint64_t *t, const uint64_t *q, uint64_t *t_dev, uint64_t *ell_dev, uint64_t *t_host, uint64_t *ell_host) {
    pd::P2 dt{d2(t), d2(t + 12), d2(t + 24)};
    pf::P2 ht{h2(t), h2(t + 12), h2(t + 24)};
    const pd::Ell de = add ? pd::ark_add(dt, d2(q), d2(q + 12)) : pd::ark_double(dt, pd::consts());
    const pf::Ell he = add ? pf::ark_add(ht, h2(q), h2(q + 12)) : pf::ark_double(ht);
    d2_st(t_dev, dt.x); d2_st(t_dev + 12, dt.y); d2_st(t_dev + 24, dt.z);
    d2_st(ell_dev, de.c0); d2_st(ell_dev + 12, de.c1); d2_st(ell_dev + 24, de.c2);
    h2_st(t_host, ht.x); h2_st(t_host + 12, ht.y); h2_st(t_host + 24, ht.z);
    h2_st(ell_host, he.c0); h2_st(ell_host + 12, he.c1); h2_st(ell_host + 24, he.c2);
}
// the whole Miller loop of (p, q), neither at infinity
void pd_miller(const uint64_t *p, const uint64_t *q, uint64_t *out_dev, uint64_t *out_host) {
    G1Affine ps; memcpy(&ps, p, sizeof ps);
    G2Affine qs; memcpy(&qs, q, sizeof qs);
    d12_st(out_dev, pd::miller_loop(fqu_from_sat(ps.x), fqu_from_sat(ps.y), fq2u_from_sat(qs.x), fq2u_from_sat(qs.y)));
    const pf::Prepared prep = pf::prepare(qs);
    h12_st(out_host, pf::miller_loop({pf::PairIn{pf::Fq64::from(ps.x), pf::Fq64::from(ps.y), &prep}}));
}
// curve + subgroup membership of an affine point (group 1: 12 u64, 2: 24 u64).  fast = 0 runs the plain [r] P ladder of the device
// header.  Bit 0 of the result: the device header's verdict, bit 1: pairing_fast.inc's endomorphism test behind the curve
// equation, bit 2: the calibration of the constants succeeded
int pd_member(int group, const uint64_t *pt, int fast) {
    const pf::Endo &en = pf::endo();
    int r = 0;
    if (group == 1) {
        G1Affine p; memcpy(&p, pt, sizeof p);
        Fq four = Fq::zero();
        four.l[0] = 4;
        const bool on = fp_sqr(p.y) == fp_add(fp_mul(fp_sqr(p.x), p.x), fp_to_mont(four));
        if (pd::g1_valid(p, fqu_from_sat(en.beta.to()), fast != 0)) r |= 1;
        if (on && pf::g1_endo_test(pf::g1_pt(p), en.beta)) r |= 2;
        if (en.fast_g1) r |= 4;
    } else {
        G2Affine p; memcpy(&p, pt, sizeof p);
        Fq four = Fq::zero();
        four.l[0] = 4;
        const Fq fm = fp_to_mont(four);
        const bool on = f_sqr(p.y) == f_add(f_mul(f_sqr(p.x), p.x), Fq2{fm, fm});
        if (pd::g2_valid(p, fq2u_from_sat(pf::to_sat(en.cx)), fq2u_from_sat(pf::to_sat(en.cy)), fast != 0)) r |= 1;
        if (on && pf::g2_endo_test(pf::g2_pt(p), en.cx, en.cy)) r |= 2;
        if (en.fast_g2) r |= 4;
    }
    return r;
}
// [k] p for a 128-bit k (2 u64): device header and the host's pt_mul; returns 0 when both say infinity, 1 when both give a point
// (out_*: 12 u64 each), -1 when they disagree about infinity
int pd_scale128(const uint64_t *p, const uint64_t *k, uint64_t *out_dev, uint64_t *out_host) {
    G1Affine ps; memcpy(&ps, p, sizeof ps);
    uint32_t k32[4];
    memcpy(k32, k, sizeof k32);
    FqU ox, oy;
    const bool have = pd::g1_scale128(fqu_from_sat(ps.x), fqu_from_sat(ps.y), k32, ox, oy);
    const pf::Pt<pf::Fq64> hp = pf::pt_mul(pf::g1_pt(ps), k, 2);
    if (have == hp.inf) return -1;
    if (!have) return 0;
    const G1Affine o{fqu_to_sat(ox), fqu_to_sat(oy)};
    memcpy(out_dev, &o, sizeof o);
    const pf::Fq64 inv = zk::h64::inv(zk::h64::mul(hp.zz, hp.zzz));
    const G1Affine ho{zk::h64::mul(hp.x, zk::h64::mul(inv, hp.zzz)).to(), zk::h64::mul(hp.y, zk::h64::mul(inv, hp.zz)).to()};
    memcpy(out_host, &ho, sizeof ho);
    return 1;
}

}  // extern "C"
