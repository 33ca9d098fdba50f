// TEST-ONLY: csrc/pairing_each_dev.cuh (what the per-proof kernels of verify_batch.hip run, one GPU lane per proof) compiled for the
// host beside the host verifier's arithmetic (csrc/pairing_fast.inc), so that each operation can be compared limb for limb on a
// machine without a GPU.  Built by tests/test_verify_each_host.py with `hipcc --offload-host-only`; ZK_PD_CHECK turns on the value-
// bound assertions of both device headers.  Every value crosses this interface in saturated Montgomery limbs (u64, ark's order).
#define ZK_PD_CHECK 1
#include "ff.cuh"
#include "ec.cuh"
#include "pairing_dev.cuh"
#include "pairing_each_dev.cuh"
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
pf::F6 h6(const uint64_t *p) { return pf::F6{h2(p), h2(p + 12), h2(p + 24)}; }
void h6_st(uint64_t *p, const pf::F6 &r) { h2_st(p, r.a0); h2_st(p + 12, r.a1); h2_st(p + 24, r.a2); }
pd::F6 d6(const uint64_t *p) { return pd::F6{d2(p), d2(p + 12), d2(p + 24)}; }
void d6_st(uint64_t *p, const pd::F6 &r) { d2_st(p, r.a0); d2_st(p + 12, r.a1); d2_st(p + 24, r.a2); }
pf::F12 h12(const uint64_t *p) { return pf::F12{h6(p), h6(p + 36)}; }
void h12_st(uint64_t *p, const pf::F12 &r) { h6_st(p, r.c0); h6_st(p + 36, r.c1); }
pd::F12 d12(const uint64_t *p) { Fq2 s[6]; memcpy(s, p, sizeof s); return pd::f12_from_sat(s); }
void d12_st(uint64_t *p, const pd::F12 &r) { Fq2 s[6]; pd::f12_to_sat(r, s); memcpy(p, s, sizeof s); }

// the Frobenius constants as the library hands them to the kernels: the host's, through saturated limbs
pd::Frob frob_dev() {
    const pf::Frob &f = pf::frob_coeffs();
    pd::Frob r;
    for (int i = 0; i < 5; i++) r.g[i] = fq2u_from_sat(pf::to_sat(f.g[i + 1]));
    return r;
}
std::vector<pd::Ell> ell_dev(const uint64_t *coeffs) {
    std::vector<pd::Ell> e(68);
    for (size_t i = 0; i < 68; i++) e[i] = pd::Ell{d2(coeffs + 36 * i), d2(coeffs + 36 * i + 12), d2(coeffs + 36 * i + 24)};
    return e;
}
pf::Prepared ell_host(const uint64_t *coeffs) {
    pf::Prepared p;
    p.infinity = false;
    p.ell.resize(68);
    for (size_t i = 0; i < 68; i++) p.ell[i] = pf::Ell{h2(coeffs + 36 * i), h2(coeffs + 36 * i + 12), h2(coeffs + 36 * i + 24)};
    return p;
}
pf::PairIn pair_host(const uint64_t *g1, const pf::Prepared *q) {
    G1Affine p; memcpy(&p, g1, sizeof p);
    return pf::PairIn{pf::Fq64::from(p.x), pf::Fq64::from(p.y), q};
}
pd::PreparedPair pair_dev(const uint64_t *g1, const pd::Ell *e) {
    G1Affine p; memcpy(&p, g1, sizeof p);
    return pd::PreparedPair{fqu_from_sat(p.x), fqu_from_sat(p.y), e};
}
std::vector<Affine<FqU>> gabc_dev(const uint64_t *gamma_abc, size_t ni) {
    std::vector<Affine<FqU>> g(ni);
    for (size_t i = 0; i < ni; i++) {
        G1Affine p; memcpy(&p, gamma_abc + 12 * i, sizeof p);
        g[i] = Affine<FqU>{fqu_from_sat(p.x), fqu_from_sat(p.y)};
    }
    return g;
}
std::vector<uint64_t> canonical(const uint64_t *mont, size_t n) {
    std::vector<uint64_t> out(4 * n + 4);
    for (size_t i = 0; i < n; i++) {
        Fr z; memcpy(&z, mont + 4 * i, sizeof z);
        const Fr c = fp_from_mont(z);
        memcpy(out.data() + 4 * i, c.l, 32);
    }
    return out;
}
}  // namespace

extern "C" {

// a^-1 at tower level 2, 6 or 12 (12 / 36 / 72 u64); the inverse of zero is zero on both sides
void ve_inv(int level, const uint64_t *a, uint64_t *out_dev, uint64_t *out_host) {
    if (level == 2) { d2_st(out_dev, pd::inv(d2(a))); h2_st(out_host, pf::inv(h2(a))); }
    else if (level == 6) { d6_st(out_dev, pd::inv(d6(a))); h6_st(out_host, pf::inv(h6(a))); }
    else { d12_st(out_dev, pd::inv(d12(a))); h12_st(out_host, pf::inv(h12(a))); }
}
// a b at tower level 2, 6 or 12 by the device header alone (for a a^-1 == 1)
void ve_mul(int level, const uint64_t *a, const uint64_t *b, uint64_t *out_dev) {
    if (level == 2) d2_st(out_dev, pd::tidy(pd::mul(d2(a), d2(b))));
    else if (level == 6) d6_st(out_dev, pd::tidy(pd::mul(d6(a), d6(b))));
    else d12_st(out_dev, pd::mul(d12(a), d12(b)));
}
// op 0: a^q, 1: a^(q^2), 2: the cyclotomic squaring, 3: a^z, 4: the final exponentiation, 5: the easy part a^((q^6 - 1)(q^2 + 1))
// (device header alone twice: an element of the cyclotomic subgroup for ops 2 and 3), 6: the plain square
void ve_f12_op(int op, const uint64_t *a, uint64_t *out_dev, uint64_t *out_host) {
    const pd::F12 x = d12(a);
    const pf::F12 hx = h12(a);
    const pd::Frob fr = frob_dev();
    switch (op) {
        case 0: d12_st(out_dev, pd::frob(x, 1, fr)); h12_st(out_host, pf::frob(hx, 1)); break;
        case 1: d12_st(out_dev, pd::frob(x, 2, fr)); h12_st(out_host, pf::frob(hx, 2)); break;
        case 2: d12_st(out_dev, pd::cyclotomic_sqr(x)); h12_st(out_host, pf::cyclotomic_sqr(hx)); break;
        case 3: d12_st(out_dev, pd::pow_z(x)); h12_st(out_host, pf::pow_z(hx)); break;
        case 4: d12_st(out_dev, pd::final_exp(x, fr)); h12_st(out_host, pf::final_exp(hx)); break;
        case 5: {
            const pd::F12 f1 = pd::mul(pd::conj(x), pd::inv(x));
            d12_st(out_dev, pd::mul(pd::frob(f1, 2, fr), f1));
            const pf::F12 g1 = pf::mul(pf::conj(hx), pf::inv(hx));
            h12_st(out_host, pf::mul(pf::frob(g1, 2), g1));
            break;
        }
        default: d12_st(out_dev, pd::sqr(x)); h12_st(out_host, pf::sqr(hx)); break;
    }
}
// the Miller loop of the prepared pairs (p0, coeffs0) and, when np == 2, (p1, coeffs1): device header and pf::miller_loop
void ve_miller_prepared(int np, const uint64_t *p0, const uint64_t *coeffs0, const uint64_t *p1, const uint64_t *coeffs1, uint64_t *out_dev, uint64_t *out_host) {
    const std::vector<pd::Ell> e0 = ell_dev(coeffs0), e1 = ell_dev(np == 2 ? coeffs1 : coeffs0);
    const pf::Prepared q0 = ell_host(coeffs0), q1 = ell_host(np == 2 ? coeffs1 : coeffs0);
    pd::PreparedPair pr[2] = {pair_dev(p0, e0.data()), pair_dev(np == 2 ? p1 : p0, np == 2 ? e1.data() : nullptr)};
    d12_st(out_dev, pd::multi_miller_loop(false, FqU::zero(), FqU::zero(), pd::F2::zero(), pd::F2::zero(), pr, 2));
    std::vector<pf::PairIn> in{pair_host(p0, &q0)};
    if (np == 2) in.push_back(pair_host(p1, &q1));
    h12_st(out_host, pf::miller_loop(in));
}
// the three pairs (a, b unprepared), (x, coeffs_g), (c, coeffs_d): out_shared = the device header's shared-squaring loop,
// out_separate = the device header's product of the three loops run apart, out_host = pf::miller_loop of the three with b prepared
void ve_miller_three(const uint64_t *a, const uint64_t *b, const uint64_t *x, const uint64_t *coeffs_g, const uint64_t *c, const uint64_t *coeffs_d,
                     uint64_t *out_shared, uint64_t *out_separate, uint64_t *out_host) {
    G1Affine as; memcpy(&as, a, sizeof as);
    G2Affine bs; memcpy(&bs, b, sizeof bs);
    const FqU ax = fqu_from_sat(as.x), ay = fqu_from_sat(as.y);
    const pd::F2 bx = fq2u_from_sat(bs.x), by = fq2u_from_sat(bs.y);
    const std::vector<pd::Ell> eg = ell_dev(coeffs_g), ed = ell_dev(coeffs_d);
    pd::PreparedPair pr[2] = {pair_dev(x, eg.data()), pair_dev(c, ed.data())};
    d12_st(out_shared, pd::multi_miller_loop(true, ax, ay, bx, by, pr, 2));
    pd::PreparedPair only_x[2] = {pr[0], pd::PreparedPair{FqU::zero(), FqU::zero(), nullptr}}, only_c[2] = {pd::PreparedPair{FqU::zero(), FqU::zero(), nullptr}, pr[1]};
    const pd::F12 fx = pd::multi_miller_loop(false, ax, ay, bx, by, only_x, 2), fc = pd::multi_miller_loop(false, ax, ay, bx, by, only_c, 2);
    d12_st(out_separate, pd::mul(pd::mul(pd::miller_loop(ax, ay, bx, by), fx), fc));
    const pf::Prepared qb = pf::prepare(bs), qg = ell_host(coeffs_g), qd = ell_host(coeffs_d);
    h12_st(out_host, pf::miller_loop({pair_host(a, &qb), pair_host(x, &qg), pair_host(c, &qd)}));
}
// gamma_abc[0] + sum z_i gamma_abc[i] (public inputs in Montgomery form, as the ABI takes them): the device header and the body of
// zkg16_verify_prepared's prepared_inputs (verify.hip) restated on pairing_fast.inc.  Returns 0 when both say infinity, 1 when both
// give a point (out_*: 12 u64), -1 when they disagree about infinity
int ve_prepared_input(const uint64_t *gamma_abc, size_t ni, const uint64_t *public_inputs, uint64_t *out_dev, uint64_t *out_host) {
    const std::vector<Affine<FqU>> g = gabc_dev(gamma_abc, ni);
    const std::vector<uint64_t> z = canonical(public_inputs, ni - 1);
    FqU ox = FqU::zero(), oy = FqU::zero();
    const bool have = pd::prepared_input(g.data(), ni, z.data(), ox, oy);
    auto pt = [&](size_t i) {
        G1Affine p; memcpy(&p, gamma_abc + 12 * i, sizeof p);
        return p.is_inf() ? pf::pt_inf<pf::Fq64>() : pf::g1_pt(p);
    };
    pf::Pt<pf::Fq64> acc = pt(0);
    for (size_t i = 1; i < ni; i++) {
        const uint64_t *k = z.data() + 4 * (i - 1);
        if (!(k[0] | k[1] | k[2] | k[3])) continue;
        acc = pf::pt_add(acc, pf::pt_mul(pt(i), k, 4));
    }
    if (have == acc.inf) return -1;
    if (!have) return 0;
    const G1Affine o{fqu_to_sat(ox), fqu_to_sat(oy)};
    memcpy(out_dev, &o, sizeof o);
    const pf::Fq64 inv = zk::h64::inv(zk::h64::mul(acc.zz, acc.zzz));
    const G1Affine ho{zk::h64::mul(acc.x, zk::h64::mul(inv, acc.zzz)).to(), zk::h64::mul(acc.y, zk::h64::mul(inv, acc.zz)).to()};
    memcpy(out_host, &ho, sizeof ho);
    return 1;
}
// one proof as a GPU lane decides it: the device header's membership tests of A, B, C (what the membership kernel runs; a flagged
// point passes) and then pd::verify_one.  1 = the proof holds
int ve_verify_one(const uint64_t *gamma_abc, size_t ni, const uint64_t *public_inputs, const uint64_t *alpha_beta, const uint64_t *coeffs_g,
                  const uint64_t *coeffs_d, const uint64_t *proof, const uint8_t *inf) {
    const pf::Endo &en = pf::endo();
    const FqU beta = fqu_from_sat(en.beta.to());
    const pd::F2 cx = fq2u_from_sat(pf::to_sat(en.cx)), cy = fq2u_from_sat(pf::to_sat(en.cy));
    G1Affine a, c; memcpy(&a, proof, sizeof a); memcpy(&c, proof + 36, sizeof c);
    G2Affine b; memcpy(&b, proof + 12, sizeof b);
    if (!inf[0] && !pd::g1_valid(a, beta, en.fast_g1)) return 0;
    if (!inf[1] && !pd::g2_valid(b, cx, cy, en.fast_g2)) return 0;
    if (!inf[2] && !pd::g1_valid(c, beta, en.fast_g1)) return 0;
    const std::vector<Affine<FqU>> g = gabc_dev(gamma_abc, ni);
    const std::vector<uint64_t> z = canonical(public_inputs, ni - 1);
    const std::vector<pd::Ell> eg = ell_dev(coeffs_g), ed = ell_dev(coeffs_d);
    Fq2 ab[6];
    memcpy(ab, alpha_beta, sizeof ab);
    const pd::EachKey key{eg.data(), ed.data(), ab};
    return pd::verify_one(proof, inf, g.data(), ni, z.data(), key, frob_dev()) ? 1 : 0;
}

}  // extern "C"
