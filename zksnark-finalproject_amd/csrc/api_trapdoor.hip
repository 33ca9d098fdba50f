// libzkg16 C ABI, part 8 of 8 (api.hip): the trapdoor route — setup-and-prove requests answered without the proving key.
// Every handler of the reference draws a trapdoor, runs circuit_specific_setup, proves once and drops the key
// (matrix_proof.rs:129-140, prime_snark.rs:112-119, fibbonaci_handler.rs:107-110, linear_equations.rs).  Whoever holds the trapdoor
// knows the discrete logs of every key point, so for a SATISFIED assignment z the proof's three logs are four dot products over the
// QAP column values at tau and a few field operations:
//   a = alpha + S_u + r delta      b = beta + S_v + s delta      c = S_l + (S_u S_v - S_w) / delta + s a + r b - r s delta
// (h(tau) Z(tau) = (sum z_k u_k)(sum z_k v_k) - sum z_k w_k for a satisfied z: the quotient is exact, Z(tau) cancels, no transform of
// the assignment is needed) and A = a G1, B = b G2, C = c G1 are the group elements the key route computes.  Affine coordinates are
// unique: the bytes are those of zkg16_setup_resident + zkg16_prove_resident.
#include <algorithm>

#include "api_internal.hpp"
#include "hostff.hpp"

using namespace zk;

namespace {
#include "trapdoor_dev.cuh"

using h64::Fr64;
Fr64 f64(const Fr &a) { return Fr64::from(a); }

// a, b, c (Montgomery) of one request from its four sums — the proof tail's 64-bit field code
void td_tail(const Fr S[4], const Fr trap[5], const Fr &dinv, const Fr &r, const Fr &s, Fr out[3]) {
    using namespace h64;
    const Fr64 Su = f64(S[0]), Sv = f64(S[1]), Sw = f64(S[2]), Sl = f64(S[3]);
    const Fr64 alpha = f64(trap[1]), beta = f64(trap[2]), delta = f64(trap[4]), r6 = f64(r), s6 = f64(s);
    const Fr64 a = add(add(alpha, Su), mul(r6, delta));
    const Fr64 b = add(add(beta, Sv), mul(s6, delta));
    Fr64 c = add(Sl, mul(sub(mul(Su, Sv), Sw), f64(dinv)));
    c = add(c, add(mul(s6, a), mul(r6, b)));
    c = sub(c, mul(mul(r6, s6), delta));
    out[0] = a.to(); out[1] = b.to(); out[2] = c.to();
}
Fr canon(const Fr &mont) { return h64::from_mont(f64(mont)).to(); }

// which trapdoor entry a call is refused for ("" = none): a zero entry (zkg16_setup refuses those too), or tau in the domain
const char *trapdoor_refusal(const Fr trap[5], int log_n) {
    static const char *const zero[5] = {"trapdoor: tau is zero", "trapdoor: alpha is zero", "trapdoor: beta is zero", "trapdoor: gamma is zero",
                                        "trapdoor: delta is zero"};
    for (int i = 0; i < 5; i++)
        if (trap[i].is_zero()) return zero[i];
    Fr zt = trap[0];
    for (int i = 0; i < log_n; i++) zt = fp_sqr(zt);
    if (zt == Fr::one()) return "trapdoor: tau lies in the evaluation domain (tau^N = 1)";
    return nullptr;
}

struct KeyOut { uint64_t *alpha_g1, *beta_g2, *gamma_g2, *delta_g2, *gamma_abc_g1; };

// requests per device pass: the three product vectors of the check and the partial sums per request within 60 % of the free HBM, at
// most 65,535 (grid.y / grid.z of the launches), lowered by option "trapdoor_pass"
size_t td_pass_size(zkg16_ctx *ctx, const R1csDev &rc, size_t chunks) {
    const size_t per = 3 * ((size_t)1 << rc.log_n) * sizeof(Fr) + chunks * 4 * sizeof(Fr) + sizeof(Fr *);
    size_t free_b = 0, total_b = 0;
    ZK_HIP(hipMemGetInfo(&free_b, &total_b));
    size_t kb = (size_t)(0.6 * (double)free_b) / per;
    if (kb > 65535) kb = 65535;
    if (ctx->opt.trapdoor_pass > 0 && (size_t)ctx->opt.trapdoor_pass < kb) kb = (size_t)ctx->opt.trapdoor_pass;
    return kb < 1 ? 1 : kb;
}

struct DrainBoth {
    zkg16_ctx *c;
    bool ok = false;
    ~DrainBoth() {
        if (ok) return;
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->wm_stream);
    }
};

// The device form on a leased lane.  Returns ZKG16_OK or ZKG16_ERR_UNSATISFIED; nothing is written unless it returns OK.
int trapdoor_device(zkg16_ctx *ctx, R1csDev &rc, WitnessDev *const *wits, size_t k, const Fr trap[5], const G1Affine &g1, const G2Affine &g2,
                    const uint64_t *r, const uint64_t *s, uint64_t *proofs_out, uint8_t *inf_out, const KeyOut &ko, float *timings_ms) {
    const double t_call = now_ms();
    const size_t nv = rc.num_variables, ni = rc.num_instance;
    const size_t chunks = (nv + TD_CHUNK - 1) / TD_CHUNK;
    float tm[5] = {0, 0, 0, 0, 0};
    EventSet evs;
    // every host buffer an asynchronous copy reads or lands in is declared before the guard, so that on an exception the guard has
    // synchronised both streams before any of them goes away
    std::vector<const Fr *> table;
    std::vector<Fr> part_h, h1, h2;
    std::vector<uint64_t> w;
    std::vector<G1Affine> o1;
    std::vector<G2Affine> o2;
    DrainBoth drain{ctx};

    // ---- the QAP at tau, once per call
    QapEval q;
    ZK_HIP(hipEventRecord(evs.ev[3], ctx->stream));
    qap_eval_run(ctx, rc, trap, q);
    ZK_HIP(hipEventRecord(evs.ev[4], ctx->stream));

    // ---- per pass: sparse product + check, dot kernel, one read-back
    const size_t kb = std::min(k, td_pass_size(ctx, rc, chunks));
    std::vector<Fr> sums(4 * k, Fr::zero());
    table.resize(kb);
    part_h.resize(kb * chunks * 4);
    DevBuf d_table(kb * sizeof(Fr *)), d_part(kb * chunks * 4 * sizeof(Fr));
    ctx->check_n_bad.assign(k, 0);
    ctx->check_first_bad.assign(k, 0);
    bool bad = false;
    for (size_t off = 0; off < k; off += kb) {
        const size_t n = std::min(kb, k - off);
        for (size_t i = 0; i < n; i++) table[i] = wits[off + i]->z.as<Fr>();
        ZK_HIP(hipMemcpyAsync(d_table.p, table.data(), n * sizeof(Fr *), hipMemcpyHostToDevice, ctx->stream));
        ctx->check_dev.ensure(2 * n * sizeof(uint64_t));
        uint64_t *res = ctx->check_dev.as<uint64_t>();
        ZK_HIP(hipEventRecord(evs.ev[0], ctx->stream));
        r1cs_check_spmv_run(ctx, rc, table[0], n > 1 ? d_table.as<const Fr *>() : nullptr, (unsigned)n, nullptr, res);
        ZK_HIP(hipEventRecord(evs.ev[1], ctx->stream));
        {
            ScopedKernelTimer kt(ctx, "trapdoor_dot_kernel", (double)nv * n);
            const TdArgs a{d_table.as<const Fr *>(), q.uvw[0].as<Fr>(), q.uvw[1].as<Fr>(), q.uvw[2].as<Fr>(), q.lg.as<Fr>(), nv, ni, d_part.as<Fr>()};
            hipLaunchKernelGGL(trapdoor_dot_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(TD_BLOCK), 0, ctx->stream, a);
            ZK_HIP(hipGetLastError());
        }
        ZK_HIP(hipEventRecord(evs.ev[2], ctx->stream));
        w.assign(2 * n, 0);
        ZK_HIP(hipMemcpyAsync(w.data(), res, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipMemcpyAsync(part_h.data(), d_part.p, n * chunks * 4 * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        if (off == 0) { ZK_HIP(hipEventElapsedTime(&ms, evs.ev[3], evs.ev[4])); tm[0] = ms; }
        ZK_HIP(hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1])); tm[1] += ms;
        ZK_HIP(hipEventElapsedTime(&ms, evs.ev[1], evs.ev[2])); tm[2] += ms;
        for (size_t i = 0; i < n; i++) {
            ctx->check_n_bad[off + i] = w[i];
            ctx->check_first_bad[off + i] = w[n + i];
            if (w[i]) bad = true;
            for (size_t c = 0; c < chunks; c++)
                for (int j = 0; j < 4; j++) sums[4 * (off + i) + j] = fp_add(sums[4 * (off + i) + j], part_h[(i * chunks + c) * 4 + j]);
        }
    }
    if (bad) {      // every pass has run: zkg16_last_check names all the failing requests
        drain.ok = true;
        return ZKG16_ERR_UNSATISFIED;
    }

    // ---- the tail on the host: 3 logs per request, canonical, behind the singles
    //   G1 scalars: lg[0 .. ni) | alpha, beta, delta, gamma | a (k) | c (k)          G2 scalars: beta, delta, gamma | b (k)
    h1.resize(4 + 2 * k);
    h2.resize(3 + k);
    h1[0] = canon(trap[1]); h1[1] = canon(trap[2]); h1[2] = canon(trap[4]); h1[3] = canon(trap[3]);
    h2[0] = h1[1]; h2[1] = h1[2]; h2[2] = h1[3];
    for (size_t i = 0; i < k; i++) {
        Fr abc[3];
        td_tail(sums.data() + 4 * i, trap, q.dinv, fr_from_abi(r + 4 * i), fr_from_abi(s + 4 * i), abc);
        h1[4 + i] = canon(abc[0]);
        h1[4 + k + i] = canon(abc[2]);
        h2[3 + i] = canon(abc[1]);
    }

    // ---- the points: one G2 pass on the second stream, one G1 pass on the main one
    const size_t n1 = ni + 4 + 2 * k, n2 = 3 + k;
    DevBuf canon1(n1 * sizeof(Fr)), canon2(n2 * sizeof(Fr)), pts1(n1 * sizeof(G1Affine)), pts2(n2 * sizeof(G2Affine));
    ZK_HIP(hipMemcpyAsync(canon1.as<Fr>() + ni, h1.data(), h1.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipMemcpyAsync(canon2.p, h2.data(), h2.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    fr_from_mont_run(ctx, q.lg.as<Fr>(), canon1.as<Fr>(), ni);
    ZK_HIP(hipEventRecord(evs.ev[0], ctx->stream));
    ZK_HIP(hipStreamWaitEvent(ctx->wm_stream, evs.ev[0], 0));
    {
        const size_t start[3] = {0, 3, n2};
        G2AffineU *ou[2] = {nullptr, nullptr};
        G2Affine *os[2] = {pts2.as<G2Affine>(), pts2.as<G2Affine>() + 3};
        StreamSwap on_second(ctx);                               // every launch helper targets ctx->stream
        fixed_base_g2_multi(ctx, g2, canon2.as<Fr>(), n2, 2, start, ou, os, false);
        ZK_HIP(hipEventRecord(evs.ev[5], ctx->stream));
    }
    {
        const size_t start[5] = {0, ni, ni + 4, ni + 4 + k, n1};
        G1AffineU *ou[4] = {nullptr, nullptr, nullptr, nullptr};
        G1Affine *os[4] = {pts1.as<G1Affine>(), pts1.as<G1Affine>() + start[1], pts1.as<G1Affine>() + start[2], pts1.as<G1Affine>() + start[3]};
        fixed_base_g1_multi(ctx, g1, canon1.as<Fr>(), n1, 4, start, ou, os, false);
    }
    ZK_HIP(hipStreamWaitEvent(ctx->stream, evs.ev[5], 0));
    ZK_HIP(hipEventRecord(evs.ev[1], ctx->stream));
    o1.resize(n1);
    o2.resize(n2);
    ZK_HIP(hipMemcpyAsync(o1.data(), pts1.p, n1 * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipMemcpyAsync(o2.data(), pts2.p, n2 * sizeof(G2Affine), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->wm_stream));
    drain.ok = true;
    {
        float ms = 0;
        ZK_HIP(hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1]));
        tm[3] = ms;
    }

    // ---- everything succeeded: write the outputs (the key outputs as zkg16_setup_resident copies them, the proofs as the tail does)
    memcpy(ko.gamma_abc_g1, o1.data(), ni * sizeof(G1Affine));
    memcpy(ko.alpha_g1, &o1[ni], sizeof(G1Affine));
    memcpy(ko.beta_g2, &o2[0], sizeof(G2Affine));
    memcpy(ko.delta_g2, &o2[1], sizeof(G2Affine));
    memcpy(ko.gamma_g2, &o2[2], sizeof(G2Affine));
    for (size_t i = 0; i < k; i++) {
        point_to_abi(o1[ni + 4 + i], proofs_out + 48 * i, inf_out + 3 * i);
        point_to_abi(o2[3 + i], proofs_out + 48 * i + 12, inf_out + 3 * i + 1);
        point_to_abi(o1[ni + 4 + k + i], proofs_out + 48 * i + 36, inf_out + 3 * i + 2);
    }
    tm[4] = (float)(now_ms() - t_call);
    if (timings_ms) memcpy(timings_ms, tm, sizeof tm);
    return ZKG16_OK;
}

void set_root_error(zkg16_ctx *root, const char *what) {
    std::lock_guard<std::mutex> lk(root->lane_mu);
    root->last_error = what;
}

}  // namespace

extern "C" {

int zkg16_prove_trapdoor_batch(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t *witness_handles, size_t k, const uint64_t trapdoor[20],
                               const uint64_t g1_gen[12], const uint64_t g2_gen[24], const uint64_t *r, const uint64_t *s, uint64_t *proofs_out,
                               uint8_t *inf_out, uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                               uint64_t *gamma_abc_g1, float *timings_ms) {
    if (!witness_handles || k == 0 || !trapdoor || !g1_gen || !g2_gen || !r || !s || !proofs_out || !inf_out || !alpha_g1 || !beta_g2 || !gamma_g2 ||
        !delta_g2 || !gamma_abc_g1)
        return ZKG16_ERR_BAD_ARG;
    ZK_LANE_BEGIN(ctx)
    Fr trap[5];
    memcpy(trap, trapdoor, sizeof trap);
    auto rc = root->r1cs.get(r1cs_handle);
    if (!rc) return ZKG16_ERR_BAD_HANDLE;
    std::vector<std::shared_ptr<WitnessDev>> refs(k);
    std::vector<WitnessDev *> wits(k);
    for (size_t i = 0; i < k; i++) {
        refs[i] = root->wits.get(witness_handles[i]);
        if (!(wits[i] = refs[i].get())) return ZKG16_ERR_BAD_HANDLE;
    }
    if (rc->prime_template) return ZKG16_ERR_UNSUPPORTED;      // no request's system: its four candidate-dependent coefficients are zero
    for (size_t i = 0; i < k; i++)
        if (wits[i]->n != rc->num_variables) return ZKG16_ERR_BAD_ARG;
    if (const char *why = trapdoor_refusal(trap, rc->log_n)) {
        set_root_error(root, why);
        return ZKG16_ERR_BAD_ARG;
    }
    const KeyOut ko{alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1};
    const int st = trapdoor_device(ctx, *rc, wits.data(), k, trap, g1_from_abi(g1_gen, 0), g2_from_abi(g2_gen, 0), r, s, proofs_out, inf_out, ko,
                                   timings_ms);
    if (st != ZKG16_OK) return st;
    ZK_LANE_END(ctx)
}

int zkg16_prove_trapdoor(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, const uint64_t trapdoor[20], const uint64_t g1_gen[12],
                         const uint64_t g2_gen[24], const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3],
                         uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24], uint64_t *gamma_abc_g1,
                         float *timings_ms) {
    return zkg16_prove_trapdoor_batch(ctx, r1cs_handle, &witness_handle, 1, trapdoor, g1_gen, g2_gen, r, s, proof_out, inf_out, alpha_g1, beta_g2,
                                      gamma_g2, delta_g2, gamma_abc_g1, timings_ms);
}

int zkg16_prove_trapdoor_host(const uint64_t *const row_ptr[3], const uint32_t *const col[3], const uint64_t *const coeff[3], size_t num_instance,
                              size_t num_constraints, size_t num_variables, const uint64_t *z, size_t k, const uint64_t trapdoor[20],
                              const uint64_t g1_gen[12], const uint64_t g2_gen[24], const uint64_t *r, const uint64_t *s, int threads,
                              uint64_t *proofs_out, uint8_t *inf_out, uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24],
                              uint64_t delta_g2[24], uint64_t *gamma_abc_g1) {
    if (!row_ptr || !col || !coeff || !z || k == 0 || !trapdoor || !g1_gen || !g2_gen || !r || !s || !proofs_out || !inf_out || !alpha_g1 ||
        !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1 || num_instance == 0 || num_variables < num_instance || threads < 0)
        return ZKG16_ERR_BAD_ARG;
    const size_t nc = num_constraints, ni = num_instance, nv = num_variables;
    int log_n = 0;
    while (((size_t)1 << log_n) < nc + ni) log_n++;
    if (log_n > 28) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    Fr trap[5];
    memcpy(trap, trapdoor, sizeof trap);
    try {
        if (const char *why = trapdoor_refusal(trap, log_n)) {
            host_last_error() = why;
            return ZKG16_ERR_BAD_ARG;
        }
        // the check is zkg16_r1cs_check_host's (it validates the CSR arrays as well)
        for (size_t q = 0; q < k; q++) {
            uint64_t n_bad = 0;
            if (const int st = zkg16_r1cs_check_host(row_ptr, col, coeff, nc, nv, z + 4 * nv * q, &n_bad, nullptr)) return st;
            if (n_bad) return ZKG16_ERR_UNSATISFIED;
        }
        using namespace h64;
        const int T = threads == 0 ? 8 : std::min(threads, 64);
        const size_t N = (size_t)1 << log_n;
        const Fr64 tau = f64(trap[0]), alpha = f64(trap[1]), beta = f64(trap[2]);
        const Fr dinv_m = fp_inv(trap[4]), ginv_m = fp_inv(trap[3]);
        const Fr64 dinv = f64(dinv_m), ginv = f64(ginv_m);
        // L_j(tau) = (Z(tau) / N) omega^j / (tau - omega^j): slices of j, one batch inversion each
        Fr64 zt = tau;
        for (int i = 0; i < log_n; i++) zt = sqr(zt);
        zt = sub(zt, Fr64::one());
        Fr n_m = Fr::zero();
        n_m.l[0] = (uint32_t)N; n_m.l[1] = (uint32_t)((uint64_t)N >> 32);
        const Fr64 scale = mul(zt, f64(fp_inv(fp_to_mont(n_m))));
        const Fr omega = fr_root_of_unity(log_n);
        std::vector<Fr64> L(N);
        {
            ThreadGroup tg;
            const size_t per = (N + T - 1) / T;
            for (int t = 0; t < T; t++) {
                const size_t lo = std::min(N, per * t), hi = std::min(N, lo + per);
                if (lo == hi) continue;
                tg.run([&, lo, hi] {
                    const Fr64 om = f64(omega);
                    std::vector<Fr64> w(hi - lo), pre(hi - lo);
                    Fr64 cur = f64(fp_pow_u64(omega, lo)), acc = Fr64::one();
                    for (size_t j = lo; j < hi; j++) {
                        w[j - lo] = cur;
                        pre[j - lo] = acc;
                        acc = mul(acc, sub(tau, cur));       // never zero: tau^N != 1
                        cur = mul(cur, om);
                    }
                    Fr64 iv = inv(acc);
                    for (size_t j = hi; j-- > lo;) {
                        const Fr64 d = mul(iv, pre[j - lo]);      // 1 / (tau - omega^j)
                        iv = mul(iv, sub(tau, w[j - lo]));
                        L[j] = mul(mul(scale, w[j - lo]), d);
                    }
                });
            }
        }
        // u, v, w: column sums by a plain loop over the CSR arrays, one thread per matrix
        std::vector<Fr64> uvw[3];
        {
            ThreadGroup tg;
            for (int m = 0; m < 3; m++)
                tg.run([&, m] {
                    std::vector<Fr64> &o = uvw[m];
                    o.assign(nv, Fr64::zero());
                    for (size_t i = 0; i < nc; i++)
                        for (uint64_t e = row_ptr[m][i]; e < row_ptr[m][i + 1]; e++)
                            o[col[m][e]] = add(o[col[m][e]], mul(f64(fr_from_abi(coeff[m] + 4 * e)), L[i]));
                    if (m == 0)
                        for (size_t j = 0; j < ni; j++) o[j] = add(o[j], L[nc + j]);
                });
        }
        std::vector<Fr64> lg(nv);
        for (size_t j = 0; j < nv; j++)
            lg[j] = mul(add(add(mul(beta, uvw[0][j]), mul(alpha, uvw[1][j])), uvw[2][j]), j < ni ? ginv : dinv);
        // a, b, c of every request
        std::vector<Fr> abc(3 * k);
        for (size_t q = 0; q < k; q++) {
            const uint64_t *zq = z + 4 * nv * q;
            Fr64 S[4] = {Fr64::zero(), Fr64::zero(), Fr64::zero(), Fr64::zero()};
            for (size_t j = 0; j < nv; j++) {
                const Fr64 zj = f64(fr_from_abi(zq + 4 * j));
                S[0] = add(S[0], mul(zj, uvw[0][j]));
                S[1] = add(S[1], mul(zj, uvw[1][j]));
                S[2] = add(S[2], mul(zj, uvw[2][j]));
                if (j >= ni) S[3] = add(S[3], mul(zj, lg[j]));
            }
            const Fr Sm[4] = {S[0].to(), S[1].to(), S[2].to(), S[3].to()};
            td_tail(Sm, trap, dinv_m, fr_from_abi(r + 4 * q), fr_from_abi(s + 4 * q), abc.data() + 3 * q);
        }
        // points by the host scalar multiplication, dealt round-robin to the threads: gamma_abc (ni) | alpha (G1) | beta, delta, gamma (G2) |
        // A, B, C per request
        const G1Affine g1 = g1_from_abi(g1_gen, 0);
        const G2Affine g2 = g2_from_abi(g2_gen, 0);
        const size_t tasks = ni + 4 + 3 * k;
        std::vector<G1Affine> gabc(ni), pa(k), pc(k);
        std::vector<G2Affine> pb(k);
        G1Affine alpha_p;
        G2Affine key2[3];
        const auto mul1 = [&](const Fr &mont) { return xyzz_to_affine(xyzz_mul(G1XYZZ::from_affine(g1), canon(mont).l)); };
        const auto mul2 = [&](const Fr &mont) { return xyzz_to_affine(xyzz_mul(G2XYZZ::from_affine(g2), canon(mont).l)); };
        {
            ThreadGroup tg;
            for (int t = 0; t < T; t++)
                tg.run([&, t] {
                    for (size_t i = (size_t)t; i < tasks; i += (size_t)T) {
                        if (i < ni) gabc[i] = mul1(lg[i].to());
                        else if (i == ni) alpha_p = mul1(trap[1]);
                        else if (i < ni + 4) key2[i - ni - 1] = mul2(trap[i - ni == 1 ? 2 : i - ni == 2 ? 4 : 3]);      // beta, delta, gamma
                        else {
                            const size_t q = (i - ni - 4) / 3, what = (i - ni - 4) % 3;
                            if (what == 0) pa[q] = mul1(abc[3 * q]);
                            else if (what == 1) pb[q] = mul2(abc[3 * q + 1]);
                            else pc[q] = mul1(abc[3 * q + 2]);
                        }
                    }
                });
        }
        memcpy(gamma_abc_g1, gabc.data(), ni * sizeof(G1Affine));
        memcpy(alpha_g1, &alpha_p, sizeof alpha_p);
        memcpy(beta_g2, &key2[0], sizeof(G2Affine));
        memcpy(delta_g2, &key2[1], sizeof(G2Affine));
        memcpy(gamma_g2, &key2[2], sizeof(G2Affine));
        for (size_t q = 0; q < k; q++) {
            point_to_abi(pa[q], proofs_out + 48 * q, inf_out + 3 * q);
            point_to_abi(pb[q], proofs_out + 48 * q + 12, inf_out + 3 * q + 1);
            point_to_abi(pc[q], proofs_out + 48 * q + 36, inf_out + 3 * q + 2);
        }
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

}  // extern "C"
