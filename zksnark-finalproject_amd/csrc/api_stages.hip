// libzkg16 C ABI, part 4 of 6 (api.hip): key generation from a known trapdoor and the stage entry points (NTT, MSM, witness map,
// fixed-base batches) with their stand-alone benchmarks.
#include "api_internal.hpp"

using namespace zk;
extern "C" {

int zkg16_setup(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t trapdoor[20], const uint64_t g1_gen[12], const uint64_t g2_gen[24],
                uint64_t *a_query, uint8_t *a_inf, uint64_t *b_g1_query, uint8_t *b_g1_inf, uint64_t *b_g2_query, uint8_t *b_g2_inf,
                uint64_t *h_query, uint64_t *l_query, uint8_t *l_inf,
                uint64_t alpha_g1[12], uint64_t beta_g1[12], uint64_t beta_g2[24], uint64_t delta_g1[12], uint64_t delta_g2[24],
                uint64_t gamma_g2[24], uint64_t *gamma_abc_g1) {
    if (!trapdoor || !g1_gen || !g2_gen || !a_query || !b_g1_query || !b_g2_query || !h_query || !l_query || !alpha_g1 || !beta_g1 || !beta_g2 ||
        !delta_g1 || !delta_g2 || !gamma_g2 || !gamma_abc_g1)
        return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto rc_ref = ctx->r1cs.get(r1cs_handle); R1csDev *rc = rc_ref.get();
    if (!rc) return ZKG16_ERR_BAD_HANDLE;
    Fr trap[5];
    memcpy(trap, trapdoor, sizeof trap);
    for (int i = 0; i < 5; i++)
        if (trap[i].is_zero()) return ZKG16_ERR_BAD_ARG;
    SetupOut o{a_query, b_g1_query, b_g2_query, h_query, l_query, gamma_abc_g1, a_inf, b_g1_inf, b_g2_inf, l_inf,
               alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, gamma_g2};
    setup_run(ctx, *rc, trap, g1_from_abi(g1_gen, 0), g2_from_abi(g2_gen, 0), o);
    ZK_API_END(ctx)
}

int zkg16_setup_resident(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t trapdoor[20], const uint64_t g1_gen[12], const uint64_t g2_gen[24],
                         uint64_t *pk_handle, uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                         uint64_t *gamma_abc_g1) {
    if (!trapdoor || !g1_gen || !g2_gen || !pk_handle || !alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto rc_ref = ctx->r1cs.get(r1cs_handle); R1csDev *rc = rc_ref.get();
    if (!rc) return ZKG16_ERR_BAD_HANDLE;
    Fr trap[5];
    memcpy(trap, trapdoor, sizeof trap);
    for (int i = 0; i < 5; i++)
        if (trap[i].is_zero()) return ZKG16_ERR_BAD_ARG;
    auto pk = std::make_unique<PkDev>();
    uint64_t beta_g1[12], delta_g1[12];
    SetupOut o{nullptr, nullptr, nullptr, nullptr, nullptr, gamma_abc_g1, nullptr, nullptr, nullptr, nullptr,
               alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, gamma_g2};
    setup_run(ctx, *rc, trap, g1_from_abi(g1_gen, 0), g2_from_abi(g2_gen, 0), o, pk.get());
    *pk_handle = ctx->next_handle++;
    ctx->pks.put(*pk_handle, std::move(pk));
    ZK_API_END(ctx)
}

// ------------------------------------------------------------------------------------------------ stages
int zkg16_ntt(zkg16_ctx *ctx, uint64_t *data, size_t log_n, int inverse, int coset) {
    if (!data) return ZKG16_ERR_BAD_ARG;
    if (log_n > 32) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    if (log_n > 28) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    ZK_API_BEGIN(ctx)
    const size_t n = (size_t)1 << log_n;
    DevBuf d(n * sizeof(Fr)), t(n * sizeof(Fr));
    ZK_HIP(hipMemcpyAsync(d.p, data, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    const Fr *res = ntt_run(ctx, d.as<Fr>(), t.as<Fr>(), (int)log_n, inverse != 0, coset != 0);
    ZK_HIP(hipMemcpyAsync(data, res, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_API_END(ctx)
}

int zkg16_bench_ntt(zkg16_ctx *ctx, size_t log_n, int inverse, int coset, int iters, float *ms_per_iter) {
    if (!ms_per_iter || iters < 1) return ZKG16_ERR_BAD_ARG;
    if (log_n > 28) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    ZK_API_BEGIN(ctx)
    const size_t n = (size_t)1 << log_n;
    DevBuf d(n * sizeof(Fr)), t(n * sizeof(Fr));
    ZK_HIP(hipMemsetAsync(d.p, 0x5a, n * sizeof(Fr), ctx->stream));       // arbitrary (unreduced) limbs: timing only
    (void)ntt_get_tables(ctx, (int)log_n);
    ntt_run(ctx, d.as<Fr>(), t.as<Fr>(), (int)log_n, inverse != 0, coset != 0);
    hipEvent_t e0, e1;
    ZK_HIP(hipEventCreate(&e0));
    ZK_HIP(hipEventCreate(&e1));
    ZK_HIP(hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters; i++) {      // ping-pong, as the witness map does
        if (i & 1) ntt_run(ctx, t.as<Fr>(), d.as<Fr>(), (int)log_n, inverse != 0, coset != 0);
        else ntt_run(ctx, d.as<Fr>(), t.as<Fr>(), (int)log_n, inverse != 0, coset != 0);
    }
    ZK_HIP(hipEventRecord(e1, ctx->stream));
    ZK_HIP(hipEventSynchronize(e1));
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_iter = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ZK_API_END(ctx)
}

// the whole R1CS -> QAP witness map (3 SpMV + 7 NTT + point-wise) alone on the device, repeated: stand-alone time per config
int zkg16_bench_witness_map(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, int iters, float *ms_per_iter) {
    if (!ms_per_iter || iters < 1) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto rc_ref = ctx->r1cs.get(r1cs_handle); R1csDev *rc = rc_ref.get();
    auto wit_ref = ctx->wits.get(witness_handle); WitnessDev *wit = wit_ref.get();
    if (!rc || !wit) return ZKG16_ERR_BAD_HANDLE;
    if (wit->n != rc->num_variables) return ZKG16_ERR_BAD_ARG;
    Fr *h = nullptr;
    witness_map_run(ctx, *rc, wit->z.as<Fr>(), &h);
    EventSet evs;
    ZK_HIP(hipEventRecord(evs.ev[0], ctx->stream));
    for (int i = 0; i < iters; i++) witness_map_run(ctx, *rc, wit->z.as<Fr>(), &h);
    ZK_HIP(hipEventRecord(evs.ev[1], ctx->stream));
    ZK_HIP(hipEventSynchronize(evs.ev[1]));
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1]));
    *ms_per_iter = ms / iters;
    ZK_API_END(ctx)
}

}  // extern "C"

namespace {

template <class A, class X>
int msm_host_entry(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars, size_t n, int iters,
                   float *ms_per_iter, uint64_t *out_affine, uint8_t *out_inf, bool g2) {
    if ((!bases || !scalars) && n) return ZKG16_ERR_BAD_ARG;
    if (!out_affine) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    DevBuf d_bases((n ? n : 1) * sizeof(typename UOf<A>::T)), d_sc((n ? n : 1) * sizeof(Fr));
    if (n) {
        upload_points<A>(ctx, d_bases.as<typename UOf<A>::T>(), bases, inf, 0, n);
        ZK_HIP(hipMemcpyAsync(d_sc.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
    }
    X total = X::inf();
    double ms_sum = 0;
    for (int it = 0; it < (iters < 1 ? 1 : iters); it++) {
        const double t0 = now_ms();
        MsmPlan plan;
        msm_plan_build(ctx, ctx->ws_h, d_sc.as<Fr>(), n, plan);
        if constexpr (sizeof(A) == sizeof(G1Affine)) total = msm_g1_exec(ctx, ctx->ws_h, plan, d_bases.as<G1AffineU>(), "msm");
        else total = msm_g2_exec(ctx, ctx->ws_h, plan, d_bases.as<G2AffineU>(), "msm");
        ms_sum += now_ms() - t0;
    }
    if (ms_per_iter) *ms_per_iter = (float)(ms_sum / (iters < 1 ? 1 : iters));
    ctx->last_msm_group = g2 ? 2 : 1;
    point_to_abi(xyzz_to_affine(total), out_affine, out_inf);
    ZK_API_END(ctx)
}

}  // namespace

extern "C" {

int zkg16_msm_g1(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical, size_t n,
                 uint64_t out_affine[12], uint8_t *out_inf) {
    return msm_host_entry<G1Affine, G1XYZZ>(ctx, bases, inf, scalars_canonical, n, 1, nullptr, out_affine, out_inf, false);
}
int zkg16_msm_g2(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical, size_t n,
                 uint64_t out_affine[24], uint8_t *out_inf) {
    return msm_host_entry<G2Affine, G2XYZZ>(ctx, bases, inf, scalars_canonical, n, 1, nullptr, out_affine, out_inf, true);
}
int zkg16_bench_msm(zkg16_ctx *ctx, int group, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical,
                    size_t n, int iters, float *ms_per_iter, uint64_t *out_affine, uint8_t *out_inf) {
    if (group == 1) return msm_host_entry<G1Affine, G1XYZZ>(ctx, bases, inf, scalars_canonical, n, iters, ms_per_iter, out_affine, out_inf, false);
    if (group == 2) return msm_host_entry<G2Affine, G2XYZZ>(ctx, bases, inf, scalars_canonical, n, iters, ms_per_iter, out_affine, out_inf, true);
    return ZKG16_ERR_BAD_ARG;
}

int zkg16_witness_map(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, uint64_t *h_out, size_t *log_n_out) {
    if (!h_out) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto rc_ref = ctx->r1cs.get(r1cs_handle); R1csDev *rc = rc_ref.get();
    auto wit_ref = ctx->wits.get(witness_handle); WitnessDev *wit = wit_ref.get();
    if (!rc || !wit) return ZKG16_ERR_BAD_HANDLE;
    if (wit->n != rc->num_variables) return ZKG16_ERR_BAD_ARG;
    Fr *h = nullptr;
    witness_map_run(ctx, *rc, wit->z.as<Fr>(), &h);
    const size_t n = (size_t)1 << rc->log_n;
    ZK_HIP(hipMemcpyAsync(h_out, h, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    if (log_n_out) *log_n_out = (size_t)rc->log_n;
    ZK_API_END(ctx)
}

int zkg16_fixed_base_g1(zkg16_ctx *ctx, const uint64_t base[12], const uint64_t *scalars_canonical, size_t n, uint64_t *out_affine,
                        uint8_t *out_inf) {
    if (!base || (!scalars_canonical && n) || (!out_affine && n)) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    if (n) {
        DevBuf d_sc(n * sizeof(Fr)), d_out(n * sizeof(G1Affine));
        ZK_HIP(hipMemcpyAsync(d_sc.p, scalars_canonical, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        fixed_base_g1_run(ctx, g1_from_abi(base, 0), d_sc.as<Fr>(), n, d_out.as<G1Affine>());
        ZK_HIP(hipMemcpyAsync(out_affine, d_out.p, n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        if (out_inf) {
            const G1Affine *o = reinterpret_cast<const G1Affine *>(out_affine);
            for (size_t i = 0; i < n; i++) out_inf[i] = o[i].is_inf() ? 1 : 0;
        }
    }
    ZK_API_END(ctx)
}

int zkg16_fixed_base_g2(zkg16_ctx *ctx, const uint64_t base[24], const uint64_t *scalars_canonical, size_t n, uint64_t *out_affine,
                        uint8_t *out_inf) {
    if (!base || (!scalars_canonical && n) || (!out_affine && n)) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    if (n) {
        DevBuf d_sc(n * sizeof(Fr)), d_out(n * sizeof(G2Affine));
        ZK_HIP(hipMemcpyAsync(d_sc.p, scalars_canonical, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        fixed_base_g2_run(ctx, g2_from_abi(base, 0), d_sc.as<Fr>(), n, d_out.as<G2Affine>());
        ZK_HIP(hipMemcpyAsync(out_affine, d_out.p, n * sizeof(G2Affine), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        if (out_inf) {
            const G2Affine *o = reinterpret_cast<const G2Affine *>(out_affine);
            for (size_t i = 0; i < n; i++) out_inf[i] = o[i].is_inf() ? 1 : 0;
        }
    }
    ZK_API_END(ctx)
}

}  // extern "C"
