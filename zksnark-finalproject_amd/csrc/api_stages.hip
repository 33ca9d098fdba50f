// libzkg16 C ABI, part 4 of 8 (api.hip): key generation from a known trapdoor and the stage entry points (NTT, MSM, witness map,
// fixed-base batches) with their stand-alone benchmarks.
#include "api_internal.hpp"
#include "r1cs_check_dev.cuh"

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

}  // extern "C"

namespace {
// a failed diagnostic call leaves no launch behind that still reads the workspace it is about to release
struct StreamDrain { zkg16_ctx *c; bool ok = false; ~StreamDrain() { if (!ok) (void)hipStreamSynchronize(c->stream); } };
}  // namespace

extern "C" {

// The bucket scatter alone (msm_bucket_sort as the plans call it) on caller-made digit codes, in a workspace of its own: ws_h, the
// slots and last_msm_group are not touched.  The results reach the caller's buffers only after everything has succeeded.
int zkg16_diag_bucket_sort(zkg16_ctx *ctx, const uint32_t *codes, size_t n, int nwin, int c, uint32_t *entries_xy, uint32_t *win_totals,
                           uint64_t *length) {
    if (!ctx || (!codes && n) || (!entries_xy && n) || !win_totals || !length || nwin < 1 || c < 2) return ZKG16_ERR_BAD_ARG;
    if (n && (uint64_t)nwin >= ((uint64_t)1 << 31) / n) return ZKG16_ERR_BAD_ARG;      // positions are 32-bit words
    ZK_API_BEGIN(ctx)
    std::vector<uint32_t> tot((size_t)nwin, 0u);
    std::vector<uint2> list;
    uint64_t len = 0;
    if (n) {
        const size_t cells = (size_t)nwin * n;
        MsmWorkspace ws;
        DevBuf d_codes(cells * sizeof(uint32_t)), d_entries(cells * sizeof(uint2));
        std::vector<uint32_t> raw((size_t)nwin + 1, 0u);
        StreamDrain drain{ctx};
        ZK_HIP(hipMemcpyAsync(d_codes.p, codes, cells * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        int sum_windows = 0;
        const uint32_t *wt = msm_bucket_sort(ctx, ws, d_codes.as<uint32_t>(), n, nwin, c, d_entries.as<uint2>(), &sum_windows);
        // nwin totals, or (many windows) the last word of the scatter's window prefix [nwin + 1]: the totals are its differences
        const bool prefix = sum_windows == 1 && nwin > 1;
        if (prefix) ZK_HIP(hipMemcpyAsync(raw.data(), wt - nwin, ((size_t)nwin + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        else ZK_HIP(hipMemcpyAsync(raw.data(), wt, (size_t)nwin * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        for (int w = 0; w < nwin; w++) tot[w] = prefix ? raw[w + 1] - raw[w] : raw[w];
        if (prefix) len = raw[nwin];
        else for (int w = 0; w < nwin; w++) len += raw[w];
        if (len > cells) throw HipError{hipErrorInvalidValue, "bucket sort: list longer than its input", __FILE__, __LINE__};
        list.resize((size_t)len);
        if (len) ZK_HIP(hipMemcpyAsync(list.data(), d_entries.p, (size_t)len * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        drain.ok = true;
    }
    if (len) memcpy(entries_xy, list.data(), (size_t)len * sizeof(uint2));
    memcpy(win_totals, tot.data(), (size_t)nwin * sizeof(uint32_t));
    *length = len;
    ZK_API_END(ctx)
}

// A term list as build_z_plans makes it — msm_plan_build, and for mask_mode 2 msm_plan_filter of the full list — in workspaces of
// its own; only the valid part (offsets[tb] entries: under sort_mode 1 the digit-0 keys sort behind it) and the offsets are copied out.
int zkg16_diag_term_list(zkg16_ctx *ctx, const uint64_t *scalars_canonical, size_t n, int batch, int window_bits, int tabled, const uint8_t *mask,
                         int mask_mode, uint32_t plan_out[4], uint32_t *entries_xy, size_t entries_cap, uint32_t *offsets, size_t offsets_cap,
                         uint64_t *length) {
    if (!ctx || (!scalars_canonical && n) || !plan_out || !length || batch < 1 || mask_mode < 0 || mask_mode > 2 || (mask_mode && !mask && n))
        return ZKG16_ERR_BAD_ARG;
    if (n && (!entries_xy || !offsets)) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    const int c = msm_plan_bits(ctx, n, window_bits, tabled != 0);
    const size_t digits = (size_t)(254 / c + 1), tb = ((size_t)1 << (c - 1)) * (size_t)batch * (tabled ? 1 : digits);
    if (tb >= ((size_t)1 << 32)) return ZKG16_ERR_BAD_ARG;
    if (n && (offsets_cap < tb + 1 || entries_cap / digits / (size_t)batch < n)) return ZKG16_ERR_BAD_ARG;
    std::vector<uint32_t> offs;
    std::vector<uint2> list;
    uint32_t len = 0;
    MsmPlan plan;
    if (n) {
        MsmWorkspace ws, ws_f;
        DevBuf d_sc((size_t)batch * n * sizeof(Fr)), d_mask(mask_mode ? n : 1);
        StreamDrain drain{ctx};
        ZK_HIP(hipMemcpyAsync(d_sc.p, scalars_canonical, (size_t)batch * n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        if (mask_mode) ZK_HIP(hipMemcpyAsync(d_mask.p, mask, n, hipMemcpyHostToDevice, ctx->stream));
        ScalarSrc src{d_sc.as<Fr>(), n, nullptr, 0, false, mask_mode == 1 ? d_mask.as<uint8_t>() : nullptr};
        src.vec_stride = n;
        src.batch = batch;
        msm_plan_build(ctx, ws, src, plan, window_bits, tabled != 0);
        const MsmWorkspace *res = &ws;
        if (mask_mode == 2) {
            MsmPlan kept;
            msm_plan_filter(ctx, ws, plan, d_mask.as<uint8_t>(), ws_f, kept);
            res = &ws_f;
        }
        if (plan.c != c || plan.nb * (size_t)plan.nwin != tb) throw HipError{hipErrorInvalidValue, "term list: plan differs from its forecast", __FILE__, __LINE__};
        offs.resize(tb + 1);
        ZK_HIP(hipMemcpyAsync(offs.data(), res->offsets.p, (tb + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        len = offs[tb];
        if ((size_t)len > plan.total_entries) throw HipError{hipErrorInvalidValue, "term list: longer than its input", __FILE__, __LINE__};
        list.resize(len);
        if (len) ZK_HIP(hipMemcpyAsync(list.data(), res->entries.p, (size_t)len * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        drain.ok = true;
    }
    plan_out[0] = (uint32_t)c;
    plan_out[1] = (uint32_t)((size_t)batch * (tabled ? 1 : digits));
    plan_out[2] = (uint32_t)digits;
    plan_out[3] = (uint32_t)tb;
    if (len) memcpy(entries_xy, list.data(), (size_t)len * sizeof(uint2));
    if (n) memcpy(offsets, offs.data(), (tb + 1) * sizeof(uint32_t));
    *length = len;
    ZK_API_END(ctx)
}

}  // extern "C"

namespace {

// zkg16_diag_msm_tabled for one group: A = the ABI's affine point, X = the XYZZ form the collection returns
template <class A, class X>
int diag_msm_tabled(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars, size_t n, int batch, int c, bool padded,
                    bool last_of_proof, uint64_t *out_affine, uint8_t *out_inf, uint64_t *table_out, uint8_t *table_inf) {
    using U = typename UOf<A>::T;
    constexpr bool g2 = sizeof(A) == sizeof(G2Affine);
    constexpr size_t words = sizeof(A) / sizeof(uint64_t);
    ZK_API_BEGIN(ctx)
    const size_t digits = (size_t)(254 / c + 1), nb = (size_t)1 << (c - 1);
    if (nb * (size_t)batch >= ((size_t)1 << 32)) return ZKG16_ERR_BAD_ARG;
    // msm_plan_build's own refusal, before anything is uploaded for it
    if (n >= ((size_t)1 << 31) || (size_t)batch * n >= ((size_t)1 << 31) || (size_t)batch * n * digits >= ((size_t)1 << 31))
        throw HipError{hipErrorInvalidValue, "msm: more than 2^31 (scalar, window) terms", __FILE__, __LINE__};
    std::vector<X> totals((size_t)batch, X::inf());
    std::vector<uint64_t> tab_h;
    std::vector<uint8_t> tab_inf;
    MsmSlot &slot = ctx->slots[0];
    struct Restore { bool &ref; const bool old; ~Restore() { ref = old; } } restore{slot.last_of_proof, slot.last_of_proof};
    DevBuf d_bases, d_sc, tab;
    StreamDrain drain{ctx};
    ctx->last_msm_group = 0;      // ws_h and slots[0] are this call's from here on; the state reads as its own once it has succeeded
    if (n) {
        d_bases.alloc(n * sizeof(U));
        d_sc.alloc((size_t)batch * n * sizeof(Fr));
        upload_points<A>(ctx, d_bases.as<U>(), bases, inf, 0, n);
        ZK_HIP(hipMemcpyAsync(d_sc.p, scalars, (size_t)batch * n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        if constexpr (g2) tab = msm_tables_build_g2(ctx, d_bases, n, c, padded);
        else tab = msm_tables_build_g1(ctx, d_bases, n, c, padded);
    }
    ScalarSrc src{d_sc.as<Fr>(), n, nullptr, 0, false, nullptr};
    src.vec_stride = n;
    src.batch = batch;
    MsmPlan plan;
    msm_plan_build(ctx, ctx->ws_h, src, plan, c, /*tabled*/ true);
    if (plan.c != c || plan.nwin != batch) throw HipError{hipErrorInvalidValue, "tabled msm: plan differs from its forecast", __FILE__, __LINE__};
    slot.last_of_proof = last_of_proof;
    if constexpr (g2) msm_g2_enqueue(ctx, ctx->ws_h, plan, tab.as<U>(), slot, padded);
    else msm_g1_enqueue(ctx, ctx->ws_h, plan, tab.as<U>(), slot, padded);
    if (batch == 1) {
        if constexpr (g2) totals[0] = msm_g2_collect(ctx, slot);
        else totals[0] = msm_g1_collect(ctx, slot);
    } else {
        msm_slot_wait(slot);
        for (int v = 0; v < batch; v++) {
            if constexpr (g2) totals[(size_t)v] = msm_g2_collect_part(slot, v);
            else totals[(size_t)v] = msm_g1_collect_part(slot, v);
        }
        slot.active = false;
    }
    if (table_out && n) {
        const size_t stride = padded ? (g2 ? ZKG16_TABLE_STRIDE_PADDED_G2 : ZKG16_TABLE_STRIDE_PADDED_G1) : sizeof(U), cells = digits * n;
        std::vector<unsigned char> raw(cells * stride);
        ZK_HIP(hipMemcpyAsync(raw.data(), tab.p, raw.size(), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        tab_h.assign(cells * words, 0);
        tab_inf.assign(cells, 0);
        for (size_t k = 0; k < cells; k++) {
            U u;
            memcpy(&u, raw.data() + k * stride, sizeof u);
            const A a = u.is_inf() ? A::inf() : A{to_sat(u.x), to_sat(u.y)};
            point_to_abi(a, tab_h.data() + k * words, &tab_inf[k]);
        }
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    drain.ok = true;
    ctx->last_msm_group = g2 ? 2 : 1;
    for (int v = 0; v < batch; v++) point_to_abi(xyzz_to_affine(totals[(size_t)v]), out_affine + (size_t)v * words, out_inf + v);
    if (table_out && n) {
        memcpy(table_out, tab_h.data(), tab_h.size() * sizeof(uint64_t));
        memcpy(table_inf, tab_inf.data(), tab_inf.size());
    }
    ZK_API_END(ctx)
}

// zkg16_diag_msm_rounds for one group
template <class A, class X>
int diag_msm_rounds(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars, size_t n, const uint8_t *part_of, int parts,
                    int c, uint64_t *out_affine, uint8_t *out_inf, uint32_t *round_entries_out) {
    using U = typename UOf<A>::T;
    constexpr bool g2 = sizeof(A) == sizeof(G2Affine);
    ZK_API_BEGIN(ctx)
    const size_t digits = (size_t)(254 / c + 1), tb = ((size_t)1 << (c - 1)) * digits;
    // msm_plan_build's own refusal, before anything is uploaded for it
    if (n >= ((size_t)1 << 31) || n * digits >= ((size_t)1 << 31))
        throw HipError{hipErrorInvalidValue, "msm: more than 2^31 (scalar, window) terms", __FILE__, __LINE__};
    X total = X::inf();
    std::vector<uint32_t> entries((size_t)parts, 0u);
    MsmSlot &slot = ctx->slots[0];
    DevBuf d_bases, d_sc, d_part;
    StreamDrain drain{ctx};
    ctx->last_msm_group = 0;      // ws_h and slots[0] are this call's from here on; the state reads as its own once it has succeeded
    if (n) {
        d_bases.alloc(n * sizeof(U));
        d_sc.alloc(n * sizeof(Fr));
        d_part.alloc(n);
        upload_points<A>(ctx, d_bases.as<U>(), bases, inf, 0, n);
        ZK_HIP(hipMemcpyAsync(d_sc.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipMemcpyAsync(d_part.p, part_of, n, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
    }
    // prove_device's rounds: per part a plan over the scalars of that part alone, accumulated as round k of the one MSM
    for (int k = 0; k < parts; k++) {
        ScalarSrc src{d_sc.as<Fr>(), n, nullptr, 0, false, nullptr};
        src.part = d_part.as<uint8_t>();
        src.want_part = k;
        MsmPlan plan;
        msm_plan_build(ctx, ctx->ws_h, src, plan, c, /*tabled*/ false);
        if (plan.c != c || plan.nb * (size_t)plan.nwin != tb) throw HipError{hipErrorInvalidValue, "msm rounds: plan differs from its forecast", __FILE__, __LINE__};
        if constexpr (g2) msm_g2_enqueue_acc(ctx, ctx->ws_h, plan, d_bases.as<U>(), slot, k);
        else msm_g1_enqueue_acc(ctx, ctx->ws_h, plan, d_bases.as<U>(), slot, k);
        // the next round's plan overwrites the list: its length is read on the stream, behind this round's accumulation
        if (n) ZK_HIP(hipMemcpyAsync(&entries[(size_t)k], ctx->ws_h.offsets.as<uint32_t>() + tb, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if constexpr (g2) {
        msm_g2_enqueue_reduce(ctx, slot);
        total = msm_g2_collect(ctx, slot);
    } else {
        msm_g1_enqueue_reduce(ctx, slot);
        total = msm_g1_collect(ctx, slot);
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    drain.ok = true;
    ctx->last_msm_group = g2 ? 2 : 1;
    point_to_abi(xyzz_to_affine(total), out_affine, out_inf);
    memcpy(round_entries_out, entries.data(), (size_t)parts * sizeof(uint32_t));
    ZK_API_END(ctx)
}

}  // namespace

extern "C" {

// One plain-key MSM fed in rounds, as prove_device runs one z-side query of a streamed assignment: per part k a plan from a ScalarSrc
// with part / want_part = k into ws_h, msm_g?_enqueue_acc(round = k) on slots[0] — round 0 into bucket_sum, later rounds into
// `buckets`, their fix-ups, then msm_bucket_merge_kernel — and that round's offsets[tb]; then one reduction and one collection.
int zkg16_diag_msm_rounds(zkg16_ctx *ctx, int group, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical, size_t n,
                          const uint8_t *part_of, int parts, int window_bits, uint64_t *out_affine, uint8_t *out_inf, uint32_t *round_entries_out) {
    if (!ctx || ((!bases || !scalars_canonical || !part_of) && n) || !out_affine || !out_inf || !round_entries_out) return ZKG16_ERR_BAD_ARG;
    if (group < 1 || group > 2 || parts < 1 || parts > 255 || window_bits < 2 || window_bits > 20) return ZKG16_ERR_BAD_ARG;
    if (group == 1) return diag_msm_rounds<G1Affine, G1XYZZ>(ctx, bases, inf, scalars_canonical, n, part_of, parts, window_bits, out_affine, out_inf, round_entries_out);
    return diag_msm_rounds<G2Affine, G2XYZZ>(ctx, bases, inf, scalars_canonical, n, part_of, parts, window_bits, out_affine, out_inf, round_entries_out);
}

// One MSM on window tables, as a proof runs one query of a key with tables: msm_tables_build_g?, a tabled msm_plan_build into ws_h, the
// enqueue on slots[0] (whose last_of_proof it sets for the call) and the collection, one value per vector of a batch; optionally the
// table itself, read at its stride and converted on the host.  zkg16_last_msm_state reports the call (nwin = batch).
int zkg16_diag_msm_tabled(zkg16_ctx *ctx, int group, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical, size_t n,
                          int batch, int window_bits, int stride_mode, int last_of_proof, uint64_t *out_affine, uint8_t *out_inf,
                          uint64_t *table_out, uint8_t *table_inf) {
    if (!ctx || ((!bases || !scalars_canonical) && n) || !out_affine || !out_inf || (table_out == nullptr) != (table_inf == nullptr)) return ZKG16_ERR_BAD_ARG;
    if (group < 1 || group > 2 || batch < 1 || window_bits < 2 || window_bits > 24 || stride_mode < 1 || stride_mode > 2 || last_of_proof < 0 ||
        last_of_proof > 1)
        return ZKG16_ERR_BAD_ARG;
    if (group == 1)
        return diag_msm_tabled<G1Affine, G1XYZZ>(ctx, bases, inf, scalars_canonical, n, batch, window_bits, stride_mode == 2, last_of_proof != 0,
                                                 out_affine, out_inf, table_out, table_inf);
    return diag_msm_tabled<G2Affine, G2XYZZ>(ctx, bases, inf, scalars_canonical, n, batch, window_bits, stride_mode == 2, last_of_proof != 0,
                                             out_affine, out_inf, table_out, table_inf);
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

// ------------------------------------------------------------------------------------------------ satisfaction (r1cs_check_dev.cuh)
namespace {

// Assignments per device pass of a stand-alone batched check: the witness map's four vectors per assignment (what zkg16_prove_batch
// reserves for them; the check itself touches three) plus `extra_per` bytes the caller keeps per assignment, within 60 % of the free
// HBM — zkg16_prove_batch's sub-batch adds its term lists and bucket arrays to the same sum, so it is never larger — at most 65,535
// (grid.z), capped by option batch_max.
size_t check_sub_size(zkg16_ctx *ctx, const R1csDev &rc, size_t extra_per) {
    const size_t per = 4 * ((size_t)1 << rc.log_n) * sizeof(Fr) + extra_per;
    size_t free_b = 0, total_b = 0;
    ZK_HIP(hipMemGetInfo(&free_b, &total_b));
    size_t kb = (size_t)(0.6 * (double)free_b) / per;
    if (ctx->opt.batch_max > 0 && (size_t)ctx->opt.batch_max < kb) kb = (size_t)ctx->opt.batch_max;
    if (kb > 65535) kb = 65535;
    return kb < 1 ? 1 : kb;
}
// pinned, device-visible block of the ctx (shared with zkg16_prove_batch, which runs on a lane under the same mutex)
void *batch_host_ensure(zkg16_ctx *ctx, size_t bytes) {
    if (ctx->batch_host_bytes < bytes) {
        if (ctx->batch_host) (void)hipHostFree(ctx->batch_host);
        ctx->batch_host = nullptr;
        ctx->batch_host_bytes = 0;
        ZK_HIP(hipHostMalloc(&ctx->batch_host, bytes, hipHostMallocDefault));
        ctx->batch_host_bytes = bytes;
    }
    return ctx->batch_host;
}
// One pass: the (batched) SpMV of `n` assignments, the patch, the kernel, and the 2 n result words read back into out_n / out_first
void check_pass(zkg16_ctx *ctx, R1csDev &rc, WitnessDev *const *wits, size_t n, const WmPatch *patch, const Fr **table, uint64_t *out_n,
                uint64_t *out_first) {
    ctx->check_dev.ensure(2 * n * sizeof(uint64_t));
    uint64_t *res = ctx->check_dev.as<uint64_t>();
    struct Drain { zkg16_ctx *c; bool ok = false; ~Drain() { if (!ok) (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    if (n == 1 && !patch) {
        r1cs_check_spmv_run(ctx, rc, wits[0]->z.as<Fr>(), nullptr, 1, nullptr, res);
    } else {
        for (size_t i = 0; i < n; i++) table[i] = wits[i]->z.as<Fr>();
        if (n == 1) r1cs_check_spmv_run(ctx, rc, table[0], nullptr, 1, patch, res);
        else r1cs_check_spmv_run(ctx, rc, nullptr, table, (unsigned)n, patch, res);
    }
    std::vector<uint64_t> w(2 * n);
    ZK_HIP(hipMemcpyAsync(w.data(), res, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));      // the one read-back
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    drain.ok = true;
    memcpy(out_n, w.data(), n * sizeof(uint64_t));
    memcpy(out_first, w.data() + n, n * sizeof(uint64_t));
}

}  // namespace

extern "C" {

int zkg16_r1cs_check_host(const uint64_t *const row_ptr[3], const uint32_t *const col[3], const uint64_t *const coeff[3], size_t num_constraints,
                          size_t num_variables, const uint64_t *z, uint64_t *n_bad, uint64_t *first_bad) {
    if (!row_ptr || !col || !coeff || !z || !n_bad || num_variables == 0) return ZKG16_ERR_BAD_ARG;
    for (int m = 0; m < 3; m++) {
        const uint64_t *rp = row_ptr[m];
        if (!rp || rp[0] != 0) return ZKG16_ERR_BAD_ARG;
        for (size_t i = 0; i < num_constraints; i++)
            if (rp[i] > rp[i + 1]) return ZKG16_ERR_BAD_ARG;
        const uint64_t nnz = rp[num_constraints];
        if (nnz && (!col[m] || !coeff[m])) return ZKG16_ERR_BAD_ARG;
        for (uint64_t k = 0; k < nnz; k++)
            if (col[m][k] >= num_variables) return ZKG16_ERR_BAD_ARG;
    }
    try {
        // the block walk of r1cs_check_kernel on the host: the SpMV's row sums (spmv_kernel's order of operations), rck::row_fails per
        // lane, rck::block_fold per block, rck::result_merge where the kernel's atomics are
        uint64_t bad = rck::result_init(0, 1), first = rck::result_init(1, 1);
        for (size_t row0 = 0; row0 < num_constraints; row0 += rck::BLOCK) {
            uint64_t ballots[rck::WAVES] = {0, 0, 0, 0};
            for (unsigned t = 0; t < rck::BLOCK && row0 + t < num_constraints; t++) {
                Fr v[3];
                for (int m = 0; m < 3; m++) {
                    Fr acc = Fr::zero();
                    for (uint64_t k = row_ptr[m][row0 + t]; k < row_ptr[m][row0 + t + 1]; k++)
                        acc = fp_add(acc, fp_mul(fr_from_abi(coeff[m] + 4 * k), fr_from_abi(z + 4 * (size_t)col[m][k])));
                    v[m] = acc;
                }
                if (rck::row_fails(v[0], v[1], v[2])) ballots[t >> 6] |= (uint64_t)1 << (t & 63u);
            }
            uint64_t count, f;
            if (rck::block_fold(ballots, row0, count, f)) rck::result_merge(bad, first, count, f);
        }
        *n_bad = bad;
        if (first_bad) *first_bad = first;
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

int zkg16_r1cs_check(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, uint64_t *n_bad, uint64_t *first_bad) {
    return zkg16_r1cs_check_batch(ctx, r1cs_handle, &witness_handle, 1, n_bad, first_bad);
}

int zkg16_r1cs_check_batch(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t *witness_handles, size_t k, uint64_t *n_bad, uint64_t *first_bad) {
    if (!witness_handles || !n_bad || k == 0) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto rc = ctx->r1cs.get(r1cs_handle);
    if (!rc) return ZKG16_ERR_BAD_HANDLE;
    std::vector<std::shared_ptr<WitnessDev>> refs(k);
    std::vector<WitnessDev *> wits(k);
    for (size_t i = 0; i < k; i++) {
        refs[i] = ctx->wits.get(witness_handles[i]);
        if (!(wits[i] = refs[i].get())) return ZKG16_ERR_BAD_HANDLE;
    }
    if (rc->prime_template) return ZKG16_ERR_UNSUPPORTED;      // no request's system: its four candidate-dependent coefficients are zero
    for (size_t i = 0; i < k; i++)
        if (wits[i]->n != rc->num_variables) return ZKG16_ERR_BAD_ARG;
    const size_t kb = std::min(k, check_sub_size(ctx, *rc, 0));
    std::vector<uint64_t> nb(k), fb(k);
    const Fr **table = kb > 1 ? static_cast<const Fr **>(batch_host_ensure(ctx, kb * sizeof(Fr *))) : nullptr;
    for (size_t off = 0; off < k; off += kb)
        check_pass(ctx, *rc, wits.data() + off, std::min(kb, k - off), nullptr, table, nb.data() + off, fb.data() + off);
    memcpy(n_bad, nb.data(), k * sizeof(uint64_t));
    if (first_bad) memcpy(first_bad, fb.data(), k * sizeof(uint64_t));
    ZK_API_END(ctx)
}

int zkg16_prime_check_batch(zkg16_ctx *ctx, uint64_t r1cs_template_handle, const uint64_t *xs, const uint64_t *js, size_t k, uint64_t *n_bad,
                            uint64_t *first_bad) {
    if (!xs || !js || !n_bad || k == 0) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto rc = ctx->r1cs.get(r1cs_template_handle);
    if (!rc) return ZKG16_ERR_BAD_HANDLE;
    if (!rc->prime_template) return ZKG16_ERR_BAD_ARG;
    std::vector<Fr> in;
    std::vector<uint32_t> ns(k);
    size_t stride = 0;
    if (const int st = prime_batch_inputs(xs, js, k, in, ns.data(), &stride)) return st;      // a refused candidate: before any device work
    const size_t kb = std::min(k, check_sub_size(ctx, *rc, rc->num_variables * sizeof(Fr)));
    std::vector<uint64_t> nb(k), fb(k);
    for (size_t off = 0; off < k; off += kb) {
        const size_t n = std::min(kb, k - off);
        std::vector<std::shared_ptr<WitnessDev>> refs;
        prime_witness_batch_assign(ctx, in.data() + off * stride, n, refs, nullptr);
        if (refs.size() != n) throw HipError{hipErrorInvalidValue, "prime check: assignments missing", __FILE__, __LINE__};
        std::vector<WitnessDev *> wits(n);
        for (size_t i = 0; i < n; i++) wits[i] = refs[i].get();
        // request i's n and -j, as prove_batch_device lays them out for wm_patch_kernel, then the assignment table
        Fr *patch_tab = static_cast<Fr *>(batch_host_ensure(ctx, n * (2 * sizeof(Fr) + sizeof(Fr *))));
        for (size_t i = 0; i < n; i++) {
            Fr c = Fr::zero();
            c.l[0] = ns[off + i];
            patch_tab[2 * i] = fp_to_mont(c);
            c.l[0] = (uint32_t)js[off + i];
            c.l[1] = (uint32_t)(js[off + i] >> 32);
            patch_tab[2 * i + 1] = fp_neg(fp_to_mont(c));
        }
        WmPatch patch{{0, 0, 0, 0}, patch_tab};
        memcpy(patch.rows, rc->patch_rows, sizeof patch.rows);
        check_pass(ctx, *rc, wits.data(), n, &patch, reinterpret_cast<const Fr **>(patch_tab + 2 * n), nb.data() + off, fb.data() + off);
    }
    memcpy(n_bad, nb.data(), k * sizeof(uint64_t));
    if (first_bad) memcpy(first_bad, fb.data(), k * sizeof(uint64_t));
    ZK_API_END(ctx)
}

}  // extern "C"
