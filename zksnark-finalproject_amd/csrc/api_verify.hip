// libzkg16 C ABI, part 6 of 8 (api.hip): batched verification.
#include "api_internal.hpp"

using namespace zk;

// ------------------------------------------------------------------------------------------------ batched verification
// (verify_batch.hpp.)  The per-proof work in kernels on a lane of the ctx: the three membership launches and the Miller launch of a
// pass are independent and run on four of the lane's streams at once; the host needs the membership verdicts first (they decide
// which C_k enter the MSM), so the MSM of sum rho_k C_k runs on the lane's main stream while the Miller kernel is still busy.
// From wire bytes (zkg16_verify_batch_wire) the three decompress launches of a pass fill the device proof array first, B on the main
// stream beside A and C on two others; everything after reads that array as if the host had uploaded it.
// Where the public inputs come from is a VbForm (verify_batch.hpp).  The prime form (zkg16_verify_prime_batch[_wire]) has none on
// the host: (x, j) go up, the inputs kernel runs in front of the membership kernels of the main stream, and the 260 multiplier sums
// are taken there once the member mask is known.  The u64 form (zkg16_verify_batch_u64[_wire]) sends its k x (num_instance - 1)
// 64-bit values up as they are: the sums kernels run where the prime form's do, a second G1 MSM over the key's points turns the
// device sums into sum_i s_i gamma_abc[i], and the per-proof pass makes X_k from the rows on the device (u64_x_kernel in the place
// of each_x_kernel).
namespace zk {
std::vector<uint8_t> vb_flags(const uint64_t *proofs, const uint8_t *inf, size_t k) {
    std::vector<uint8_t> fl(3 * k);
    for (size_t i = 0; i < k; i++) {
        const uint64_t *pr = proofs + 48 * i;
        const size_t at[4] = {0, 12, 36, 48};
        for (int j = 0; j < 3; j++) {
            uint64_t any = 0;
            for (size_t t = at[j]; t < at[j + 1]; t++) any |= pr[t];
            fl[3 * i + j] = inf[3 * i + j] || !any ? 1 : 0;
        }
    }
    return fl;
}
void vb_membership_chunk(const VbStreams &s, const uint64_t *pts, const uint8_t *fl, size_t n, const VbEndo &en, uint8_t *m3) {
    vb_membership_launch(s.main, 1, pts, 48, fl, 3, n, en, m3, 3);
    vb_membership_launch(s.c, 1, pts + 36, 48, fl + 2, 3, n, en, m3 + 2, 3);
    vb_membership_launch(s.b, 2, pts + 12, 48, fl + 1, 3, n, en, m3 + 1, 3);
}
void vb_wire_decode(const VbStreams &s, hipEvent_t e_c, hipEvent_t e_b, const uint8_t *d_wire, size_t k, size_t pass, const VbEndo &en, uint64_t *d_proofs,
                    uint8_t *d_inf, uint8_t *d_st) {
    for (size_t off = 0; off < k; off += pass) {
        const size_t n = std::min(pass, k - off);
        const uint8_t *by = d_wire + 192 * off;
        uint64_t *pts = d_proofs + 48 * off;
        uint8_t *fl = d_inf + 3 * off, *st3 = d_st + 3 * off;
        vb_decompress_launch(s.main, 2, by + 48, 192, n, 0, en, pts + 12, 48, fl + 1, 3, st3 + 1, 3);
        vb_decompress_launch(s.c, 1, by, 192, n, 0, en, pts, 48, fl, 3, st3, 3);
        vb_decompress_launch(s.b, 1, by + 144, 192, n, 0, en, pts + 36, 48, fl + 2, 3, st3 + 2, 3);
    }
    vb_join(s, e_c, e_b);
}
}  // namespace zk

namespace {
void vb_publish(zkg16_ctx *root, const float tm[V_COUNT]) {
    std::lock_guard<std::mutex> lk(root->lane_mu);
    memcpy(root->vb_timings, tm, sizeof root->vb_timings);
}
// which gamma_abc points are the point at infinity: all-zero limbs (load_pt's rule)
std::vector<uint8_t> vb_zero_points(const uint64_t *pts, size_t n) {
    std::vector<uint8_t> fl(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t any = 0;
        for (size_t t = 0; t < 12; t++) any |= pts[12 * i + t];
        fl[i] = any ? 0 : 1;
    }
    return fl;
}

// The per-proof pass on the lane's main stream: the proofs idx[0 .. n) (null: 0 .. n - 1) of the k x 48 limbs / k x 3 flags already on
// the device, each with its public inputs, in launches of VB_PASS.  The key is converted and uploaded once per call.  By the form:
// Limbs — the inputs of the listed proofs go up as canonical limbs.  Prime — they are written on the device from its (x, j) and
// digests, so nothing travels per proof but its index.  U64 — X_k of every listed proof is made from its row of values on the device
// (all the X launches first, between two events of their own: *x_ms, when asked), then the Miller and final-exponentiation launches.
// Returns the kernels' time in ms (device events)
float vb_each_pass(zkg16_ctx *ctx, const VbKey &key, const VbForm &form, const uint64_t *d_proofs, const uint8_t *d_inf, const uint32_t *idx, size_t n,
                   uint8_t *verdict, float *x_ms = nullptr) {
    if (!n) return 0;
    hipStream_t st = ctx->stream;
    const bool limbs = form.kind == VbKind::Limbs, prime = form.kind == VbKind::Prime, u64 = form.kind == VbKind::U64;
    const size_t ni = key.num_instance, per = 4 * (ni - 1), pass = std::min(n, VB_PASS);
    std::vector<uint32_t> words(vb_each_key_count(ni));
    vb_each_key_words(key, words.data());
    std::vector<uint64_t> z(limbs ? std::max<size_t>(n * per, 1) : 1);
    for (size_t j = 0; j < n && per && limbs; j++) vb_scalars_canonical(form.public_inputs + per * (idx ? idx[j] : j), ni - 1, z.data() + per * j);
    DevBuf d_key(words.size() * 4), d_z(prime ? n * per * 8 : u64 ? 0 : z.size() * 8), d_idx(idx ? n * 4 : 0), d_scratch(vb_each_scratch_bytes(pass)), d_verdict(n);
    DevBuf d_xk(u64 ? vb_each_x_bytes(n) : 0), d_have(u64 ? n : 0);
    VbEvents evs;
    ZK_HIP(hipMemcpyAsync(d_key.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    if (limbs) ZK_HIP(hipMemcpyAsync(d_z.p, z.data(), z.size() * 8, hipMemcpyHostToDevice, st));
    if (idx) ZK_HIP(hipMemcpyAsync(d_idx.p, idx, n * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipEventRecord(evs.ev[0], st));
    if (u64) {
        const uint32_t *pts = d_key.as<uint32_t>() + vb_each_key_points_at();
        for (size_t off = 0; off < n; off += VB_PASS)
            vb_u64_x_launch(st, pts, ni, idx ? form.d_values : form.d_values + (ni - 1) * off, idx ? d_idx.as<uint32_t>() + off : nullptr, std::min(VB_PASS, n - off),
                            d_xk.as<uint8_t>() + vb_each_x_bytes(off), d_have.as<uint8_t>() + off);
        ZK_HIP(hipEventRecord(evs.ev[2], st));
        for (size_t off = 0; off < n; off += VB_PASS)
            vb_each_tail_launch(st, d_key.as<uint32_t>(), idx ? d_idx.as<uint32_t>() + off : nullptr, std::min(VB_PASS, n - off), idx ? d_proofs : d_proofs + 48 * off,
                                idx ? d_inf : d_inf + 3 * off, d_xk.as<uint8_t>() + vb_each_x_bytes(off), d_have.as<uint8_t>() + off, d_scratch.p,
                                d_verdict.as<uint8_t>() + off);
    }
    for (size_t off = 0; off < n && prime; off += VB_PASS)
        vb_prime_z_launch(st, idx ? d_idx.as<uint32_t>() + off : nullptr, std::min(VB_PASS, n - off), idx ? form.d_xs : form.d_xs + off,
                          idx ? form.d_js : form.d_js + off, idx ? form.d_dig : form.d_dig + 8 * off, d_z.as<uint64_t>() + per * off);
    for (size_t off = 0; off < n && !u64; off += VB_PASS)
        vb_each_launch(st, d_key.as<uint32_t>(), ni, idx ? d_idx.as<uint32_t>() + off : nullptr, std::min(VB_PASS, n - off), idx ? d_proofs : d_proofs + 48 * off,
                       idx ? d_inf : d_inf + 3 * off, d_z.as<uint64_t>() + per * off, d_scratch.p, d_verdict.as<uint8_t>() + off);
    ZK_HIP(hipEventRecord(evs.ev[1], st));
    ZK_HIP(hipMemcpyAsync(verdict, d_verdict.p, n, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    if (u64 && x_ms) *x_ms += vb_elapsed(evs.ev[0], evs.ev[2]);
    return vb_elapsed(evs.ev[0], evs.ev[1]);
}

// The device form of every batch entry point.  wire == null: b.proofs / b.inf are the caller's limbs and flags.  wire != null (k x 192
// bytes): b.proofs / b.inf are null; the proofs are decoded on the device, unvalidated, and the decoded limbs and flags come back
// once for the MSM's bases and vb_decide.  A proof with a point that did not decode is left out like one that fails membership;
// decode_status (nullable, k x 3): the decode kernel's statuses, 5 where a decoded point failed membership.
// form: Limbs — b.public_inputs are the inputs.  Prime — b.public_inputs is null; the inputs kernel runs beside the membership
// kernels, the 260 sums of the member proofs are taken on the device once the membership verdicts are back, and the host expands
// inputs (from the 32-byte digests it then downloads) only when bisecting asks for them.  U64 — b.public_inputs is null as well;
// the values go up beside the proofs, the num_instance sums of the member proofs are taken where the prime form's are,
// sum_i s_i gamma_abc[i] is a second MSM of the ctx on those device sums, and the host expands values to Montgomery limbs only when
// bisecting asks for them.  The form's device pointers are filled in here.
int vb_device(zkg16_ctx *ctx, const VbKey &key, VbForm &form, VbBatch b, const uint8_t *wire, int *ok, uint8_t *ok_each, uint8_t *decode_status, double t_all) {
    const size_t k = b.k;
    const bool prime = form.kind == VbKind::Prime, u64 = form.kind == VbKind::U64;
    float tm[V_COUNT] = {0};
    ZK_LANE_BEGIN(ctx)
    const VbStreams s = vb_streams(ctx);
    hipStream_t s_main = s.main, s_mil = ctx->wm_stream;
    VbEvents evs;
    hipEvent_t e_up = evs.ev[0], e_a = evs.ev[1], e_c = evs.ev[2], e_b = evs.ev[3], e_mil = evs.ev[4], e_p0 = evs.ev[5], e_p1 = evs.ev[6], e_m0 = evs.ev[7],
               e_d0 = evs.ev[8], e_d1 = evs.ev[9], e_i0 = evs.ev[10], e_i1 = evs.ev[11], e_s0 = evs.ev[12], e_s1 = evs.ev[13];
    const size_t half = (k + 1) / 2;
    DevBuf d_proofs(k * 48 * 8), d_inf(3 * k), d_rho(k * 16), d_mem3(3 * k), d_live(k), d_f(k * 72 * 8), d_tmp(2 * half * 72 * 8);
    DevBuf d_wire(wire ? k * 192 : 0), d_st(wire ? 3 * k : 0);
    const size_t ni = key.num_instance, um = ni - 1;      // the prime form's key has 260 points: ni sums in both forms that take them
    DevBuf d_xs(prime ? k * 8 : 0), d_js(prime ? k * 8 : 0), d_dig(prime ? k * 32 : 0), d_values(u64 ? k * um * 8 : 0);
    DevBuf d_part(prime ? vb_prime_sums_blocks(k) * 260 * 32 : u64 ? vb_u64_sums_partial_words(k, um) * 8 : 0), d_sums(prime || u64 ? ni * 32 : 0);
    std::vector<uint64_t> sums(prime || u64 ? ni * 4 : 0), expanded;
    std::vector<uint32_t> digests;
    const VbEndo en = vb_endo();
    std::vector<uint64_t> dec_proofs;
    std::vector<uint8_t> dec_inf, dec_st, flags;
    if (wire) {
        upload_h2d(ctx, d_wire.p, wire, k * 192);
        ZK_HIP(hipMemcpyAsync(d_rho.p, b.rho, k * 16, hipMemcpyHostToDevice, s_main));
        vb_fork(s, e_d0);
        vb_wire_decode(s, e_c, e_b, d_wire.as<uint8_t>(), k, VB_PASS, en, d_proofs.as<uint64_t>(), d_inf.as<uint8_t>(), d_st.as<uint8_t>());
        ZK_HIP(hipEventRecord(e_d1, s_main));
        // the decoded proofs travel to the host behind the kernels below; they are first read after the membership verdicts
        dec_proofs.resize(48 * k);
        dec_inf.resize(3 * k);
        dec_st.resize(3 * k);
        b.proofs = dec_proofs.data();
        b.inf = dec_inf.data();
    } else {
        // as zkg16_verify_batch_host reads them (a valid proof whose C = O came as zero limbs without its flag is valid here too)
        flags = vb_flags(b.proofs, b.inf, k);
        b.inf = flags.data();
        upload_h2d(ctx, d_proofs.p, b.proofs, k * 48 * 8);
        ZK_HIP(hipMemcpyAsync(d_inf.p, b.inf, 3 * k, hipMemcpyHostToDevice, s_main));
        ZK_HIP(hipMemcpyAsync(d_rho.p, b.rho, k * 16, hipMemcpyHostToDevice, s_main));
    }
    if (u64) {
        upload_h2d(ctx, d_values.p, form.values, k * um * 8);
        form.d_values = d_values.as<uint64_t>();
    }
    vb_fork(s, e_up, s_mil);
    ZK_HIP(hipEventRecord(e_m0, s_mil));
    if (prime) {
        // 16 bytes per proof up, one SHA-256 block per lane: in front of the membership kernels of the main stream
        ZK_HIP(hipMemcpyAsync(d_xs.p, form.xs, k * 8, hipMemcpyHostToDevice, s_main));
        ZK_HIP(hipMemcpyAsync(d_js.p, form.js, k * 8, hipMemcpyHostToDevice, s_main));
        ZK_HIP(hipEventRecord(e_i0, s_main));
        for (size_t off = 0; off < k; off += VB_PASS)
            vb_prime_inputs_launch(s_main, d_xs.as<uint64_t>() + off, d_js.as<uint64_t>() + off, std::min(VB_PASS, k - off), d_dig.as<uint32_t>() + 8 * off, nullptr,
                                   nullptr);
        ZK_HIP(hipEventRecord(e_i1, s_main));
        form.d_xs = d_xs.as<uint64_t>();
        form.d_js = d_js.as<uint64_t>();
        form.d_dig = d_dig.as<uint32_t>();
    }
    for (size_t off = 0; off < k; off += VB_PASS) {
        const size_t n = std::min(VB_PASS, k - off);
        const uint64_t *pts = d_proofs.as<uint64_t>() + 48 * off;
        const uint8_t *fl = d_inf.as<uint8_t>() + 3 * off;
        uint8_t *m3 = d_mem3.as<uint8_t>() + 3 * off;
        // membership first: where two of these streams share a hardware queue, the short kernels must not sit behind the long one
        vb_membership_chunk(s, pts, fl, n, en, m3);
        vb_miller_launch(s_mil, pts, 48, fl, pts + 12, 48, fl + 1, 3, d_rho.as<uint64_t>() + 2 * off, n, d_f.as<uint64_t>() + 72 * off);
    }
    const double t_launched = now_ms();
    ZK_HIP(hipEventRecord(e_a, s_main));
    vb_join(s, e_c, e_b, e_mil, s_mil);
    std::vector<uint8_t> mem3(3 * k), member(k);
    ZK_HIP(hipMemcpyAsync(mem3.data(), d_mem3.p, 3 * k, hipMemcpyDeviceToHost, s_main));
    if (wire) {
        ZK_HIP(hipMemcpyAsync(dec_proofs.data(), d_proofs.p, k * 48 * 8, hipMemcpyDeviceToHost, s_main));
        ZK_HIP(hipMemcpyAsync(dec_inf.data(), d_inf.p, 3 * k, hipMemcpyDeviceToHost, s_main));
        ZK_HIP(hipMemcpyAsync(dec_st.data(), d_st.p, 3 * k, hipMemcpyDeviceToHost, s_main));
    }
    ZK_HIP(hipStreamSynchronize(s_main));
    // host clock, launch to verdicts on the host (what the MSM below waits for), not kernel time: measured, it equals the Miller
    // kernel's time — the verdicts do not reach the host before that kernel ends
    tm[V_MEMBERSHIP] = (float)(now_ms() - t_launched);
    if (wire) tm[V_DECODE] = vb_elapsed(e_d0, e_d1);
    size_t n_live = 0;
    for (size_t i = 0; i < k; i++) {
        bool good = mem3[3 * i] && mem3[3 * i + 1] && mem3[3 * i + 2];
        // an undecodable point left zero limbs behind, which no curve holds; the status decides all the same
        if (wire) good = good && !dec_st[3 * i] && !dec_st[3 * i + 1] && !dec_st[3 * i + 2];
        n_live += member[i] = good ? 1 : 0;
    }
    if (wire && decode_status)
        for (size_t j = 0; j < 3 * k; j++) decode_status[j] = dec_st[j] ? dec_st[j] : (mem3[j] ? 0 : 5);
    const uint64_t *proofs = b.proofs, *rho = b.rho;
    const uint8_t *inf = b.inf;
    // sum rho_k C_k over the member proofs: the ctx's G1 MSM, beside the Miller kernel
    uint64_t sum_c[12] = {0};
    uint8_t sum_c_inf = 1;
    if (n_live) {
        const double t0 = now_ms();
        std::vector<uint64_t> bases(12 * k), sc(4 * k, 0);
        std::vector<uint8_t> binf(k);
        for (size_t i = 0; i < k; i++) {
            memcpy(&bases[12 * i], proofs + 48 * i + 36, 96);
            binf[i] = inf[3 * i + 2] || !member[i] ? 1 : 0;
            if (member[i]) { sc[4 * i] = rho[2 * i]; sc[4 * i + 1] = rho[2 * i + 1]; }
        }
        DevBuf d_bases(k * sizeof(G1AffineU)), d_sc(k * sizeof(Fr));
        upload_points<G1Affine>(ctx, d_bases.as<G1AffineU>(), bases.data(), binf.data(), 0, k);
        ZK_HIP(hipMemcpyAsync(d_sc.p, sc.data(), k * sizeof(Fr), hipMemcpyHostToDevice, s_main));
        ZK_HIP(hipStreamSynchronize(s_main));
        MsmPlan plan;
        msm_plan_build(ctx, ctx->ws_h, d_sc.as<Fr>(), k, plan);
        const G1XYZZ total = msm_g1_exec(ctx, ctx->ws_h, plan, d_bases.as<G1AffineU>(), "verify_batch_msm");
        point_to_abi(xyzz_to_affine(total), sum_c, &sum_c_inf);
        tm[V_MSM] = (float)(now_ms() - t0);
    }
    // the product of the member proofs' Miller values
    ZK_HIP(hipMemcpyAsync(d_live.p, member.data(), k, hipMemcpyHostToDevice, s_main));
    uint64_t sum_x[12] = {0};
    uint8_t sum_x_inf = 1;
    if (prime || u64) {
        // s_i = sum rho_k z_{k,i} over the member proofs, while the Miller kernel is still busy
        ZK_HIP(hipEventRecord(e_s0, s_main));
        if (prime)
            vb_prime_sums_launch(s_main, form.d_xs, form.d_js, form.d_dig, d_rho.as<uint64_t>(), d_live.as<uint8_t>(), k, d_part.as<uint64_t>(), d_sums.as<uint64_t>());
        else
            vb_u64_sums_launch(s_main, form.d_values, um, d_rho.as<uint64_t>(), d_live.as<uint8_t>(), k, d_part.as<uint64_t>(), d_sums.as<uint64_t>());
        ZK_HIP(hipEventRecord(e_s1, s_main));
        ZK_HIP(hipMemcpyAsync(sums.data(), d_sums.p, ni * 32, hipMemcpyDeviceToHost, s_main));
    }
    if (u64 && n_live) {
        // sum_i s_i gamma_abc[i]: the sums stay where they are — below 2^224 < r, they are canonical scalars as they lie
        const std::vector<uint8_t> ginf = vb_zero_points(key.gamma_abc_g1, ni);
        DevBuf d_gbases(ni * sizeof(G1AffineU));
        upload_points<G1Affine>(ctx, d_gbases.as<G1AffineU>(), key.gamma_abc_g1, ginf.data(), 0, ni);
        ZK_HIP(hipStreamSynchronize(s_main));
        MsmPlan plan;
        msm_plan_build(ctx, ctx->ws_h, d_sums.as<Fr>(), ni, plan);
        const G1XYZZ total = msm_g1_exec(ctx, ctx->ws_h, plan, d_gbases.as<G1AffineU>(), "verify_batch_u64_msm");
        point_to_abi(xyzz_to_affine(total), sum_x, &sum_x_inf);
    }
    ZK_HIP(hipStreamWaitEvent(s_main, e_mil, 0));
    ZK_HIP(hipEventRecord(e_p0, s_main));
    const uint64_t *d_prod = vb_product_launch(s_main, d_f.as<uint64_t>(), d_live.as<uint8_t>(), k, d_tmp.as<uint64_t>());
    ZK_HIP(hipEventRecord(e_p1, s_main));
    uint64_t prod[72];
    ZK_HIP(hipMemcpyAsync(prod, d_prod, sizeof prod, hipMemcpyDeviceToHost, s_main));
    ZK_HIP(hipStreamSynchronize(s_main));
    tm[V_MILLER] = vb_elapsed(e_m0, e_mil);      // both on the Miller stream
    tm[V_PRODUCT] = vb_elapsed(e_p0, e_p1);
    if (prime) {
        tm[V_PRIME_INPUTS] = vb_elapsed(e_i0, e_i1);
        tm[V_PRIME_SUMS] = vb_elapsed(e_s0, e_s1);
    }
    if (u64) tm[V_U64_SUMS] = vb_elapsed(e_s0, e_s1);
    // the K Miller values leave the device only when the batch equation failed and the caller wants to know where
    std::vector<uint64_t> miller;
    // ... and when bisecting has used its budget of range tests, the proofs it left undecided stay here for the per-proof pass
    VbEach each;
    each.after = (size_t)ctx->opt.verify_each_after;
    if (u64) {
        // every further range test costs num_instance host scalar multiplications here, the per-proof pass a fixed number of launches:
        // unless the caller set the option, that pass decides every member proof right after the test of the whole batch
        each.count_whole = true;
        if (!ctx->opt.verify_each_after_set) each.after = 1;
    }
    each.decide = [&](const uint32_t *idx, size_t n, uint8_t *verdict) {
        tm[V_EACH] += vb_each_pass(ctx, key, form, d_proofs.as<uint64_t>(), d_inf.as<uint8_t>(), idx, n, verdict, tm + V_U64_X);
    };
    VbInputs inputs;
    if (prime || u64) {
        inputs.sums = sums.data();
        if (u64) {
            inputs.sum_x = sum_x;
            inputs.sum_x_inf = &sum_x_inf;
        }
        inputs.expand = [&]() -> const uint64_t * {
            if (prime) {
                digests.resize(8 * k);
                ZK_HIP(hipMemcpy(digests.data(), d_dig.p, k * 32, hipMemcpyDeviceToHost));
            }
            return vb_form_expand(key, form, k, prime ? digests.data() : nullptr, expanded);
        };
    }
    vb_decide(key, b, member.data(), [&]() -> const uint64_t * {
        miller.resize(72 * k);
        ZK_HIP(hipMemcpy(miller.data(), d_f.p, k * 72 * 8, hipMemcpyDeviceToHost));
        return miller.data();
    }, prod, sum_c, &sum_c_inf, 0, ok, ok_each, tm + V_HOST, &each, prime || u64 ? &inputs : nullptr);
    // the verdicts above came from host-expanded inputs then, and are right; a device whose sums are wrong is reported all the same
    if (inputs.sums_refused)
        throw HipError{hipErrorUnknown, u64 ? "u64_rho_sums_kernel: s_0 differs from the host's sum of the multipliers"
                                            : "prime_rho_sums_kernel: s_0 differs from the host's sum of the multipliers", __FILE__, __LINE__};
    tm[V_RANGE_TESTS] = (float)each.range_tests;
    tm[V_TOTAL] = (float)(now_ms() - t_all);
    vb_publish(root, tm);
    ZK_LANE_END(ctx)
}

// Every batch entry point: the checks, the host form below the entry's threshold, vb_device above it.  from_wire: proof_bytes
// (k x 192) are the proofs, and proofs / inf are null; else proofs / inf are the limbs and flags, and proof_bytes / decode_status null
int vb_entry(zkg16_ctx *ctx, const VbKey &key, VbForm form, const uint64_t *proofs, const uint8_t *inf, bool from_wire, const uint8_t *proof_bytes,
             const uint64_t *rho, size_t k, int *ok, uint8_t *ok_each, uint8_t *decode_status) {
    if (!ctx || !ok || (from_wire ? !proof_bytes : !proofs || !inf)) return ZKG16_ERR_BAD_ARG;
    int rc = vb_check_batch(key, form, k);
    if (rc == ZKG16_OK) rc = vb_check_rho(rho, k);
    if (rc != ZKG16_OK) return rc;
    const double t_all = now_ms();
    VbBatch b{form.public_inputs, proofs, inf, rho, k};
    if (k >= (size_t)(from_wire ? ctx->opt.verify_wire_min : ctx->opt.verify_batch_min)) return vb_device(ctx, key, form, b, proof_bytes, ok, ok_each, decode_status, t_all);
    float tm[V_COUNT] = {0};
    try {
        std::vector<uint64_t> made, dec_proofs;
        std::vector<uint8_t> dec_inf, st, dead;
        if (from_wire) {
            // status 5 costs the subgroup tests a second time (vb_host makes its own): only for a caller who asks for the statuses
            dec_proofs.resize(48 * k);
            dec_inf.resize(3 * k);
            st.resize(3 * k);
            dead.resize(k);
            vb_wire_decode_host(proof_bytes, k, decode_status ? 1 : 0, 0, dec_proofs.data(), dec_inf.data(), st.data());
            tm[V_DECODE] = (float)(now_ms() - t_all);
            for (size_t i = 0; i < k; i++) dead[i] = st[3 * i] || st[3 * i + 1] || st[3 * i + 2] ? 1 : 0;
            b.proofs = dec_proofs.data();
            b.inf = dec_inf.data();
        }
        b.public_inputs = vb_form_expand(key, form, k, nullptr, made);
        vb_host(key, b, 0, ok, ok_each, from_wire ? dead.data() : nullptr);
        if (from_wire && decode_status) memcpy(decode_status, st.data(), 3 * k);
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    tm[V_TOTAL] = (float)(now_ms() - t_all);
    tm[V_HOST_FORM] = 1;
    vb_publish(ctx, tm);
    return ZKG16_OK;
}

// Both per-proof entry points: membership of every proof, then the per-proof pass over the ones that passed
int vb_each_entry(zkg16_ctx *ctx, const VbKey &key, VbForm form, const uint64_t *proofs, const uint8_t *inf, size_t k, uint8_t *ok_each) {
    if (!ctx || !ok_each || !proofs || !inf) return ZKG16_ERR_BAD_ARG;
    const int rc = vb_check_batch(key, form, k);
    if (rc != ZKG16_OK) return rc;
    ZK_LANE_BEGIN(ctx)
    const VbStreams s = vb_streams(ctx);
    // zkg16_verify_prepared reads all-zero limbs as the point at infinity whatever the flag says: the same here
    const std::vector<uint8_t> fl = vb_flags(proofs, inf, k);
    const size_t values_bytes = form.kind == VbKind::U64 ? k * (key.num_instance - 1) * 8 : 0;
    VbEvents evs;
    DevBuf d_proofs(k * 48 * 8), d_inf(3 * k), d_mem3(3 * k), d_values(values_bytes);
    const VbEndo en = vb_endo();
    upload_h2d(ctx, d_proofs.p, proofs, k * 48 * 8);
    if (form.kind == VbKind::U64) {
        upload_h2d(ctx, d_values.p, form.values, values_bytes);
        form.d_values = d_values.as<uint64_t>();
    }
    ZK_HIP(hipMemcpyAsync(d_inf.p, fl.data(), 3 * k, hipMemcpyHostToDevice, s.main));
    vb_fork(s, evs.ev[0]);
    for (size_t off = 0; off < k; off += VB_PASS)
        vb_membership_chunk(s, d_proofs.as<uint64_t>() + 48 * off, d_inf.as<uint8_t>() + 3 * off, std::min(VB_PASS, k - off), en, d_mem3.as<uint8_t>() + 3 * off);
    vb_join(s, evs.ev[1], evs.ev[2]);
    std::vector<uint8_t> mem3(3 * k);
    ZK_HIP(hipMemcpyAsync(mem3.data(), d_mem3.p, 3 * k, hipMemcpyDeviceToHost, s.main));
    ZK_HIP(hipStreamSynchronize(s.main));
    // proofs that failed membership are never listed
    std::vector<uint32_t> idx;
    for (size_t i = 0; i < k; i++)
        if (mem3[3 * i] && mem3[3 * i + 1] && mem3[3 * i + 2]) idx.push_back((uint32_t)i);
    std::vector<uint8_t> verdict(idx.size());
    (void)vb_each_pass(ctx, key, form, d_proofs.as<uint64_t>(), d_inf.as<uint8_t>(), idx.size() == k ? nullptr : idx.data(), idx.size(), verdict.data());
    memset(ok_each, 0, k);
    for (size_t j = 0; j < idx.size(); j++) ok_each[idx[j]] = verdict[j] ? 1 : 0;
    ZK_LANE_END(ctx)
}
}  // namespace

extern "C" {

int zkg16_verify_batch(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                       const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *public_inputs, const uint64_t *proofs, const uint8_t *inf,
                       const uint64_t *rho, size_t k, int *ok, uint8_t *ok_each) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_entry(ctx, key, vb_limbs(public_inputs), proofs, inf, false, nullptr, rho, k, ok, ok_each, nullptr);
}

int zkg16_verify_batch_wire(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                            const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *public_inputs, const uint8_t *proof_bytes,
                            const uint64_t *rho, size_t k, int *ok, uint8_t *ok_each, uint8_t *decode_status) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_entry(ctx, key, vb_limbs(public_inputs), nullptr, nullptr, true, proof_bytes, rho, k, ok, ok_each, decode_status);
}

int zkg16_verify_each(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                      const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *public_inputs, const uint64_t *proofs, const uint8_t *inf, size_t k,
                      uint8_t *ok_each) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_each_entry(ctx, key, vb_limbs(public_inputs), proofs, inf, k, ok_each);
}

// ---- the prime form: K requests of one trapdoor under the extended key (zkg16_prime_vk_extend), their inputs made on the device
int zkg16_verify_prime_batch(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                             const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *xs, const uint64_t *js, const uint64_t *proofs, const uint8_t *inf,
                             const uint64_t *rho, size_t k, int *ok, uint8_t *ok_each) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_entry(ctx, key, vb_prime(xs, js), proofs, inf, false, nullptr, rho, k, ok, ok_each, nullptr);
}

int zkg16_verify_prime_batch_wire(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                                  const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *xs, const uint64_t *js, const uint8_t *proof_bytes,
                                  const uint64_t *rho, size_t k, int *ok, uint8_t *ok_each, uint8_t *decode_status) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_entry(ctx, key, vb_prime(xs, js), nullptr, nullptr, true, proof_bytes, rho, k, ok, ok_each, decode_status);
}

// Stage entries: the inputs kernel and the sums kernels by themselves
int zkg16_prime_inputs_batch(zkg16_ctx *ctx, const uint64_t *xs, const uint64_t *js, size_t k, uint8_t *digests, uint32_t *n_out, uint64_t *public_inputs) {
    if (!ctx || ((!xs || !js || !digests || !n_out) && k)) return ZKG16_ERR_BAD_ARG;
    if (!k) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    hipStream_t st = ctx->stream;
    DevBuf d_xs(k * 8), d_js(k * 8), d_dig(k * 32), d_n(k * 4), d_pub(public_inputs ? k * 257 * 32 : 0);
    ZK_HIP(hipMemcpyAsync(d_xs.p, xs, k * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_js.p, js, k * 8, hipMemcpyHostToDevice, st));
    for (size_t off = 0; off < k; off += VB_PASS)
        vb_prime_inputs_launch(st, d_xs.as<uint64_t>() + off, d_js.as<uint64_t>() + off, std::min(VB_PASS, k - off), d_dig.as<uint32_t>() + 8 * off,
                               d_n.as<uint32_t>() + off, public_inputs ? d_pub.as<uint64_t>() + 4 * 257 * off : nullptr);
    ZK_HIP(hipMemcpyAsync(digests, d_dig.p, k * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(n_out, d_n.p, k * 4, hipMemcpyDeviceToHost, st));
    if (public_inputs) ZK_HIP(hipMemcpyAsync(public_inputs, d_pub.p, k * 257 * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_LANE_END(ctx)
}

int zkg16_prime_rho_sums(zkg16_ctx *ctx, const uint64_t *xs, const uint64_t *js, const uint64_t *rho, const uint8_t *live, size_t k, uint64_t *sums) {
    if (!ctx || ((!xs || !js || !rho || !sums) && k) || k >> 32) return ZKG16_ERR_BAD_ARG;
    if (!k) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    hipStream_t st = ctx->stream;
    DevBuf d_xs(k * 8), d_js(k * 8), d_dig(k * 32), d_rho(k * 16), d_live(live ? k : 0), d_part(vb_prime_sums_blocks(k) * 260 * 32), d_sums(260 * 32);
    ZK_HIP(hipMemcpyAsync(d_xs.p, xs, k * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_js.p, js, k * 8, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_rho.p, rho, k * 16, hipMemcpyHostToDevice, st));
    if (live) ZK_HIP(hipMemcpyAsync(d_live.p, live, k, hipMemcpyHostToDevice, st));
    for (size_t off = 0; off < k; off += VB_PASS)
        vb_prime_inputs_launch(st, d_xs.as<uint64_t>() + off, d_js.as<uint64_t>() + off, std::min(VB_PASS, k - off), d_dig.as<uint32_t>() + 8 * off, nullptr, nullptr);
    vb_prime_sums_launch(st, d_xs.as<uint64_t>(), d_js.as<uint64_t>(), d_dig.as<uint32_t>(), d_rho.as<uint64_t>(), live ? d_live.as<uint8_t>() : nullptr, k,
                         d_part.as<uint64_t>(), d_sums.as<uint64_t>());
    ZK_HIP(hipMemcpyAsync(sums, d_sums.p, 260 * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_LANE_END(ctx)
}

// ---- the u64 form: a key whose public inputs are plain 64-bit values, values = k x (num_instance - 1) u64
int zkg16_verify_batch_u64(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                           const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *values, const uint64_t *proofs, const uint8_t *inf, const uint64_t *rho,
                           size_t k, int *ok, uint8_t *ok_each) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_entry(ctx, key, vb_u64(values), proofs, inf, false, nullptr, rho, k, ok, ok_each, nullptr);
}

int zkg16_verify_batch_u64_wire(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                                const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *values, const uint8_t *proof_bytes, const uint64_t *rho,
                                size_t k, int *ok, uint8_t *ok_each, uint8_t *decode_status) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_entry(ctx, key, vb_u64(values), nullptr, nullptr, true, proof_bytes, rho, k, ok, ok_each, decode_status);
}

int zkg16_verify_each_u64(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72], const uint64_t *gamma_neg_coeffs,
                          const uint64_t *delta_neg_coeffs, size_t n_coeffs, const uint64_t *values, const uint64_t *proofs, const uint8_t *inf, size_t k,
                          uint8_t *ok_each) {
    const VbKey key{gamma_abc_g1, num_instance, alpha_beta, gamma_neg_coeffs, delta_neg_coeffs, n_coeffs};
    return vb_each_entry(ctx, key, vb_u64(values), proofs, inf, k, ok_each);
}

// Stage entries: the sums kernels and the X kernel by themselves
int zkg16_u64_rho_sums(zkg16_ctx *ctx, const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t k, uint64_t *sums) {
    if (!ctx || m == 0 || ((!values || !rho || !sums) && k) || k >> 32) return ZKG16_ERR_BAD_ARG;
    if (!k) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    hipStream_t st = ctx->stream;
    DevBuf d_values(k * m * 8), d_rho(k * 16), d_live(live ? k : 0), d_part(vb_u64_sums_partial_words(k, m) * 8), d_sums((m + 1) * 32);
    upload_h2d(ctx, d_values.p, values, k * m * 8);
    ZK_HIP(hipMemcpyAsync(d_rho.p, rho, k * 16, hipMemcpyHostToDevice, st));
    if (live) ZK_HIP(hipMemcpyAsync(d_live.p, live, k, hipMemcpyHostToDevice, st));
    vb_u64_sums_launch(st, d_values.as<uint64_t>(), m, d_rho.as<uint64_t>(), live ? d_live.as<uint8_t>() : nullptr, k, d_part.as<uint64_t>(), d_sums.as<uint64_t>());
    ZK_HIP(hipMemcpyAsync(sums, d_sums.p, (m + 1) * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_LANE_END(ctx)
}

int zkg16_u64_prepared_inputs(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t *values, const uint32_t *idx, size_t n,
                              uint64_t *x_out, uint8_t *inf_out) {
    if (!ctx || !gamma_abc_g1 || num_instance < 2 || ((!values || !x_out || !inf_out) && n) || n >> 32) return ZKG16_ERR_BAD_ARG;
    if (!n) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    hipStream_t st = ctx->stream;
    const size_t m = num_instance - 1;
    size_t rows = n;
    if (idx) {
        rows = 0;
        for (size_t j = 0; j < n; j++) rows = std::max<size_t>(rows, (size_t)idx[j] + 1);
    }
    std::vector<uint32_t> words(vb_points_count(num_instance));
    vb_points_words(gamma_abc_g1, num_instance, words.data());
    DevBuf d_pts(words.size() * 4), d_values(rows * m * 8), d_idx(idx ? n * 4 : 0), d_xk(vb_each_x_bytes(n)), d_have(n);
    ZK_HIP(hipMemcpyAsync(d_pts.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    upload_h2d(ctx, d_values.p, values, rows * m * 8);
    if (idx) ZK_HIP(hipMemcpyAsync(d_idx.p, idx, n * 4, hipMemcpyHostToDevice, st));
    for (size_t off = 0; off < n; off += VB_PASS)
        vb_u64_x_launch(st, d_pts.as<uint32_t>(), num_instance, idx ? d_values.as<uint64_t>() : d_values.as<uint64_t>() + m * off,
                        idx ? d_idx.as<uint32_t>() + off : nullptr, std::min(VB_PASS, n - off), d_xk.as<uint8_t>() + vb_each_x_bytes(off), d_have.as<uint8_t>() + off);
    std::vector<uint8_t> xk(vb_each_x_bytes(n)), have(n);
    ZK_HIP(hipMemcpyAsync(xk.data(), d_xk.p, xk.size(), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(have.data(), d_have.p, n, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    for (size_t j = 0; j < n; j++) {
        inf_out[j] = have[j] ? 0 : 1;
        if (have[j]) vb_point_limbs(xk.data() + vb_each_x_bytes(j), x_out + 12 * j);
        else memset(x_out + 12 * j, 0, 96);
    }
    ZK_LANE_END(ctx)
}

int zkg16_final_exp_batch(zkg16_ctx *ctx, const uint64_t *f, size_t n, uint64_t *out) {
    if (!ctx || ((!f || !out) && n)) return ZKG16_ERR_BAD_ARG;
    if (!n) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    DevBuf d_f(n * 576);
    upload_h2d(ctx, d_f.p, f, n * 576);
    for (size_t off = 0; off < n; off += VB_PASS)
        vb_final_exp_launch(ctx->stream, d_f.as<uint64_t>() + 72 * off, std::min(VB_PASS, n - off), d_f.as<uint64_t>() + 72 * off);
    ZK_HIP(hipMemcpyAsync(out, d_f.p, n * 576, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_LANE_END(ctx)
}

int zkg16_points_decompress_batch(zkg16_ctx *ctx, int group, const uint8_t *bytes, size_t n, uint64_t *out, uint8_t *inf, int validate, int *status) {
    if (!ctx || (group != 1 && group != 2) || ((!bytes || !out || !inf) && n)) return ZKG16_ERR_BAD_ARG;
    if (!n) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    const size_t w = group == 1 ? 12 : 24, nb = group == 1 ? 48 : 96;
    DevBuf d_b(n * nb), d_p(n * w * 8), d_i(n), d_s(n);
    upload_h2d(ctx, d_b.p, bytes, n * nb);
    const VbEndo en = vb_endo();
    for (size_t off = 0; off < n; off += VB_PASS)
        vb_decompress_launch(ctx->stream, group, d_b.as<uint8_t>() + nb * off, nb, std::min(VB_PASS, n - off), validate, en, d_p.as<uint64_t>() + w * off, w,
                             d_i.as<uint8_t>() + off, 1, d_s.as<uint8_t>() + off, 1);
    std::vector<uint8_t> st(n);
    ZK_HIP(hipMemcpyAsync(out, d_p.p, n * w * 8, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipMemcpyAsync(inf, d_i.p, n, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipMemcpyAsync(st.data(), d_s.p, n, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    bool any_bad = false;
    for (size_t i = 0; i < n; i++) {
        if (status) status[i] = st[i];
        any_bad = any_bad || st[i];
    }
    if (any_bad) return ZKG16_ERR_BAD_ARG;
    ZK_LANE_END(ctx)
}

int zkg16_miller_loop_batch(zkg16_ctx *ctx, const uint64_t *g1, const uint8_t *g1_inf, const uint64_t *g2, const uint8_t *g2_inf, size_t n, uint64_t *f_out) {
    if (!ctx || ((!g1 || !g2 || !f_out) && n)) return ZKG16_ERR_BAD_ARG;
    if (!n) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    DevBuf d_g1(n * 96), d_g2(n * 192), d_i1(n), d_i2(n), d_f(n * 576);
    upload_h2d(ctx, d_g1.p, g1, n * 96);
    upload_h2d(ctx, d_g2.p, g2, n * 192);
    if (g1_inf) ZK_HIP(hipMemcpyAsync(d_i1.p, g1_inf, n, hipMemcpyHostToDevice, ctx->stream));
    if (g2_inf) ZK_HIP(hipMemcpyAsync(d_i2.p, g2_inf, n, hipMemcpyHostToDevice, ctx->stream));
    for (size_t off = 0; off < n; off += VB_PASS)
        vb_miller_launch(ctx->stream, d_g1.as<uint64_t>() + 12 * off, 12, g1_inf ? d_i1.as<uint8_t>() + off : nullptr, d_g2.as<uint64_t>() + 24 * off, 24,
                         g2_inf ? d_i2.as<uint8_t>() + off : nullptr, 1, nullptr, std::min(VB_PASS, n - off), d_f.as<uint64_t>() + 72 * off);
    ZK_HIP(hipMemcpyAsync(f_out, d_f.p, n * 576, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_LANE_END(ctx)
}

int zkg16_point_check_batch(zkg16_ctx *ctx, int group, const uint64_t *points, const uint8_t *inf, size_t n, uint8_t *ok_out) {
    if (!ctx || (group != 1 && group != 2) || ((!points || !ok_out) && n)) return ZKG16_ERR_BAD_ARG;
    if (!n) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    const size_t w = group == 1 ? 12 : 24;
    DevBuf d_p(n * w * 8), d_i(n), d_ok(n);
    upload_h2d(ctx, d_p.p, points, n * w * 8);
    if (inf) ZK_HIP(hipMemcpyAsync(d_i.p, inf, n, hipMemcpyHostToDevice, ctx->stream));
    const VbEndo en = vb_endo();
    for (size_t off = 0; off < n; off += VB_PASS)
        vb_membership_launch(ctx->stream, group, d_p.as<uint64_t>() + w * off, w, inf ? d_i.as<uint8_t>() + off : nullptr, 1, std::min(VB_PASS, n - off), en,
                             d_ok.as<uint8_t>() + off, 1);
    ZK_HIP(hipMemcpyAsync(ok_out, d_ok.p, n, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_LANE_END(ctx)
}
int zkg16_verify_batch_timings(zkg16_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms || cap < 0) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(ctx->lane_mu);
    const int n = cap < V_COUNT ? cap : V_COUNT;
    memcpy(ms, ctx->vb_timings, n * sizeof(float));
    return n;
}

}  // extern "C"
