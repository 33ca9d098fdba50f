// libzkg16 C ABI, part 7 of 8 (api.hip): re-randomising.
#include "api_internal.hpp"

using namespace zk;

// ------------------------------------------------------------------------------------------------ re-randomising
// (rerandomize_dev.cuh.)  A' = r1^-1 A, B' = r1 B + (r1 r2) delta, C' = C + r2 A for k proofs of one key: the G2 kernel on the lane's
// main stream, the G1 kernel beside it on a second one.  From wire bytes the decompress and membership kernels run in front as they
// do for zkg16_verify_batch_wire, nothing comes back in between (the kernels read the statuses and verdicts where they lie), and the
// compress kernel turns the results into the bytes that travel back.
namespace {
// why a call is refused, or null; *text names the proof and the multiplier
const char *rr_refusal(const uint64_t *delta, const void *proofs, const uint64_t *r1, const uint64_t *r2, size_t k, const void *out, const void *out2, std::string *text) {
    if (k == 0) return "no proofs";
    if (!delta || !proofs || !r1 || !r2 || !out || !out2) return "a null pointer";
    uint64_t any = 0;
    for (int t = 0; t < 24; t++) any |= delta[t];
    if (!any) return "delta_g2 is all-zero limbs";
    uint64_t mod[4];
    for (int i = 0; i < 4; i++) mod[i] = (uint64_t)FrP::mod(2 * i) | (uint64_t)FrP::mod(2 * i + 1) << 32;
    for (size_t i = 0; i < k; i++)
        for (int which = 0; which < 2; which++) {
            const uint64_t *v = (which ? r2 : r1) + 4 * i;
            bool less = false;
            for (int t = 0; t < 4; t++) less = v[t] < mod[t] || (v[t] == mod[t] && less);
            const bool zero = !(v[0] | v[1] | v[2] | v[3]);
            if (zero || !less) {
                char buf[96];
                snprintf(buf, sizeof buf, "r%d of proof %zu is %s", which + 1, i, zero ? "zero" : "not below r");
                *text = buf;
                return text->c_str();
            }
        }
    return nullptr;
}
int rr_refuse(zkg16_ctx *ctx, const char *entry, const char *why) {
    const std::string text = std::string(entry) + ": " + why;
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->lane_mu);
        ctx->last_error = text;
    } else {
        host_last_error() = text;
    }
    return ZKG16_ERR_BAD_ARG;
}
void rr_host(const uint64_t *delta, const uint64_t *proofs, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2, size_t k, int threads, uint64_t *out,
             uint8_t *out_inf) {
    vb_parallel(k, threads, 1, [&](size_t lo, size_t hi) { vb_rerandomize_host_range(proofs, inf, delta, r1, r2, lo, hi, out, out_inf); });
}
// the wire form on the host: decode (validating), the host form, encode; a proof that did not decode gets zero bytes
void rr_host_wire(const uint64_t *delta, const uint8_t *bytes, const uint64_t *r1, const uint64_t *r2, size_t k, uint8_t *bytes_out, uint8_t *st) {
    std::vector<uint64_t> proofs(48 * k), out(48 * k);
    std::vector<uint8_t> inf(3 * k), out_inf(3 * k);
    vb_wire_decode_host(bytes, k, 1, 0, proofs.data(), inf.data(), st);
    rr_host(delta, proofs.data(), inf.data(), r1, r2, k, 0, out.data(), out_inf.data());
    for (size_t i = 0; i < k; i++) {
        uint8_t *b = bytes_out + 192 * i;
        if (st[3 * i] || st[3 * i + 1] || st[3 * i + 2]) {
            memset(b, 0, 192);
            continue;
        }
        (void)zkg16_points_compress(1, out.data() + 48 * i, out_inf.data() + 3 * i, 1, b);
        (void)zkg16_points_compress(2, out.data() + 48 * i + 12, out_inf.data() + 3 * i + 1, 1, b + 48);
        (void)zkg16_points_compress(1, out.data() + 48 * i + 36, out_inf.data() + 3 * i + 2, 1, b + 144);
    }
}
void rr_publish(zkg16_ctx *root, const float tm[R_COUNT]) {
    std::lock_guard<std::mutex> lk(root->lane_mu);
    memcpy(root->rr_timings, tm, sizeof root->rr_timings);
}
bool rr_any_failed(const uint8_t *st, size_t k) {
    bool any = false;
    for (size_t j = 0; j < 3 * k; j++) any = any || st[j];
    return any;
}

// The device form.  wire == null: proofs / inf are the caller's limbs and flags, and proofs_out / inf_out take the results.
// wire != null (k x 192 bytes): bytes_out takes k x 192 bytes and st (k x 3) the statuses of the validating host decoder
int rr_device(zkg16_ctx *ctx, const uint64_t *delta, const uint64_t *proofs, const uint8_t *inf, const uint8_t *wire, const uint64_t *r1, const uint64_t *r2, size_t k,
              uint64_t *proofs_out, uint8_t *inf_out, uint8_t *bytes_out, uint8_t *st, double t_all) {
    float tm[R_COUNT] = {0};
    ZK_LANE_BEGIN(ctx)
    const VbStreams s = vb_streams(ctx);
    hipStream_t s_main = s.main, s_c = s.c;
    const size_t pass = ctx->opt.rerandomize_pass > 0 ? (size_t)ctx->opt.rerandomize_pass : VB_PASS;
    VbEvents evs;
    hipEvent_t e_0 = evs.ev[0], e_up = evs.ev[1], e_c = evs.ev[2], e_b = evs.ev[3], e_dec = evs.ev[4], e_c2 = evs.ev[5], e_b2 = evs.ev[6], e_mem = evs.ev[7],
               e_g1a = evs.ev[8], e_g1b = evs.ev[9], e_g2b = evs.ev[10], e_cmp = evs.ev[11], e_rb = evs.ev[12];
    DevBuf d_proofs(k * 48 * 8), d_inf(3 * k), d_r1(k * 32), d_r2(k * 32), d_delta(24 * 8), d_out(k * 48 * 8), d_oinf(3 * k);
    DevBuf d_wire(wire ? k * 192 : 0), d_st(wire ? 3 * k : 0), d_mem3(wire ? 3 * k : 0), d_bytes(wire ? k * 192 : 0);
    std::vector<uint8_t> flags;
    ZK_HIP(hipEventRecord(e_0, s_main));
    if (wire) {
        upload_h2d(ctx, d_wire.p, wire, k * 192);
    } else {
        // load_pt's rule on the flags, as the verifiers apply it; the kernels look at the limbs as well
        std::vector<uint8_t> none;
        if (!inf) none.assign(3 * k, 0);
        flags = vb_flags(proofs, inf ? inf : none.data(), k);
        upload_h2d(ctx, d_proofs.p, proofs, k * 48 * 8);
        upload_h2d(ctx, d_inf.p, flags.data(), 3 * k);
    }
    upload_h2d(ctx, d_r1.p, r1, k * 32);
    upload_h2d(ctx, d_r2.p, r2, k * 32);
    upload_h2d(ctx, d_delta.p, delta, 24 * 8);
    vb_fork(s, e_up);
    const uint8_t *st3 = nullptr, *mem3 = nullptr;
    if (wire) {
        const VbEndo en = vb_endo();
        vb_wire_decode(s, e_c, e_b, d_wire.as<uint8_t>(), k, pass, en, d_proofs.as<uint64_t>(), d_inf.as<uint8_t>(), d_st.as<uint8_t>());
        vb_fork(s, e_dec);
        for (size_t off = 0; off < k; off += pass)
            vb_membership_chunk(s, d_proofs.as<uint64_t>() + 48 * off, d_inf.as<uint8_t>() + 3 * off, std::min(pass, k - off), en,
                                d_mem3.as<uint8_t>() + 3 * off);
        vb_join(s, e_c2, e_b2);
        st3 = d_st.as<uint8_t>();
        mem3 = d_mem3.as<uint8_t>();
    }
    ZK_HIP(hipEventRecord(e_mem, s_main));
    ZK_HIP(hipStreamWaitEvent(s_c, e_mem, 0));
    ZK_HIP(hipEventRecord(e_g1a, s_c));
    for (size_t off = 0; off < k; off += pass)
        vb_rerandomize_launch(s_c, s_main, d_proofs.as<uint64_t>() + 48 * off, d_inf.as<uint8_t>() + 3 * off, d_delta.as<uint64_t>(), d_r1.as<uint64_t>() + 4 * off,
                              d_r2.as<uint64_t>() + 4 * off, st3 ? st3 + 3 * off : nullptr, mem3 ? mem3 + 3 * off : nullptr, std::min(pass, k - off),
                              d_out.as<uint64_t>() + 48 * off, d_oinf.as<uint8_t>() + 3 * off);
    ZK_HIP(hipEventRecord(e_g1b, s_c));
    ZK_HIP(hipEventRecord(e_g2b, s_main));
    ZK_HIP(hipStreamWaitEvent(s_main, e_g1b, 0));
    std::vector<uint8_t> dec_st, mem;
    if (wire) {
        for (size_t off = 0; off < k; off += pass) {
            const size_t n = std::min(pass, k - off);
            const uint64_t *pts = d_out.as<uint64_t>() + 48 * off;
            const uint8_t *fl = d_oinf.as<uint8_t>() + 3 * off;
            uint8_t *by = d_bytes.as<uint8_t>() + 192 * off;
            vb_compress_launch(s_main, 1, pts, 48, fl, 3, n, st3 + 3 * off, mem3 + 3 * off, by, 192);
            vb_compress_launch(s_main, 2, pts + 12, 48, fl + 1, 3, n, st3 + 3 * off, mem3 + 3 * off, by + 48, 192);
            vb_compress_launch(s_main, 1, pts + 36, 48, fl + 2, 3, n, st3 + 3 * off, mem3 + 3 * off, by + 144, 192);
        }
        ZK_HIP(hipEventRecord(e_cmp, s_main));
        dec_st.resize(3 * k);
        mem.resize(3 * k);
        ZK_HIP(hipMemcpyAsync(bytes_out, d_bytes.p, k * 192, hipMemcpyDeviceToHost, s_main));
        ZK_HIP(hipMemcpyAsync(dec_st.data(), d_st.p, 3 * k, hipMemcpyDeviceToHost, s_main));
        ZK_HIP(hipMemcpyAsync(mem.data(), d_mem3.p, 3 * k, hipMemcpyDeviceToHost, s_main));
    } else {
        ZK_HIP(hipEventRecord(e_cmp, s_main));
        ZK_HIP(hipMemcpyAsync(proofs_out, d_out.p, k * 48 * 8, hipMemcpyDeviceToHost, s_main));
        ZK_HIP(hipMemcpyAsync(inf_out, d_oinf.p, 3 * k, hipMemcpyDeviceToHost, s_main));
    }
    ZK_HIP(hipEventRecord(e_rb, s_main));
    ZK_HIP(hipStreamSynchronize(s_main));
    if (wire)
        for (size_t j = 0; j < 3 * k; j++) st[j] = dec_st[j] ? dec_st[j] : (mem[j] ? 0 : 5);
    tm[R_UPLOAD] = vb_elapsed(e_0, e_up);
    if (wire) tm[R_DECODE] = vb_elapsed(e_up, e_mem);
    tm[R_G1] = vb_elapsed(e_g1a, e_g1b);
    tm[R_G2] = vb_elapsed(e_mem, e_g2b);
    if (wire) tm[R_COMPRESS] = vb_elapsed(e_g2b, e_cmp);      // from the end of the G2 kernel: the wait for the G1 kernel, if any, is in it
    tm[R_READBACK] = vb_elapsed(e_cmp, e_rb);
    tm[R_TOTAL] = (float)(now_ms() - t_all);
    rr_publish(root, tm);
    ZK_LANE_END(ctx)
}
template <class Form>
int rr_answer_on_host(zkg16_ctx *ctx, double t_all, Form &&form) {
    float tm[R_COUNT] = {0};
    try {
        form();
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    tm[R_TOTAL] = (float)(now_ms() - t_all);
    tm[R_HOST_FORM] = 1;
    rr_publish(ctx, tm);
    return ZKG16_OK;
}
}  // namespace

extern "C" {

int zkg16_rerandomize_batch_host(const uint64_t delta_g2[24], const uint64_t *proofs, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2, size_t k, int threads,
                                 uint64_t *proofs_out, uint8_t *inf_out) {
    std::string text;
    if (const char *why = rr_refusal(delta_g2, proofs, r1, r2, k, proofs_out, inf_out, &text)) return rr_refuse(nullptr, "zkg16_rerandomize_batch_host", why);
    try {
        rr_host(delta_g2, proofs, inf, r1, r2, k, threads, proofs_out, inf_out);
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

int zkg16_rerandomize_batch(zkg16_ctx *ctx, const uint64_t delta_g2[24], const uint64_t *proofs, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2, size_t k,
                            uint64_t *proofs_out, uint8_t *inf_out) {
    if (!ctx) return ZKG16_ERR_BAD_ARG;
    std::string text;
    if (const char *why = rr_refusal(delta_g2, proofs, r1, r2, k, proofs_out, inf_out, &text)) return rr_refuse(ctx, "zkg16_rerandomize_batch", why);
    const double t_all = now_ms();
    if (k < (size_t)ctx->opt.rerandomize_min) return rr_answer_on_host(ctx, t_all, [&] { rr_host(delta_g2, proofs, inf, r1, r2, k, 0, proofs_out, inf_out); });
    return rr_device(ctx, delta_g2, proofs, inf, nullptr, r1, r2, k, proofs_out, inf_out, nullptr, nullptr, t_all);
}

int zkg16_rerandomize_batch_wire(zkg16_ctx *ctx, const uint64_t delta_g2[24], const uint8_t *proof_bytes, const uint64_t *r1, const uint64_t *r2, size_t k,
                                 uint8_t *bytes_out, uint8_t *status) {
    if (!ctx) return ZKG16_ERR_BAD_ARG;
    std::string text;
    if (const char *why = rr_refusal(delta_g2, proof_bytes, r1, r2, k, bytes_out, bytes_out, &text)) return rr_refuse(ctx, "zkg16_rerandomize_batch_wire", why);
    const double t_all = now_ms();
    std::vector<uint8_t> st;
    try {
        st.resize(3 * k);
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    const int rc = k < (size_t)ctx->opt.rerandomize_min
                       ? rr_answer_on_host(ctx, t_all, [&] { rr_host_wire(delta_g2, proof_bytes, r1, r2, k, bytes_out, st.data()); })
                       : rr_device(ctx, delta_g2, nullptr, nullptr, proof_bytes, r1, r2, k, nullptr, nullptr, bytes_out, st.data(), t_all);
    if (rc != ZKG16_OK) return rc;
    if (status) memcpy(status, st.data(), 3 * k);
    else if (rr_any_failed(st.data(), k)) return rr_refuse(ctx, "zkg16_rerandomize_batch_wire", "a proof did not decode and status is null");
    return ZKG16_OK;
}

int zkg16_points_compress_batch(zkg16_ctx *ctx, int group, const uint64_t *points, const uint8_t *inf, size_t n, uint8_t *out) {
    if (!ctx || (group != 1 && group != 2) || ((!points || !out) && n)) return ZKG16_ERR_BAD_ARG;
    if (!n) return ZKG16_OK;
    ZK_LANE_BEGIN(ctx)
    const size_t w = group == 1 ? 12 : 24, nb = group == 1 ? 48 : 96;
    DevBuf d_p(n * w * 8), d_i(inf ? n : 0), d_b(n * nb);
    upload_h2d(ctx, d_p.p, points, n * w * 8);
    if (inf) ZK_HIP(hipMemcpyAsync(d_i.p, inf, n, hipMemcpyHostToDevice, ctx->stream));
    for (size_t off = 0; off < n; off += VB_PASS)
        vb_compress_launch(ctx->stream, group, d_p.as<uint64_t>() + w * off, w, inf ? d_i.as<uint8_t>() + off : nullptr, 1, std::min(VB_PASS, n - off), nullptr, nullptr,
                           d_b.as<uint8_t>() + nb * off, nb);
    ZK_HIP(hipMemcpyAsync(out, d_b.p, n * nb, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_LANE_END(ctx)
}

int zkg16_rerandomize_timings(zkg16_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms || cap < 0) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(ctx->lane_mu);
    const int n = cap < R_COUNT ? cap : R_COUNT;
    memcpy(ms, ctx->rr_timings, n * sizeof(float));
    return n;
}

}  // extern "C"
