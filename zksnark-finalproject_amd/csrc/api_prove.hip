// libzkg16 C ABI, part 3 of 8 (api.hip): the prove pipeline and its O(1) host tail.  Mirrors ark-groth16 0.4
// `create_proof_with_reduction_and_matrices` + `create_proof_with_assignment` (src/prover.rs) as the reference
// reaches them from src/arkworks/backend/matrix_proof.rs:139-140.
//
// prove_device (one proof, possibly a shard, in rounds, or a group rank) and prove_batch_device (K proofs in one pass) stay two
// functions — they differ in the collect phase, in rounds, in wm_first and in group support — but every step they have in common
// is ONE function below, called by both in the same order: that is what keeps proof k of a batch byte-identical to the single proof.
#include "api_internal.hpp"
#include "group.hpp"

using namespace zk;

namespace {

// A throw between the first enqueue and the last collect (e.g. out of memory in a slot's bucket array) must not leave
// kernels of this proof in flight: the next proof on the ctx rewrites extra_host and reuses the workspaces and slots.
struct DrainOnError {
    zkg16_ctx *c;
    bool ok = false;
    ~DrainOnError() {
        if (ok) return;
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->wm_stream);
        for (auto &sl : c->slots) {
            if (sl.stream) (void)hipStreamSynchronize(sl.stream);
            sl.active = sl.pending_reduce = sl.fixups_pending = sl.last_of_proof = false;
        }
    }
};

// Every launch helper targets ctx->stream: while this guard lives, the witness map's stream takes its place (option wm_concurrent;
// measured in one process, n = 32: 18.15 vs 18.58 ms in order; n = 12: 10.05 vs 11.16 ms).  The block it is declared in ends before
// the next launch on the main stream.
struct WmStreamSwap {
    zkg16_ctx *c;
    const bool on;
    explicit WmStreamSwap(zkg16_ctx *ctx) : c(ctx), on(ctx->opt.wm_concurrent != 0) { if (on) std::swap(c->stream, c->wm_stream); }
    ~WmStreamSwap() { if (on) std::swap(c->stream, c->wm_stream); }
    WmStreamSwap(const WmStreamSwap &) = delete;
    WmStreamSwap &operator=(const WmStreamSwap &) = delete;
};

// ---- option "check_satisfied": the pass's witness map fills 2 K device words (n_bad | first_bad: r1cs_check_run) right after its
// SpMV; they are read when the pass's results have been collected — all its device work is over by then — and appended to the
// lane's verdicts, which the entry point consults before it writes anything.  Off: a null pointer, no allocation, no launch.
uint64_t *check_begin(zkg16_ctx *ctx, size_t K) {
    if (!ctx->opt.check_satisfied) return nullptr;
    ctx->check_dev.ensure(2 * K * sizeof(uint64_t));
    return ctx->check_dev.as<uint64_t>();
}
void check_collect(zkg16_ctx *ctx, const uint64_t *words, size_t K) {
    if (!words) return;
    std::vector<uint64_t> w(2 * K);
    ZK_HIP(hipMemcpy(w.data(), words, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    ctx->check_n_bad.insert(ctx->check_n_bad.end(), w.begin(), w.begin() + K);
    ctx->check_first_bad.insert(ctx->check_first_bad.end(), w.begin() + K, w.end());
}
void check_reset(zkg16_ctx *ctx) {
    ctx->check_n_bad.clear();
    ctx->check_first_bad.clear();
}
bool check_failed(const zkg16_ctx *ctx) {
    for (const uint64_t n : ctx->check_n_bad)
        if (n) return true;
    return false;
}

// The z-side term lists: `z` (A and L) and, when more than 5 % of the terms (the z slice + the r, s, -rs slots) have the point at
// infinity as their B base, `zb` without those terms (B1 and B2) — worth a second (0.3 ms) list.
struct ZPlans {
    MsmPlan z, zb;
    bool b_sparse = false;
    const MsmPlan &b() const { return b_sparse ? zb : z; }
};
void build_z_plans(zkg16_ctx *ctx, ScalarSrc zsrc, const PkDev &pk, MsmWorkspace &ws_z, MsmWorkspace &ws_zb, ZPlans &p) {
    p.b_sparse = pk.b_skipped * 20 > (pk.z_hi - pk.z_lo) + 3;
    const int tz = pk.tab_c_z;
    msm_plan_build(ctx, ws_z, zsrc, p.z, tz, tz != 0);
    if (!p.b_sparse) return;
    // B1 and B2 share a plan without the terms whose bases are infinity (see b_density_mask_kernel)
    // (measured: 128x128 with window tables 154.5 -> 153.65 ms, 32x32 11.97 -> 11.68; with a plain key 168.55 -> 169.2, so only with tables
    // unless option b_filter = 1 asks for it)
    if ((ctx->opt.b_filter == 1 || (ctx->opt.b_filter == 0 && tz != 0)) && ctx->opt.sort_mode == 0) {
        msm_plan_filter(ctx, ws_z, p.z, pk.b_mask.as<uint8_t>(), ws_zb, p.zb);
    } else {
        zsrc.mask = pk.b_mask.as<uint8_t>();
        msm_plan_build(ctx, ws_zb, zsrc, p.zb, tz, tz != 0);
    }
}
// The four z-side accumulations on the main stream, G2 first: its long reduction then hides behind the G1 accumulations.
void enqueue_z_accs(zkg16_ctx *ctx, PkDev &pk, const ZPlans &p, int round) {
    MsmWorkspace &wsb = p.b_sparse ? ctx->ws_zb : ctx->ws_z;
    msm_g2_enqueue_acc(ctx, wsb, p.b(), pk.b2.as<G2AffineU>(), ctx->slots[0], round, pk.pad_z_g2);
    msm_g1_enqueue_acc(ctx, ctx->ws_z, p.z, pk.l.as<G1AffineU>(), ctx->slots[2], round, pk.pad_z_g1);
    msm_g1_enqueue_acc(ctx, ctx->ws_z, p.z, pk.a.as<G1AffineU>(), ctx->slots[3], round, pk.pad_z_g1);
    msm_g1_enqueue_acc(ctx, wsb, p.b(), pk.b1.as<G1AffineU>(), ctx->slots[4], round, pk.pad_z_g1);
}
// ... and their reductions (B2, L, A, B1), whose first packet is a wait
void enqueue_z_reduces(zkg16_ctx *ctx) {
    msm_g2_enqueue_reduce(ctx, ctx->slots[0]);
    msm_g1_enqueue_reduce(ctx, ctx->slots[2]);
    msm_g1_enqueue_reduce(ctx, ctx->slots[3]);
    msm_g1_enqueue_reduce(ctx, ctx->slots[4]);
}

// s (A + alpha) and r (B1 + beta) of an un-sharded proof, formed as soon as A / B1 is collected (Partials::have_early)
G1XYZZ early_s_a(const PkDev &pk, G1XYZZ a, const Fr &s) {
    xyzz_madd(a, pk.alpha_g1, false);
    return xyzz_mul(a, fp_from_mont(s).l);
}
G1XYZZ early_r_b1(const PkDev &pk, G1XYZZ b1, const Fr &r) {
    xyzz_madd(b1, pk.beta_g1, false);
    return xyzz_mul(b1, fp_from_mont(r).l);
}

// T_ACC_* / T_RED_* from the slots' event pairs, T_HORNER_* from their host times
void record_msm_timings(zkg16_ctx *ctx, bool h_ran, bool z_ran) {
    const int slot_of[5] = {1, 2, 3, 4, 0};     // H, L, A, B1, B2
    for (int k = 0; k < 5; k++) {
        MsmSlot &sl = ctx->slots[slot_of[k]];
        const bool ran = k == 0 ? h_ran : z_ran;
        float acc_ms = 0, red_ms = 0;
        if (ran && sl.acc_start && hipEventElapsedTime(&acc_ms, sl.acc_start, sl.acc_done) != hipSuccess) { acc_ms = 0; (void)hipGetLastError(); }
        if (ran && sl.red_start && hipEventElapsedTime(&red_ms, sl.red_start, sl.red_done) != hipSuccess) { red_ms = 0; (void)hipGetLastError(); }
        ctx->timings[T_ACC_H + k] = acc_ms;
        ctx->timings[T_RED_H + k] = red_ms;
    }
    ctx->timings[T_HORNER_H] = h_ran ? ctx->slots[1].collect_host_ms : 0;
    ctx->timings[T_HORNER_Z] = z_ran ? ctx->slots[0].collect_host_ms + ctx->slots[2].collect_host_ms + ctx->slots[3].collect_host_ms + ctx->slots[4].collect_host_ms : 0;
}
// the device times of a pass from its events (0-1: z-side sort, 2-3: witness map, 3-4: h-side sort) and its wall time since t0
void record_pass_timings(zkg16_ctx *ctx, const hipEvent_t *ev, double t0) {
    float ms;
    ctx->timings[T_SPMV] = 0;
    ZK_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
    ctx->timings[T_WITNESS_MAP] = ms;
    ZK_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ctx->timings[T_SORT] = ms;
    ZK_HIP(hipEventElapsedTime(&ms, ev[3], ev[4]));
    ctx->timings[T_SORT] += ms;
    ctx->timings[T_TOTAL] = (float)(now_ms() - t0);
}

// Host tail (a9): A = alpha + MSM_a, B = beta + MSM_b, C = s*A + r*B1 + MSM_l + MSM_h.
// (r*delta, s*delta and -rs*delta already ride inside the MSMs as three extra (base, scalar) slots.)
void prove_tail_pts(const G1Affine &alpha_g1, const G1Affine &beta_g1, const G2Affine &beta_g2, const Fr &r, const Fr &s,
                    const Partials &p, uint64_t *proof_out, uint8_t *inf_out) {
    G1XYZZ A = p.a;
    xyzz_madd(A, alpha_g1, false);
    G1XYZZ B1 = p.b1;
    xyzz_madd(B1, beta_g1, false);
    G2XYZZ B2 = p.b2;
    xyzz_madd(B2, beta_g2, false);
    G1XYZZ C, rB;
    if (p.have_early) {
        C = p.s_a;
        rB = p.r_b1;
    } else {
        const Fr rc = fp_from_mont(r), sc = fp_from_mont(s);
        C = xyzz_mul(A, sc.l);
        rB = xyzz_mul(B1, rc.l);
    }
    xyzz_add(C, rB);
    xyzz_add(C, p.l);
    xyzz_add(C, p.h);
    point_to_abi(xyzz_to_affine(A), proof_out, inf_out);
    point_to_abi(xyzz_to_affine(B2), proof_out + 12, inf_out + 1);
    point_to_abi(xyzz_to_affine(C), proof_out + 36, inf_out + 2);
}

}  // namespace

namespace zk {

// The device part of a proof: witness map + the five MSMs over this ctx's pk shard.  A shard is a pair of index ranges:
// [z_lo, z_hi) of the a / b_g1 / b_g2 / l queries and [h_lo, h_hi) of h_query.  A rank whose h range is empty skips the
// witness map and the H MSM altogether, one whose z range is empty (and which does not carry the r, s, -rs terms) skips the
// four z-side MSMs — this is what lets the ranks of a multi-GPU proof take different roles (zkg16_shard_plan).
// zp (zkg16_prove_matrix): the assignment is still being produced — part k of it becomes valid when zp->produce(k) has queued
// its kernels on the main stream.  The z-side MSMs then run in rounds, one per part, over the terms of that part only (digits
// of the other scalars count as zero), each round's buckets are summed into the MSM's bucket array and ONE reduction follows;
// the witness map waits for the last part.
// grp (zkg16_prove_group): this rank's share of a split witness map instead of the whole one.
void prove_device(zkg16_ctx *ctx, PkDev &pk, R1csDev &rc, WitnessDev &wit, const Fr &r, const Fr &s, Partials &out,
                  const std::function<void()> *before_witness_map, const ZParts *zp, GroupRank *grp, bool may_check) {
    const size_t m_total = rc.num_variables;
    if (wit.n != m_total || pk.m_total != m_total) throw HipError{hipErrorInvalidValue, "prove: assignment / key length mismatch", __FILE__, __LINE__};
    const size_t N = (size_t)1 << rc.log_n;
    if (pk.n_h_total != N - 1) throw HipError{hipErrorInvalidValue, "prove: h_query length != N-1", __FILE__, __LINE__};
    EventSet evs;                         // 0-1: z-side sort (main stream), 2-4: witness map / h-side sort (aux stream)
    hipEvent_t *ev = evs.ev;
    DrainOnError drain{ctx};
    ctx->batch_terms_set = false;
    check_reset(ctx);
    // group calls never check (may_check false: with a split witness map no rank sees every row); a rank without an h range runs no SpMV
    uint64_t *const chk = (may_check && pk.h_hi > pk.h_lo && !grp) ? check_begin(ctx, 1) : nullptr;
    const double t0 = now_ms();

    // ---- main stream: the z-side scalar vector (z-slice || r, s, -rs), read in place by the digit kernel -> digits -> sort.
    // It does not depend on the witness map, so the G2 accumulation can start while h is still being computed on the aux stream.
    const size_t nz = pk.z_hi - pk.z_lo;
    const size_t nh = pk.h_hi - pk.h_lo;
    const bool z_side = nz > 0 || pk.blinding;
    ZPlans plans;
    MsmPlan plan_h;
    out.h = out.l = out.a = out.b1 = G1XYZZ::inf();
    out.b2 = G2XYZZ::inf();
    ZK_HIP(hipEventRecord(ev[0], ctx->stream));
    ctx->ws_z.last_tb = ctx->ws_zb.last_tb = ctx->ws_h.last_tb = 0;
    ctx->last_msm_group = 0;              // ws_h and slots[0] are the proof's from here on: zkg16_last_msm_state reports zeros
    const bool trace = getenv("ZKG16_TRACE_HOST") != nullptr;
    const int parts = zp ? zp->parts : 1;
    const bool rounds = parts > 1 && z_side && zp->part_of != nullptr;
    // ---- the four z-side accumulations go onto the main stream BEFORE the witness map's ~40 launches (enqueue_z_accs); their
    // reductions only after those launches (enqueue_z_reduces).  Kernel trace at n = 32: queued after the witness map, the G2
    // accumulation started 2.0 ms into the proof with its inputs ready at 0.6 ms.
    // (Tried and dropped, 128x128: sorting the B-side list first and the full list on another stream underneath the G2
    // accumulation, with the witness map held back until the first list exists — the accumulation then starts 9 instead of
    // 15 ms into the proof, and the proof takes the same 171-172 ms: kernels that share the device slow each other by about
    // what the overlap saves, the proof is the SUM of its kernels' work.  A high-priority witness-map stream: +1 ms.)
    if (zp && !rounds)
        for (int k = 0; k < parts; k++) zp->produce(k);       // no rounds (one part, or no z side here): the whole assignment first
    if (z_side) {
        if (!ctx->extra_host) ZK_HIP(hipHostMalloc(&ctx->extra_host, 3 * sizeof(Fr), hipHostMallocDefault));
        Fr *extra = reinterpret_cast<Fr *>(ctx->extra_host);
        extra[0] = pk.blinding ? r : Fr::zero();              // the r/s/-rs terms are added by one shard only
        extra[1] = pk.blinding ? s : Fr::zero();
        extra[2] = pk.blinding ? fp_neg(fp_mul(r, s)) : Fr::zero();
        // the digit kernel reads the three extra scalars straight from this pinned (device-visible) host buffer: no host-to-device
        // copy is queued; the buffer is rewritten only by the next proof, which starts after this one has been collected
        for (int k = 0; k < (rounds ? parts : 1); k++) {
            if (rounds) zp->produce(k);
            ScalarSrc zsrc{wit.z.as<Fr>() + pk.z_lo, nz, extra, 3, true, nullptr};
            if (rounds) { zsrc.part = zp->part_of; zsrc.want_part = k; }
            build_z_plans(ctx, zsrc, pk, ctx->ws_z, ctx->ws_zb, plans);
            if (rounds) enqueue_z_accs(ctx, pk, plans, k);
        }
    }
    ZK_HIP(hipEventRecord(ev[1], ctx->stream));
    if (zp) ZK_HIP(hipEventRecord(ev[5], ctx->stream));       // z is complete once the main stream gets here
    // the z-side accumulations either start at once (their kernels and the witness map's then share the device) or wait for the
    // witness map, which then has the device to itself and lets the h-side sort run underneath the accumulations.  Measured: with
    // window tables 128x128 154.5 vs 153.65 ms (32x32 11.7 vs 12.2, 46x46 19.7 vs 20.3), with a plain key 128x128 168.6 vs 171.2 —
    // so by default only from 2^23 on and only for keys with tables; never when the matrices are still being uploaded on the
    // witness map's stream (the accumulations are what hides that).
    const int wm_first = (!nh || rounds) ? 0 : ctx->opt.wm_first >= 0 ? ctx->opt.wm_first : (rc.log_n >= 23 && pk.tab_c_h != 0 && !before_witness_map) ? 1 : 0;
    if (z_side && !wm_first && !rounds) enqueue_z_accs(ctx, pk, plans, -1);

    // ---- R1CS -> QAP witness map (a3-a5 of SURVEY.md 8a) and the h-side sort, on a third stream concurrently with the z-side work
    {
        WmStreamSwap on_wm_stream(ctx);
        // zkg16_prove (host pointers): the matrices are uploaded here, on the witness map's stream, while the z-side
        // accumulations queued above already keep the device busy
        if (before_witness_map) (*before_witness_map)();
        if (zp) ZK_HIP(hipStreamWaitEvent(ctx->stream, ev[5], 0));
        ZK_HIP(hipEventRecord(ev[2], ctx->stream));
        Fr *h = nullptr;
        if (nh && grp) group_witness_map_run(ctx, rc, wit.z.as<Fr>(), &h, *grp);
        else if (nh) witness_map_run(ctx, rc, wit.z.as<Fr>(), &h, nullptr, chk);
        ZK_HIP(hipEventRecord(ev[3], ctx->stream));
        if (nh) {
            const ScalarSrc hsrc{h + pk.h_lo, nh, nullptr, 0, true, nullptr};
            msm_plan_build(ctx, ctx->ws_h, hsrc, plan_h, pk.tab_c_h ? pk.tab_c_h : ctx->opt.window_bits_h, pk.tab_c_h != 0);
        }
        ZK_HIP(hipEventRecord(ev[4], ctx->stream));
    }
    if (wm_first) {
        ZK_HIP(hipStreamWaitEvent(ctx->stream, wm_first == 2 ? ev[4] : ev[3], 0));
        if (z_side) enqueue_z_accs(ctx, pk, plans, -1);
    }
    if (z_side) enqueue_z_reduces(ctx);
    if (trace) fprintf(stderr, "host: z-side msms queued at %.3f ms\n", now_ms() - t0);

    // ---- H last: it is the only MSM that waits for the witness map; then collect — each MSM's host Horner overlaps the
    // device work still queued behind it.  (With the witness map first H could go second — its list sorted underneath the G2
    // accumulation — and L, with a quarter of H's buckets and nothing to do on the host afterwards, last: measured 154.7 against
    // 153.65 ms, the shorter tail does not pay for the earlier scatter.)
    ZK_HIP(hipStreamWaitEvent(ctx->stream, ev[4], 0));
    ctx->slots[1].last_of_proof = true;
    if (nh) msm_g1_enqueue(ctx, ctx->ws_h, plan_h, pk.h.as<G1AffineU>(), ctx->slots[1], pk.pad_h);
    if (trace) fprintf(stderr, "host: h queued at %.3f ms\n", now_ms() - t0);
    double tprev = now_ms();
    auto lap = [&](ProofTiming slot) { const double t = now_ms(); ctx->timings[slot] = (float)(t - tprev); tprev = t; };
    const bool early = pk.full;
    auto collect_b2 = [&] { out.b2 = msm_g2_collect(ctx, ctx->slots[0]); };
    auto collect_l = [&] { out.l = msm_g1_collect(ctx, ctx->slots[2]); };
    auto collect_a = [&] {
        out.a = msm_g1_collect(ctx, ctx->slots[3]);
        if (early) out.s_a = early_s_a(pk, out.a, s);
    };
    auto collect_b1 = [&] {
        out.b1 = msm_g1_collect(ctx, ctx->slots[4]);
        if (early) out.r_b1 = early_r_b1(pk, out.b1, r);
    };
    // A plain key's MSMs come back as one sum per window (and per weight bit with the bit-sliced reduction): ~0.3 ms of host
    // additions per G1 MSM and ~1 ms for the G2 one.  One after the other they outlast the device on small and mid-size circuits
    // (8x8: 2.4 ms of host work in a 4.4 ms proof), so each collect gets its own thread: it waits for its MSM's event, then combines.
    const bool threaded = z_side && ctx->opt.collect_threads != 0 &&
                          (ctx->opt.collect_threads == 1 || ctx->slots[0].nwin > 1 || ctx->slots[2].nwin > 1);
    if (z_side && threaded) {
        std::exception_ptr err[4];
        {
            ThreadGroup tg;
            const int device = ctx->device;
            auto guarded = [&err, device](int i, auto &job) {
                return [&err, device, i, &job] {
                    try {
                        (void)hipSetDevice(device);
                        job();
                    } catch (...) {
                        err[i] = std::current_exception();
                    }
                };
            };
            tg.run(guarded(0, collect_b2));
            tg.run(guarded(1, collect_l));
            tg.run(guarded(2, collect_a));
            tg.run(guarded(3, collect_b1));
            try {
                if (nh) out.h = msm_g1_collect(ctx, ctx->slots[1]);
                else ZK_HIP(hipStreamSynchronize(ctx->stream));
            } catch (...) {
                tg.join();
                throw;
            }
            lap(T_GAP_H);
            tg.join();
        }
        for (auto &e : err)
            if (e) std::rethrow_exception(e);
        out.have_early = early;
        ctx->timings[T_GAP_L] = ctx->timings[T_GAP_A] = ctx->timings[T_GAP_B1] = 0;
        lap(T_GAP_B2);      // what the slowest z-side collect took beyond H's
    } else {
        if (z_side) {
            collect_b2(); lap(T_GAP_B2);
            collect_l(); lap(T_GAP_L);
            collect_a(); lap(T_GAP_A);
            collect_b1(); lap(T_GAP_B1);
            out.have_early = early;
        } else {
            ctx->timings[T_GAP_L] = ctx->timings[T_GAP_A] = ctx->timings[T_GAP_B1] = ctx->timings[T_GAP_B2] = 0;
        }
        if (nh) out.h = msm_g1_collect(ctx, ctx->slots[1]);
        else ZK_HIP(hipStreamSynchronize(ctx->stream));
        lap(T_GAP_H);
    }
    record_msm_timings(ctx, nh > 0, z_side);
    record_pass_timings(ctx, ev, t0);
    check_collect(ctx, chk, 1);
    drain.ok = true;
}

void prove_tail(PkDev &pk, const Fr &r, const Fr &s, const Partials &p, uint64_t *proof_out, uint8_t *inf_out) {
    prove_tail_pts(pk.alpha_g1, pk.beta_g1, pk.beta_g2, r, s, p, proof_out, inf_out);
}

void partials_to_abi(const Partials &p, uint64_t out[72], uint8_t inf[5]) {
    point_to_abi(xyzz_to_affine(p.h), out, inf);
    point_to_abi(xyzz_to_affine(p.l), out + 12, inf + 1);
    point_to_abi(xyzz_to_affine(p.a), out + 24, inf + 2);
    point_to_abi(xyzz_to_affine(p.b1), out + 36, inf + 3);
    point_to_abi(xyzz_to_affine(p.b2), out + 48, inf + 4);
}
void sum_partials(Partials &p, const uint64_t *partials, const uint8_t *partial_inf, int n_ranks) {
    p.h = p.l = p.a = p.b1 = G1XYZZ::inf();
    p.b2 = G2XYZZ::inf();
    for (int k = 0; k < n_ranks; k++) {
        const uint64_t *q = partials + 72 * (size_t)k;
        const uint8_t *f = partial_inf + 5 * (size_t)k;
        xyzz_madd(p.h, g1_from_abi(q, f[0]), false);
        xyzz_madd(p.l, g1_from_abi(q + 12, f[1]), false);
        xyzz_madd(p.a, g1_from_abi(q + 24, f[2]), false);
        xyzz_madd(p.b1, g1_from_abi(q + 36, f[3]), false);
        xyzz_madd(p.b2, g2_from_abi(q + 48, f[4]), false);
    }
}

}  // namespace zk

namespace {

// [k] p for a small scalar: as many doublings as k has bits (a prime candidate's n is below 2^20)
G1XYZZ g1_mul_u64(const G1Affine &p, uint64_t k) {
    G1XYZZ acc = G1XYZZ::inf();
    for (int i = 63; i >= 0; i--) {
        acc = xyzz_dbl(acc);
        if ((k >> i) & 1) xyzz_madd(acc, p, false);
    }
    return acc;
}
// What turns a proof on the PrimeCircuit's template key into request k's (zkg16_prove_prime_batch): n[k] and -j[k] go into A z and
// C z at the template's patch rows before the transforms (WmPatch), and n[k] U — what the request's a_query[0] has over the
// template's, times z[0] = 1 — into the A partial before s (A + alpha) is taken.
struct PrimeCorr {
    const uint32_t *n;
    const uint64_t *j;
    G1Affine U;
    uint32_t rows[4];
};

// ---- zkg16_prove_batch: K proofs of one circuit on one whole resident key in one device pass.  Each MSM has ONE plan over the K
// scalar vectors (msm_plan_build with ScalarSrc::batch: one digit launch, one scatter; the K proofs' bucket sets are windows of it),
// one accumulation, its fix-ups and one reduction chain; the witness map is one SpMV and seven transforms over all K assignments
// (witness_map_run_batch), whose K h vectors the H plan reads in place.  The host then combines each proof's window sums and
// finishes the proof on up to 8 threads (one with option collect_threads = 2) —
// the same operations in the same order as prove_device + prove_tail, so proof k is byte-identical to zkg16_prove_resident's.
// pc: the per-proof corrections of proofs on the PrimeCircuit's template key (PrimeCorr).
void prove_batch_device(zkg16_ctx *ctx, PkDev &pk, R1csDev &rc, WitnessDev *const *wits, size_t K, const Fr *r, const Fr *s,
                        uint64_t *proofs_out, uint8_t *inf_out, const PrimeCorr *pc = nullptr) {
    const size_t N = (size_t)1 << rc.log_n;
    const size_t nh = N - 1;
    if (pk.z_lo != 0 || !pk.full) throw HipError{hipErrorInvalidValue, "prove_batch: a shard key", __FILE__, __LINE__};
    EventSet evs;                         // as prove_device: 0-1 z-side sort, 2-3 the witness map, 3-4 the h-side sort
    hipEvent_t *ev = evs.ev;
    DrainOnError drain{ctx};
    const double t0 = now_ms();
    // pinned, device-visible: the 3K extra scalars (r, s, -rs of every proof), the K x 2 patch values (n, -j: template proofs only) and
    // the K assignment pointers, read by the kernels in place; rewritten only by the next batch on this lane, which starts after this
    // one has been collected
    const size_t host_bytes = (3 + 2) * K * sizeof(Fr) + K * sizeof(void *);
    if (ctx->batch_host_bytes < host_bytes) {
        if (ctx->batch_host) (void)hipHostFree(ctx->batch_host);
        ctx->batch_host = nullptr;
        ctx->batch_host_bytes = 0;
        ZK_HIP(hipHostMalloc(&ctx->batch_host, host_bytes, hipHostMallocDefault));
        ctx->batch_host_bytes = host_bytes;
    }
    Fr *extra = reinterpret_cast<Fr *>(ctx->batch_host);
    Fr *patch_tab = extra + 3 * K;
    const Fr **vecs = reinterpret_cast<const Fr **>(extra + 5 * K);
    WmPatch patch{{0, 0, 0, 0}, patch_tab};
    uint64_t *const chk = check_begin(ctx, K);
    for (size_t k = 0; pc && k < K; k++) {
        Fr c = Fr::zero();
        c.l[0] = pc->n[k];
        patch_tab[2 * k] = fp_to_mont(c);
        c.l[0] = (uint32_t)pc->j[k];
        c.l[1] = (uint32_t)(pc->j[k] >> 32);
        patch_tab[2 * k + 1] = fp_neg(fp_to_mont(c));
    }
    if (pc) memcpy(patch.rows, pc->rows, sizeof patch.rows);
    for (size_t k = 0; k < K; k++) {
        extra[3 * k] = pk.blinding ? r[k] : Fr::zero();
        extra[3 * k + 1] = pk.blinding ? s[k] : Fr::zero();
        extra[3 * k + 2] = pk.blinding ? fp_neg(fp_mul(r[k], s[k])) : Fr::zero();
        vecs[k] = wits[k]->z.as<Fr>() + pk.z_lo;
    }
    ZPlans plans;
    MsmPlan plan_h;
    ZK_HIP(hipEventRecord(ev[0], ctx->stream));
    ctx->ws_z.last_tb = ctx->ws_zb.last_tb = ctx->ws_h.last_tb = 0;
    ctx->last_msm_group = 0;              // ws_h and slots[0] are the proof's from here on: zkg16_last_msm_state reports zeros
    {
        ScalarSrc zsrc{nullptr, pk.z_hi - pk.z_lo, extra, 3, true, nullptr};
        zsrc.vecs = vecs;
        zsrc.batch = (int)K;
        build_z_plans(ctx, zsrc, pk, ctx->ws_z, ctx->ws_zb, plans);
    }
    ZK_HIP(hipEventRecord(ev[1], ctx->stream));
    enqueue_z_accs(ctx, pk, plans, -1);
    {
        WmStreamSwap on_wm_stream(ctx);
        ZK_HIP(hipEventRecord(ev[2], ctx->stream));
        Fr *hv = nullptr;
        if (K == 1) witness_map_run(ctx, rc, wits[0]->z.as<Fr>(), &hv, pc ? &patch : nullptr, chk);
        else witness_map_run_batch(ctx, rc, vecs, (unsigned)K, &hv, pc ? &patch : nullptr, chk);      // vecs: the K assignments (z_lo = 0)
        ZK_HIP(hipEventRecord(ev[3], ctx->stream));
        ScalarSrc hsrc{hv + pk.h_lo, nh, nullptr, 0, true, nullptr};
        hsrc.vec_stride = N;
        hsrc.batch = (int)K;
        msm_plan_build(ctx, ctx->ws_h, hsrc, plan_h, pk.tab_c_h ? pk.tab_c_h : ctx->opt.window_bits_h, pk.tab_c_h != 0);
        ZK_HIP(hipEventRecord(ev[4], ctx->stream));
    }
    enqueue_z_reduces(ctx);
    ZK_HIP(hipStreamWaitEvent(ctx->stream, ev[4], 0));
    ctx->slots[1].last_of_proof = true;
    msm_g1_enqueue(ctx, ctx->ws_h, plan_h, pk.h.as<G1AffineU>(), ctx->slots[1], pk.pad_h);

    // ---- host: the proofs are spread over threads; the z-side combination (+ s (A + alpha), r (B1 + beta)) runs while the
    // device still works on H, then H's and the tail
    std::vector<Partials> parts(K);
    const int nth = ctx->opt.collect_threads == 0 ? 1 : (int)(K < 8 ? K : 8);
    const int device = ctx->device;
    auto run_pool = [&](const std::function<void(size_t)> &job) {
        if (nth == 1) {                   // one proof, or option collect_threads = 2: on this thread
            for (size_t k = 0; k < K; k++) job(k);
            return;
        }
        std::atomic<size_t> next{0};
        std::vector<std::exception_ptr> err(nth);
        {
            ThreadGroup tg;
            for (int t = 0; t < nth; t++)
                tg.run([&, t] {
                    try {
                        (void)hipSetDevice(device);
                        for (size_t k; (k = next++) < K;) job(k);
                    } catch (...) {
                        err[t] = std::current_exception();
                    }
                });
        }
        for (auto &e : err)
            if (e) std::rethrow_exception(e);
    };
    double tprev = now_ms();
    for (int i : {0, 2, 3, 4}) msm_slot_wait(ctx->slots[i]);
    ctx->timings[T_GAP_B2] = (float)(now_ms() - tprev);
    tprev = now_ms();
    float host_z_ms = 0;
    run_pool([&](size_t k) {
        Partials &p = parts[k];
        p.b2 = msm_g2_collect_part(ctx->slots[0], (int)k);
        p.l = msm_g1_collect_part(ctx->slots[2], (int)k);
        p.a = msm_g1_collect_part(ctx->slots[3], (int)k);
        if (pc) xyzz_add(p.a, g1_mul_u64(pc->U, pc->n[k]));
        p.b1 = msm_g1_collect_part(ctx->slots[4], (int)k);
        if (pk.full) {
            p.s_a = early_s_a(pk, p.a, s[k]);
            p.r_b1 = early_r_b1(pk, p.b1, r[k]);
            p.have_early = true;
        }
    });
    host_z_ms = (float)(now_ms() - tprev);
    tprev = now_ms();
    msm_slot_wait(ctx->slots[1]);
    ctx->timings[T_GAP_H] = (float)(now_ms() - tprev);
    tprev = now_ms();
    run_pool([&](size_t k) {
        parts[k].h = msm_g1_collect_part(ctx->slots[1], (int)k);
        prove_tail(pk, r[k], s[k], parts[k], proofs_out + 48 * k, inf_out + 3 * k);
    });
    ctx->timings[T_HOST_TAIL] = (float)(now_ms() - tprev);
    for (auto &sl : ctx->slots) {
        sl.active = false;
        sl.collect_host_ms = 0;
    }
    record_msm_timings(ctx, true, true);
    ctx->timings[T_HORNER_H] = 0;               // H's combination is part of T_HOST_TAIL (with the tails)
    ctx->timings[T_HORNER_Z] = host_z_ms;       // the other four's, with s (A + alpha) and r (B1 + beta)
    ctx->timings[T_GAP_L] = ctx->timings[T_GAP_A] = ctx->timings[T_GAP_B1] = 0;
    record_pass_timings(ctx, ev, t0);
    check_collect(ctx, chk, K);
    drain.ok = true;
}

// Proofs per device pass of a batch on (pk, rc): terms per proof of the z and h lists (every list stays under 2^31 terms), and what
// grows with K on the device — both lists' entries, codes and scatter intermediates (20 B a term; the B list may be a second z list),
// the witness map's four vectors, and the bucket arrays of the five MSMs with their reduction buffers (taken as 2x the G1 / G2
// buckets), plus `extra_per_proof` bytes the caller keeps per proof — within 60 % of the free HBM.  Option batch_max caps it.
size_t batch_sub_size(zkg16_ctx *ctx, const PkDev *pk, const R1csDev *rc, size_t extra_per_proof) {
    const size_t N = (size_t)1 << rc->log_n;
    const size_t m = rc->num_variables;
    const size_t dz = msm_plan_digits(ctx, m + 3, pk->tab_c_z, pk->tab_c_z != 0), dh = msm_plan_digits(ctx, N - 1, pk->tab_c_h ? pk->tab_c_h : ctx->opt.window_bits_h, pk->tab_c_h != 0);
    const size_t tz = (m + 3) * dz, th = (N - 1) * dh;
    const size_t term_cap = ((size_t)1 << 31) - 1;
    size_t kb = term_cap / (tz > th ? tz : th);
    {
        const size_t cz = pk->tab_c_z ? (size_t)pk->tab_c_z : msm_plan_bits(ctx, m + 3, 0, false);
        const size_t ch = pk->tab_c_h ? (size_t)pk->tab_c_h : msm_plan_bits(ctx, N - 1, ctx->opt.window_bits_h, false);
        const size_t bz = ((size_t)1 << (cz - 1)) * (pk->tab_c_z ? 1 : dz), bh = ((size_t)1 << (ch - 1)) * (pk->tab_c_h ? 1 : dh);
        const size_t per_proof = (2 * tz + th) * 20 + 4 * N * sizeof(Fr) + 2 * (bz * (3 * sizeof(G1XYZZ) + sizeof(G2XYZZ)) + bh * sizeof(G1XYZZ)) + extra_per_proof;
        size_t free_b = 0, total_b = 0;
        ZK_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t kmem = (size_t)(0.6 * (double)free_b) / per_proof;
        if (kmem < kb) kb = kmem;
    }
    if (ctx->opt.batch_max > 0 && (size_t)ctx->opt.batch_max < kb) kb = (size_t)ctx->opt.batch_max;
    if (kb > 65535) kb = 65535;
    if (kb < 1) kb = 1;
    return kb;
}
// after a pass of prove_batch_device: its timings into acc and, for a batch of several passes, its lists' lengths into terms
void batch_pass_account(zkg16_ctx *ctx, float acc[T_COUNT], uint64_t terms[3], bool one_pass) {
    for (int i = 0; i < T_COUNT; i++) acc[i] += ctx->timings[i];
    if (one_pass) return;                 // zkg16_last_term_counts reads its lists as after a single proof
    MsmWorkspace *w[3] = {&ctx->ws_z, &ctx->ws_zb, &ctx->ws_h};
    for (int i = 0; i < 3; i++) {
        uint32_t v = 0;
        if (w[i]->last_tb && w[i]->offsets.p)
            ZK_HIP(hipMemcpy(&v, w[i]->offsets.as<uint32_t>() + w[i]->last_tb, sizeof v, hipMemcpyDeviceToHost));
        terms[i] += v;
    }
}
// A batch of k proofs on (pk, rc) in sub-batches that fit (batch_sub_size): pass(off, n, proofs, infs) proves requests
// [off, off + n) — through prove_batch_device — into staged outputs, which reach proofs_out / inf_out only when every pass has
// succeeded: a call that fails (pass throws) writes nothing.  Publishes the summed timings and term counts of the passes;
// -> the passes' summed T_TOTAL, or a negative value — nothing written — when option "check_satisfied" found an unsatisfied
// assignment in any pass (every pass still runs: zkg16_last_check names all of them).
template <class Pass>
float prove_in_passes(zkg16_ctx *ctx, const PkDev *pk, const R1csDev *rc, size_t k, size_t extra_per_proof, uint64_t *proofs_out,
                      uint8_t *inf_out, Pass &&pass) {
    const size_t kb = batch_sub_size(ctx, pk, rc, extra_per_proof);
    std::vector<uint64_t> proofs(48 * k);
    std::vector<uint8_t> infs(3 * k);
    const double t0 = now_ms();
    float acc[T_COUNT] = {0};
    uint64_t terms[3] = {0, 0, 0};
    check_reset(ctx);
    for (size_t off = 0; off < k; off += kb) {
        pass(off, k - off < kb ? k - off : kb, proofs.data() + 48 * off, infs.data() + 3 * off);
        batch_pass_account(ctx, acc, terms, kb >= k);
    }
    for (int i = 0; i < T_COUNT; i++) ctx->timings[i] = acc[i];
    ctx->timings[T_TOTAL] = (float)(now_ms() - t0);
    for (int i = 0; i < 3; i++) ctx->batch_terms[i] = terms[i];
    ctx->batch_terms_set = kb < k;
    if (check_failed(ctx)) return -1.0f;
    memcpy(proofs_out, proofs.data(), proofs.size() * sizeof(uint64_t));
    memcpy(inf_out, infs.data(), infs.size());
    return acc[T_TOTAL];
}

// ---- what every proving entry point checks before it starts, in the order all of them report it: an unknown handle
// (ZKG16_ERR_BAD_HANDLE) before a key shard the entry does not take, before any shape (ZKG16_ERR_BAD_ARG).
enum class Shard { accepted, bad_arg, unsupported };      // zkg16_prove_partial | one-proof entries | batch entries (shards: _partial / _group)
int shard_status(const PkDev &pk, Shard policy) {
    if (pk.full || policy == Shard::accepted) return ZKG16_OK;
    return policy == Shard::bad_arg ? ZKG16_ERR_BAD_ARG : ZKG16_ERR_UNSUPPORTED;
}
bool key_fits(const PkDev &pk, size_t num_variables, size_t num_instance, int log_n) {
    return pk.m_total == num_variables && pk.num_instance == num_instance && pk.n_h_total == ((size_t)1 << log_n) - 1;
}
struct ProveHandles {
    std::shared_ptr<PkDev> pk;
    std::shared_ptr<R1csDev> rc;
    std::vector<std::shared_ptr<WitnessDev>> wit_refs;
    std::vector<WitnessDev *> wits;
};
// matrix_total != 0: the request brings no assignment handle but is a MatrixCircuit's, of that many variables and four instance ones
int lookup_handles(zkg16_ctx *root, uint64_t pk_h, uint64_t r1cs_h, const uint64_t *wit_h, size_t n_wit, Shard policy, size_t matrix_total,
                   ProveHandles &h) {
    h.pk = root->pks.get(pk_h);
    h.rc = root->r1cs.get(r1cs_h);
    if (!h.pk || !h.rc) return ZKG16_ERR_BAD_HANDLE;
    h.wit_refs.resize(n_wit);
    h.wits.resize(n_wit);
    for (size_t i = 0; i < n_wit; i++) {
        h.wit_refs[i] = root->wits.get(wit_h[i]);
        h.wits[i] = h.wit_refs[i].get();
        if (!h.wits[i]) return ZKG16_ERR_BAD_HANDLE;
    }
    if (const int st = shard_status(*h.pk, policy)) return st;
    if (!key_fits(*h.pk, h.rc->num_variables, h.rc->num_instance, h.rc->log_n)) return ZKG16_ERR_BAD_ARG;
    if (matrix_total && (matrix_total != h.rc->num_variables || h.rc->num_instance != 4)) return ZKG16_ERR_BAD_ARG;      // not the MatrixCircuit of this size
    for (size_t i = 0; i < n_wit; i++)
        if (h.wits[i]->n != h.rc->num_variables) return ZKG16_ERR_BAD_ARG;
    return ZKG16_OK;
}

// the host tail of a proof whose device part prove_device has just timed
void finish_proof(zkg16_ctx *ctx, PkDev &pk, const Fr &r, const Fr &s, const Partials &p, uint64_t *proof_out, uint8_t *inf_out) {
    const double t0 = now_ms();
    prove_tail(pk, r, s, p, proof_out, inf_out);
    ctx->timings[T_HOST_TAIL] = (float)(now_ms() - t0);
    ctx->timings[T_TOTAL] += ctx->timings[T_HOST_TAIL];
}

std::vector<Fr> frs_from_abi(const uint64_t *l, size_t k) {
    std::vector<Fr> v(k);
    for (size_t i = 0; i < k; i++) v[i] = fr_from_abi(l + 4 * i);
    return v;
}

// ---- the spine of the four zkg16_prove_*_batch entries that build their own assignments (no witness handle exists at any time):
// per sub-batch (prove_in_passes) assign(off, nb, wit_refs, &dev_ms) makes the assignments of requests [off, off + nb) — the entry
// offsets its inputs and staged side outputs there — and prove_batch_device proves them under r, s of those requests, after which the
// sub-batch's assignments go back.  pc: the prime entry's corrections; its assign step points n and j at the sub-batch.  What assign
// throws passes through.  -> the assign steps' summed device time and prove_in_passes' answer (negative: unsatisfied, nothing written).
struct BatchTimes {
    double wit_ms = 0;
    float prove_ms = 0;
};
template <class Assign>
BatchTimes prove_assigned_batch(zkg16_ctx *ctx, const ProveHandles &h, size_t k, const uint64_t *r, const uint64_t *s, size_t extra_per_proof,
                                uint64_t *proofs_out, uint8_t *inf_out, Assign &&assign, const PrimeCorr *pc = nullptr) {
    const std::vector<Fr> rr = frs_from_abi(r, k), ss = frs_from_abi(s, k);
    BatchTimes t;
    t.prove_ms = prove_in_passes(ctx, h.pk.get(), h.rc.get(), k, extra_per_proof, proofs_out, inf_out,
                                 [&](size_t off, size_t nb, uint64_t *proofs, uint8_t *infs) {
        std::vector<std::shared_ptr<WitnessDev>> wit_refs;
        float dev_ms = 0;
        assign(off, nb, wit_refs, &dev_ms);
        t.wit_ms += dev_ms;
        std::vector<WitnessDev *> wits(nb);
        for (size_t i = 0; i < nb; i++) wits[i] = wit_refs[i].get();
        prove_batch_device(ctx, *h.pk, *h.rc, wits.data(), nb, rr.data() + off, ss.data() + off, proofs, infs, pc);
    });
    return t;
}
// their timings_ms (nullable, 4): the entry's host pre-work, the assign steps, proving, the whole call
void batch_times_out(float *timings_ms, double host_ms, const BatchTimes &t, double t_call) {
    if (!timings_ms) return;
    timings_ms[0] = (float)host_ms;
    timings_ms[1] = (float)t.wit_ms;
    timings_ms[2] = t.prove_ms;
    timings_ms[3] = (float)(now_ms() - t_call);
}

}  // namespace

extern "C" {

int zkg16_prove_partial(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, uint64_t witness_handle,
                        const uint64_t r[4], const uint64_t s[4], uint64_t partial_out[72], uint8_t partial_inf[5]) {
    if (!r || !s || !partial_out || !partial_inf) return ZKG16_ERR_BAD_ARG;
    ZK_LANE_BEGIN(ctx)
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, &witness_handle, 1, Shard::accepted, 0, h)) return st;
    Partials p;
    prove_device(ctx, *h.pk, *h.rc, *h.wits[0], fr_from_abi(r), fr_from_abi(s), p);
    if (check_failed(ctx)) return ZKG16_ERR_UNSATISFIED;
    partials_to_abi(p, partial_out, partial_inf);
    ZK_LANE_END(ctx)
}

int zkg16_prove_finish(zkg16_ctx *ctx, uint64_t pk_handle, const uint64_t r[4], const uint64_t s[4],
                       const uint64_t *partials, const uint8_t *partial_inf, int n_ranks, uint64_t proof_out[48], uint8_t inf_out[3]) {
    if (!r || !s || !partials || !partial_inf || n_ranks < 1 || !proof_out || !inf_out) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto pk_ref = ctx->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    Partials p;
    sum_partials(p, partials, partial_inf, n_ranks);
    prove_tail(*pk, fr_from_abi(r), fr_from_abi(s), p, proof_out, inf_out);
    ZK_API_END(ctx)
}

int zkg16_combine_partials(const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                           const uint64_t r[4], const uint64_t s[4], const uint64_t *partials, const uint8_t *partial_inf,
                           int n_ranks, uint64_t proof_out[48], uint8_t inf_out[3]) {
    if (!alpha_g1 || !beta_g1 || !beta_g2 || !r || !s || !partials || !partial_inf || n_ranks < 1 || !proof_out || !inf_out)
        return ZKG16_ERR_BAD_ARG;
    Partials p;
    sum_partials(p, partials, partial_inf, n_ranks);
    prove_tail_pts(g1_from_abi(alpha_g1, 0), g1_from_abi(beta_g1, 0), g2_from_abi(beta_g2, 0), fr_from_abi(r), fr_from_abi(s), p,
                   proof_out, inf_out);
    return ZKG16_OK;
}

int zkg16_prove_resident(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, uint64_t witness_handle,
                         const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3]) {
    if (!r || !s || !proof_out || !inf_out) return ZKG16_ERR_BAD_ARG;
    ZK_LANE_BEGIN(ctx)
    ProveHandles h;      // sharded keys go through prove_partial/finish
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, &witness_handle, 1, Shard::bad_arg, 0, h)) return st;
    Partials p;
    const Fr rr = fr_from_abi(r), ss = fr_from_abi(s);
    prove_device(ctx, *h.pk, *h.rc, *h.wits[0], rr, ss, p);
    if (check_failed(ctx)) return ZKG16_ERR_UNSATISFIED;
    finish_proof(ctx, *h.pk, rr, ss, p, proof_out, inf_out);
    ZK_LANE_END(ctx)
}

// K proofs of one circuit on one whole resident key (prove_batch_device), in sub-batches that fit: every term list under 2^31
// terms, at most 65,535 proofs (the grid.z / grid.y of the batched launches), and the workspaces that grow with K within 60 % of
// the free HBM (option batch_max caps the sub-batch; no result changes).  The proofs are staged on the host and written out only
// when every sub-batch has succeeded: a call that fails writes nothing.
int zkg16_prove_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, const uint64_t *witness_handles, size_t k,
                      const uint64_t *r, const uint64_t *s, uint64_t *proofs_out, uint8_t *inf_out) {
    if (!witness_handles || !r || !s || !proofs_out || !inf_out || k == 0) return ZKG16_ERR_BAD_ARG;
    ZK_LANE_BEGIN(ctx)
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, witness_handles, k, Shard::unsupported, 0, h)) return st;
    const std::vector<Fr> rr = frs_from_abi(r, k), ss = frs_from_abi(s, k);
    const float ms = prove_in_passes(ctx, h.pk.get(), h.rc.get(), k, 0, proofs_out, inf_out, [&](size_t off, size_t n, uint64_t *proofs, uint8_t *infs) {
        prove_batch_device(ctx, *h.pk, *h.rc, h.wits.data() + off, n, rr.data() + off, ss.data() + off, proofs, infs);
    });
    if (ms < 0) return ZKG16_ERR_UNSATISFIED;
    ZK_LANE_END(ctx)
}

// One MatrixCircuit request on matrices that are already resident: what the reference times as `proving_time`
// (matrix_proof.rs:138-145: Groth16::prove re-synthesises the circuit, then proves) with the per-request part of the synthesis —
// the assignment — produced WHILE the proof runs.  The three native sponges run on three host threads (sequential by
// construction); as soon as a quarter of their permutations is done the device expands those into their S-box values and the four
// z-side MSMs start on the terms that exist (prove_device's rounds); the witness map and the H MSM follow the last part.
int zkg16_prove_matrix(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t n, const uint64_t *a, const uint64_t *b,
                       const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3], uint64_t public_inputs[12],
                       float *timings_ms) {
    if (!r || !s || !proof_out || !inf_out || !a || !b || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    if (!ctx) return ZKG16_ERR_BAD_ARG;
    const double t_call = now_ms();
    std::unique_ptr<MatrixWitnessStream, void (*)(MatrixWitnessStream *)> ms(nullptr, matrix_stream_free);
    try {
        // the chains start before the ctx is locked: they need neither it nor the device
        ms.reset(matrix_stream_start(n, a, b, ctx->opt.matrix_parts, ctx->opt.matrix_slice_min, ctx->opt.matrix_parts != 1));
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    ZK_LANE_BEGIN(ctx)
    const size_t total = matrix_stream_total(ms.get());
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, nullptr, 0, Shard::bad_arg, total, h)) return st;
    WitnessDev wit;
    wit.n = total;
    wit.z.alloc(total * sizeof(Fr));
    // a throw below must not leave the stream object's copies and kernels in flight behind its destruction (DrainOnError, inside
    // prove_device, covers the proof's own streams and slots)
    struct MatrixStreamDrain { zkg16_ctx *c; ~MatrixStreamDrain() { (void)hipStreamSynchronize(c->stream); } } stream_drain{ctx};
    matrix_stream_attach(ms.get(), ctx, wit.z.as<Fr>(), 3);
    ZParts zp;
    zp.parts = matrix_stream_parts(ms.get());
    zp.part_of = matrix_stream_part_of(ms.get());
    MatrixWitnessStream *msp = ms.get();
    zp.produce = [ctx, msp](int k) { matrix_stream_produce(msp, ctx, k); };
    Partials p;
    const Fr rr = fr_from_abi(r), ss = fr_from_abi(s);
    prove_device(ctx, *h.pk, *h.rc, wit, rr, ss, p, nullptr, &zp);      // without part_of (matrix_parts = 1): the assignment first, then the proof
    if (check_failed(ctx)) return ZKG16_ERR_UNSATISFIED;
    finish_proof(ctx, *h.pk, rr, ss, p, proof_out, inf_out);
    if (public_inputs) matrix_stream_hashes(ms.get(), public_inputs);
    if (timings_ms) {
        timings_ms[0] = (float)matrix_stream_chain_ms(ms.get());
        timings_ms[1] = (float)zp.parts;
        timings_ms[2] = (float)(now_ms() - t_call);
    }
    ZK_LANE_END(ctx)
}

// K requests of the matrix handler on one resident key and the MatrixCircuit's resident matrices: per sub-batch (batch_sub_size with
// the assignment itself added per proof) the host chains, the batched witness pass (witness.hip: matrix_batch_assign) and
// prove_batch_device, after which the sub-batch's assignments go back.  No witness handle exists at any time; proofs and public inputs
// are staged and written only when every sub-batch has succeeded.  The chains of sub-batch j + 1 do not run beside the proving of
// sub-batch j: timings_ms (chains, witness passes, proving, whole call) is there to tell whether that would pay.
int zkg16_prove_matrix_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t n, const uint64_t *a, const uint64_t *b, size_t k,
                             const uint64_t *r, const uint64_t *s, uint64_t *proofs_out, uint8_t *inf_out, uint64_t *public_inputs,
                             float *timings_ms) {
    if (!a || !b || !r || !s || !proofs_out || !inf_out || k == 0 || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    const double t_call = now_ms();
    ZK_LANE_BEGIN(ctx)
    const size_t total = matrix_witness_total(n), nn = n * n;
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, nullptr, 0, Shard::unsupported, total, h)) return st;
    if (k > SIZE_MAX / (total * sizeof(Fr))) return ZKG16_ERR_BAD_ARG;
    std::vector<uint64_t> pubs(12 * k);
    double chain_ms = 0;
    const BatchTimes t = prove_assigned_batch(ctx, h, k, r, s, total * sizeof(Fr), proofs_out, inf_out,
                                              [&](size_t off, size_t nb, std::vector<std::shared_ptr<WitnessDev>> &wit_refs, float *dev_ms) {
        const uint64_t *ao = a + off * nn, *bo = b + off * nn;
        MatrixBatchChains mc;
        if (sponge_chains_on_device(ctx, 3 * nb)) matrix_batch_chains_device(mc, n, nb, pubs.data() + 12 * off);
        else matrix_batch_chains(mc, n, ao, bo, nb, ctx->opt.matrix_batch_threads, pubs.data() + 12 * off);
        chain_ms += mc.ms;
        matrix_batch_assign(ctx, mc, ao, bo, wit_refs, dev_ms);
    });
    if (t.prove_ms < 0) return ZKG16_ERR_UNSATISFIED;
    if (public_inputs) memcpy(public_inputs, pubs.data(), pubs.size() * sizeof(uint64_t));
    batch_times_out(timings_ms, chain_ms, t, t_call);
    ZK_LANE_END(ctx)
}

// K requests of the Fibonacci handler on one resident key and the FibonacciCircuit's resident matrices of `steps` rounds: the two
// coefficients of the result once per call (circuits.hip: fibonacci_coeffs), then per sub-batch the one-launch assignment pass
// (witness.hip: fibonacci_batch_assign) and prove_batch_device, after which the sub-batch's assignments go back.  No witness handle
// exists at any time; proofs and public inputs are staged and written only when every sub-batch has succeeded.
int zkg16_prove_fibonacci_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t steps, const uint64_t *a, const uint64_t *b,
                                size_t k, const uint64_t *r, const uint64_t *s, uint64_t *proofs_out, uint8_t *inf_out, uint64_t *public_inputs,
                                float *timings_ms) {
    if (!a || !b || !r || !s || !proofs_out || !inf_out || k == 0 || steps > ZKG16_FIBONACCI_STEPS_MAX) return ZKG16_ERR_BAD_ARG;
    const double t_call = now_ms();
    ZK_LANE_BEGIN(ctx)
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, nullptr, 0, Shard::unsupported, 0, h)) return st;
    if (h.rc->num_variables != FIBONACCI_VARS || h.rc->num_instance != FIBONACCI_INSTANCE || h.rc->num_constraints != steps + 1)
        return ZKG16_ERR_BAD_ARG;       // not the FibonacciCircuit of this round count
    if (k > SIZE_MAX / (48 * sizeof(uint64_t))) return ZKG16_ERR_BAD_ARG;
    const double t_coeff = now_ms();
    Fr ca, cb;
    fibonacci_coeffs(steps, ca, cb);
    const double coeff_ms = now_ms() - t_coeff;
    std::vector<uint64_t> pubs(12 * k);
    const BatchTimes t = prove_assigned_batch(ctx, h, k, r, s, FIBONACCI_VARS * sizeof(Fr), proofs_out, inf_out,
                                              [&](size_t off, size_t nb, std::vector<std::shared_ptr<WitnessDev>> &wit_refs, float *dev_ms) {
        fibonacci_batch_assign(ctx, ca, cb, a + off, b + off, nb, wit_refs, pubs.data() + 12 * off, dev_ms);
    });
    if (t.prove_ms < 0) return ZKG16_ERR_UNSATISFIED;
    if (public_inputs) memcpy(public_inputs, pubs.data(), pubs.size() * sizeof(uint64_t));
    batch_times_out(timings_ms, coeff_ms, t, t_call);
    ZK_LANE_END(ctx)
}

// K requests of the linear-equations handler on one resident key and the n-system's resident matrices: per sub-batch the two-launch
// assignment pass (witness.hip: linear_batch_assign) and prove_batch_device, after which the sub-batch's assignments go back.  No
// witness handle exists at any time; proofs and solutions are staged and written only when every sub-batch has succeeded.  A zero
// diagonal entry anywhere ends the call after the handle checks and before any device work (option "linear_solver" = 0); under 1 the
// assignment pass solves by elimination and a singular request ends the call at that sub-batch's synchronisation.
int zkg16_prove_linear_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t n, const uint64_t *a, const uint64_t *b, size_t k,
                             const uint64_t *r, const uint64_t *s, uint64_t *proofs_out, uint8_t *inf_out, uint64_t *x_out, float *timings_ms) {
    if (!a || !b || !r || !s || !proofs_out || !inf_out || k == 0 || n == 0 || n > ZKG16_LINEAR_N_MAX) return ZKG16_ERR_BAD_ARG;
    const double t_call = now_ms();
    ZK_LANE_BEGIN(ctx)
    const LinearDims d(n);
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, nullptr, 0, Shard::unsupported, 0, h)) return st;
    if (h.rc->num_variables != d.vars() || h.rc->num_instance != d.ni || h.rc->num_constraints != d.nc)
        return ZKG16_ERR_BAD_ARG;       // not the linear-equations circuit of this size
    if (k > SIZE_MAX / (d.vars() * sizeof(Fr))) return ZKG16_ERR_BAD_ARG;
    const double t_check = now_ms();
    size_t bad_req = 0, bad_row = 0;
    const bool elim = ctx->opt.linear_solver == 1;      // elimination: a zero diagonal entry may be solvable, the kernel's status words decide
    if (!elim && linear_zero_diagonal(n, a, k, &bad_req, &bad_row)) {
        char buf[160];
        snprintf(buf, sizeof buf, "zkg16_prove_linear_batch: request %zu has a zero diagonal entry in row %zu", bad_req, bad_row);
        ctx->last_error = buf;
        if (ctx != root) { std::lock_guard<std::mutex> l(root->lane_mu); root->last_error = buf; }
        return ZKG16_ERR_UNSUPPORTED;
    }
    const double check_ms = now_ms() - t_check;
    std::vector<uint64_t> xs(4 * k * n);
    // per proof: the assignment, its input and x; the elimination's global workspace where it is used (one per workgroup, at most one per request)
    const size_t elim_extra = elim && !linear_elim_in_lds(ctx, n) ? n * (n + 1) * sizeof(Fr) + sizeof(uint32_t) : 0;
    BatchTimes t;
    try {
        t = prove_assigned_batch(ctx, h, k, r, s, d.vars() * sizeof(Fr) + (n * n + n) * sizeof(uint64_t) + n * sizeof(Fr) + elim_extra, proofs_out, inf_out,
                                 [&](size_t off, size_t nb, std::vector<std::shared_ptr<WitnessDev>> &wit_refs, float *dev_ms) {
            try {
                linear_batch_assign(ctx, n, a + off * n * n, b + off * n, nb, wit_refs, xs.data() + 4 * off * n, dev_ms);
            } catch (const LinearSingular &e) {
                throw LinearSingular{off + e.req, e.col};       // the request's index in the call
            }
        });
    } catch (const LinearSingular &e) {         // nothing was written: proofs and solutions are staged
        char buf[200];
        snprintf(buf, sizeof buf, "zkg16_prove_linear_batch: request %zu is singular: columns 0..%zu of a are linearly dependent (column %zu)", e.req, e.col, e.col);
        ctx->last_error = buf;
        if (ctx != root) { std::lock_guard<std::mutex> l(root->lane_mu); root->last_error = buf; }
        return ZKG16_ERR_UNSUPPORTED;
    }
    if (t.prove_ms < 0) return ZKG16_ERR_UNSATISFIED;
    if (x_out) memcpy(x_out, xs.data(), xs.size() * sizeof(uint64_t));
    batch_times_out(timings_ms, check_ms, t, t_call);
    ZK_LANE_END(ctx)
}

// K prime requests on the template key: every request's inputs first (a refused candidate ends the call before any device work),
// then per sub-batch the batched assignment (prime_device.hip) and prove_batch_device with the per-proof corrections; the
// assignments go back after each sub-batch.  Each request's gamma_abc_g1[0] is formed on the host.  Everything is staged and
// written only when every sub-batch has succeeded.
int zkg16_prove_prime_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, const uint64_t corr[36], const uint64_t gamma_abc0_template[12],
                            const uint64_t *xs, const uint64_t *js, size_t k, const uint64_t *r, const uint64_t *s, uint64_t *proofs_out,
                            uint8_t *inf_out, uint64_t *gamma_abc0_out, uint64_t *public_inputs, float *timings_ms) {
    if (!corr || !gamma_abc0_template || !xs || !js || !r || !s || !proofs_out || !inf_out || !gamma_abc0_out || k == 0) return ZKG16_ERR_BAD_ARG;
    const double t_call = now_ms();
    ZK_LANE_BEGIN(ctx)
    ProveHandles h;
    if (const int st = lookup_handles(root, pk_handle, r1cs_handle, nullptr, 0, Shard::unsupported, 0, h)) return st;
    if (!h.rc->prime_template) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / (257 * 4 * sizeof(uint64_t))) return ZKG16_ERR_BAD_ARG;
    std::vector<Fr> in;
    std::vector<uint32_t> ns(k);
    size_t stride = 0;
    const double t_in = now_ms();
    if (const int st = prime_batch_inputs(xs, js, k, in, ns.data(), &stride)) return st;
    const double in_ms = now_ms() - t_in;
    PrimeCorr pc;
    pc.U = g1_from_abi(corr, 0);
    memcpy(pc.rows, h.rc->patch_rows, sizeof pc.rows);
    const G1Affine v_n = g1_from_abi(corr + 12, 0), v_j = g1_from_abi(corr + 24, 0), g0 = g1_from_abi(gamma_abc0_template, 0);
    std::vector<uint64_t> gammas(12 * k), pubs(public_inputs ? 257 * 4 * k : 0);
    const BatchTimes t = prove_assigned_batch(ctx, h, k, r, s, h.rc->num_variables * sizeof(Fr), proofs_out, inf_out,
                                              [&](size_t off, size_t nb, std::vector<std::shared_ptr<WitnessDev>> &wit_refs, float *dev_ms) {
        prime_witness_batch_assign(ctx, in.data() + off * stride, nb, wit_refs, dev_ms);
        pc.n = ns.data() + off;
        pc.j = js + off;
    }, &pc);
    if (t.prove_ms < 0) return ZKG16_ERR_UNSATISFIED;
    for (size_t i = 0; i < k; i++) {      // gamma_abc_g1[0] = the template's + n V_n - j V_j
        G1XYZZ g = G1XYZZ::from_affine(g0);
        xyzz_add(g, g1_mul_u64(v_n, ns[i]));
        xyzz_add(g, xyzz_neg(g1_mul_u64(v_j, js[i])));
        point_to_abi(xyzz_to_affine(g), gammas.data() + 12 * i, nullptr);
        if (public_inputs) (void)zkg16_prime_public_inputs(xs[i], js[i], pubs.data() + 257 * 4 * i);      // fails on a null pointer only
    }
    memcpy(gamma_abc0_out, gammas.data(), gammas.size() * sizeof(uint64_t));
    if (public_inputs) memcpy(public_inputs, pubs.data(), pubs.size() * sizeof(uint64_t));
    batch_times_out(timings_ms, in_ms, t, t_call);
    ZK_LANE_END(ctx)
}

// k Poseidon hashes in one call on a lane: at least "sponge_chains_min" chains are walked by wit_chain_batch_kernel, fewer by the
// host form (on "matrix_batch_threads" threads).  elems: k vectors of n Montgomery Fr; out[i] = zkg16_poseidon_hash(elems_i, n).
int zkg16_poseidon_hash_batch(zkg16_ctx *ctx, const uint64_t *elems, size_t n, size_t k, uint64_t *out) {
    if (!ctx || !elems || !out || n == 0 || k == 0) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / 32 / n || (n + 1) / 2 > 0xffffffffu) return ZKG16_ERR_BAD_ARG;
    if (!sponge_chains_on_device(ctx, k)) return zkg16_poseidon_hash_batch_host(elems, n, k, ctx->opt.matrix_batch_threads, out);
    ZK_LANE_BEGIN(ctx)
    sponge_hash_batch_device(ctx, 0, elems, n, k, out);
    ZK_LANE_END(ctx)
}
// hash_matrix for k matrices of n^2 u64: hashes[i] = hash_a of zkg16_matrix_sponge_states(n, m_i, .).  Routed as above.
int zkg16_matrix_hash_batch(zkg16_ctx *ctx, size_t n, const uint64_t *m, size_t k, uint64_t *hashes) {
    if (!ctx || !m || !hashes || k == 0 || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / 32 / (n * n)) return ZKG16_ERR_BAD_ARG;
    if (!sponge_chains_on_device(ctx, k)) return zkg16_matrix_hash_batch_host(n, m, k, ctx->opt.matrix_batch_threads, hashes);
    ZK_LANE_BEGIN(ctx)
    sponge_hash_batch_device(ctx, 1, m, n * n, k, hashes);
    ZK_LANE_END(ctx)
}

int zkg16_prove(zkg16_ctx *ctx, uint64_t pk_handle, const uint64_t r[4], const uint64_t s[4],
                const uint64_t *a_row_ptr, const uint32_t *a_col, const uint64_t *a_coeff,
                const uint64_t *b_row_ptr, const uint32_t *b_col, const uint64_t *b_coeff,
                const uint64_t *c_row_ptr, const uint32_t *c_col, const uint64_t *c_coeff,
                size_t num_instance, size_t num_constraints, const uint64_t *full_assignment, size_t n_assign,
                uint64_t proof_out[48], uint8_t inf_out[3]) {
    if (!r || !s || !proof_out || !inf_out || !full_assignment || n_assign == 0) return ZKG16_ERR_BAD_ARG;
    ZK_LANE_BEGIN(ctx)
    // the matrices arrive as host pointers: no r1cs or assignment handle to look up, the key's checks in the same order
    auto pk_ref = root->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    if (const int st = shard_status(*pk, Shard::bad_arg)) return st;
    const uint64_t *rp[3] = {a_row_ptr, b_row_ptr, c_row_ptr};
    const uint32_t *col[3] = {a_col, b_col, c_col};
    const uint64_t *cf[3] = {a_coeff, b_coeff, c_coeff};
    std::unique_ptr<R1csDev> rc;
    const int st = r1cs_create(rp, col, cf, num_instance, num_constraints, n_assign, rc);
    if (st) return st;
    if (!key_fits(*pk, n_assign, num_instance, rc->log_n)) return ZKG16_ERR_BAD_ARG;
    // the assignment first (the z-side MSMs need only it); the matrices follow inside prove_device, behind the accumulations
    WitnessDev wit;
    wit.n = n_assign;
    wit.z.alloc(n_assign * sizeof(Fr));
    upload_h2d(ctx, wit.z.p, full_assignment, n_assign * sizeof(Fr));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    const std::function<void()> upload = [&]() { r1cs_copy(ctx, *rc, rp, col, cf); };
    Partials p;
    const Fr rr = fr_from_abi(r), ss = fr_from_abi(s);
    prove_device(ctx, *pk, *rc, wit, rr, ss, p, &upload);
    if (check_failed(ctx)) return ZKG16_ERR_UNSATISFIED;
    finish_proof(ctx, *pk, rr, ss, p, proof_out, inf_out);
    ZK_LANE_END(ctx)
}

}  // extern "C"
