// What the files behind the C ABI (include/zkg16.h) share: api.hip (ctx, lanes, options, instrumentation), api_keys.hip (key /
// R1CS / assignment residency), api_prove.hip (the prove pipeline and its host tail), api_stages.hip (setup and the stage entry
// points), api_group.hip (device groups), api_verify.hip (batched verification), api_rerandomize.hip (re-randomising) and
// api_trapdoor.hip (setup-and-prove requests).  None of them holds a kernel.
#pragma once
#include <chrono>
#include <exception>

#include "common.hpp"
#include "verify_batch.hpp"

namespace zk {

// ---- zkg16_ctx::timings (zkg16_last_timings; device.py names them).  The layout is ABI: it does not move.  The array keeps its
// declared size, PROOF_TIMING_SLOTS = 24; the 22 slots below are the ones in use.
enum ProofTiming : int {
    T_SPMV = 0,            // always 0 (the SpMV is part of the witness map)
    T_WITNESS_MAP = 1,     // device time of the witness map
    T_SORT = 2,            // device time of digits + sort of both scalar vectors
    // host-observed completion gaps of H, L, A, B1, B2 (collected in the order B2, L, A, B1, H — the first gap contains most of the
    // device time: NOT a breakdown)
    T_GAP_H = 3, T_GAP_L = 4, T_GAP_A = 5, T_GAP_B1 = 6, T_GAP_B2 = 7,
    T_HOST_TAIL = 8,       // the O(1) host tail (a batch: H's combination and the tails of all its proofs)
    T_TOTAL = 9,           // wall time of the proving call
    // device time of the bucket accumulation (+ fix-ups) of H, L, A, B1, B2 and of their bucket reductions, from event pairs on the
    // streams they ran on — the per-stage times upstream's spans ("Compute C" = H + L, "Compute A", "Compute B in G1", "Compute B in
    // G2": ark-groth16 prover.rs) correspond to.  Kernels of different MSMs overlap, so these sum to more than the proof.
    T_ACC_H = 10, T_ACC_L = 11, T_ACC_A = 12, T_ACC_B1 = 13, T_ACC_B2 = 14,
    T_RED_H = 15, T_RED_L = 16, T_RED_A = 17, T_RED_B1 = 18, T_RED_B2 = 19,
    T_HORNER_H = 20,       // host Horner of H's window sums (after the last device event of the proof: exposed)
    T_HORNER_Z = 21,       // ... of the other four (they overlap H's device work)
    T_COUNT = 22
};
// ---- zkg16_ctx::vb_timings (zkg16_verify_batch_timings), ABI as well
enum VerifyTiming : int {
    V_MEMBERSHIP = 0,      // launch to membership verdicts on the host (host clock)
    V_MILLER = 1,          // scaling + Miller kernel
    V_PRODUCT = 2,         // product tree
    V_MSM = 3,             // sum rho_k C_k
    V_HOST = 4,            // host equation (vb_decide writes this slot and the next)
    V_BISECT = 5,          // bisecting
    V_TOTAL = 6,           // wall time of the call
    V_HOST_FORM = 7,       // 1 when the host form answered
    V_DECODE = 8,          // decoding the wire bytes (zkg16_verify_batch_wire)
    V_EACH = 9,            // the per-proof pass that took over from bisecting (0: it did not run)
    V_RANGE_TESTS = 10,    // range tests bisecting made
    V_PRIME_INPUTS = 11,   // the prime form: the inputs kernel (device events; 0 when the host form answered or the call was not a prime call)
    V_PRIME_SUMS = 12,     // ... and the sums kernels
    V_U64_SUMS = 13,       // the u64 form: the sums kernels (device events; 0 when the host form answered or the call was not a u64 call)
    V_U64_X = 14,          // ... and the X kernel of its per-proof pass (0 when that pass did not run)
    V_COUNT = 15
};
// ---- zkg16_ctx::rr_timings (zkg16_rerandomize_timings), ABI as well
enum RerandomizeTiming : int {
    R_UPLOAD = 0,          // proofs (limbs or wire bytes), multipliers and delta to the device (device events, as the next five)
    R_DECODE = 1,          // the decompress and membership kernels (zkg16_rerandomize_batch_wire only)
    R_G1 = 2,              // the G1 kernel: A' and C'
    R_G2 = 3,              // the G2 kernel: B' (it runs beside the G1 kernel, so the two sum to more than the call)
    R_COMPRESS = 4,        // the compress kernel (zkg16_rerandomize_batch_wire only)
    R_READBACK = 5,        // results to the host
    R_TOTAL = 6,           // wall time of the call
    R_HOST_FORM = 7,       // 1 when the host form answered
    R_COUNT = 8
};
// ---- zkg16_ctx::pkc_timings (zkg16_pk_check_timings), ABI as well
enum PkCheckTiming : int {
    K_A = 0, K_B1 = 1, K_B2 = 2, K_H = 3, K_L = 4,      // the kernel of each query of the last key check (device events on the streams they ran on: they overlap)
    K_TOTAL = 5,           // wall time of that check, its one synchronisation included
    K_BULK_KERNEL = 6,     // the last zkg16_points_check_bulk: its kernel (device events)
    K_BULK_UPLOAD = 7,     // ... and the upload and conversion in front of it (host clock)
    K_COUNT = 8
};
static_assert(K_COUNT == PK_CHECK_TIMING_SLOTS, "timing slots");
// ---- zkg16_ctx::pkb_timings (zkg16_pk_bytes_timings), ABI as well
enum PkBytesTiming : int {
    B_COPY = 0,            // host time in the staging ring: bytes copied into / out of its pinned halves and the waits for their transfers (host clock)
    B_A = 1, B_B1 = 2, B_B2 = 3, B_H = 4, B_L = 5,      // the decode / encode / read kernels of each query, first piece to last (device events; the copies of later pieces overlap them)
    B_VK = 6,              // gamma_abc_g1 on the device and the single points on the host (host clock)
    B_CHECK = 7,           // the key check of a validated load (K_TOTAL of that check; 0 otherwise)
    B_TOTAL = 8,           // wall time of the call
    B_COUNT = 9
};
static_assert(B_COUNT == PK_BYTES_TIMING_SLOTS, "timing slots");
static_assert(T_COUNT <= PROOF_TIMING_SLOTS && V_COUNT == VERIFY_TIMING_SLOTS && R_COUNT == RERANDOMIZE_TIMING_SLOTS, "timing slots");
// the last refusal of a host-only entry point on this thread (zkg16_last_error(NULL)); api.hip
std::string &host_last_error();

int fail(zkg16_ctx *ctx, const HipError &e);      // api.hip: the error's text into ctx->last_error -> its status

#define ZK_API_BEGIN(ctx)                         \
    if (!(ctx)) return ZKG16_ERR_BAD_ARG;         \
    std::lock_guard<std::mutex> _lk((ctx)->mu);   \
    try {                                         \
        ZK_HIP(hipSetDevice((ctx)->device));
#define ZK_API_END(ctx)                           \
    }                                             \
    catch (const HipError &e) { return fail((ctx), e); } \
    catch (const std::bad_alloc &) { return ZKG16_ERR_OOM; } \
    return ZKG16_OK;

inline double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---- lanes (common.hpp: zkg16_ctx::lanes).  Proving entry points take a free lane for the duration of the call; everything
// else (key / matrix / assignment residency, setup, the stage entry points) runs on the root under its mutex.
// A free lane of `root` for one proof: the lowest free one (a single caller always gets lane 0 = the root itself, so nothing
// changes for it); callers beyond opt_lanes wait.  The lane's mutex is held for the lease.  (api.hip)
struct LaneLease {
    zkg16_ctx *root, *lane = nullptr;
    int idx = -1;
    double t0 = 0;
    std::unique_lock<std::mutex> held;
    std::shared_lock<std::shared_mutex> keys;
    explicit LaneLease(zkg16_ctx *r);
    ~LaneLease();
    LaneLease(const LaneLease &) = delete;
    LaneLease &operator=(const LaneLease &) = delete;
};
inline zkg16_ctx *lane_of(zkg16_ctx *root, int idx) { return idx <= 0 || idx > 7 || !root->lanes[idx - 1] ? root : root->lanes[idx - 1].get(); }
// the proving entry points: `ctx` is rebound to the leased lane for the body, `root` keeps the handle maps
#define ZK_LANE_BEGIN(ctx)                        \
    if (!(ctx)) return ZKG16_ERR_BAD_ARG;         \
    zkg16_ctx *const root = (ctx);                \
    try {                                         \
        LaneLease _lease(root);                   \
        (ctx) = _lease.lane;                      \
        try {                                     \
            ZK_HIP(hipSetDevice((ctx)->device));
#define ZK_LANE_END(ctx)                          \
        } catch (const HipError &e) {             \
            const int _rc = fail((ctx), e);       \
            if ((ctx) != root) { std::lock_guard<std::mutex> _l(root->lane_mu); root->last_error = (ctx)->last_error; } \
            return _rc;                           \
        }                                         \
    } catch (const HipError &e) { return fail(root, e); } \
    catch (const std::bad_alloc &) { return ZKG16_ERR_OOM; } \
    return ZKG16_OK;

// ---- host <-> ABI conversions (u64 limbs and u32 limbs share the little-endian byte layout)
inline Fr fr_from_abi(const uint64_t *l) {
    Fr v;
    memcpy(&v, l, sizeof v);
    return v;
}
inline G1Affine g1_from_abi(const uint64_t *l, int inf) {
    G1Affine p;
    if (inf) return G1Affine::inf();
    memcpy(&p, l, sizeof p);
    return p;
}
inline G2Affine g2_from_abi(const uint64_t *l, int inf) {
    G2Affine p;
    if (inf) return G2Affine::inf();
    memcpy(&p, l, sizeof p);
    return p;
}
template <class A>
void point_to_abi(const A &p, uint64_t *out, uint8_t *inf) {
    if (p.is_inf()) {
        memset(out, 0, sizeof p);
        if (inf) *inf = 1;
    } else {
        memcpy(out, &p, sizeof p);
        if (inf) *inf = 0;
    }
}

// ---- uploads (api_keys.hip)
template <class A> struct UOf;
template <> struct UOf<G1Affine> { using T = G1AffineU; };
template <> struct UOf<G2Affine> { using T = G2AffineU; };
// Upload a slice [lo, hi) of a saturated affine query vector and convert it into the unsaturated device form at
// dst[0 .. hi-lo); flagged-infinity points become (0,0).  A = G1Affine or G2Affine.
template <class A>
void upload_points(zkg16_ctx *ctx, typename UOf<A>::T *dst, const uint64_t *src, const uint8_t *inf, size_t lo, size_t hi);
template <class A>
void upload_one(zkg16_ctx *ctx, typename UOf<A>::T *dst, const A &p);
// host -> device copy of a large pageable buffer through the ctx's pinned ring, queued on ctx->stream
void upload_h2d(zkg16_ctx *ctx, void *dst, const void *src, size_t bytes);
// validate + allocate an R1CS (nothing is copied yet) / queue the copies of its three matrices on ctx->stream
int r1cs_create(const uint64_t *const rp[3], const uint32_t *const col[3], const uint64_t *const cf[3], size_t num_instance,
                size_t num_constraints, size_t num_variables, std::unique_ptr<R1csDev> &out);
void r1cs_copy(zkg16_ctx *ctx, R1csDev &r, const uint64_t *const rp[3], const uint32_t *const col[3], const uint64_t *const cf[3]);

// ---- membership of resident points (pk_check.hip; kernels: pk_check_dev.cuh).  Launches on `st`, nothing synchronises.
// res: two device words per array, {number of bad points, smallest bad index}; pk_check_init_launch writes {0, UINT64_MAX} into
// `slots` of them, pk_check_launch folds the verdicts of n U-form affine entries at base + i * stride (bytes) into one
void pk_check_init_launch(hipStream_t st, uint64_t *res, int slots);
void pk_check_launch(hipStream_t st, int group, const void *base, size_t stride, size_t n, const VbEndo &en, uint64_t *res);
// The five queries of a resident key or shard (a, b_g1, b_g2, h, l) and its five single points (api_keys.hip): what zkg16_pk_check
// returns.  One synchronisation
struct PkCheckResult {
    uint64_t n_bad[5], first_bad[5];
    uint32_t single_mask;
    bool ok() const { return !single_mask && !(n_bad[0] | n_bad[1] | n_bad[2] | n_bad[3] | n_bad[4]); }
};
void pk_check_run(zkg16_ctx *ctx, const PkDev &pk, PkCheckResult &out);

// ---- a key's points between wire bytes and the resident form (pk_bytes.hip; kernels: pk_bytes_dev.cuh).  Launches on `st`, nothing
// synchronises.  res: two device words per array, {points with a decode status, smallest (index << 3 | status)};
// pk_bytes_init_launch writes {0, UINT64_MAX} into `slots` of them
void pk_bytes_init_launch(hipStream_t st, uint64_t *res, int slots);
// n encodings of one group back to back (48 / 96 bytes, device) -> U-form affine entries at out + i * stride (bytes), (0, 0) for the
// point at infinity and for a refused encoding; `first` is added to the index a failure reports
void pk_bytes_decode_launch(hipStream_t st, int group, const uint8_t *bytes, size_t n, void *out, size_t stride, size_t first, uint64_t *res);
// n U-form entries at base + i * stride -> the bytes of zkg16_points_compress, back to back / the limbs and flags of zkg16_pk_load
void pk_bytes_encode_launch(hipStream_t st, int group, const void *base, size_t stride, size_t n, uint8_t *out);
void pk_bytes_read_launch(hipStream_t st, int group, const void *base, size_t stride, size_t n, uint64_t *limbs, uint8_t *inf);

// events of one proof, destroyed on every exit path
struct EventSet {
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    EventSet() { for (auto &e : ev) ZK_HIP(hipEventCreate(&e)); }
    ~EventSet() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    EventSet(const EventSet &) = delete;
    EventSet &operator=(const EventSet &) = delete;
};

// Every launch helper targets ctx->stream: while this guard lives the ctx's second stream takes its place, on every way out
struct StreamSwap {
    zkg16_ctx *c;
    explicit StreamSwap(zkg16_ctx *ctx) : c(ctx) { std::swap(c->stream, c->wm_stream); }
    ~StreamSwap() { std::swap(c->stream, c->wm_stream); }
    StreamSwap(const StreamSwap &) = delete;
    StreamSwap &operator=(const StreamSwap &) = delete;
};

// ---- batched verification and re-randomising on a lane (api_verify.hip defines what is declared here; api_rerandomize.hip)
const size_t VB_PASS = 65536;          // pairs / points per launch: one wave per SIMD of a 256-CU device
struct VbEvents {
    hipEvent_t ev[14] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    VbEvents() { for (auto &e : ev) ZK_HIP(hipEventCreate(&e)); }
    ~VbEvents() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    VbEvents(const VbEvents &) = delete;
    VbEvents &operator=(const VbEvents &) = delete;
};
inline float vb_elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
}
// The flags the kernels read: zkg16_verify_prepared and the host form read all-zero limbs as the point at infinity whatever the flag
// says, the kernels go by the flag alone (all-zero limbs are on no curve and would fail membership), so the flag is set for them
std::vector<uint8_t> vb_flags(const uint64_t *proofs, const uint8_t *inf, size_t k);
// The lane's main stream and the two beside it that the per-point kernels of A, B and C spread over
struct VbStreams {
    hipStream_t main, c, b;
};
inline VbStreams vb_streams(zkg16_ctx *ctx) { return VbStreams{ctx->stream, ctx->slots[1].stream, ctx->slots[2].stream}; }
// fork: e is recorded on the main stream, and `also` (if any), c and b wait for it, in that order
inline void vb_fork(const VbStreams &s, hipEvent_t e, hipStream_t also = nullptr) {
    ZK_HIP(hipEventRecord(e, s.main));
    if (also) ZK_HIP(hipStreamWaitEvent(also, e, 0));
    for (hipStream_t st : {s.c, s.b}) ZK_HIP(hipStreamWaitEvent(st, e, 0));
}
// join: the main stream waits for what c and b hold now (e_c, e_b recorded there); e_also (if any) is recorded on `also` in between
inline void vb_join(const VbStreams &s, hipEvent_t e_c, hipEvent_t e_b, hipEvent_t e_also = nullptr, hipStream_t also = nullptr) {
    ZK_HIP(hipEventRecord(e_c, s.c));
    ZK_HIP(hipEventRecord(e_b, s.b));
    if (e_also) ZK_HIP(hipEventRecord(e_also, also));
    ZK_HIP(hipStreamWaitEvent(s.main, e_c, 0));
    ZK_HIP(hipStreamWaitEvent(s.main, e_b, 0));
}
// The three membership launches of one chunk of n proofs (48 limbs and 3 flags each; verdicts m3, 3 a proof): A on the main
// stream, C and B beside it.
void vb_membership_chunk(const VbStreams &s, const uint64_t *pts, const uint8_t *fl, size_t n, const VbEndo &en, uint8_t *m3);
// The wire decode of k proofs (192 bytes each, on the device) in launches of `pass`, unvalidated: B (two powers and an inversion) on
// the main stream, A and C (one power each) beside it, then the join (e_c, e_b).  The side streams already wait for the bytes.
// Limbs (k x 48), flags and statuses (k x 3 each) land where the membership launches read them
void vb_wire_decode(const VbStreams &s, hipEvent_t e_c, hipEvent_t e_b, const uint8_t *d_wire, size_t k, size_t pass, const VbEndo &en, uint64_t *d_proofs,
                    uint8_t *d_inf, uint8_t *d_st);

// ---- the prove pipeline (api_prove.hip), as far as the device groups need it
struct GroupRank;      // group.hpp
struct Partials {
    G1XYZZ h, l, a, b1;
    G2XYZZ b2;
    // un-sharded proofs: s*(a + alpha) and r*(b1 + beta) are formed on the host as soon as A and B1 are collected, while the
    // device still works on the remaining MSMs (they are ~0.35 ms of the 0.4 ms host tail)
    bool have_early = false;
    G1XYZZ s_a, r_b1;
};
void prove_device(zkg16_ctx *ctx, PkDev &pk, R1csDev &rc, WitnessDev &wit, const Fr &r, const Fr &s, Partials &out,
                  const std::function<void()> *before_witness_map = nullptr, const ZParts *zp = nullptr, GroupRank *grp = nullptr,
                  bool may_check = true);      // false (group calls): option "check_satisfied" is not looked at
void prove_tail(PkDev &pk, const Fr &r, const Fr &s, const Partials &p, uint64_t *proof_out, uint8_t *inf_out);
// the record of zkg16_prove_partial (h, l, a, b1 | b2 as affine limbs, one infinity flag each), and the sum of n_ranks of them
void partials_to_abi(const Partials &p, uint64_t out[72], uint8_t inf[5]);
void sum_partials(Partials &p, const uint64_t *partials, const uint8_t *partial_inf, int n_ranks);

}  // namespace zk
