// libzkg16 C ABI (include/zkg16.h), part 1 of 8: the ctx itself — kernel timer, streams, lanes, the device allocation cache,
// zkg16_init / zkg16_destroy, options and instrumentation.  The other parts: api_keys.hip (key / R1CS / witness residency),
// api_prove.hip (the prove pipeline and its O(1) host tail), api_stages.hip (setup and the stage entry points), api_group.hip (device
// groups), api_verify.hip (batched verification), api_rerandomize.hip (re-randomising), api_trapdoor.hip (setup-and-prove requests);
// api_internal.hpp is what they share.
//
// There is NO CPU fallback: without a HIP device zkg16_init fails with ZKG16_ERR_NO_DEVICE.
#include "api_internal.hpp"

using namespace zk;

namespace zk {
ScopedKernelTimer::ScopedKernelTimer(zkg16_ctx *c, const char *n, double u, hipStream_t st)
    : ctx(c), name(n), units(u), stream(st ? st : c->stream) {
    if (!ctx->opt.kernel_timing) return;
    if (ctx->opt.kernel_timing_accumulate_only && strncmp(n, "msm_accumulate", 14) != 0) return;
    ZK_HIP(hipEventCreate(&e0));
    ZK_HIP(hipEventCreate(&e1));
    ZK_HIP(hipEventRecord(e0, stream));
}
ScopedKernelTimer::~ScopedKernelTimer() {
    if (!e0) return;
    (void)hipEventRecord(e1, stream);
    ctx->pending_events.push_back(PendingEvent{name, units, e0, e1});
}
void kernel_timer_resolve(zkg16_ctx *ctx) {
    if (ctx->pending_events.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->wm_stream);
    for (auto &sl : ctx->slots)
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    for (auto &p : ctx->pending_events) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
            auto &s = ctx->kstats[p.name];
            s.launches++;
            s.ms += ms;
            s.units += p.units;
        }
        (void)hipEventDestroy(p.e0);
        (void)hipEventDestroy(p.e1);
    }
    ctx->pending_events.clear();
}
}  // namespace zk

namespace {

const char *k_version = "zkg16 0.1 (gfx950; BLS12-381 Groth16 prove hot path)";

// everything zkg16_set_option and zkg16_kernel_timing set; opt_lanes lives on the root alone (under lane_mu) and is not copied
void copy_options(zkg16_ctx *dst, const zkg16_ctx *src) { dst->opt = src->opt; }
void create_streams(zkg16_ctx *ctx) {
    // Plain (equal-priority) streams.  Measured at n = 32: main low / witness-map high priority 16.6 ms per proof,
    // reversed 16.2 ms, no priorities 15.0 ms (profiles/kernel_timeline_r1_*.txt).
    ZK_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ZK_HIP(hipStreamCreateWithFlags(&ctx->wm_stream, hipStreamNonBlocking));
    // HIP hands streams to its 4 hardware queues round-robin in creation order, and which streams end up sharing a queue
    // moves a proof by ~4 % (13.9 vs 14.5 ms at n = 32).  All of a ctx's streams are therefore created here, in the order
    // the measured-best pairing needs (main | witness map | B2, L, A, B1, H reductions).  (A further ctx of the same
    // process starts three queues on; two such contexts together measured 76 proofs/s, two aligned ones 73.)
    for (int i : {0, 2, 3, 4, 1}) ZK_HIP(hipStreamCreateWithFlags(&ctx->slots[i].stream, hipStreamNonBlocking));
}
// everything a ctx (root or lane) owns on the device
void teardown(zkg16_ctx *ctx) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->wm_stream);
    if (ctx->extra_host) (void)hipHostFree(ctx->extra_host);
    if (ctx->batch_host) (void)hipHostFree(ctx->batch_host);
    ctx->batch_host = nullptr;
    ctx->batch_host_bytes = 0;
    if (ctx->mbatch_host) (void)hipHostFree(ctx->mbatch_host);
    ctx->mbatch_host = nullptr;
    ctx->mbatch_host_bytes = 0;
    ctx->mbatch_dev.release();
    if (ctx->circuit_stage) (void)hipHostFree(ctx->circuit_stage);
    ctx->circuit_stage = nullptr;
    ctx->circuit_stage_bytes = 0;
    for (int i = 0; i < 2; i++) {
        if (ctx->stage_host[i]) (void)hipHostFree(ctx->stage_host[i]);
        if (ctx->stage_done[i]) (void)hipEventDestroy(ctx->stage_done[i]);
    }
    for (auto &sl : ctx->slots) {
        if (sl.wsums_host) (void)hipHostFree(sl.wsums_host);
        if (sl.acc_done) (void)hipEventDestroy(sl.acc_done);
        if (sl.red_done) (void)hipEventDestroy(sl.red_done);
        if (sl.acc_start) (void)hipEventDestroy(sl.acc_start);
        if (sl.red_start) (void)hipEventDestroy(sl.red_start);
        sl.buckets.release();
        sl.bucket_sum.release();
        sl.wsums_dev.release();
        sl.seg_head.release();
        sl.seg_tail.release();
        sl.seg_meta.release();
        sl.long_list.release();
        sl.long_sums.release();
        sl.red_a.release(); sl.red_b.release(); sl.red_c.release();
        if (sl.stream) { (void)hipStreamSynchronize(sl.stream); (void)hipStreamDestroy(sl.stream); }
    }
    if (ctx->wm_stream) (void)hipStreamDestroy(ctx->wm_stream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
}
}  // namespace

namespace zk {
int fail(zkg16_ctx *ctx, const HipError &e) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", e.what, hipGetErrorString(e.err), e.file, e.line);
    if (ctx) ctx->last_error = buf;
    (void)hipGetLastError();
    if (e.err == hipErrorOutOfMemory) return ZKG16_ERR_OOM;
    if (e.err == hipErrorInvalidValue && strstr(e.what, "domain")) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    return ZKG16_ERR_HIP;
}

std::string &host_last_error() {
    static thread_local std::string text;
    return text;
}

LaneLease::LaneLease(zkg16_ctx *r) : root(r) {
    {
        std::unique_lock<std::mutex> lk(root->lane_mu);
        const int cap = root->opt_lanes < 1 ? 1 : root->opt_lanes > 8 ? 8 : root->opt_lanes;
        root->lane_cv.wait(lk, [&] {
            for (int i = 0; i < cap; i++)
                if (!root->lane_busy[i]) { idx = i; return true; }
            return false;
        });
        if (idx > 0 && !root->lanes[idx - 1]) {
            ZK_HIP(hipSetDevice(root->device));
            auto l = std::make_unique<zkg16_ctx>();
            l->device = root->device;
            l->num_cus = root->num_cus;
            l->root = root;
            copy_options(l.get(), root);
            try {
                create_streams(l.get());
            } catch (...) {
                teardown(l.get());
                throw;
            }
            root->lanes[idx - 1] = std::move(l);
        }
        root->lane_busy[idx] = true;
        lane = idx == 0 ? root : root->lanes[idx - 1].get();
    }
    held = std::unique_lock<std::mutex>(lane->mu);
    keys = std::shared_lock<std::shared_mutex>(root->key_rw);
    t0 = now_ms();
}
LaneLease::~LaneLease() {
    if (idx < 0) return;
    const double t1 = now_ms();
    if (keys.owns_lock()) keys.unlock();
    if (held.owns_lock()) held.unlock();
    {
        std::lock_guard<std::mutex> lk(root->lane_mu);
        root->lane_busy[idx] = false;
        root->last_lane = idx;
        if (root->lane_log.size() >= 256) root->lane_log.erase(root->lane_log.begin(), root->lane_log.begin() + 128);
        root->lane_log.push_back(zkg16_ctx::LaneLogEntry{idx, t0, t1});
    }
    root->lane_cv.notify_one();
}
}  // namespace zk

namespace zk {
// ---- device allocation cache (see common.hpp)
namespace {
struct DevCache {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void *> free_blocks;     // by (device, size)
    size_t cached_bytes = 0;
    static constexpr size_t LIMIT = (size_t)96 << 30, MIN_CACHED = (size_t)1 << 20;
};
DevCache &dev_cache() {
    static DevCache c;
    return c;
}
}  // namespace
void *dev_acquire(size_t bytes, size_t *got) {
    DevCache &c = dev_cache();
    if (bytes >= DevCache::MIN_CACHED) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(c.mu);
        auto it = c.free_blocks.lower_bound(std::make_pair(dev, bytes));
        if (it != c.free_blocks.end() && it->first.first == dev && it->first.second <= bytes + bytes / 4) {      // at most 25 % larger than asked
            void *p = it->second;
            *got = it->first.second;
            c.cached_bytes -= it->first.second;
            c.free_blocks.erase(it);
            return p;
        }
    }
    void *p = nullptr;
    const bool trace = getenv("ZKG16_TRACE_ALLOC") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&p, bytes);
    if (trace) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > 1.0) fprintf(stderr, "dev_acquire: hipMalloc of %.1f MB took %.2f ms\n", bytes / 1048576.0, ms);
    }
    if (e != hipSuccess) {                      // out of memory with blocks parked in the cache: give them back and retry once
        (void)hipGetLastError();
        dev_cache_flush();
        ZK_HIP(hipMalloc(&p, bytes));
    }
    *got = bytes;
    return p;
}
void dev_release(void *p, size_t bytes) noexcept {
    DevCache &c = dev_cache();
    if (bytes >= DevCache::MIN_CACHED) {
        const bool trace = getenv("ZKG16_TRACE_ALLOC") != nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        (void)hipDeviceSynchronize();           // what hipFree would have done
        if (trace) {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms > 1.0) fprintf(stderr, "dev_release: sync before caching %.1f MB took %.2f ms\n", bytes / 1048576.0, ms);
        }
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.cached_bytes + bytes <= DevCache::LIMIT) {
            c.free_blocks.emplace(std::make_pair(dev, bytes), p);
            c.cached_bytes += bytes;
            return;
        }
    }
    const bool trace = getenv("ZKG16_TRACE_ALLOC") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    (void)hipFree(p);
    if (trace) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > 1.0) fprintf(stderr, "dev_release: hipFree of %.1f MB took %.2f ms\n", bytes / 1048576.0, ms);
    }
}
uint64_t dev_cached_bytes() {
    DevCache &c = dev_cache();
    int cur = 0;
    (void)hipGetDevice(&cur);
    std::lock_guard<std::mutex> lk(c.mu);
    uint64_t sum = 0;
    for (auto &kv : c.free_blocks)
        if (kv.first.first == cur) sum += kv.first.second;
    return sum;
}
void dev_cache_flush() noexcept {
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto &kv : c.free_blocks) {
        (void)hipSetDevice(kv.first.first);
        (void)hipFree(kv.second);
    }
    (void)hipSetDevice(cur);
    c.free_blocks.clear();
    c.cached_bytes = 0;
}
}  // namespace zk
extern "C" {

const char *zkg16_version(void) { return k_version; }

const char *zkg16_strerror(int status) {
    switch (status) {
        case ZKG16_OK: return "ok";
        case ZKG16_ERR_BAD_ARG: return "bad argument";
        case ZKG16_ERR_DOMAIN_TOO_LARGE: return "evaluation domain too large (ark: PolynomialDegreeTooLarge)";
        case ZKG16_ERR_HIP: return "HIP runtime error";
        case ZKG16_ERR_OOM: return "out of memory";
        case ZKG16_ERR_NO_DEVICE: return "no HIP device (this library has no CPU fallback)";
        case ZKG16_ERR_BAD_HANDLE: return "unknown handle";
        case ZKG16_ERR_UNSUPPORTED: return "unsupported";
        case ZKG16_ERR_UNSATISFIED: return "an assignment does not satisfy its R1CS (option check_satisfied, or a trapdoor-route call)";
        default: return "unknown status";
    }
}

// without a ctx: the last refusal of a host-only entry point on the calling thread (empty until one has refused)
const char *zkg16_last_error(zkg16_ctx *ctx) { return ctx ? ctx->last_error.c_str() : zk::host_last_error().c_str(); }

int zkg16_init(const int *device_ids, int n_devices, zkg16_ctx **out) {
    if (!out) return ZKG16_ERR_BAD_ARG;
    *out = nullptr;
    if (n_devices != 1 && !(n_devices == 0 && !device_ids)) return ZKG16_ERR_UNSUPPORTED;   // one GPU per ctx / process
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return ZKG16_ERR_NO_DEVICE;
    }
    const int dev = (n_devices == 1 && device_ids) ? device_ids[0] : 0;
    if (dev < 0 || dev >= count) return ZKG16_ERR_BAD_ARG;
    auto *ctx = new (std::nothrow) zkg16_ctx();
    if (!ctx) return ZKG16_ERR_OOM;
    ctx->device = dev;
    try {
        ZK_HIP(hipSetDevice(dev));
        hipDeviceProp_t prop;
        ZK_HIP(hipGetDeviceProperties(&prop, dev));
        ctx->num_cus = prop.multiProcessorCount;
        // the code object holds gfx950 kernels only (no fallback path, no other ISA): any other device is "no device"
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            ctx->last_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
            delete ctx;
            return ZKG16_ERR_NO_DEVICE;
        }
        create_streams(ctx);
    } catch (const HipError &e) {
        int rc = fail(ctx, e);
        delete ctx;
        return rc;
    }
    *out = ctx;
    return ZKG16_OK;
}

void zkg16_destroy(zkg16_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (auto &l : ctx->lanes)
        if (l) {
            {
                std::lock_guard<std::mutex> lk(l->mu);      // a proof still running on that lane finishes first
                teardown(l.get());
            }
            l.reset();
        }
    teardown(ctx);
    ctx->pks.clear();
    ctx->r1cs.clear();
    ctx->wits.clear();
    ctx->prime_dev.reset();
    ctx->ntt_tables.clear();
    delete ctx;
    dev_cache_flush();      // a destroyed ctx really returns its memory (other live contexts simply allocate afresh)
}

}  // extern "C"
namespace {
// One validation per option: `v` within [lo, hi] (and `also`) -> the option takes `stored`, which is `v` unless the option normalises it.
int set_option_one(zkg16_ctx *ctx, const char *name, int64_t v) {
    zkg16_ctx::Options &o = ctx->opt;
    const auto is = [name](const char *n) { return !strcmp(name, n); };
    const auto set = [v](int &dst, int64_t lo, int64_t hi, int64_t stored, bool also = true) {
        if (v < lo || v > hi || !also) return (int)ZKG16_ERR_BAD_ARG;
        dst = (int)stored;
        return (int)ZKG16_OK;
    };
    if (is("window_bits")) return set(o.window_bits, 0, 20, v, v != 1);      // 0 = by length, else 2..20
    if (is("min_seg")) return set(o.min_seg, 0, 4096, v);
    if (is("ntt_mode")) return set(o.ntt_mode, 0, 3, v, v != 2);             // 3: unsaturated, but three passes above 2^22
    // 4 = classic everywhere (0 restores the default, 3); 5 = bit-sliced wherever it applies; 6 = the default without the bit-sliced form
    if (is("reduce_mode")) return set(o.reduce_mode, 0, 6, v == 0 ? 3 : v == 4 ? 0 : v);
    if (is("g1_waves")) return set(o.g1_waves, 0, 4, v);
    if (is("fixup_aux")) return set(o.fixup_aux, INT64_MIN, INT64_MAX, v ? 1 : 0);
    if (is("window_bits_h")) return set(o.window_bits_h, 0, 20, v, v != 1);
    if (is("wm_concurrent")) { o.wm_concurrent = (int)v; return ZKG16_OK; }   // -1 auto (default), 0 in-order, 1 third stream
    // 1 (default; also 0): the last seven stages by lane exchanges, the others one per LDS trip; 2: every stage through the LDS;
    // 3: the top seven stages by lane exchanges too; 4: two per trip (radix 4)
    if (is("ntt_radix")) return set(o.ntt_radix, 0, 4, v == 0 ? 1 : v);
    if (is("ntt_xcd")) return set(o.ntt_xcd, 0, 2, v == 2 ? 0 : 1);          // 1 (default): XCD-aware tile order in the NTT passes; 2 = off (0 restores the default)
    // entry stride of window tables built after this call (zkg16_pk_precompute; an existing table keeps its layout): 0 = by table size (default), 1 = packed, 2 = padded
    if (is("table_stride")) return set(o.table_stride, 0, 2, v);
    if (is("acc_debug")) return set(o.acc_debug, 0, 15, v);                  // timing probes of the accumulation kernels; results are WRONG while set
    if (is("sort_mode")) return set(o.sort_mode, 0, 1, v);                   // 0 (default): hand-written wave-ballot bucket scatter; 1: rocPRIM device radix sort
    // bit 0: G1, bit 1: G2 software-pipelined gather; 0 (default) and 4: neither.  With four G1 waves per SIMD and window tables the
    // plain form (gather right before its addition) measured 153.6 against 157.4 ms per 128x128 proof, and the same at every other
    // size and with plain keys (profiles/ab_options_r2_final.txt)
    if (is("acc_pipeline")) return set(o.acc_pipeline, 0, 4, v == 4 ? 0 : v);
    if (is("fuse_pointwise")) return set(o.fuse_pointwise, INT64_MIN, INT64_MAX, v ? 1 : 0);      // 1 (default): the point-wise product on the load of the last transform; 0: own pass
    // 6 (default; also 0): C only inverse-transformed (poly.hip: wm_transforms); 7: arkworks' seven
    if (is("wm_transforms")) return set(o.wm_transforms, 0, 7, v == 7 ? 7 : 6, v == 0 || v >= 6);
    // -1 (default): 1 from 2^23 on for keys with window tables; 0: z-side accumulations start at once; 1: after the witness map; 2: after the h-side sort too
    if (is("wm_first")) return set(o.wm_first, -1, 2, v);
    if (is("spmv_dict")) return set(o.spmv_dict, 0, 2, v);                   // 0 / 1 (default): 16-bit coefficient dictionary in the SpMV; 2: 32-byte coefficients
    // B-side term list = the sorted full list minus the masked terms: 0 (default) with window tables, 1 always; 2: second sort
    if (is("b_filter")) return set(o.b_filter, 0, 2, v);
    // host combination of the MSMs' window sums: 0 = by key kind (threads for plain keys), 1 = always threaded, 2 = never
    if (is("collect_threads")) return set(o.collect_threads, 0, 2, v == 0 ? -1 : v == 2 ? 0 : 1);
    // setup's fixed-base windows: 0 = by batch size, else 4..14 (ladder-built table) or 16 / 18 / 20 (two-level)
    if (is("fixed_base_bits")) return set(o.fixed_base_bits, 0, 20, v, v == 0 || (v >= 4 && !(v > 14 && (v & 1))));
    // G2 bucket accumulation: 0 / 1 (default) = Fq2 products as two fused two-product reductions (LDS-parked operands), 2 = Karatsuba with three
    if (is("g2_lazy")) return set(o.g2_lazy, 0, 2, v == 2 ? 0 : 1);
    // G1 bucket accumulation (plain loop): 0 / 1 (default) = every field product inlined, 2 = products as device-function calls (the earlier loop)
    if (is("g1_inline")) return set(o.g1_inline, 0, 2, v == 2 ? 0 : 1);
    // G2 bucket accumulation: 1 (default) = every Fq2 value split over a pair of lanes (component 0 on the even lane, 1 on the odd one),
    // two waves per SIMD; 0 = one lane per point.  Proofs are byte-identical; stored bucket representatives may differ within their bounds
    if (is("g2_split")) return set(o.g2_split, 0, 1, v);
    // ... and the products of its loop: 0 / 2 (default) = inlined, 1 = device-function calls
    if (is("g2_split_form")) return set(o.g2_split_form, 0, 2, v == 2 ? 0 : v);
    // default G1 / G2 bucket accumulation loops: 1 (default) = mixed additions without the carry passes their results do not need,
    // 0 = the earlier additions (xyzz_madd_inline, xyzz_madd_lazy)
    if (is("acc_lazy")) return set(o.acc_lazy, 0, 1, v);
    // zkg16_prove_matrix: slices of the host sponges the proof is fed in (0 = five growing slices; k = k equal ones; 1 = no overlap: assignment first)
    if (is("matrix_parts")) return set(o.matrix_parts, 0, 8, v);
    // ... and the fewest permutations a slice may hold: the slice count is lowered until it does (0 restores the default, 512; tests set 1)
    if (is("matrix_slice_min")) return set(o.matrix_slice_min, 0, 1 << 20, v == 0 ? MATRIX_SLICE_MIN_DEFAULT : v);
    // zkg16_prove_batch / zkg16_prove_matrix_batch: proofs per device pass, 0 = as many as fit (free HBM, 2^31 terms per list)
    if (is("batch_max")) return set(o.batch_max, 0, 65535, v);
    // zkg16_witness_matrix_batch / zkg16_prove_matrix_batch: host threads of the sponge chains, 0 = 8
    if (is("matrix_batch_threads")) return set(o.matrix_batch_threads, 0, 16, v);
    // the batched witness kernels: cap on either grid dimension, 0 = 65535 (tests set 1..3 to run the loops at small K)
    if (is("matrix_batch_grid")) return set(o.matrix_batch_grid, 0, 65535, v);
    // zkg16_witness_linear_batch / zkg16_prove_linear_batch: 0 (default) = the reference's forward substitution, 1 = Gaussian elimination
    if (is("linear_solver")) return set(o.linear_solver, 0, 1, v);
    // wit_linear_elim_kernel: the largest n whose working matrix lies in LDS, 0 = 64 (tests set 1..7 to run the global workspace at small n)
    if (is("linear_elim_lds_max")) return set(o.linear_elim_lds_max, 0, 64, v);
    // calls with at least this many sponge chains (3K for assignments, k for hashes) walk them on the device (0 restores the default;
    // 1 = always; above 2^32 = never)
    if (is("sponge_chains_min")) {
        if (v < 0) return ZKG16_ERR_BAD_ARG;
        o.sponge_chains_min = v == 0 ? ZKG16_SPONGE_CHAINS_MIN_DEFAULT : v;
        return ZKG16_OK;
    }
    // wit_chain_batch_kernel: permutations of a chain per launch, 0 = 256 (tests set 1 and 4 to carry states between launches)
    if (is("sponge_chain_segment")) return set(o.sponge_chain_segment, 0, 65535, v);
    // zkg16_verify_batch: batches shorter than this go to the host form (0 restores the default; 1 = always the device)
    if (is("verify_batch_min")) return set(o.verify_batch_min, 0, 1 << 30, v == 0 ? ZKG16_VERIFY_BATCH_MIN_DEFAULT : v);
    // zkg16_verify_batch_wire: batches shorter than this are decoded and answered on the host (0 restores the default; 1 = always the device)
    if (is("verify_wire_min")) return set(o.verify_wire_min, 0, 1 << 30, v == 0 ? ZKG16_VERIFY_WIRE_MIN_DEFAULT : v);
    // zkg16_verify_batch[_wire] with ok_each: range tests bisecting may make before the per-proof pass decides what is left
    // (0 restores the default; 1 = after the first; above 2K = never)
    if (is("verify_each_after")) {
        const int rc = set(o.verify_each_after, 0, 1 << 30, v == 0 ? ZKG16_VERIFY_EACH_AFTER_DEFAULT : v);
        if (rc == ZKG16_OK) o.verify_each_after_set = v != 0;      // the u64 entries have a default of their own (zkg16_verify_batch_u64)
        return rc;
    }
    // zkg16_rerandomize_batch[_wire]: batches shorter than this go to the host form (0 restores the default; 1 = always the device)
    if (is("rerandomize_min")) return set(o.rerandomize_min, 0, 1 << 30, v == 0 ? ZKG16_RERANDOMIZE_MIN_DEFAULT : v);
    // ... and proofs per launch (0 = 65,536)
    if (is("rerandomize_pass")) return set(o.rerandomize_pass, 0, 65536, v);
    // 0 (default): the proving calls prove whatever they are handed; 1: they check (A z)(B z) == C z after the SpMV and refuse with ZKG16_ERR_UNSATISFIED
    if (is("check_satisfied")) return set(o.check_satisfied, 0, 1, v);
    // 0 (default): zkg16_pk_load / zkg16_pk_load_range copy what they are handed; 1: they run zkg16_pk_check on the uploaded key and refuse a bad one
    if (is("pk_validate")) return set(o.pk_validate, 0, 1, v);
    // zkg16_pk_load_bytes / zkg16_pk_save / zkg16_pk_read: points per piece of a query (0 = 524,288)
    if (is("pk_bytes_piece")) return set(o.pk_bytes_piece, 0, 1 << 19, v);
    // zkg16_prove_trapdoor_batch: requests per device pass (0 = 65,535)
    if (is("trapdoor_pass")) return set(o.trapdoor_pass, 0, 65535, v);
    if (is("reduce_chunk")) return set(o.reduce_chunk, 0, 64, v, (v & (v - 1)) == 0);      // 0 = default, else a power of two up to 64
    return ZKG16_ERR_UNSUPPORTED;
}
}  // namespace
extern "C" {

// Options apply to every lane of the ctx (a lane created later copies the root's).  "lanes": proofs this ctx runs at a time
// (1..8, default 2; callers beyond that wait).
int zkg16_set_option(zkg16_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return ZKG16_ERR_BAD_ARG;
    if (!strcmp(name, "lanes")) {
        if (value < 1 || value > 8) return ZKG16_ERR_BAD_ARG;
        std::lock_guard<std::mutex> lk(ctx->lane_mu);
        ctx->opt_lanes = (int)value;
        return ZKG16_OK;
    }
    int rc;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        rc = set_option_one(ctx, name, value);
    }
    if (rc != ZKG16_OK) return rc;
    std::vector<zkg16_ctx *> ls;
    {
        std::lock_guard<std::mutex> lk(ctx->lane_mu);
        for (auto &l : ctx->lanes)
            if (l) ls.push_back(l.get());
    }
    for (zkg16_ctx *l : ls) {
        std::lock_guard<std::mutex> lk(l->mu);
        (void)set_option_one(l, name, value);
    }
    return ZKG16_OK;
}

// ------------------------------------------------------------------------------------------------ instrumentation
int zkg16_last_timings(zkg16_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms) return 0;
    int last;
    { std::lock_guard<std::mutex> lk(ctx->lane_mu); last = ctx->last_lane; }
    zkg16_ctx *l = lane_of(ctx, last);
    std::lock_guard<std::mutex> lk(l->mu);
    const int n = cap < T_COUNT ? cap : T_COUNT;
    for (int i = 0; i < n; i++) ms[i] = l->timings[i];
    return n;
}

// The verdicts of the last proving call that ran with option "check_satisfied", from the lane of the proof that finished last (as
// zkg16_last_timings): *k_out = its proofs (0: that call did not check), min(cap, k) of them written.  Returns the number written.
int zkg16_last_check(zkg16_ctx *ctx, uint64_t *n_bad, uint64_t *first_bad, size_t cap, size_t *k_out) {
    if (!ctx) return 0;
    int last;
    { std::lock_guard<std::mutex> lk(ctx->lane_mu); last = ctx->last_lane; }
    zkg16_ctx *l = lane_of(ctx, last);
    std::lock_guard<std::mutex> lk(l->mu);
    const size_t k = l->check_n_bad.size(), n = cap < k ? cap : k;
    if (k_out) *k_out = k;
    for (size_t i = 0; i < n; i++) {
        if (n_bad) n_bad[i] = l->check_n_bad[i];
        if (first_bad) first_bad[i] = l->check_first_bad[i];
    }
    return (int)n;
}

// Lengths of the sorted (scalar, window) term lists of the last proof on this ctx = mixed additions per MSM that uses the list:
// [0] the z list (A and L), [1] the B list (B1 and B2; 0 = they used the z list), [2] the h list.  Synchronises the ctx.
int zkg16_last_term_counts(zkg16_ctx *ctx, uint64_t counts[3]) {
    if (!counts || !ctx) return ZKG16_ERR_BAD_ARG;
    int last;
    { std::lock_guard<std::mutex> lk(ctx->lane_mu); last = ctx->last_lane; }
    zkg16_ctx *root = ctx;
    ctx = lane_of(root, last);
    ZK_API_BEGIN(ctx)
    if (ctx->batch_terms_set) {           // a batch: the lists of all its sub-batches
        for (int i = 0; i < 3; i++) counts[i] = ctx->batch_terms[i];
        return ZKG16_OK;
    }
    ZK_HIP(hipDeviceSynchronize());
    MsmWorkspace *w[3] = {&ctx->ws_z, &ctx->ws_zb, &ctx->ws_h};
    for (int i = 0; i < 3; i++) {
        uint32_t v = 0;
        if (w[i]->last_tb && w[i]->offsets.p)
            ZK_HIP(hipMemcpy(&v, w[i]->offsets.as<uint32_t>() + w[i]->last_tb, sizeof v, hipMemcpyDeviceToHost));
        counts[i] = v;
    }
    ZK_API_END(ctx)
}

// G1 accumulation waves per SIMD of the last proof's three term lists (z, B, h; 0 = list not built): the occupancy the
// bucket accumulations actually ran at, which is the row of the bare-loop microbenchmark bench.py must compare them with.
int zkg16_last_acc_waves(zkg16_ctx *ctx, int waves[3]) {
    if (!ctx || !waves) return ZKG16_ERR_BAD_ARG;
    int last;
    { std::lock_guard<std::mutex> lk(ctx->lane_mu); last = ctx->last_lane; }
    zkg16_ctx *l = lane_of(ctx, last);
    std::lock_guard<std::mutex> lk(l->mu);
    MsmWorkspace *w[3] = {&l->ws_z, &l->ws_zb, &l->ws_h};
    for (int i = 0; i < 3; i++) waves[i] = w[i]->last_tb ? (int)(w[i]->last_lanes_g1 / ((uint32_t)l->num_cus * 4u * 64u)) : 0;
    return ZKG16_OK;
}

// What the last zkg16_msm_g1 / zkg16_msm_g2 / zkg16_bench_msm / zkg16_diag_msm_tabled on this ctx ran as (it used ws_h and slots[0] of the root; a later proof
// on lane 0 takes them over and clears last_msm_group): out = { c, nwin, entries, seg_len, fixup_items, fixup_chains, bit_sliced, two_level_k }.  The four device words are
// copied here, after the call has returned; the MSM itself records nothing for this.  All zero before the first such call and after such a proof.
int zkg16_last_msm_state(zkg16_ctx *ctx, uint32_t out[8]) {
    if (!ctx || !out) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const MsmSlot &s = ctx->slots[0];
    const MsmWorkspace &w = ctx->ws_h;
    if (ctx->last_msm_group) {
        v[0] = (uint32_t)s.c;
        v[1] = (uint32_t)s.nwin;
        if (w.last_tb && w.offsets.p && w.seg_params.p && s.long_list.p) {
            uint32_t q[2] = {0, 0};
            ZK_HIP(hipMemcpy(&v[2], w.offsets.as<uint32_t>() + w.last_tb, sizeof(uint32_t), hipMemcpyDeviceToHost));
            ZK_HIP(hipMemcpy(&v[3], w.seg_params.as<uint32_t>() + (ctx->last_msm_group == 2 ? 1 : 0), sizeof(uint32_t), hipMemcpyDeviceToHost));
            ZK_HIP(hipMemcpy(q, s.long_list.p, sizeof q, hipMemcpyDeviceToHost));
            v[4] = q[0];
            v[5] = q[1];
            v[6] = (uint32_t)s.bit_sliced;
            v[7] = (uint32_t)s.two_level_k;
        }
    }
    for (int i = 0; i < 8; i++) out[i] = v[i];
    ZK_API_END(ctx)
}

// waves of the accumulation kernels (as launched with the ctx's current options) that fit one SIMD at once: [0] G1, [1] G2
int zkg16_acc_resident_waves(zkg16_ctx *ctx, int waves[2]) {
    if (!waves) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    waves[0] = msm_acc_resident_waves(ctx, false);
    waves[1] = msm_acc_resident_waves(ctx, true);
    ZK_API_END(ctx)
}

// Which SpMV path an r1cs handle is on (poly.hip builds both structures the second time the witness map runs on the handle):
// out = dict_state (0 not tried, 1 dictionary in use, 2 plain kernel for good), ndict, perm_ok, spmv_uses.  Launches nothing.
int zkg16_r1cs_spmv_state(zkg16_ctx *ctx, uint64_t r1cs_handle, uint32_t out[4]) {
    if (!ctx || !out) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto rc_ref = ctx->r1cs.get(r1cs_handle); R1csDev *rc = rc_ref.get();
    if (!rc) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lazy(rc->lazy_mu);
    out[0] = (uint32_t)rc->dict_state;
    out[1] = rc->ndict;
    out[2] = rc->perm_ok ? 1u : 0u;
    out[3] = (uint32_t)rc->spmv_uses;
    return ZKG16_OK;
}

// the lanes (host intervals, steady-clock ms) of the most recent proofs on this ctx: rows of (lane, start, end); returns the
// number of rows written.  Two proofs whose intervals intersect on different lanes ran at the same time.
int zkg16_lane_log(zkg16_ctx *ctx, double *rows, int cap_rows) {
    if (!ctx || !rows || cap_rows < 0) return 0;
    std::lock_guard<std::mutex> lk(ctx->lane_mu);
    const int n = (int)ctx->lane_log.size() < cap_rows ? (int)ctx->lane_log.size() : cap_rows;
    for (int i = 0; i < n; i++) {
        const auto &e = ctx->lane_log[ctx->lane_log.size() - n + i];
        rows[3 * i] = e.lane; rows[3 * i + 1] = e.t0_ms; rows[3 * i + 2] = e.t1_ms;
    }
    return n;
}

}  // extern "C"
namespace {
std::vector<zkg16_ctx *> all_lanes(zkg16_ctx *root) {
    std::vector<zkg16_ctx *> v{root};
    std::lock_guard<std::mutex> lk(root->lane_mu);
    for (auto &l : root->lanes)
        if (l) v.push_back(l.get());
    return v;
}
}  // namespace
extern "C" {

int zkg16_kernel_timing(zkg16_ctx *ctx, int enable) {
    if (!ctx) return ZKG16_ERR_BAD_ARG;
    for (zkg16_ctx *l : all_lanes(ctx)) {
        std::lock_guard<std::mutex> lk(l->mu);
        l->opt.kernel_timing = enable != 0;
        l->opt.kernel_timing_accumulate_only = enable == 2;
    }
    return ZKG16_OK;
}

// summed over the lanes of the ctx
int zkg16_kernel_stats(zkg16_ctx *ctx, const char *kernel_name, uint64_t *launches, double *total_ms, double *units) {
    if (!ctx || !kernel_name) return ZKG16_ERR_BAD_ARG;
    uint64_t n = 0;
    double ms = 0, u = 0;
    for (zkg16_ctx *l : all_lanes(ctx)) {
        std::lock_guard<std::mutex> lk(l->mu);
        (void)hipSetDevice(l->device);
        kernel_timer_resolve(l);
        auto it = l->kstats.find(kernel_name);
        if (it == l->kstats.end()) continue;
        n += it->second.launches;
        ms += it->second.ms;
        u += it->second.units;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    if (units) *units = u;
    return ZKG16_OK;
}

void zkg16_kernel_stats_reset(zkg16_ctx *ctx) {
    if (!ctx) return;
    for (zkg16_ctx *l : all_lanes(ctx)) {
        std::lock_guard<std::mutex> lk(l->mu);
        (void)hipSetDevice(l->device);
        kernel_timer_resolve(l);
        l->kstats.clear();
    }
}

}  // extern "C"
