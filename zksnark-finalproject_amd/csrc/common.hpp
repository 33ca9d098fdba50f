// Shared host-side plumbing for libzkg16: context, device buffers, error handling, kernel timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/zkg16.h"
#include "ec.cuh"
#include "ff.cuh"

namespace zk {

struct HipError {
    hipError_t err;
    const char *what;
    const char *file;
    int line;
};

#define ZK_HIP(expr)                                                 \
    do {                                                             \
        hipError_t _e = (expr);                                      \
        if (_e != hipSuccess) throw zk::HipError{_e, #expr, __FILE__, __LINE__}; \
    } while (0)

// Device allocations go through a small process-wide cache: the reference's request flow builds and drops a proving key
// (GBs) per request, and hipMalloc / hipFree of buffers that size cost up to seconds on a busy allocator (n = 128: setup
// measured between 0.47 s and 8 s for identical requests before the cache).  dev_release() synchronises the device first,
// exactly as hipFree does, so a cached block is never handed out while a kernel may still touch it.
void *dev_acquire(size_t bytes, size_t *got);      // api.hip; throws HipError
void dev_release(void *p, size_t bytes) noexcept;
void dev_cache_flush() noexcept;
uint64_t dev_cached_bytes();                       // parked in the cache for the current device: free to the next large request

// Helper threads of one host-side job.  A std::thread that goes out of scope while joinable calls std::terminate, and the
// constructor itself can throw (EAGAIN): behind a C ABI neither may take the process down.  run() starts fn on a new thread,
// or — when none can be started — runs it right here; the destructor joins whatever was started, on every exit path.
class ThreadGroup {
    std::vector<std::thread> th_;
  public:
    ThreadGroup() = default;
    ThreadGroup(const ThreadGroup &) = delete;
    ThreadGroup &operator=(const ThreadGroup &) = delete;
    template <class Fn>
    void run(Fn fn) {
        try {
            th_.emplace_back(fn);
        } catch (const std::system_error &) {
            fn();
        }
    }
    void join() {
        for (auto &t : th_)
            if (t.joinable()) t.join();
        th_.clear();
    }
    ~ThreadGroup() { join(); }
};

// RAII device buffer.  Throws HipError on failure (mapped to a status at the ABI edge).
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    explicit DevBuf(size_t n) { alloc(n); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        p = dev_acquire(n, &bytes);
    }
    void ensure(size_t n) { if (n > bytes) alloc(n); }
    void release() { if (p) { dev_release(p, bytes); p = nullptr; bytes = 0; } }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// fixed-base scalar multiplication (setup): window table of the last generator used + scratch, kept across calls
struct FixedBaseCache {
    // window tables of the two most recently used generators (a request uses the standard generator to derive its own
    // random one, then that one for the whole key) + scratch shared by both
    struct Entry { std::vector<uint8_t> key; DevBuf table; uint64_t stamp = 0; int wbits = 0; } e[2];
    uint64_t clock = 0;
    DevBuf sums, pref, win_bases, table_xyzz;
};

// Per-kernel HIP-event timing on the ctx stream (bench.py's roofline leg reads these).
struct KernelStat { uint64_t launches = 0; double ms = 0, units = 0; };
struct PendingEvent;

struct NttTables {          // per domain size, built on device on first use
    int log_n = 0;
    std::mutex mu;          // the tables below that are built on first use (g_u / gi_u, wu): lanes of one ctx share this object
    DevBuf w;               // w[j]  = omega_N^j,            j < N
    DevBuf wu;              // the same in the unsaturated form (36 B per entry); only built for N > 2^22
    DevBuf g;               // g[i]  = 7^i                   (coset fft pre-multiply)
    DevBuf gi;              // gi[i] = 7^-i * N^-1           (coset ifft post-multiply)
    // the same two tables for the unsaturated kernels with the form conversion folded in (built on first use): a load there
    // skips the conversion product, which leaves a factor 2^-5 per pass behind; g_u = 2^10 g (its product is a full
    // conversion), gi_u = 2^(5 * passes) gi puts the missing factors back at the last store
    DevBuf g_u, gi_u;
    int u_passes = 0;
    Fr n_inv;               // N^-1 (plain ifft post-multiply)
    Fr zinv;                // (7^N - 1)^-1 : 1 / Z on the coset (witness map)
};

struct PkDev {              // proving key shard resident in HBM (affine AoS; (0,0) = infinity)
    size_t num_instance = 0, m_total = 0;            // m_total = num_instance + num_witness (full key)
    size_t z_lo = 0, z_hi = 0;                       // index range of the a/b1/b2 (and padded l) queries kept here
    size_t h_lo = 0, h_hi = 0, n_h_total = 0;        // index range of h_query kept here
    DevBuf a, b1, l;                                 // G1AffineU[z_hi - z_lo + 3]  (three trailing slots: r, s, -rs terms)
    DevBuf b2;                                       // G2AffineU[z_hi - z_lo + 3]
    DevBuf h;                                        // G1AffineU[h_hi - h_lo]
    DevBuf b_mask;                                   // u8[z_hi - z_lo + 3]: 1 where the term's base is infinity in both B queries
    size_t b_skipped = 0;                            // number of such terms (B-side plan is separate when this is worth a sort)
    G1Affine alpha_g1, beta_g1, delta_g1;            // host copies for the tail
    G2Affine beta_g2, delta_g2;
    bool blinding = true;                            // this shard's MSMs carry the r*delta, s*delta, -rs*delta terms
    bool full = true;                                // whole key (all ranges + blinding terms): zkg16_prove / _resident
    // window tables (zkg16_pk_precompute): a / b1 / l / b2 hold [254 / tab_c_z + 1][z_hi - z_lo + 3] points, h [254 / tab_c_h + 1][n_h];
    // level 0 is the query itself.  0 = no table.
    int tab_c_z = 0, tab_c_h = 0;
    // entry stride of those tables (zkg16_table_layout; option "table_stride" when they were built): false = packed, 112 / 224 bytes, so
    // level 0 reads as the plain query; true = 128 / 256 bytes in every level (PadAffine in msm.hip).  Per table kind: the three G1
    // z-side tables, the G2 one, the h-side one.  Always false without a table.
    bool pad_z_g1 = false, pad_z_g2 = false, pad_h = false;
};

struct R1csDev {
    size_t num_instance = 0, num_constraints = 0, num_variables = 0;
    int log_n = 0;
    DevBuf rp[3], col[3], cf[3];
    size_t nnz[3] = {0, 0, 0};
    // coefficient dictionary (poly.hip): R1CS coefficients are a few hundred distinct field elements (215 in the 128x128
    // MatrixCircuit's 86.6 M non-zeros), so the SpMV reads a 16-bit index per non-zero instead of 32 bytes.  Built on the
    // device the second time the witness map runs on this handle (a handle used once never pays for it); dict_state: 0 = not tried, 1 = in use, 2 = too many distinct values
    DevBuf ci[3], dict;
    uint32_t ndict = 0;
    int dict_state = 0;
    int spmv_uses = 0;              // witness maps run on this handle so far (the structures are built on the second)
    // rows ordered by length, longest first (poly.hip): lane t of the SpMV takes row perm[t], so the 64 rows of a wave have about
    // the same number of non-zeros.  Built with the dictionary; null = natural order
    DevBuf perm[3];
    bool perm_ok = false;
    std::mutex lazy_mu;             // the dictionary / row order are built once, by whichever lane gets there first
    // a rank's rows of a split witness map (group.hip): the rows i with i mod m in [lo, hi), in the order above when it existed
    // (from_perm), else natural; one per share this handle has served (under lazy_mu)
    struct RowShare { uint64_t m = 0, lo = 0, hi = 0; bool from_perm = false; DevBuf list[3]; size_t n[3] = {0, 0, 0}; };
    std::vector<std::shared_ptr<RowShare>> row_shares;
    // the PrimeCircuit's template (zkg16_r1cs_prime_template): the four column-0 coefficients that differ between candidates are
    // zero, and a request's n / -j go into A z (rows patch_rows[0..2]) and C z (row patch_rows[3]) after the SpMV (WmPatch)
    bool prime_template = false;
    uint32_t patch_rows[4] = {0, 0, 0, 0};
};

// backing: set when z is a view into an allocation several assignments share (zkg16_witness_matrix_batch: one per batch); the view is
// detached, not released, and the allocation goes back when the last assignment holding it is gone.
struct WitnessDev {
    size_t n = 0;
    DevBuf z;
    std::shared_ptr<DevBuf> backing;
    WitnessDev() = default;
    WitnessDev(const WitnessDev &) = delete;
    WitnessDev &operator=(const WitnessDev &) = delete;
    ~WitnessDev() {
        if (backing) { z.p = nullptr; z.bytes = 0; }
    }
};
struct PrimeDev;            // prime_device.hip: the recorded PrimeCircuit resident on a ctx

// handle -> resident object.  Objects are shared_ptr: a proof in flight on one lane keeps its key / matrices / assignment alive
// when another caller frees the handle meanwhile (the memory goes back when that proof ends).
template <class T>
class HandleMap {
    std::mutex mu_;
    std::map<uint64_t, std::shared_ptr<T>> m_;
  public:
    std::shared_ptr<T> get(uint64_t h) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = m_.find(h);
        return it == m_.end() ? nullptr : it->second;
    }
    void put(uint64_t h, std::shared_ptr<T> v) {
        std::lock_guard<std::mutex> lk(mu_);
        m_[h] = std::move(v);
    }
    void erase(uint64_t h) {
        std::shared_ptr<T> dying;           // destroyed outside the lock (a DevBuf release synchronises the device)
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = m_.find(h);
            if (it == m_.end()) return;
            dying = std::move(it->second);
            m_.erase(it);
        }
    }
    void clear() {
        std::map<uint64_t, std::shared_ptr<T>> dying;
        {
            std::lock_guard<std::mutex> lk(mu_);
            dying.swap(m_);
        }
    }
};

struct MsmSlot {            // one in-flight MSM: written by the accumulate half (main stream), read by the reduce half (aux)
    DevBuf buckets, wsums_dev, seg_head, seg_tail, seg_meta, long_list, long_sums, red_a, red_b, red_c;
    DevBuf bucket_sum;              // an MSM fed in several rounds (streamed assignment): round 0 accumulates here, later rounds into `buckets` and are merged in
    hipStream_t stream = nullptr;   // this MSM's reduction runs here
    void *wsums_host = nullptr;   // pinned
    size_t host_bytes = 0;
    hipEvent_t acc_done = nullptr, red_done = nullptr;
    hipEvent_t acc_start = nullptr, red_start = nullptr;   // with acc_done / red_done: device time of this MSM's two halves (zkg16_last_timings)
    int nwin = 0, c = 0;
    bool active = false;
    bool pending_reduce = false;    // accumulation queued, reduction not yet (msm_*_enqueue_reduce)
    bool last_of_proof = false;     // this MSM's reduction is the tail of the proof (nothing left to overlap it)
    bool fixups_pending = false;    // fix-ups go with the reduction (aux stream) instead of the accumulation (main stream)
    alignas(16) unsigned char acc_args[128] = {0};
    unsigned acc_grid = 0;
    int two_level_k = 0;            // K of the work-efficient reduction when it was used for this MSM (0 = classic)
    float collect_host_ms = 0;      // host part of msm_collect (the Horner over windows / weight bits) of the last MSM on this slot
    int bit_sliced = 0;             // > 0: the bit-sliced reduction ran with this many weight bits (two_level_k = its chunk size)
    void *red_buckets = nullptr;
    size_t red_nb = 0;
    int batch = 1;                  // vectors of a batch plan (zkg16_prove_batch): nwin / batch windows each
};

struct MsmWorkspace {       // grown on demand, reused across proofs
    DevBuf keys, entries, offsets, seg_params, scalars, stage, sort_temp, codes;
    size_t last_tb = 0;         // offsets[last_tb] = length of the term list built last (0: none) — zkg16_last_term_counts
    uint32_t last_lanes_g1 = 0; // lanes of the G1 accumulation grid the last plan on this workspace asked for (zkg16_last_acc_waves)
};

// sizes of zkg16_ctx::timings (22 slots in use, declared with two to spare) and ::vb_timings
constexpr int PROOF_TIMING_SLOTS = 24, VERIFY_TIMING_SLOTS = 15, RERANDOMIZE_TIMING_SLOTS = 8, PK_CHECK_TIMING_SLOTS = 8, PK_BYTES_TIMING_SLOTS = 9;

}  // namespace zk

// zkg16_verify_batch answers batches shorter than this on the host: the smallest measured K at which the device form beat the host
// form on eight threads (profiles/verify_batch_timing_r8.txt)
#define ZKG16_VERIFY_BATCH_MIN_DEFAULT 1024
// the smallest measured K at which zkg16_verify_batch_wire beat both host-decoding routes in every round: 0.094 ms per proof against
// 0.239 (host decode + host form on 8 threads) and 0.245 (host decode + kernels); at K = 64 it lost, 0.361 against 0.270
// (profiles/verify_wire_timing_r9.txt)
#define ZKG16_VERIFY_WIRE_MIN_DEFAULT 256
// the range tests bisecting may make before the proofs still undecided go to the per-proof pass: ceil(T_each / t_range) at
// K = 1024 = ceil(47.72 ms / 2.156 ms) = 23, rounded UP to a power of two — one bad proof needs up to 2 log2 K range tests
// (19 to 22 measured at K = 16,384), and 16 would send that case to the pass (profiles/verify_each_timing_r10.txt)
#define ZKG16_VERIFY_EACH_AFTER_DEFAULT 32
// calls with at least this many sponge chains (3K for assignments, k for hashes) walk them on the device.  INT64_MAX = never: in
// profiles/sponge_chains_timing.txt the device wins zkg16_witness_matrix_batch from 3072 chains and zkg16_matrix_hash_batch from 1024 at
// every measured n, but zkg16_prove_matrix_batch (chain count = a sub-batch's) only at n = 8 — no count wins on every entry
#define ZKG16_SPONGE_CHAINS_MIN_DEFAULT INT64_MAX
// zkg16_rerandomize_batch[_wire] answer batches shorter than this through the host form: the smallest measured K at which both device
// forms beat zkg16_rerandomize_batch_host on eight threads in all three rounds, 0.092 (limbs) and 0.109 (wire) against 0.163 ms per
// proof; at K = 64 they lost, 0.367 and 0.432 against 0.168 — a device call costs 24 to 28 ms whatever K is
// (profiles/rerandomize_timing.txt)
#define ZKG16_RERANDOMIZE_MIN_DEFAULT 256
// zkg16_prove_matrix: fewest permutations a slice of the streamed assignment may hold (witness.hip: matrix_stream_slices)
#define MATRIX_SLICE_MIN_DEFAULT 512

struct zkg16_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string last_error;
    std::map<int, std::unique_ptr<zk::NttTables>> ntt_tables;     // root only (guarded by ntt_mu): lanes share the tables
    std::mutex ntt_mu;
    zk::HandleMap<zk::PkDev> pks;                                 // root only
    zk::HandleMap<zk::R1csDev> r1cs;
    zk::HandleMap<zk::WitnessDev> wits;
    std::atomic<uint64_t> next_handle{1};
    // ---- lanes: a ctx proves up to `opt_lanes` proofs at a time (actix workers call prove concurrently: src/main.rs:37-43).  A
    // lane is a zkg16_ctx of its own — streams, MSM workspaces and slots, witness-map vectors, pinned buffers — whose `root` is
    // the ctx the caller holds; keys, matrices, assignments and NTT tables live in the root and are shared (HBM grows by a
    // lane's workspaces, not by a second copy of the key and its window tables).  Lane 0 is the root itself; further lanes are
    // created when a second caller arrives while the first is still proving.
    zkg16_ctx *root = nullptr;
    std::unique_ptr<zkg16_ctx> lanes[7];                          // root: lanes 1 .. 7, created on first use (fixed slots: readers never see a resize)
    std::mutex lane_mu;
    std::condition_variable lane_cv;
    bool lane_busy[8] = {false, false, false, false, false, false, false, false};
    int opt_lanes = 2;
    int last_lane = 0;                                            // lane of the proof that finished last (zkg16_last_timings)
    std::shared_mutex key_rw;                                     // proofs: shared; in-place changes of a resident key (zkg16_pk_precompute): exclusive
    struct LaneLogEntry { int lane; double t0_ms, t1_ms; };
    std::vector<LaneLogEntry> lane_log;                           // root (under lane_mu): the last proofs' lanes and host intervals
    zk::MsmWorkspace ws_z, ws_h, ws_zb;               // one workspace per scalar vector (z, h, and z masked by the B-query density)
    hipStream_t wm_stream = nullptr;                  // witness map + h-side sort of a proof, concurrent with the z-side MSMs
    zk::MsmSlot slots[5];                             // B2, H, L, A, B1 of one proof
    int last_msm_group = 0;                           // the last zkg16_msm_g1 / _g2 / zkg16_bench_msm on this ctx: 1 = G1, 2 = G2 (ws_h and slots[0]: zkg16_last_msm_state)
    void *extra_host = nullptr;                       // pinned staging for the r, s, -rs scalars
    void *stage_host[2] = {nullptr, nullptr};         // pinned staging ring of upload_h2d (api_keys.hip)
    hipEvent_t stage_done[2] = {nullptr, nullptr};
    zk::DevBuf poly[4];                               // a, b, c, tmp vectors of the witness map
    // zkg16_prove_batch: pinned staging of the 3K extra scalars and the K assignment pointers (the K h vectors live in poly)
    void *batch_host = nullptr;
    size_t batch_host_bytes = 0;
    bool batch_terms_set = false;                     // the last proving call was a batch: its term counts (summed over sub-batches)
    uint64_t batch_terms[3] = {0, 0, 0};
    // zkg16_witness_matrix_batch: pinned staging of a batch's a | b, entering states, instances and z pointers, and its device copy
    void *mbatch_host = nullptr;
    size_t mbatch_host_bytes = 0;
    zk::DevBuf mbatch_dev;
    // option "check_satisfied": the device words of the pass in flight (n_bad[K] | first_bad[K]) and the verdicts of the last proving
    // call on this lane (zkg16_last_check); neither exists while the option is off
    zk::DevBuf check_dev;
    std::vector<uint64_t> check_n_bad, check_first_bad;
    float timings[zk::PROOF_TIMING_SLOTS] = {0};      // zkg16_last_timings; the slots are named in api_internal.hpp (ProofTiming)
    // ---- zkg16_set_option / zkg16_kernel_timing: everything a lane copies from its root in one assignment (api.hip: copy_options).
    // opt_lanes is not here: it lives on the root alone, under lane_mu.
    struct Options {
        bool kernel_timing = false;
        bool kernel_timing_accumulate_only = false;       // zkg16_kernel_timing(ctx, 2): only the bucket-accumulation launches
        int window_bits = 0;
        int min_seg = 0;                              // shortest per-lane run of sorted entries in an accumulation (0 = default)
        int ntt_mode = 1;                             // 1: unsaturated (29-bit limb) butterflies, 0: saturated
        int reduce_mode = 3;                          // 0 classic (log-depth scan over all chunks), 1 work-efficient two-level, 2 = 1 except the proof's last MSM, 3 (default) = 2 from 16-bit windows on and bit-sliced for single bucket sets <= 2^19, 5 = bit-sliced wherever it applies
        int b_filter = 0;                             // B-side term list filtered out of the full one: 0 = with window tables (default), 1 = always, 2 = never (second sort)
        int spmv_dict = 0;                            // 0/1: coefficient dictionary in the SpMV (default); 2: plain kernel
        int wm_first = -1;                            // see zkg16_set_option "wm_first"
        int g1_waves = 0;                             // G1 accumulation waves per SIMD in the one resident round (0 = 2)
        int fixup_aux = 0;                            // 1: fix-up kernels on the MSM's reduction stream
        int window_bits_h = 0;                        // the H MSM's own plan (it is the last one: its reduction is not hidden)
        int reduce_chunk = 0;
        int wm_concurrent = -1;
        int ntt_radix = 1;                            // 1 (default): the last seven butterfly stages by lane exchanges (ds_bpermute / DPP), 2: every stage through the LDS, 4: two stages per LDS trip
        int ntt_xcd = 1;                              // NTT tiles in XCD-aware order (ntt.hip: xcd_tile)
        int table_stride = 0;                         // window tables built from now on: 0 = by table size (padded from ZKG16_TABLE_STRIDE_PAD_MIN_BYTES on), 1 = packed entries, 2 = padded to whole cache lines (zkg16_table_layout)
        int acc_debug = 0;                            // timing probes (wrong results): see AccArgs::debug
        int sort_mode = 0;                            // 0: hand-written bucket scatter (bucket_sort.hip), 1: rocPRIM radix sort
        int acc_pipeline = 0;                         // bit 0 / 1: G1 / G2 accumulation gathers the next base behind the last (inlined) product (default: neither)
        int collect_threads = -1;                     // -1: the z-side MSMs' window sums are combined on their own host threads when the key is plain; 1 always; 0 never
        int fixed_base_bits = 0;                      // setup's fixed-base window width (0 = by batch size; even widths >= 16 are built in two levels)
        int g2_lazy = 1;                              // G2 accumulation: Fq2 products with one reduction per component, operands parked in LDS (ffu.cuh: fq2u_mul_lazy)
        int acc_lazy = 1;                             // default G1 / G2 accumulation loops: the mixed addition without the carry passes its results do not need (ec.cuh: xyzz_madd_inline_lc, xyzz_madd_lazy_lc); 0: xyzz_madd_inline / xyzz_madd_lazy
        int g2_split = 1;                             // G2 accumulation with every Fq2 value split over a lane pair, two waves per SIMD (g2split.cuh; msm.hip: msm_accumulate_split_kernel); acc_lazy selects its addition; acc_pipeline bit 1 and g2_lazy = 2 keep their one-lane loops; 0: the one-lane loop
        int g2_split_form = 0;                        // the split loop's products: 0 / 2 = inlined (default), 1 = device-function calls (msm.hip: g2_split_form)
        int g1_inline = 1;                            // G1 accumulation (plain loop): every field product inlined (ec.cuh: xyzz_madd_inline); 0: products as calls
        int matrix_parts = 0;                         // zkg16_prove_matrix: gadget slices the assignment arrives in (0 = five growing slices, k = k equal ones, 1 = no overlap)
        int matrix_slice_min = MATRIX_SLICE_MIN_DEFAULT;      // zkg16_prove_matrix: the slice count is lowered until a slice holds this many permutations (tests set 1)
        int fuse_pointwise = 1;                       // the point-wise product on the load of the last transform (0: its own pass)
        int wm_transforms = 6;                        // witness map: 6 (default) = C only inverse-transformed, subtracted on the last store; 7 = arkworks' sequence
        int batch_max = 0;                            // zkg16_prove_batch / zkg16_prove_matrix_batch: proofs per device pass (0 = as many as fit)
        int matrix_batch_threads = 0;                 // zkg16_witness_matrix_batch / zkg16_prove_matrix_batch: host threads of the sponge chains (0 = 8)
        int matrix_batch_grid = 0;                    // cap on either grid dimension of the batched witness kernels (0 = 65535): beyond it they loop
        int linear_solver = 0;                        // the linear route's solver: 0 = the reference's forward substitution on the lower triangle, 1 = Gaussian elimination (linear_elim_dev.cuh)
        int linear_elim_lds_max = 0;                  // wit_linear_elim_kernel: the largest n whose working matrix lies in LDS (0 = 64); above it a global workspace
        int64_t sponge_chains_min = ZKG16_SPONGE_CHAINS_MIN_DEFAULT;             // calls with at least this many sponge chains walk them on the device; above 2^32: never
        int sponge_chain_segment = 0;                 // permutations of a chain per launch of wit_chain_batch_kernel (0 = 256)
        int verify_batch_min = ZKG16_VERIFY_BATCH_MIN_DEFAULT;                   // zkg16_verify_batch: shorter batches are answered by the host form (the measured crossover)
        int verify_wire_min = ZKG16_VERIFY_WIRE_MIN_DEFAULT;                     // zkg16_verify_batch_wire: shorter batches are decoded and answered on the host (the measured crossover)
        int check_satisfied = 0;                      // 1: the proving calls check their assignments after the SpMV (r1cs_check_kernel) and refuse unsatisfied ones
        int verify_each_after = ZKG16_VERIFY_EACH_AFTER_DEFAULT;                 // zkg16_verify_batch[_wire] with ok_each: range tests before the per-proof pass takes over
        int rerandomize_min = ZKG16_RERANDOMIZE_MIN_DEFAULT;                     // zkg16_rerandomize_batch[_wire]: shorter batches are answered by the host form
        int rerandomize_pass = 0;                     // zkg16_rerandomize_batch[_wire]: proofs per launch (0 = 65,536; tests lower it to reach several passes at small k)
        int trapdoor_pass = 0;                        // zkg16_prove_trapdoor_batch: requests per device pass (0 = 65,535; tests lower it to reach several passes at small k)
        int pk_validate = 0;                          // 1: zkg16_pk_load / zkg16_pk_load_range check every point of the key on the device (zkg16_pk_check) before the handle exists and refuse a bad key
        int pk_bytes_piece = 0;                       // zkg16_pk_load_bytes / zkg16_pk_save / zkg16_pk_read: points per piece of a query (0 = 524,288: two pieces of G2 bytes in flight are 96 MiB of HBM beside the key; tests lower it to reach several pieces at small keys)
        int verify_each_after_set = 0;                // 1: the caller set "verify_each_after" (the u64 entries read an unset option as 1; the stored value cannot tell unset from 32)
    } opt;
    std::map<std::string, zk::KernelStat> kstats;
    std::vector<zk::PendingEvent> pending_events;
    void *circuit_stage = nullptr;                    // pinned staging block of zkg16_circuit_load (root ctx; grown on demand)
    size_t circuit_stage_bytes = 0;
    float vb_timings[zk::VERIFY_TIMING_SLOTS] = {0};                    // zkg16_verify_batch_timings (root: the last batch verified on any lane)
    float pkc_timings[zk::PK_CHECK_TIMING_SLOTS] = {0};                 // zkg16_pk_check_timings (under mu: the last zkg16_pk_check / zkg16_points_check_bulk / validated load)
    float pkb_timings[zk::PK_BYTES_TIMING_SLOTS] = {0};                 // zkg16_pk_bytes_timings (under mu: the last zkg16_pk_load_bytes / zkg16_pk_save / zkg16_pk_read)
    float rr_timings[zk::RERANDOMIZE_TIMING_SLOTS] = {0};               // zkg16_rerandomize_timings (root: the last batch re-randomised on any lane)
    int num_cus = 256;
    bool lds_attr_fixup[2] = {false, false}, lds_attr_ntt = false, lds_attr_linear_elim = false;      // hipFuncSetAttribute(max dynamic LDS) done on this device
    zk::FixedBaseCache fb_g1, fb_g2;
    zk::DevBuf poseidon_dev;                          // Poseidon MDS + round constants, Montgomery form (witness.hip), uploaded on first use
    std::shared_ptr<zk::PrimeDev> prime_dev;          // PrimeCircuit template + witness program (prime_device.hip), root only, uploaded on first use
};

namespace zk {

// Brackets one kernel launch with a HIP-event pair on the ctx stream when ctx->opt.kernel_timing is on.
// Recording is asynchronous (no host sync inside the timed region); pairs are resolved when stats are read.
struct PendingEvent { std::string name; double units; hipEvent_t e0, e1; };

struct ScopedKernelTimer {
    zkg16_ctx *ctx;
    const char *name;
    double units;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t stream;
    ScopedKernelTimer(zkg16_ctx *c, const char *n, double u, hipStream_t st = nullptr);
    ~ScopedKernelTimer();
};
void kernel_timer_resolve(zkg16_ctx *ctx);

// ---- entry points implemented per translation unit
// Out of place: returns `dst`, which holds the transform of `src`; `src` is scratch afterwards.  pw: optional fused
// point-wise stage on the input, src[i] <- (src[i] * b[i] - c[i]) * zinv (the witness map's (ab - c)/Z); with c null,
// src[i] <- src[i] * b[i], b being the output of a transform whose last store carried NttLast::pw_operand.
struct NttPointwise { const Fr *b, *c; Fr zinv; };
// optional extras on the store of a transform's last pass (the six-transform witness map, poly.hip):
//   scale       the results are multiplied by *scale as well (not with a coset ifft: its store multiplies by a table);
//   pw_operand  ... and by the factor the one-product fused load (pw with c null) expects of its operand b (U-form: 2^5);
//   sub         dst[k] <- result - dst[k]: dst holds the subtrahend, read by the thread that then overwrites it.
struct NttLast { const Fr *scale; bool pw_operand, sub; };
Fr *ntt_run(zkg16_ctx *ctx, Fr *src, Fr *dst, int log_n, bool inverse, bool coset, const NttPointwise *pw = nullptr,
            const NttLast *last = nullptr);
// nvec transforms at once: vector v at src / dst (and pw->b / pw->c) + v * vec_stride, every pass one launch over all of them
Fr *ntt_run_batch(zkg16_ctx *ctx, Fr *src, Fr *dst, int log_n, bool inverse, bool coset, const NttPointwise *pw, unsigned nvec, size_t vec_stride,
                  const NttLast *last = nullptr);
NttTables *ntt_get_tables(zkg16_ctx *ctx, int log_n);
// a rank's share of a two-pass transform (split witness map): tiles {lo0, n0, lo1, n1} of the column and of the row pass, and
// what runs between the two passes (the exchange); see ntt_run_share in ntt.hip
struct NttShare {
    unsigned cols[4], rows[4];
    std::function<void()> between;
};
Fr *ntt_run_share(zkg16_ctx *ctx, Fr *src, Fr *dst, int log_n, bool inverse, bool coset, const NttPointwise *pw, const NttShare &share,
                  const NttLast *last = nullptr);
bool ntt_two_pass_shape(int log_n, int ntt_mode, int *log_n1, int *log_n2, int *tile_log);

// rows: null = every row of the domain; else lane t of matrix i computes row list[i][t], t < n[i] (a rank's share, group.hip)
struct SpmvRows { const uint32_t *list[3]; size_t n[3]; };
void spmv_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, Fr *a, Fr *b, Fr *c, const SpmvRows *rows = nullptr, const Fr *const *zs = nullptr,
              unsigned nvec = 1);
void pointwise_h_run(zkg16_ctx *ctx, Fr *ab_a, const Fr *b, const Fr *c /* null: ab only */, const Fr &zinv, size_t n);
void fr_from_mont_run(zkg16_ctx *ctx, const Fr *in, Fr *out, size_t n);
// patch (proofs on the PrimeCircuit's template): between the SpMV and the transforms vector v gets add[2 v] added to a[rows[0..2]] and
// add[2 v + 1] to c[rows[3]] (wm_patch_kernel); add is a device-visible table of nvec x 2 Montgomery values
struct WmPatch { uint32_t rows[4]; const Fr *add; };
// check (nullable; option "check_satisfied"): device words n_bad[nvec] | first_bad[nvec] that r1cs_check_run fills from a, b, c right
// after the SpMV and the patch, on the same stream, before the first transform
void witness_map_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, Fr **h_out, const WmPatch *patch = nullptr, uint64_t *check = nullptr);
void witness_map_run_batch(zkg16_ctx *ctx, R1csDev &m, const Fr *const *zs, unsigned nvec, Fr **h_out, const WmPatch *patch = nullptr,
                           uint64_t *check = nullptr);
// (A z)_i (B z)_i == (C z)_i for i < nc on nvec vectors of a / b / c, vector v at + v * stride (r1cs_check_dev.cuh): res (device, 2 nvec
// words) <- n_bad[v] at res[v], first_bad[v] at res[nvec + v].  Two launches on ctx->stream, no synchronisation.
void r1cs_check_run(zkg16_ctx *ctx, size_t nc, const Fr *a, const Fr *b, const Fr *c, size_t stride, unsigned nvec, uint64_t *res);
// the SpMV of nvec assignments into ctx->poly[0..2] (grown as needed), the patch, and the check into res: what the stand-alone check
// entries run (zs null with nvec == 1: z)
void r1cs_check_spmv_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, const Fr *const *zs, unsigned nvec, const WmPatch *patch, uint64_t *res);

// Scalar-vector side of Pippenger (shared by every MSM over the same scalars).
struct MsmPlan {
    size_t n = 0;            // scalars
    int c = 0, nwin = 0;     // window bits, window count (bucket sets: 1 with window tables)
    int nwin_digits = 0;     // digits per scalar = 254 / c + 1 (= nwin without tables)
    bool tabled = false;     // the bases are a window table [nwin_digits][n] (msm_tables_build): every digit lands in ONE bucket set
    size_t nb = 0;           // buckets per window = 2^(c-1)
    size_t total_entries = 0;            // upper bound n * windows (the exact count lives on the device)
    uint32_t lanes_g1 = 0, lanes_g2 = 0; // lanes of one resident round of accumulation waves (2 waves per SIMD; G2: one wave of 64 one-lane segments or two waves of 32 lane pairs)
    int batch = 1;           // scalar vectors (zkg16_prove_batch): nwin = batch x the windows of one
};
void msm_plan_build(zkg16_ctx *ctx, MsmWorkspace &ws, const Fr *scalars_canonical, size_t n, MsmPlan &plan, int window_bits = 0);
int msm_plan_bits(zkg16_ctx *ctx, size_t n, int window_bits, bool tabled);          // the c msm_plan_build picks
size_t msm_plan_digits(zkg16_ctx *ctx, size_t n, int window_bits, bool tabled);     // and 254 / c + 1
// The scalar vector where it lives: n_main elements at `main` then n_extra at `extra`; `mont` = arkworks' Montgomery form
// (converted inside the digit kernel); mask[i] != 0 zeroes scalar i (B-query density filter).  All device pointers.
// part / want_part (streamed assignments, witness.hip): when part != nullptr only the scalars i with part[i] == want_part take
// part in this plan (the others count as zero: they may not even be computed yet).
// batch > 1: that many vectors, vector v's main part at vecs[v] (a device-visible pointer table) or, without one, at
// main + v * vec_stride, its extras at extra + v * n_extra.
struct ScalarSrc { const Fr *main; size_t n_main; const Fr *extra; size_t n_extra; bool mont; const uint8_t *mask; const uint8_t *part = nullptr; int want_part = 0;
                   const Fr *const *vecs = nullptr; size_t vec_stride = 0; int batch = 1; };
void msm_plan_build(zkg16_ctx *ctx, MsmWorkspace &ws, const ScalarSrc &src, MsmPlan &plan, int window_bits = 0, bool tabled = false);
// window tables of a resident key: bases[n] -> new buffer [254 / c + 1][n], level w = 2^(c w) * base (msm.hip)
// padded: entries at the whole-cache-line stride 128 (G1) / 256 (G2) bytes instead of 112 / 224, level 0 included (zkg16_table_layout)
DevBuf msm_tables_build_g1(zkg16_ctx *ctx, const DevBuf &bases, size_t n, int c, bool padded);
DevBuf msm_tables_build_g2(zkg16_ctx *ctx, const DevBuf &bases, size_t n, int c, bool padded);
// n points of entry_bytes each copied from one entry stride to another (bytes, multiples of 16), queued on ctx->stream
void msm_bases_restride(zkg16_ctx *ctx, const void *src, size_t src_stride, void *dst, size_t dst_stride, size_t entry_bytes, size_t n);
// the term list of `plan_src` without the terms whose scalar index i has mask[i] != 0 (stable compaction; msm.hip)
void msm_plan_filter(zkg16_ctx *ctx, const MsmWorkspace &ws_src, const MsmPlan &plan_src, const uint8_t *mask, MsmWorkspace &ws_dst, MsmPlan &plan_dst);
void msm_sort_keys(zkg16_ctx *ctx, MsmWorkspace &ws, size_t count, unsigned key_bits);   // sort.hip (rocPRIM radix sort; option sort_mode 1)
// bucket_sort.hip: hand-written wave-ballot counting scatter (default); returns the per-window entry counts (device)
// (*sum_windows, nullable: how many values at the returned pointer add up to the list's length — nwin, or 1 for lists of many windows)
const uint32_t *msm_bucket_sort(zkg16_ctx *ctx, MsmWorkspace &ws, const uint32_t *codes, size_t n, int nwin, int c, uint2 *entries,
                                int *sum_windows = nullptr);
void radix_sort_hi32(zkg16_ctx *ctx, const uint64_t *in, uint64_t *out, size_t count, unsigned key_bits, DevBuf &temp, const char *timer_name);
// setup.hip: Groth16 key generation from a known trapdoor (discrete logs on device, then fixed-base batches)
struct SetupOut {
    uint64_t *a_query, *b_g1_query, *b_g2_query, *h_query, *l_query, *gamma_abc_g1;
    uint8_t *a_inf, *b_g1_inf, *b_g2_inf, *l_inf;
    uint64_t *alpha_g1, *beta_g1, *beta_g2, *delta_g1, *delta_g2, *gamma_g2;
};
// the QAP at tau (qap_eval_run): u, v, w [num_variables], lg = (beta u + alpha v + w) / (gamma for the instance columns, delta for the
// others), L = the Lagrange values L_j(tau), j < N, and the host values Z(tau), 1 / delta, 1 / gamma
struct QapEval {
    DevBuf uvw[3], lg, L, scratch[8];
    Fr zt, dinv, ginv;
};
void qap_eval_run(zkg16_ctx *ctx, const R1csDev &m, const Fr trap[5], QapEval &q);      // throws when tau^N = 1
void setup_run(zkg16_ctx *ctx, const R1csDev &m, const Fr trap[5], const G1Affine &g1, const G2Affine &g2, const SetupOut &out, PkDev *resident = nullptr);
void fr_powers_run(zkg16_ctx *ctx, Fr *out, const Fr &base, const Fr &scale, size_t n);
// Bases side: window sums -> host; returns the MSM value (XYZZ) after the host Horner.
// the two halves of an enqueue, for callers that interleave other launches between them (prove_device)
// round: -1 = the whole MSM in one accumulation (default); k >= 0 = round k of an MSM whose terms arrive in several rounds
// (same plan geometry every round): the rounds' bucket arrays are summed and ONE reduction follows (msm_*_enqueue_reduce)
int msm_acc_resident_waves(zkg16_ctx *ctx, bool g2);
// padded: `bases` is a window table built with padded entries (PkDev::pad_*), read at its own compile-time stride
void msm_g1_enqueue_acc(zkg16_ctx *ctx, MsmWorkspace &ws, const MsmPlan &plan, const G1AffineU *bases, MsmSlot &slot, int round = -1, bool padded = false);
void msm_g2_enqueue_acc(zkg16_ctx *ctx, MsmWorkspace &ws, const MsmPlan &plan, const G2AffineU *bases, MsmSlot &slot, int round = -1, bool padded = false);
void msm_g1_enqueue_reduce(zkg16_ctx *ctx, MsmSlot &slot);
void msm_g2_enqueue_reduce(zkg16_ctx *ctx, MsmSlot &slot);
void msm_g1_enqueue(zkg16_ctx *ctx, MsmWorkspace &ws, const MsmPlan &plan, const G1AffineU *bases, MsmSlot &slot, bool padded = false);
void msm_g2_enqueue(zkg16_ctx *ctx, MsmWorkspace &ws, const MsmPlan &plan, const G2AffineU *bases, MsmSlot &slot, bool padded = false);
G1XYZZ msm_g1_collect(zkg16_ctx *ctx, MsmSlot &slot);
G2XYZZ msm_g2_collect(zkg16_ctx *ctx, MsmSlot &slot);
// a batch plan's slot: msm_slot_wait once, then vector v's value (const: threads may combine different vectors at once)
void msm_slot_wait(MsmSlot &slot);
G1XYZZ msm_g1_collect_part(const MsmSlot &slot, int v);
G2XYZZ msm_g2_collect_part(const MsmSlot &slot, int v);
G1XYZZ msm_g1_exec(zkg16_ctx *ctx, MsmWorkspace &ws, const MsmPlan &plan, const G1AffineU *bases, const char *tag);
G2XYZZ msm_g2_exec(zkg16_ctx *ctx, MsmWorkspace &ws, const MsmPlan &plan, const G2AffineU *bases, const char *tag);
// saturated (arkworks) affine points -> the unsaturated device form, on the ctx stream
void convert_g1_bases(zkg16_ctx *ctx, const G1Affine *in, G1AffineU *out, size_t n);
void convert_g2_bases(zkg16_ctx *ctx, const G2Affine *in, G2AffineU *out, size_t n);

// circuits.hip: the MatrixCircuit's R1CS of size n as a plan (matrix_plan.hpp), and its reference instantiation on the host
struct MatrixPlan;
bool matrix_plan_build(size_t n, MatrixPlan &plan);
void matrix_plan_instantiate_host(const MatrixPlan &plan, uint64_t *const rp[3], uint32_t *const col[3], Fr *const cf[3]);

// matrix_r1cs.hip: that R1CS written by kernels into a new R1csDev (status: a zkg16_status when the result is null)
std::shared_ptr<R1csDev> matrix_r1cs_on_device(zkg16_ctx *ctx, size_t n, int *status);

// prime_device.hip: the PrimeCircuit of candidate (x, j) on the device, from the template the root ctx keeps resident (status: a
// zkg16_status when the result is null; ZKG16_ERR_UNSUPPORTED for the candidates zkg16_circuit_prime refuses)
std::shared_ptr<R1csDev> prime_r1cs_on_device(zkg16_ctx *ctx, uint64_t x, uint64_t j, int *status);
std::shared_ptr<WitnessDev> prime_witness_on_device(zkg16_ctx *ctx, uint64_t x, uint64_t j, int *status);
// the template (the j >= 1 form with the four candidate-dependent coefficients zero) as an R1csDev marked prime_template
std::shared_ptr<R1csDev> prime_r1cs_template_on_device(zkg16_ctx *ctx, int *status);
// k assignments in one pass.  prime_batch_inputs (host only): request i's slots | sources at in[i * stride ..) and its n in ns
// (nullable) — or the status of the first refused candidate, nothing written.  prime_witness_batch_assign: on ctx->stream (a
// lane's, or the root's under its mutex) one upload of those inputs and the z addresses out of the ctx's pinned staging, the two
// batched launches, one synchronisation; the assignments share one allocation (WitnessDev::backing).  Throws HipError (the stream
// drained) / std::bad_alloc.
int prime_batch_inputs(const uint64_t *xs, const uint64_t *js, size_t k, std::vector<Fr> &in, uint32_t *ns, size_t *stride);
void prime_witness_batch_assign(zkg16_ctx *ctx, const Fr *in, size_t k, std::vector<std::shared_ptr<WitnessDev>> &out, float *dev_ms);

// witness.hip: the MatrixCircuit's assignment arriving on the device in parts (zkg16_witness_matrix: all at once;
// zkg16_prove_matrix: while the proof is already running).  slices_wanted gadget slices -> parts = slices + 1.
struct MatrixWitnessStream;
// the slice boundaries (permutation indices, bounds[0] = 0 .. bounds[slices] = perms) -> slices; slice_min < 1 = the default
int matrix_stream_slices(size_t perms, int slices_wanted, int slice_min, uint32_t bounds[9]);
MatrixWitnessStream *matrix_stream_start(size_t n, const uint64_t *a, const uint64_t *b, int slices_wanted, int slice_min, bool overlap);   // host chains start here
int matrix_stream_parts(const MatrixWitnessStream *ms);
size_t matrix_stream_total(const MatrixWitnessStream *ms);
const uint8_t *matrix_stream_part_of(const MatrixWitnessStream *ms);       // device, total + n_extra bytes (null with one slice)
void matrix_stream_attach(MatrixWitnessStream *ms, zkg16_ctx *ctx, Fr *z, size_t n_extra);
void matrix_stream_produce(MatrixWitnessStream *ms, zkg16_ctx *ctx, int k);  // blocks for the chains, then queues part k on ctx->stream
double matrix_stream_chain_ms(const MatrixWitnessStream *ms);
void matrix_stream_hashes(const MatrixWitnessStream *ms, uint64_t out[12]);
void matrix_stream_free(MatrixWitnessStream *ms);

// The assignments of a *_batch_assign become witness handles of ctx (under its mutex), all or nothing (witness.hip): wits.size()
// consecutive handles written to handles_out -> ZKG16_OK, or none registered, nothing written -> ZKG16_ERR_OOM.
int witness_batch_register(zkg16_ctx *ctx, std::vector<std::shared_ptr<WitnessDev>> &wits, uint64_t *handles_out);

// K requests of one size in one pass (zkg16_witness_matrix_batch, zkg16_prove_matrix_batch).  matrix_batch_chains: the 3k host chains
// on `threads` threads (0 = 8), no ctx; the 12 k hash limbs go to `hashes`, which must stay valid for matrix_batch_assign.  That
// one queues the uploads and the two batched launches on ctx->stream (under ctx's mutex) and synchronises it: k assignments in one
// shared allocation.  Throws HipError (the stream drained) / std::bad_alloc.
struct MatrixBatchChains {
    size_t n = 0, k = 0, perms = 0;
    std::vector<uint64_t> states;           // k x 3 x perms x 12
    uint64_t *hashes = nullptr;             // k x 12
    double ms = 0;                          // wall
    bool on_device = false;                 // the chains are walked by matrix_batch_assign (wit_chain_batch_kernel), which fills hashes
};
size_t matrix_witness_total(size_t n);
void matrix_batch_chains(MatrixBatchChains &c, size_t n, const uint64_t *a, const uint64_t *b, size_t k, int threads, uint64_t *hashes);
// The chains of a call on the device instead (option "sponge_chains_min" against the call's chain count): matrix_batch_chains_device
// only describes the batch — nothing runs on the host, c.ms = 0 — and matrix_batch_assign walks the chains (sponge_chain_dev.cuh) and
// writes the hashes when it has synchronised.  sponge_hash_batch_device: k hashes of k vectors of `count` Montgomery Fr (form 0) or
// u64 (form 1) on ctx->stream; `out` is written only on success.
bool sponge_chains_on_device(const zkg16_ctx *ctx, size_t chains);
void matrix_batch_chains_device(MatrixBatchChains &c, size_t n, size_t k, uint64_t *hashes);
void sponge_hash_batch_device(zkg16_ctx *ctx, int form, const uint64_t *data, size_t count, size_t k, uint64_t *out);
void matrix_batch_assign(zkg16_ctx *ctx, const MatrixBatchChains &c, const uint64_t *a, const uint64_t *b,
                         std::vector<std::shared_ptr<WitnessDev>> &out, float *dev_ms);

// K Fibonacci requests of one round count in one pass (zkg16_witness_fibonacci_batch, zkg16_prove_fibonacci_batch).  The
// FibonacciCircuit of `steps` has 4 instance variables, 1 witness and steps + 1 rows; its result is linear in the inputs,
// result = ca a + cb b.  fibonacci_coeffs (circuits.hip, host): ca, cb by the mirror's additive chain on (1, 0) and (0, 1).
// fibonacci_batch_assign (witness.hip): on ctx->stream (a lane's, or the root's under its mutex) one upload of a | b and the z addresses
// out of the ctx's pinned staging, one launch, the public inputs read back, one synchronisation; the assignments share one allocation
// (WitnessDev::backing).  pubs: k x 12 limbs (a | b | result), written after the synchronisation.  Throws HipError (the stream
// drained) / std::bad_alloc.
constexpr size_t FIBONACCI_VARS = 5, FIBONACCI_INSTANCE = 4;
void fibonacci_coeffs(size_t steps, Fr &ca, Fr &cb);
void fibonacci_batch_assign(zkg16_ctx *ctx, const Fr &ca, const Fr &cb, const uint64_t *a, const uint64_t *b, size_t k,
                            std::vector<std::shared_ptr<WitnessDev>> &out, uint64_t *pubs, float *dev_ms);

// K linear-equation requests of one size n in one pass (zkg16_witness_linear_batch, zkg16_prove_linear_batch).  LinearDims: the
// n-system's dimensions (zkg16.h gives the layout).  linear_zero_diagonal (circuits.hip, host): the first (request, row) whose diagonal
// entry is zero, which every entry refuses before any other work.  linear_r1cs_build (circuits.hip, host): the three matrices from
// the closed form into arrays sized by LinearDims.  linear_batch_assign (witness.hip): on ctx->stream (a lane's, or the root's under
// its mutex) one upload of a | b out of the ctx's pinned staging, the solve launch (one wave per request) and the fill launch, x read
// back, one synchronisation; the assignments share one allocation (WitnessDev::backing).  x: k x n x 4 limbs, written after the
// synchronisation.  Throws HipError (the stream drained) / std::bad_alloc.
struct LinearDims {
    size_t ni, nw, nc, nnz[3];
    explicit LinearDims(size_t n) : ni(1 + n * (n + 1)), nw(n * (2 * n + 1)), nc(n * (n + 1)), nnz{2 * n * n + 2 * n, n * n + n, n * n} {}
    size_t vars() const { return ni + nw; }
};
// Option "linear_solver" = 1 (Gaussian elimination, linear_elim_dev.cuh): linear_batch_assign launches wit_linear_elim_kernel in the
// solve kernel's place and throws LinearSingular {first singular request of the call's k, the smallest c for which columns 0..c of a
// are linearly dependent} after the synchronisation.  linear_elim_in_lds: whether a request's working matrix stays in LDS (else
// n (n + 1) Fr of global workspace per workgroup).  linear_solve_general (circuits.hip, host): the same elimination for one request
// -> the status word, 0 or 1 + c; x is written only for 0.
struct LinearSingular { size_t req, col; };
bool linear_elim_in_lds(const zkg16_ctx *ctx, size_t n);
uint32_t linear_solve_general(size_t n, const uint64_t *a, const uint64_t *b, Fr *x);
bool linear_zero_diagonal(size_t n, const uint64_t *a, size_t k, size_t *req, size_t *row);
void linear_r1cs_build(size_t n, uint64_t *const rp[3], uint32_t *const col[3], Fr *const cf[3]);
void linear_batch_assign(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, size_t k,
                         std::vector<std::shared_ptr<WitnessDev>> &out, uint64_t *x, float *dev_ms);

// An assignment that becomes valid in parts while its proof is already running (prove_device): produce(k) blocks until part k
// can be made, then queues on ctx->stream whatever writes it; part_of[i] = the part variable i (and the trailing r, s, -rs slots)
// belongs to.
struct ZParts {
    int parts = 1;
    const uint8_t *part_of = nullptr;
    std::function<void(int)> produce;
};

size_t b_density_mask_run(zkg16_ctx *ctx, const G1AffineU *b1, const G2AffineU *b2, size_t n, uint8_t *mask);
// device outputs; either may be null: saturated (arkworks layout, host-bound) and/or unsaturated (device-resident key)
void fixed_base_g1_run(zkg16_ctx *ctx, const G1Affine &base, const Fr *scalars_canonical, size_t n, G1Affine *out_sat, G1AffineU *out_u = nullptr);
void fixed_base_g2_run(zkg16_ctx *ctx, const G2Affine &base, const Fr *scalars_canonical, size_t n, G2Affine *out_sat, G2AffineU *out_u = nullptr);
// several scalar ranges in one pass (<= 8): range k = [start[k], start[k+1]) of the n concatenated scalars -> out_u[k] / out_sat[k]
// sync = false: everything is left queued on ctx->stream (the caller synchronises before touching the outputs)
void fixed_base_g1_multi(zkg16_ctx *ctx, const G1Affine &base, const Fr *scalars_canonical, size_t n, int nseg, const size_t *start,
                         G1AffineU *const *out_u, G1Affine *const *out_sat, bool sync = true);
void fixed_base_g2_multi(zkg16_ctx *ctx, const G2Affine &base, const Fr *scalars_canonical, size_t n, int nseg, const size_t *start,
                         G2AffineU *const *out_u, G2Affine *const *out_sat, bool sync = true);

}  // namespace zk
