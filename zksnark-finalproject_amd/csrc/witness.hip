// MatrixCircuit assignment generated ON THE DEVICE ("host-side circuit synthesis in C++ / on GPU").
//
// The reference's `proving_time` (/root/reference/src/arkworks/backend/matrix_proof.rs:138-145) covers
// `Groth16::prove(&pk, circuit, rng)`, which re-synthesises the circuit: the assignment z = instance || witness of
// MatrixCircuit (matrix_proof_of_work/constraints.rs:101-128) is recomputed on every request.  Its layout (same as
// circuits.hip's zkg16_circuit_matrix_witness, which is what the tests compare against byte for byte):
//
//   [1, hash_a, hash_b, hash_c] | a (n^2) | b (n^2) | sponge(a) gadget | sponge(b) gadget | n^2 zeros (constraints.rs:84)
//   | per (i, j): 0 (the sum's seed, :87) then the n products a_ik b_kj (:91) | sponge(c) gadget
//
// with each sponge gadget = per Poseidon permutation the five products x^2, x^4, x^8, x^16, x^17 of every S-box input that
// is not a constant (hashing_utils.rs:737-802: 8 full + 29 partial rounds, alpha = 17 -> 265 values; the first permutation
// of a hash has a constant capacity lane in round 0 -> 260).  75 % of z are those sponge values.
//
// Split of the work:
//   * A sponge is a sequential chain — permutation p + 1 needs the state permutation p leaves (hasher.rs:17-27) — so the
//     three chains run natively on three host threads over 64-bit limbs (hostff.hpp), recording only the state in front
//     of every permutation (96 B each).  c = a b comes first on the third thread, over the integers: every entry is
//     below n 2^128 < r, so no reduction is involved.
//   * Everything else is data-parallel and happens on the device, written in place into the buffer
//     zkg16_prove_resident reads: the u64 -> Montgomery conversions, the n^3 products, and for each of the 3 ceil(n^2/2)
//     permutations its 265 S-box values from the recorded entering state (one lane per permutation).
// Nothing of z crosses PCIe: the upload is a, b (16 n^2 B) + the entering states (288 B per two matrix entries) instead
// of 32 B per variable (278 MB at 128x128).
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "common.hpp"
#include "hostff.hpp"

using namespace zk;
using zk::h64::Fr64;

namespace {

#include "poseidon_params.inc"

constexpr int P_ROUNDS = POSEIDON_FULL + POSEIDON_PARTIAL, P_HALF = POSEIDON_FULL / 2;
constexpr size_t PERM_WITNESSES = 265, FIRST_PERM_SKIPPED = 5;

typedef unsigned __int128 u128;

#include "poseidon_h64.inc"

Fr64 fr64_from_u64(uint64_t v) {
    Fr64 c = Fr64::zero();
    c.l[0] = v;
    return h64::to_mont(c);
}

// c = a b over the integers (entries < n 2^128 < r), as Montgomery Fr.  bt = b transposed.
void matmul_u64(size_t n, const uint64_t *a, const uint64_t *b, Fr64 *c) {
    std::vector<uint64_t> bt(n * n);
    for (size_t k = 0; k < n; k++)
        for (size_t j = 0; j < n; j++) bt[j * n + k] = b[k * n + j];
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            u128 lo = 0;
            uint64_t hi = 0;
            const uint64_t *ar = a + i * n, *br = bt.data() + j * n;
            for (size_t k = 0; k < n; k++) {
                const u128 p = (u128)ar[k] * br[k];
                lo += p;
                hi += lo < p ? 1 : 0;
            }
            Fr64 v = Fr64::zero();
            v.l[0] = (uint64_t)lo; v.l[1] = (uint64_t)(lo >> 64); v.l[2] = hi;
            c[i * n + j] = h64::to_mont(v);
        }
}

struct MatrixChains {
    size_t n = 0, nn = 0, perms = 0;
    std::vector<Fr64> elems[3];         // a, b, c as Montgomery Fr
    std::vector<Fr64> states[3];        // perms x 3 each
    Fr64 hash[3];
    std::atomic<size_t> done[3];        // permutations of chain h whose entering state has been written
    std::thread th[3];
    bool started[3] = {false, false, false};
    std::chrono::steady_clock::time_point t0;
    double chain_ms = 0;
    const uint64_t *a = nullptr, *b = nullptr;

    void chain(int h) {
        if (h == 2) matmul_u64(n, a, b, elems[2].data());
        else {
            const uint64_t *src = h == 0 ? a : b;
            for (size_t i = 0; i < nn; i++) elems[h][i] = fr64_from_u64(src[i]);
        }
        hash[h] = sponge_chain(elems[h].data(), nn, states[h].data(), &done[h]);
    }
    // the three chains, one host thread each (the third multiplies the matrices first).  inline_last: the third chain runs on the
    // calling thread (the one-shot entry point: nothing to overlap it with); otherwise all three run beside the caller, which
    // feeds the device from their progress (zkg16_prove_matrix).  a, b must stay valid until join().
    void start(size_t n_, const uint64_t *a_, const uint64_t *b_, bool inline_last) {
        t0 = std::chrono::steady_clock::now();
        n = n_; nn = n * n; a = a_; b = b_;
        perms = (nn + POSEIDON_RATE - 1) / POSEIDON_RATE;
        for (int h = 0; h < 3; h++) {
            elems[h].resize(nn);
            states[h].resize(3 * perms);
            done[h].store(0);
        }
        (void)pparams();
        // a thread that cannot be started (EAGAIN) is not fatal: its chain runs on the caller instead (in join at the latest)
        for (int h = 0; h < (inline_last ? 2 : 3); h++) {
            try {
                th[h] = std::thread([this, h]() { chain(h); });
                started[h] = true;
            } catch (const std::system_error &) {
            }
        }
        if (inline_last) { chain(2); ran_inline[2] = true; }
    }
    bool ran_inline[3] = {false, false, false};
    bool joined = false;
    void join() {
        if (joined) return;
        for (int h = 0; h < 3; h++) {
            if (started[h]) { th[h].join(); started[h] = false; ran_inline[h] = true; }
            else if (!ran_inline[h]) { chain(h); ran_inline[h] = true; }
        }
        chain_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        joined = true;
    }
    // blocks until every chain has recorded the entering states of its permutations [0, upto)
    void wait_for(size_t upto) {
        for (int h = 0; h < 3; h++) {
            if (!started[h] && !ran_inline[h]) { chain(h); ran_inline[h] = true; }      // its thread never started
            while (done[h].load(std::memory_order_acquire) < upto) std::this_thread::sleep_for(std::chrono::microseconds(30));
        }
    }
    ~MatrixChains() {
        for (int h = 0; h < 3; h++)
            if (started[h]) th[h].join();
    }
};

// The chains of k requests on a pool of host threads (zkg16_matrix_sponge_states_batch).  A chain is sequential by construction, so
// the unit of work is a whole chain: 3k independent tasks handed out by one shared counter, the c chains first — they multiply the
// matrices before they hash, so they are the longest and must not be what the pool waits for at the end.  The caller is one of the
// `threads` workers; a thread that cannot be started runs its worker on the caller (ThreadGroup), which then takes whatever tasks
// are left.  states (nullable): k x 3 x perms x 3, request-major, then a, b, c; hashes: k x 3.  Throws std::bad_alloc.
void matrix_chains_batch(size_t n, const uint64_t *a, const uint64_t *b, size_t k, int threads, Fr64 *states, Fr64 *hashes) {
    const size_t nn = n * n, perms = (nn + POSEIDON_RATE - 1) / POSEIDON_RATE, tasks = 3 * k;
    size_t nth = threads <= 0 ? 8 : threads > 16 ? 16 : (size_t)threads;
    if (nth > tasks) nth = tasks;
    (void)pparams();
    std::atomic<size_t> next{0};
    std::atomic<bool> oom{false};
    auto worker = [&]() {
        try {
            std::vector<Fr64> elems(nn);
            for (size_t t; (t = next.fetch_add(1)) < tasks;) {
                const int h = t < k ? 2 : t < 2 * k ? 0 : 1;
                const size_t i = t < k ? t : t < 2 * k ? t - k : t - 2 * k;
                const uint64_t *ai = a + i * nn, *bi = b + i * nn;
                if (h == 2) matmul_u64(n, ai, bi, elems.data());
                else {
                    const uint64_t *src = h == 0 ? ai : bi;
                    for (size_t e = 0; e < nn; e++) elems[e] = fr64_from_u64(src[e]);
                }
                hashes[3 * i + h] = sponge_chain(elems.data(), nn, states ? states + (3 * i + h) * 3 * perms : nullptr, nullptr);
            }
        } catch (const std::bad_alloc &) {
            oom.store(true);
        }
    };
    {
        ThreadGroup tg;
        for (size_t t = 1; t < nth; t++) tg.run(worker);
        worker();
    }
    if (oom.load()) throw std::bad_alloc();
}

// k independent chains of `count` elements each on the same pool (zkg16_poseidon_hash_batch_host, zkg16_matrix_hash_batch_host):
// data = k x count Montgomery Fr, or with u64_elems k x count u64 taken to Montgomery form first.  out: k hashes.
void hash_chains_batch(bool u64_elems, const uint64_t *data, size_t count, size_t k, int threads, Fr64 *out) {
    size_t nth = threads <= 0 ? 8 : threads > 16 ? 16 : (size_t)threads;
    if (nth > k) nth = k;
    (void)pparams();
    std::atomic<size_t> next{0};
    std::atomic<bool> oom{false};
    auto worker = [&]() {
        try {
            std::vector<Fr64> elems(count);
            for (size_t t; (t = next.fetch_add(1)) < k;) {
                if (u64_elems)
                    for (size_t e = 0; e < count; e++) elems[e] = fr64_from_u64(data[t * count + e]);
                else memcpy(elems.data(), data + 4 * t * count, count * sizeof(Fr64));
                out[t] = sponge_chain(elems.data(), count, nullptr, nullptr);
            }
        } catch (const std::bad_alloc &) {
            oom.store(true);
        }
    };
    {
        ThreadGroup tg;
        for (size_t t = 1; t < nth; t++) tg.run(worker);
        worker();
    }
    if (oom.load()) throw std::bad_alloc();
}
// the host forms behind their argument checks; hashes are staged so that a failure leaves `out` alone
int hash_batch_host(bool u64_elems, const uint64_t *data, size_t count, size_t k, int threads, uint64_t *out) {
    try {
        std::vector<Fr64> hs(k);
        hash_chains_batch(u64_elems, data, count, k, threads, hs.data());
        memcpy(out, hs.data(), k * sizeof(Fr64));
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

#ifndef ZKG16_HOST_ONLY        // (tests/test_host_sanitize.py compiles the host chains alone, without kernels, under ASan)
// ------------------------------------------------------------------------------------------------ device
struct PoseidonDev { Fr mds[3][3], ark[P_ROUNDS][3]; };

__device__ __forceinline__ void st32(Fr *p, const Fr &v) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ Fr ld32(const Fr *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 lo = q[0], hi = q[1];
    Fr v;
    v.l[0] = lo.x; v.l[1] = lo.y; v.l[2] = lo.z; v.l[3] = lo.w; v.l[4] = hi.x; v.l[5] = hi.y; v.l[6] = hi.z; v.l[7] = hi.w;
    return v;
}

// z[0] = 1 | a, b as Montgomery Fr | n^2 zeros | per (i, j): 0, then a_ik b_kj for k < n.  One lane per element.
struct FillArgs {
    const uint64_t *a, *b;
    Fr *z;
    size_t n, nn, off_a, off_mc, off_mm, total;       // total = 2 nn (a, b) + nn (zeros) + nn (n + 1) (sums' seeds + products)
};
__global__ void __launch_bounds__(256) wit_matrix_fill_kernel(FillArgs g) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= g.total) return;
    if (t == 0) st32(g.z, Fr::one());
    Fr v = Fr::zero();
    Fr *dst;
    if (t < 2 * g.nn) {
        v.l[0] = (uint32_t)(t < g.nn ? g.a[t] : g.b[t - g.nn]);
        v.l[1] = (uint32_t)((t < g.nn ? g.a[t] : g.b[t - g.nn]) >> 32);
        v = fp_to_mont(v);
        dst = g.z + g.off_a + t;
    } else if (t < 3 * g.nn) {
        dst = g.z + g.off_mc + (t - 2 * g.nn);
    } else {
        const size_t e = t - 3 * g.nn, cell = e / (g.n + 1), k1 = e % (g.n + 1);
        dst = g.z + g.off_mm + e;
        if (k1) {
            const size_t i = cell / g.n, j = cell % g.n, k = k1 - 1;
            const uint64_t x = g.a[i * g.n + k], y = g.b[k * g.n + j];
            const uint64_t lo = x * y, hi = __umul64hi(x, y);
            v.l[0] = (uint32_t)lo; v.l[1] = (uint32_t)(lo >> 32); v.l[2] = (uint32_t)hi; v.l[3] = (uint32_t)(hi >> 32);
            v = fp_to_mont(v);       // the product of two F::from(u64) values, taken in Fr (constraints.rs:91): below 2^128 < r
        }
    }
    st32(dst, v);
}

// One lane per Poseidon permutation: from the state in front of it (host chain) the 265 values its S-boxes allocate, in the
// gadget's allocation order (round by round, lane 0..2, x^2, x^4, x^8, x^16, x^17), written where the sponge's segment of z
// puts them.  blockIdx.y = hash (a, b, c).
struct SpongeArgs {
    const Fr *states[3];            // perms x 3 each
    Fr *out[3];                     // first witness of each hash's gadget
    const PoseidonDev *params;
    uint32_t p_lo, p_hi;            // permutations [p_lo, p_hi) of every hash
};
__global__ void __launch_bounds__(64) wit_sponge_kernel(SpongeArgs g) {
    const uint32_t p = g.p_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.p_hi) return;
    const int h = blockIdx.y;
    const PoseidonDev *pp = g.params;
    Fr st[3];
    for (int i = 0; i < 3; i++) st[i] = ld32(g.states[h] + 3 * (size_t)p + i);
    Fr *out = g.out[h] + (p == 0 ? 0 : (size_t)p * PERM_WITNESSES - FIRST_PERM_SKIPPED);
    for (int r = 0; r < P_ROUNDS; r++) {
        const bool full = r < P_HALF || r >= P_HALF + POSEIDON_PARTIAL;
        for (int i = 0; i < 3; i++) st[i] = fp_add(st[i], pp->ark[r][i]);
        for (int i = 0; i < (full ? 3 : 1); i++) {
            const Fr x = st[i];
            const Fr x2 = fp_sqr(x), x4 = fp_sqr(x2), x8 = fp_sqr(x4), x16 = fp_sqr(x8), x17 = fp_mul(x16, x);
            if (!(p == 0 && r == 0 && i == 0)) {        // the capacity lane of a fresh sponge is a constant: no witnesses
                st32(out, x2); st32(out + 1, x4); st32(out + 2, x8); st32(out + 3, x16); st32(out + 4, x17);
                out += 5;
            }
            st[i] = x17;
        }
        Fr nst[3];
        for (int i = 0; i < 3; i++) {
            Fr acc = fp_mul(st[0], pp->mds[i][0]);
            acc = fp_add(acc, fp_mul(st[1], pp->mds[i][1]));
            nst[i] = fp_add(acc, fp_mul(st[2], pp->mds[i][2]));
        }
        for (int i = 0; i < 3; i++) st[i] = nst[i];
    }
}

// ---- K requests in one pass (zkg16_witness_matrix_batch).  The same two passes with the request as a grid dimension: one array
// of all a | b (k x 2 n^2), one of all entering states (k x 3 x perms x 3, the layout of matrix_chains_batch) and one of the K
// instance triples are read, and every request is written through a device-visible table of the K z pointers — the form the batched
// SpMV and digit kernels read the assignments in.  Both grids stay within 65,535 per dimension and loop over what is beyond.
struct FillBatchArgs {
    const uint64_t *ab;             // k x (a | b)
    const Fr *inst;                 // k x (hash_a, hash_b, hash_c); null with INST = false
    Fr *const *z;                   // k
    size_t k, n, nn, off_a, off_mc, off_mm, total;    // total = 4 (instance) + 2 nn (a, b) + nn (zeros) + nn (n + 1)
};
// INST = false (the chains run on the device): slots 1..3 are left to wit_chain_batch_kernel and g.inst is not read.  An instantiation
// of its own, so that the host route's kernel stays instruction for instruction what it was.
template <bool INST>
__global__ void __launch_bounds__(256) wit_matrix_fill_batch_kernel(FillBatchArgs g) {
    for (size_t req = blockIdx.y; req < g.k; req += gridDim.y) {
        const uint64_t *a = g.ab + req * 2 * g.nn, *b = a + g.nn;
        Fr *z = g.z[req];
        for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.total; t += (size_t)gridDim.x * blockDim.x) {
            Fr v = Fr::zero();
            Fr *dst;
            if (t < 4) {
                if (!INST && t) continue;
                dst = z + t;
                v = t == 0 ? Fr::one() : ld32(g.inst + 3 * req + (t - 1));
            } else if (t < 4 + 2 * g.nn) {
                const size_t e = t - 4;
                const uint64_t x = e < g.nn ? a[e] : b[e - g.nn];
                v.l[0] = (uint32_t)x;
                v.l[1] = (uint32_t)(x >> 32);
                v = fp_to_mont(v);
                dst = z + g.off_a + e;
            } else if (t < 4 + 3 * g.nn) {
                dst = z + g.off_mc + (t - 4 - 2 * g.nn);
            } else {
                const size_t e = t - 4 - 3 * g.nn, cell = e / (g.n + 1), k1 = e % (g.n + 1);
                dst = z + g.off_mm + e;
                if (k1) {
                    const size_t i = cell / g.n, j = cell % g.n, kk = k1 - 1;
                    const uint64_t x = a[i * g.n + kk], y = b[kk * g.n + j];
                    const uint64_t lo = x * y, hi = __umul64hi(x, y);
                    v.l[0] = (uint32_t)lo; v.l[1] = (uint32_t)(lo >> 32); v.l[2] = (uint32_t)hi; v.l[3] = (uint32_t)(hi >> 32);
                    v = fp_to_mont(v);
                }
            }
            st32(dst, v);
        }
    }
}

// One lane per permutation of any chain of any request: lane q of the k x 3 x perms entering states, so that a wave is full even
// where one request has fewer than 64 permutations per chain (8x8: 32).  The values and their order are wit_sponge_kernel's.
struct SpongeBatchArgs {
    const Fr *states;               // k x 3 x perms x 3
    Fr *const *z;                   // k
    const PoseidonDev *params;
    size_t off[3];                  // first witness of each hash's gadget within an assignment
    size_t lanes, perms;            // lanes = k x 3 x perms
};
__global__ void __launch_bounds__(64) wit_sponge_batch_kernel(SpongeBatchArgs g) {
    const PoseidonDev *pp = g.params;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < g.lanes; q += (size_t)gridDim.x * blockDim.x) {
        const size_t chain = q / g.perms, p = q % g.perms, req = chain / 3;
        const int h = (int)(chain % 3);
        Fr st[3];
        for (int i = 0; i < 3; i++) st[i] = ld32(g.states + 3 * q + i);
        Fr *out = g.z[req] + g.off[h] + (p == 0 ? 0 : p * PERM_WITNESSES - FIRST_PERM_SKIPPED);
        for (int r = 0; r < P_ROUNDS; r++) {
            const bool full = r < P_HALF || r >= P_HALF + POSEIDON_PARTIAL;
            for (int i = 0; i < 3; i++) st[i] = fp_add(st[i], pp->ark[r][i]);
            for (int i = 0; i < (full ? 3 : 1); i++) {
                const Fr x = st[i];
                const Fr x2 = fp_sqr(x), x4 = fp_sqr(x2), x8 = fp_sqr(x4), x16 = fp_sqr(x8), x17 = fp_mul(x16, x);
                if (!(p == 0 && r == 0 && i == 0)) {
                    st32(out, x2); st32(out + 1, x4); st32(out + 2, x8); st32(out + 3, x16); st32(out + 4, x17);
                    out += 5;
                }
                st[i] = x17;
            }
            Fr nst[3];
            for (int i = 0; i < 3; i++) {
                Fr acc = fp_mul(st[0], pp->mds[i][0]);
                acc = fp_add(acc, fp_mul(st[1], pp->mds[i][1]));
                nst[i] = fp_add(acc, fp_mul(st[2], pp->mds[i][2]));
            }
            for (int i = 0; i < 3; i++) st[i] = nst[i];
        }
    }
}

// ---- the chains of a large batch walked on the device (option "sponge_chains_min"): one lane per chain, so each permutation is
// computed once and its S-box values are written by the lane that needs its result anyway (sponge_chain_dev.cuh).  Chains are numbered
// hash-major — all a chains, then b, then c — so that a wave holds one kind of loader except where k is no multiple of 64.  A chain is
// walked in launches of at most "sponge_chain_segment" permutations, its state carried in `state` between them: no launch runs for
// seconds (a 128x128 chain is 8,192 permutations), and other lanes' kernels get in between.
#include "sponge_chain_dev.cuh"
struct ChainBatchArgs {
    const void *data;               // form 2: k x (a | b) u64; form 0: k x count Fr; form 1: k x count u64
    Fr *state;                      // chains x 3, read when p_lo > 0, written when p_hi < perms
    Fr *hashes;                     // form 2: k x 3 (request-major: the public inputs); else k.  Written by the chain's last launch
    Fr *const *z;                   // form 2: k assignments
    const PoseidonDev *params;
    size_t off[3];                  // form 2: first witness of each hash's gadget within an assignment
    size_t k, n, count, chains;     // count = elements per chain (form 2: n^2); chains = 3 k in form 2, else k
    uint32_t p_lo, p_hi, perms;
    int form;
};
template <bool ASSIGN>
__global__ void __launch_bounds__(64) wit_chain_batch_kernel(ChainBatchArgs g) {
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.chains; c += (size_t)gridDim.x * blockDim.x) {
        const size_t h = ASSIGN ? c / g.k : 0, req = ASSIGN ? c % g.k : c;
        ChainLoadAny ld;
        if (ASSIGN) {
            const uint64_t *a = static_cast<const uint64_t *>(g.data) + req * 2 * g.count;
            ld = ChainLoadAny{h == 2 ? 2 : 1, h == 0 ? a : a + g.count, a, a + g.count, g.n};
        } else {
            ld = ChainLoadAny{g.form, g.form == 0 ? static_cast<const void *>(static_cast<const Fr *>(g.data) + req * g.count)
                                                  : static_cast<const void *>(static_cast<const uint64_t *>(g.data) + req * g.count),
                              nullptr, nullptr, 0};
        }
        Fr st[3];
        for (int i = 0; i < 3; i++) st[i] = g.p_lo ? ld32(g.state + 3 * c + i) : Fr::zero();
        Fr *out = ASSIGN ? g.z[req] + g.off[h] : nullptr;
        const Fr hash = sponge_chain_walk<ASSIGN>(*g.params, ld, g.count, g.p_lo, g.p_hi, st, out);
        if (g.p_hi < g.perms) {
            for (int i = 0; i < 3; i++) st32(g.state + 3 * c + i, st[i]);
        } else if (ASSIGN) {
            st32(g.hashes + 3 * req + h, hash);
            st32(g.z[req] + 1 + h, hash);
        } else {
            st32(g.hashes + req, hash);
        }
    }
}

// ---- K Fibonacci requests of one round count (zkg16_witness_fibonacci_batch): one lane per request.  The assignment is 1 | a | b |
// result | 0, and result = ca a + cb b with the two coefficients the host took from the mirror's chain (fibonacci_coeffs), so a lane
// costs four field products and one addition whatever `steps` is.  Every operation reduces fully, so the sum is the canonical value
// the host chain ends on.  The lane writes through the table of the K z pointers and leaves a | b | result in `pub` as well.
struct FibBatchArgs {
    const uint64_t *ab;             // k x (a, b)
    Fr *const *z;                   // k
    Fr *pub;                        // k x 3
    Fr ca, cb;
    size_t k;
};
__global__ void __launch_bounds__(64) wit_fibonacci_batch_kernel(FibBatchArgs g) {
    for (size_t req = (size_t)blockIdx.x * blockDim.x + threadIdx.x; req < g.k; req += (size_t)gridDim.x * blockDim.x) {
        Fr v[2];
        for (int i = 0; i < 2; i++) {
            const uint64_t x = g.ab[2 * req + i];
            v[i] = Fr::zero();
            v[i].l[0] = (uint32_t)x;
            v[i].l[1] = (uint32_t)(x >> 32);
            v[i] = fp_to_mont(v[i]);
        }
        const Fr res = fp_add(fp_mul(g.ca, v[0]), fp_mul(g.cb, v[1]));
        Fr *z = g.z[req], *pub = g.pub + 3 * req;
        st32(z, Fr::one());
        st32(z + 1, v[0]); st32(z + 2, v[1]); st32(z + 3, res);
        st32(z + 4, Fr::zero());
        st32(pub, v[0]); st32(pub + 1, v[1]); st32(pub + 2, res);
    }
}

// ---- K linear-equation requests of one size (zkg16_witness_linear_batch): the solve, then the fill (linear_dev.cuh holds the
// arithmetic and its value bounds: every element is fully reduced wherever it is stored).
// Solve: one 64-lane wave per request — a lone lane on serial Fr work is what DESIGN §2.8.1 measured.  LDS holds one Fr per row: first
// 1 / a_ii, which lane i mod 64 computes, and from row i's end on y_i = x_i R^2, the form the later rows multiply the u64 entries with.
// Row i: every lane sums its j < i, the partial sums cross the wave by limb exchanges, lane 0 forms x_i, writes it to `x` and swaps
// the LDS slot.  The block is one wave, so the barrier after each row is a wave barrier; its trip counts depend on blockIdx alone.
// n <= ZKG16_LINEAR_N_MAX = 1024: at most 32 KB of LDS.
#include "linear_dev.cuh"
struct LinearBatchArgs {
    const uint64_t *a, *b;          // k x n x n, k x n
    Fr *x;                          // k x n
    Fr *z;                          // k x vars: the assignments, one after the other
    size_t n, k, vars;
};
__device__ __forceinline__ Fr linear_xchg(const Fr &v, int off) {
    Fr o;
    for (int i = 0; i < 8; i++) o.l[i] = (uint32_t)__shfl_xor((int)v.l[i], off, LINEAR_LANES);
    return o;
}
__global__ void __launch_bounds__(LINEAR_LANES) wit_linear_solve_kernel(LinearBatchArgs g) {
    extern __shared__ uint4 linear_lds[];
    Fr *y = reinterpret_cast<Fr *>(linear_lds);
    const int lane = (int)threadIdx.x;
    const size_t n = g.n;
    for (size_t req = blockIdx.x; req < g.k; req += gridDim.x) {
        const uint64_t *a = g.a + req * n * n, *b = g.b + req * n;
        Fr *x = g.x + req * n;
        for (size_t i = (size_t)lane; i < n; i += LINEAR_LANES) y[i] = linear_diag_inv(a[i * n + i]);
        __syncthreads();
        for (size_t i = 0; i < n; i++) {
            Fr v = linear_partial(a + i * n, y, i, lane);
            for (int off = LINEAR_LANES / 2; off; off >>= 1) v = linear_fold_step(v, linear_xchg(v, off));
            if (lane == 0) {
                const Fr xi = linear_finish(b[i], v, y[i]);
                st32(x + i, xi);
                y[i] = linear_keep(xi);
            }
            __syncthreads();            // y[i] is row i + 1's; the next request's inverses come after the last row's barrier
        }
    }
}
// Fill: a grid-stride loop over the k x vars elements, one lane per element, so consecutive lanes write consecutive 32-byte elements.
__global__ void __launch_bounds__(256) wit_linear_fill_kernel(LinearBatchArgs g) {
    const size_t total = g.k * g.vars;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t req = e / g.vars, t = e % g.vars;
        st32(g.z + e, linear_fill_value(g.n, g.a + req * g.n * g.n, g.b + req * g.n, g.x + req * g.n, t));
    }
}

// ---- the solve by elimination (option "linear_solver" = 1; linear_elim_dev.cuh holds the phases, their value bounds and the status
// rule).  One workgroup of 256 lanes per request, a grid-stride loop over the requests.  LDS: inv[n] | pick[2], status | order[n], and
// behind them the working matrix M when n <= the LDS bound (option "linear_elim_lds_max", 64 by default: 133,120 + 2,336 bytes of 160 KiB);
// above it M is the workgroup's slice of a workspace in global memory (g.work), which __syncthreads orders like the LDS.
// Per request 4 n + 2 barriers whatever the data: one after the load, three per column (offers in | pivot placed | rows reduced), one
// after the inversions, one per column of the back substitution.  The offers of column c meet in pick[c & 1]; lane 0 resets the
// other word while it places the pivot, which nobody reads between those two barriers.  A singular request gets x = 0.
#include "linear_elim_dev.cuh"
struct LinearElimArgs {
    const uint64_t *a, *b;          // k x n x n, k x n
    Fr *x;                          // k x n
    uint32_t *status;               // k: 0, or 1 + the column without a pivot
    Fr *work;                       // gridDim.x x n (n + 1); unused by the LDS form
    size_t n, k;
};
template <bool IN_LDS>
__global__ void __launch_bounds__(LINEAR_ELIM_LANES) wit_linear_elim_kernel(LinearElimArgs g) {
    extern __shared__ uint4 linear_lds[];           // all of it dynamic: a static word would come off the 160 KiB the launch may ask for
    const int lane = (int)threadIdx.x;
    const size_t n = g.n;
    Fr *inv = reinterpret_cast<Fr *>(linear_lds);
    uint32_t *pick = reinterpret_cast<uint32_t *>(inv + n), &status = pick[2], *order = pick + 8;
    Fr *M = IN_LDS ? inv + n + 1 + (n + 7) / 8 : g.work + (size_t)blockIdx.x * n * (n + 1);
    for (size_t req = blockIdx.x; req < g.k; req += gridDim.x) {
        Fr *x = g.x + req * n;
        linear_elim_load(n, g.a + req * n * n, g.b + req * n, M, order, lane, LINEAR_ELIM_LANES);
        if (lane == 0) { pick[0] = pick[1] = (uint32_t)n; status = 0; }
        __syncthreads();
        for (size_t c = 0; c < n; c++) {
            const uint32_t offer = linear_elim_offer(n, M, order, c, lane, LINEAR_ELIM_LANES);
            if (offer < n) atomicMin(&pick[c & 1], offer);
            __syncthreads();
            if (lane == 0) {
                const uint32_t k = pick[c & 1];
                if (k < n) linear_elim_swap(order, c, k);
                else if (status == 0) status = (uint32_t)(1 + c);
                pick[(c + 1) & 1] = (uint32_t)n;
            }
            __syncthreads();
            if (status == 0) linear_elim_reduce(n, M, order, c, lane, LINEAR_ELIM_LANES);
            __syncthreads();
        }
        const bool ok = status == 0;
        if (ok) linear_elim_invert(n, M, order, inv, lane, LINEAR_ELIM_LANES);
        else for (size_t i = (size_t)lane; i < n; i += LINEAR_ELIM_LANES) st32(x + i, Fr::zero());
        __syncthreads();
        for (size_t c = n; c-- > 0;) {
            if (ok) {
                const Fr xc = linear_elim_back(n, M, order, inv, c, lane, LINEAR_ELIM_LANES);
                if (lane == 0) st32(x + c, xc);
            }
            __syncthreads();
        }
        if (lane == 0) g.status[req] = status;      // the next request's reset of `status` is this lane's too
    }
}

// part_of[i] = the part of a streamed assignment in which variable i becomes valid: 0 = what needs only a and b (the constant,
// a, b, the zeros, the products; also the three trailing r / s / -rs slots of the z-side scalar vector), 1 + s = the S-box
// values of the permutations of slice s of every sponge, the last part also the three hashes.
struct PartArgs {
    uint8_t *part_of;
    size_t total, n_all, off_ha, off_hb, off_mc, off_hc, hw;
    uint32_t bounds[10];
    int slices;
};
__global__ void __launch_bounds__(256) wit_part_of_kernel(PartArgs g) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n_all) return;
    int part = 0;
    if (i >= 1 && i <= 3) part = g.slices;
    else if (i < g.total) {
        size_t o = g.total;
        if (i >= g.off_ha && i < g.off_ha + g.hw) o = i - g.off_ha;
        else if (i >= g.off_hb && i < g.off_hb + g.hw) o = i - g.off_hb;
        else if (i >= g.off_hc) o = i - g.off_hc;
        if (o != g.total) {
            const uint32_t p = o < PERM_WITNESSES - FIRST_PERM_SKIPPED ? 0u : (uint32_t)((o + FIRST_PERM_SKIPPED) / PERM_WITNESSES);
            int sl = 0;
            while (sl + 1 < g.slices && p >= g.bounds[sl + 1]) sl++;
            part = 1 + sl;
        }
    }
    g.part_of[i] = (uint8_t)part;
}

#endif  // ZKG16_HOST_ONLY
}  // namespace

#ifndef ZKG16_HOST_ONLY
namespace zk {

struct MatrixWitnessLayout {
    size_t n, nn, hw, ni, off_a, off_b, off_ha, off_hb, off_mc, off_mm, off_hc, total;
    explicit MatrixWitnessLayout(size_t n_) {
        n = n_; nn = n * n; ni = 4;
        hw = (nn + POSEIDON_RATE - 1) / POSEIDON_RATE * PERM_WITNESSES - FIRST_PERM_SKIPPED;
        off_a = ni; off_b = off_a + nn; off_ha = off_b + nn; off_hb = off_ha + hw; off_mc = off_hb + hw; off_mm = off_mc + nn;
        off_hc = off_mm + nn * (n + 1); total = off_hc + hw;
    }
};

// The assignment of one MatrixCircuit request arriving on the device in parts: part 0 needs only a and b, part 1 + s the
// entering states of slice s of the three host chains (common.hpp: MatrixWitnessStream is opaque to api_prove.hip).
struct MatrixWitnessStream {
    MatrixWitnessLayout L;
    MatrixChains mc;
    int slices = 1;
    bool overlap = false;                   // the proof runs while the parts arrive: part_of is built
    std::vector<uint32_t> bounds;           // slices + 1 permutation indices
    DevBuf d_ab, d_states, part_of;
    Fr *z = nullptr;
    const uint64_t *a = nullptr, *b = nullptr;
    Fr inst[3];
    explicit MatrixWitnessStream(size_t n) : L(n) {}
};

// The slices a streamed assignment of `perms` permutations per sponge arrives in: bounds[0 .. slices] are permutation indices, 0 first
// and perms last.  slices_wanted = 0: growing slices.  The device needs longer for a slice's terms than the host chain for its states
// (128x128: 84 ms of z-side accumulation against 61 ms of chain), so once started it never waits again — what counts is
// starting early: a first slice of 6 %, each later one about as long as the device is busy with the one before.
// slice_min (option "matrix_slice_min", default 512): the slice count is lowered until a slice holds at least that many permutations —
// a slice shorter than ~4 ms of host chain is all fixed cost on the device side.  At least 1, so no slice is ever empty.
int matrix_stream_slices(size_t perms, int slices_wanted, int slice_min, uint32_t bounds[9]) {
    static const double grow[5] = {0.06, 0.20, 0.45, 0.80, 1.0};
    if (slice_min < 1) slice_min = MATRIX_SLICE_MIN_DEFAULT;
    int k = slices_wanted == 0 ? 5 : slices_wanted < 1 ? 1 : slices_wanted > 8 ? 8 : slices_wanted;
    const bool growing = slices_wanted == 0 && perms >= 4096;
    if (!growing && slices_wanted == 0) k = 4;
    while (k > 1 && !growing && perms / k < (size_t)slice_min) k--;
    for (int i = 0; i <= k; i++)
        bounds[i] = growing ? (i == 0 ? 0u : (uint32_t)((double)perms * grow[i - 1] + 0.5)) : (uint32_t)(perms * (size_t)i / k);
    bounds[k] = (uint32_t)perms;
    return k;
}

MatrixWitnessStream *matrix_stream_start(size_t n, const uint64_t *a, const uint64_t *b, int slices_wanted, int slice_min, bool overlap) {
    auto *ms = new MatrixWitnessStream(n);
    ms->a = a; ms->b = b;
    const size_t perms = (ms->L.nn + POSEIDON_RATE - 1) / POSEIDON_RATE;
    uint32_t bounds[9];
    const int k = matrix_stream_slices(perms, slices_wanted, slice_min, bounds);
    ms->slices = overlap ? k : 1;           // without overlap the assignment arrives as a whole: one slice, whatever was asked for
    ms->overlap = overlap;
    if (overlap) ms->bounds.assign(bounds, bounds + k + 1);
    else ms->bounds = {0u, (uint32_t)perms};
    try {
        ms->mc.start(n, a, b, !overlap);
    } catch (...) {
        delete ms;
        throw;
    }
    return ms;
}
int matrix_stream_parts(const MatrixWitnessStream *ms) { return ms->slices + 1; }
size_t matrix_stream_total(const MatrixWitnessStream *ms) { return ms->L.total; }
const uint8_t *matrix_stream_part_of(const MatrixWitnessStream *ms) { return ms->overlap ? ms->part_of.as<uint8_t>() : nullptr; }
double matrix_stream_chain_ms(const MatrixWitnessStream *ms) { return ms->mc.chain_ms; }
void matrix_stream_hashes(const MatrixWitnessStream *ms, uint64_t out[12]) {
    for (int h = 0; h < 3; h++) memcpy(out + 4 * h, ms->mc.hash[h].l, 32);
}
void matrix_stream_free(MatrixWitnessStream *ms) { delete ms; }

// device buffers of the request; z: total (+ whatever the caller appends) elements.  n_extra: trailing slots of the z-side scalar
// vector (r, s, -rs) that part_of must cover too.
static void poseidon_dev_ensure(zkg16_ctx *ctx) {
    if (ctx->poseidon_dev.p) return;
    const PoseidonH &ph = pparams();
    PoseidonDev pd;
    static_assert(sizeof(PoseidonDev) == sizeof(Fr64) * (9 + 3 * P_ROUNDS), "layout");
    memcpy(pd.mds, ph.mds, sizeof pd.mds);
    memcpy(pd.ark, ph.ark, sizeof pd.ark);
    ctx->poseidon_dev.alloc(sizeof pd);
    ZK_HIP(hipMemcpy(ctx->poseidon_dev.p, &pd, sizeof pd, hipMemcpyHostToDevice));
}

void matrix_stream_attach(MatrixWitnessStream *ms, zkg16_ctx *ctx, Fr *z, size_t n_extra) {
    const MatrixWitnessLayout &L = ms->L;
    poseidon_dev_ensure(ctx);
    ms->z = z;
    ms->d_ab.alloc(2 * L.nn * sizeof(uint64_t));
    ms->d_states.alloc(3 * ms->mc.perms * 3 * sizeof(Fr));
    if (ms->overlap) {
        const size_t n_all = L.total + n_extra;
        ms->part_of.alloc(n_all);
        PartArgs g;
        g.part_of = ms->part_of.as<uint8_t>();
        g.total = L.total; g.n_all = n_all; g.off_ha = L.off_ha; g.off_hb = L.off_hb; g.off_mc = L.off_mc; g.off_hc = L.off_hc; g.hw = L.hw;
        g.slices = ms->slices;
        for (int i = 0; i <= ms->slices; i++) g.bounds[i] = ms->bounds[i];
        hipLaunchKernelGGL(wit_part_of_kernel, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
}

// Queues on ctx->stream what makes part k of z valid; blocks on the host first until the chains have got that far.
void matrix_stream_produce(MatrixWitnessStream *ms, zkg16_ctx *ctx, int k) {
    const MatrixWitnessLayout &L = ms->L;
    Fr *z = ms->z;
    if (k == 0) {
        ZK_HIP(hipMemcpyAsync(ms->d_ab.p, ms->a, L.nn * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipMemcpyAsync(ms->d_ab.as<uint64_t>() + L.nn, ms->b, L.nn * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        FillArgs g;
        g.a = ms->d_ab.as<uint64_t>(); g.b = g.a + L.nn; g.z = z; g.n = L.n; g.nn = L.nn;
        g.off_a = L.off_a; g.off_mc = L.off_mc; g.off_mm = L.off_mm; g.total = 3 * L.nn + L.nn * (L.n + 1);
        ScopedKernelTimer kt(ctx, "wit_matrix_fill_kernel", (double)g.total);
        hipLaunchKernelGGL(wit_matrix_fill_kernel, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
        return;
    }
    const uint32_t p_lo = ms->bounds[k - 1], p_hi = ms->bounds[k];
    const size_t perms = ms->mc.perms;
    if (k == ms->slices) ms->mc.join();          // the hashes exist once the chains have ended
    else ms->mc.wait_for(p_hi);
    for (int h = 0; h < 3; h++)
        ZK_HIP(hipMemcpyAsync(ms->d_states.as<Fr>() + (size_t)h * 3 * perms + 3 * (size_t)p_lo, ms->mc.states[h].data() + 3 * (size_t)p_lo,
                              3 * (size_t)(p_hi - p_lo) * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    if (k == ms->slices) {
        for (int h = 0; h < 3; h++) memcpy(ms->inst[h].l, ms->mc.hash[h].l, 32);
        ZK_HIP(hipMemcpyAsync(z + 1, ms->inst, sizeof ms->inst, hipMemcpyHostToDevice, ctx->stream));
    }
    SpongeArgs g;
    for (int h = 0; h < 3; h++) g.states[h] = ms->d_states.as<Fr>() + (size_t)h * 3 * perms;
    g.out[0] = z + L.off_ha; g.out[1] = z + L.off_hb; g.out[2] = z + L.off_hc;
    g.params = ctx->poseidon_dev.as<PoseidonDev>();
    g.p_lo = p_lo; g.p_hi = p_hi;
    ScopedKernelTimer kt(ctx, "wit_sponge_kernel", 3.0 * (double)(p_hi - p_lo));
    hipLaunchKernelGGL(wit_sponge_kernel, dim3((unsigned)((p_hi - p_lo + 63) / 64), 3), dim3(64), 0, ctx->stream, g);
    ZK_HIP(hipGetLastError());
}

// ---- K requests in one pass
size_t matrix_witness_total(size_t n) { return MatrixWitnessLayout(n).total; }

void matrix_batch_chains(MatrixBatchChains &c, size_t n, const uint64_t *a, const uint64_t *b, size_t k, int threads, uint64_t *hashes) {
    static_assert(sizeof(Fr64) == 32, "layout");
    const auto t0 = std::chrono::steady_clock::now();
    c.n = n; c.k = k;
    c.perms = (n * n + POSEIDON_RATE - 1) / POSEIDON_RATE;
    c.states.resize(k * 3 * c.perms * 12);
    matrix_chains_batch(n, a, b, k, threads, reinterpret_cast<Fr64 *>(c.states.data()), reinterpret_cast<Fr64 *>(hashes));
    c.hashes = hashes;
    c.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Whether a call with this many chains walks them on the device (option "sponge_chains_min": 1 = always, above 2^32 = never).
bool sponge_chains_on_device(const zkg16_ctx *ctx, size_t chains) {
    const int64_t m = ctx->opt.sponge_chains_min;
    return m <= ((int64_t)1 << 32) && chains >= (uint64_t)m;
}
// the device route's stand-in for matrix_batch_chains: nothing runs here, matrix_batch_assign walks the chains and fills `hashes`
void matrix_batch_chains_device(MatrixBatchChains &c, size_t n, size_t k, uint64_t *hashes) {
    c.n = n; c.k = k;
    c.perms = (n * n + POSEIDON_RATE - 1) / POSEIDON_RATE;
    c.states.clear();
    c.hashes = hashes;
    c.on_device = true;
    c.ms = 0;
}

// launches of at most "sponge_chain_segment" permutations until every chain of `g` has ended
static void chain_batch_launch(zkg16_ctx *ctx, ChainBatchArgs g, bool assign) {
    const size_t cap = ctx->opt.matrix_batch_grid > 0 ? (size_t)ctx->opt.matrix_batch_grid : 65535;
    const uint32_t seg = ctx->opt.sponge_chain_segment > 0 ? (uint32_t)ctx->opt.sponge_chain_segment : 256;
    const size_t bx = (g.chains + 63) / 64;
    const dim3 grid((unsigned)(bx < cap ? bx : cap));
    for (uint32_t p = 0; p < g.perms;) {
        g.p_lo = p;
        g.p_hi = g.perms - p > seg ? p + seg : g.perms;
        ScopedKernelTimer kt(ctx, "wit_chain_batch_kernel", (double)g.chains * (double)(g.p_hi - g.p_lo));
        if (assign) hipLaunchKernelGGL(wit_chain_batch_kernel<true>, grid, dim3(64), 0, ctx->stream, g);
        else hipLaunchKernelGGL(wit_chain_batch_kernel<false>, grid, dim3(64), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
        p = g.p_hi;
    }
}

void mbatch_staging_ensure(zkg16_ctx *ctx, size_t bytes) {
    if (ctx->mbatch_host_bytes < bytes) {           // nothing reads the old block: every call ends with the stream drained
        if (ctx->mbatch_host) (void)hipHostFree(ctx->mbatch_host);
        ctx->mbatch_host = nullptr;
        ctx->mbatch_host_bytes = 0;
        ZK_HIP(hipHostMalloc(&ctx->mbatch_host, bytes, hipHostMallocDefault));
        ctx->mbatch_host_bytes = bytes;
    }
    ctx->mbatch_dev.ensure(bytes);
}

// k hashes on ctx->stream (a lane's, under its mutex): form 0 = k vectors of `count` Montgomery Fr, form 1 = k vectors of `count` u64.
// One upload, the chain launches, one read-back through the ctx's pinned staging; `out` is written only when all of it succeeded.
void sponge_hash_batch_device(zkg16_ctx *ctx, int form, const uint64_t *data, size_t count, size_t k, uint64_t *out) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t elem = form == 0 ? sizeof(Fr) : sizeof(uint64_t);
    const size_t in_bytes = up(k * count * elem), st_bytes = up(k * 3 * sizeof(Fr)), out_bytes = up(k * sizeof(Fr));
    poseidon_dev_ensure(ctx);
    mbatch_staging_ensure(ctx, in_bytes + st_bytes + out_bytes);
    uint8_t *hs = static_cast<uint8_t *>(ctx->mbatch_host), *ds = ctx->mbatch_dev.as<uint8_t>();
    memcpy(hs, data, k * count * elem);
    struct Drain { zkg16_ctx *c; bool ok = false; ~Drain() { if (!ok) (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    ZK_HIP(hipMemcpyAsync(ds, hs, k * count * elem, hipMemcpyHostToDevice, ctx->stream));
    ChainBatchArgs g = {};
    g.data = ds;
    g.state = reinterpret_cast<Fr *>(ds + in_bytes);
    g.hashes = reinterpret_cast<Fr *>(ds + in_bytes + st_bytes);
    g.z = nullptr;
    g.params = ctx->poseidon_dev.as<PoseidonDev>();
    g.k = k; g.n = 0; g.count = count; g.chains = k;
    g.perms = (uint32_t)((count + POSEIDON_RATE - 1) / POSEIDON_RATE);
    g.form = form;
    chain_batch_launch(ctx, g, false);
    ZK_HIP(hipMemcpyAsync(hs + in_bytes + st_bytes, ds + in_bytes + st_bytes, k * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    drain.ok = true;
    memcpy(out, hs + in_bytes + st_bytes, k * sizeof(Fr));
}

// The k assignments of `c`'s requests on ctx->stream, under ctx's mutex: three copies out of the ctx's pinned staging (a | b, the
// entering states, the instances with the z pointers), the two batched launches, one synchronisation.  With the chains on the device
// (c.on_device): a | b and the z pointers go up, the fill pass leaves slots 1..3 to wit_chain_batch_kernel, which takes the place of
// the per-permutation pass, and the k x 3 hashes come back once into c.hashes.  The assignments share one
// allocation, which goes back when the last of them is gone (WitnessDev::backing).  When this throws the stream has been drained.
void matrix_batch_assign(zkg16_ctx *ctx, const MatrixBatchChains &c, const uint64_t *a, const uint64_t *b,
                         std::vector<std::shared_ptr<WitnessDev>> &out, float *dev_ms) {
    const MatrixWitnessLayout L(c.n);
    const size_t k = c.k, perms = c.perms;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const bool dev = c.on_device;                   // st: the carried states of the 3k chains instead of every entering state
    const size_t ab_bytes = up(k * 2 * L.nn * sizeof(uint64_t)), st_bytes = up(k * 3 * (dev ? 1 : perms) * 3 * sizeof(Fr));
    const size_t tab_bytes = up(k * (3 * sizeof(Fr) + sizeof(Fr *))), bytes = ab_bytes + st_bytes + tab_bytes;
    const size_t cap = ctx->opt.matrix_batch_grid > 0 ? (size_t)ctx->opt.matrix_batch_grid : 65535;
    poseidon_dev_ensure(ctx);
    mbatch_staging_ensure(ctx, bytes);
    auto backing = std::make_shared<DevBuf>(k * L.total * sizeof(Fr));
    std::vector<std::shared_ptr<WitnessDev>> wits(k);
    for (size_t i = 0; i < k; i++) {
        wits[i] = std::make_shared<WitnessDev>();
        wits[i]->n = L.total;
        wits[i]->backing = backing;
        wits[i]->z.p = backing->as<Fr>() + i * L.total;
        wits[i]->z.bytes = L.total * sizeof(Fr);
    }
    uint8_t *hs = static_cast<uint8_t *>(ctx->mbatch_host), *ds = ctx->mbatch_dev.as<uint8_t>();
    uint64_t *h_ab = reinterpret_cast<uint64_t *>(hs);
    for (size_t i = 0; i < k; i++) {
        memcpy(h_ab + i * 2 * L.nn, a + i * L.nn, L.nn * sizeof(uint64_t));
        memcpy(h_ab + i * 2 * L.nn + L.nn, b + i * L.nn, L.nn * sizeof(uint64_t));
    }
    if (!dev) {
        memcpy(hs + ab_bytes, c.states.data(), k * 3 * perms * 3 * sizeof(Fr));
        memcpy(hs + ab_bytes + st_bytes, c.hashes, k * 3 * sizeof(Fr));
    }
    Fr **h_tab = reinterpret_cast<Fr **>(hs + ab_bytes + st_bytes + k * 3 * sizeof(Fr));
    for (size_t i = 0; i < k; i++) h_tab[i] = wits[i]->z.as<Fr>();

    hipEvent_t e0, e1;
    ZK_HIP(hipEventCreate(&e0));
    struct EvGuard { hipEvent_t e; ~EvGuard() { (void)hipEventDestroy(e); } } g0{e0};
    ZK_HIP(hipEventCreate(&e1));
    EvGuard g1{e1};
    struct Drain { zkg16_ctx *c; bool ok = false; ~Drain() { if (!ok) (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    ZK_HIP(hipEventRecord(e0, ctx->stream));
    ZK_HIP(hipMemcpyAsync(ds, hs, k * 2 * L.nn * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    const size_t tab_off = ab_bytes + st_bytes + k * 3 * sizeof(Fr);
    if (dev) {
        ZK_HIP(hipMemcpyAsync(ds + tab_off, hs + tab_off, k * sizeof(Fr *), hipMemcpyHostToDevice, ctx->stream));
    } else {
        ZK_HIP(hipMemcpyAsync(ds + ab_bytes, hs + ab_bytes, k * 3 * perms * 3 * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipMemcpyAsync(ds + ab_bytes + st_bytes, hs + ab_bytes + st_bytes, k * (3 * sizeof(Fr) + sizeof(Fr *)), hipMemcpyHostToDevice, ctx->stream));
    }
    Fr *const *d_tab = reinterpret_cast<Fr *const *>(ds + tab_off);
    {
        FillBatchArgs g;
        g.ab = reinterpret_cast<const uint64_t *>(ds);
        g.inst = dev ? nullptr : reinterpret_cast<const Fr *>(ds + ab_bytes + st_bytes);
        g.z = d_tab;
        g.k = k; g.n = L.n; g.nn = L.nn; g.off_a = L.off_a; g.off_mc = L.off_mc; g.off_mm = L.off_mm;
        g.total = 4 + 3 * L.nn + L.nn * (L.n + 1);
        const size_t bx = (g.total + 255) / 256;
        ScopedKernelTimer kt(ctx, "wit_matrix_fill_batch_kernel", (double)g.total * (double)k);
        const dim3 grid((unsigned)(bx < cap ? bx : cap), (unsigned)(k < cap ? k : cap));
        if (dev) hipLaunchKernelGGL(wit_matrix_fill_batch_kernel<false>, grid, dim3(256), 0, ctx->stream, g);
        else hipLaunchKernelGGL(wit_matrix_fill_batch_kernel<true>, grid, dim3(256), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
    if (dev) {
        ChainBatchArgs g = {};
        g.data = ds;
        g.state = reinterpret_cast<Fr *>(ds + ab_bytes);
        g.hashes = reinterpret_cast<Fr *>(ds + ab_bytes + st_bytes);
        g.z = d_tab;
        g.params = ctx->poseidon_dev.as<PoseidonDev>();
        g.off[0] = L.off_ha; g.off[1] = L.off_hb; g.off[2] = L.off_hc;
        g.k = k; g.n = L.n; g.count = L.nn; g.chains = 3 * k;
        g.perms = (uint32_t)perms;
        g.form = 2;
        chain_batch_launch(ctx, g, true);
        ZK_HIP(hipMemcpyAsync(hs + ab_bytes + st_bytes, ds + ab_bytes + st_bytes, k * 3 * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    } else {
        SpongeBatchArgs g;
        g.states = reinterpret_cast<const Fr *>(ds + ab_bytes);
        g.z = d_tab;
        g.params = ctx->poseidon_dev.as<PoseidonDev>();
        g.off[0] = L.off_ha; g.off[1] = L.off_hb; g.off[2] = L.off_hc;
        g.perms = perms;
        g.lanes = k * 3 * perms;
        const size_t bx = (g.lanes + 63) / 64;
        ScopedKernelTimer kt(ctx, "wit_sponge_batch_kernel", (double)g.lanes);
        hipLaunchKernelGGL(wit_sponge_batch_kernel, dim3((unsigned)(bx < cap ? bx : cap)), dim3(64), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipEventRecord(e1, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));      // the staging is free again, and the assignments are whole
    drain.ok = true;
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (dev_ms) *dev_ms = ms;
    if (dev) memcpy(c.hashes, hs + ab_bytes + st_bytes, k * 3 * sizeof(Fr));
    out = std::move(wits);
}

// The k assignments of one round count on ctx->stream, under ctx's mutex: a | b and the z addresses go up in one copy out of the
// ctx's pinned staging, one launch, the k x 3 public inputs come back, one synchronisation.  The assignments share one allocation
// (WitnessDev::backing).  `pubs` (nullable) is written only when all of it succeeded; when this throws the stream has been drained.
void fibonacci_batch_assign(zkg16_ctx *ctx, const Fr &ca, const Fr &cb, const uint64_t *a, const uint64_t *b, size_t k,
                            std::vector<std::shared_ptr<WitnessDev>> &out, uint64_t *pubs, float *dev_ms) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t ab_bytes = up(k * 2 * sizeof(uint64_t)), tab_bytes = up(k * sizeof(Fr *)), pub_bytes = k * 3 * sizeof(Fr);
    const size_t cap = ctx->opt.matrix_batch_grid > 0 ? (size_t)ctx->opt.matrix_batch_grid : 65535;
    mbatch_staging_ensure(ctx, ab_bytes + tab_bytes + pub_bytes);
    auto backing = std::make_shared<DevBuf>(k * FIBONACCI_VARS * sizeof(Fr));
    std::vector<std::shared_ptr<WitnessDev>> wits(k);
    for (size_t i = 0; i < k; i++) {
        wits[i] = std::make_shared<WitnessDev>();
        wits[i]->n = FIBONACCI_VARS;
        wits[i]->backing = backing;
        wits[i]->z.p = backing->as<Fr>() + i * FIBONACCI_VARS;
        wits[i]->z.bytes = FIBONACCI_VARS * sizeof(Fr);
    }
    uint8_t *hs = static_cast<uint8_t *>(ctx->mbatch_host), *ds = ctx->mbatch_dev.as<uint8_t>();
    uint64_t *h_ab = reinterpret_cast<uint64_t *>(hs);
    Fr **h_tab = reinterpret_cast<Fr **>(hs + ab_bytes);
    for (size_t i = 0; i < k; i++) {
        h_ab[2 * i] = a[i];
        h_ab[2 * i + 1] = b[i];
        h_tab[i] = wits[i]->z.as<Fr>();
    }
    hipEvent_t e0, e1;
    ZK_HIP(hipEventCreate(&e0));
    struct EvGuard { hipEvent_t e; ~EvGuard() { (void)hipEventDestroy(e); } } g0{e0};
    ZK_HIP(hipEventCreate(&e1));
    EvGuard g1{e1};
    struct Drain { zkg16_ctx *c; bool ok = false; ~Drain() { if (!ok) (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    ZK_HIP(hipEventRecord(e0, ctx->stream));
    ZK_HIP(hipMemcpyAsync(ds, hs, ab_bytes + k * sizeof(Fr *), hipMemcpyHostToDevice, ctx->stream));
    {
        FibBatchArgs g;
        g.ab = reinterpret_cast<const uint64_t *>(ds);
        g.z = reinterpret_cast<Fr *const *>(ds + ab_bytes);
        g.pub = reinterpret_cast<Fr *>(ds + ab_bytes + tab_bytes);
        g.ca = ca; g.cb = cb;
        g.k = k;
        const size_t bx = (k + 63) / 64;
        ScopedKernelTimer kt(ctx, "wit_fibonacci_batch_kernel", (double)k);
        hipLaunchKernelGGL(wit_fibonacci_batch_kernel, dim3((unsigned)(bx < cap ? bx : cap)), dim3(64), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipMemcpyAsync(hs + ab_bytes + tab_bytes, ds + ab_bytes + tab_bytes, pub_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipEventRecord(e1, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));      // the staging is free again, and the assignments are whole
    drain.ok = true;
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (dev_ms) *dev_ms = ms;
    if (pubs) memcpy(pubs, hs + ab_bytes + tab_bytes, pub_bytes);
    out = std::move(wits);
}

// whether the elimination keeps a request's working matrix in LDS: n up to option "linear_elim_lds_max" (0 = LINEAR_ELIM_LDS_N)
bool linear_elim_in_lds(const zkg16_ctx *ctx, size_t n) {
    return n <= (size_t)(ctx->opt.linear_elim_lds_max > 0 ? ctx->opt.linear_elim_lds_max : LINEAR_ELIM_LDS_N);
}

// The k assignments of one size on ctx->stream, under ctx's mutex: a | b go up in one copy out of the ctx's pinned staging (8 bytes
// per input value; the assignments lie one after the other in one allocation, so no address table travels), the solve and the fill
// launch, the k x n solutions come back, one synchronisation.  `x` (nullable) is written only when all of it succeeded; when this
// throws the stream has been drained.  Option "linear_solver" = 0: no request has a zero diagonal entry, the entries have checked.
// 1: the elimination kernel takes the solve kernel's place and the k status words come back with x; a singular request throws
// LinearSingular after the synchronisation, nothing written.
void linear_batch_assign(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, size_t k,
                         std::vector<std::shared_ptr<WitnessDev>> &out, uint64_t *x, float *dev_ms) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const LinearDims d(n);
    const size_t vars = d.vars(), a_bytes = k * n * n * sizeof(uint64_t), in_bytes = a_bytes + k * n * sizeof(uint64_t);
    const size_t x_off = up(in_bytes), x_bytes = k * n * sizeof(Fr);
    const size_t cap = ctx->opt.matrix_batch_grid > 0 ? (size_t)ctx->opt.matrix_batch_grid : 65535;
    const bool elim = ctx->opt.linear_solver == 1, elim_lds = linear_elim_in_lds(ctx, n);
    const size_t st_bytes = elim ? k * sizeof(uint32_t) : 0;        // the status words lie behind x: one copy brings both back
    mbatch_staging_ensure(ctx, x_off + x_bytes + st_bytes);
    auto backing = std::make_shared<DevBuf>(k * vars * sizeof(Fr));
    std::vector<std::shared_ptr<WitnessDev>> wits(k);
    for (size_t i = 0; i < k; i++) {
        wits[i] = std::make_shared<WitnessDev>();
        wits[i]->n = vars;
        wits[i]->backing = backing;
        wits[i]->z.p = backing->as<Fr>() + i * vars;
        wits[i]->z.bytes = vars * sizeof(Fr);
    }
    uint8_t *hs = static_cast<uint8_t *>(ctx->mbatch_host), *ds = ctx->mbatch_dev.as<uint8_t>();
    memcpy(hs, a, a_bytes);
    memcpy(hs + a_bytes, b, in_bytes - a_bytes);
    hipEvent_t e0, e1;
    ZK_HIP(hipEventCreate(&e0));
    struct EvGuard { hipEvent_t e; ~EvGuard() { (void)hipEventDestroy(e); } } g0{e0};
    ZK_HIP(hipEventCreate(&e1));
    EvGuard g1{e1};
    struct Drain { zkg16_ctx *c; bool ok = false; ~Drain() { if (!ok) (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    ZK_HIP(hipEventRecord(e0, ctx->stream));
    ZK_HIP(hipMemcpyAsync(ds, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    LinearBatchArgs g;
    g.a = reinterpret_cast<const uint64_t *>(ds);
    g.b = reinterpret_cast<const uint64_t *>(ds + a_bytes);
    g.x = reinterpret_cast<Fr *>(ds + x_off);
    g.z = backing->as<Fr>();
    g.n = n; g.k = k; g.vars = vars;
    DevBuf elim_work;
    if (elim) {
        const unsigned blocks = (unsigned)(k < cap ? k : cap);
        const size_t small = (n + 1 + (n + 7) / 8) * sizeof(Fr), m_bytes = n * (n + 1) * sizeof(Fr), lds = small + (elim_lds ? m_bytes : 0);
        LinearElimArgs e;
        e.a = g.a; e.b = g.b; e.x = g.x;
        e.status = reinterpret_cast<uint32_t *>(ds + x_off + x_bytes);
        e.work = nullptr;
        e.n = n; e.k = k;
        if (!elim_lds) {
            elim_work.alloc(blocks * m_bytes);
            e.work = elim_work.as<Fr>();
        } else if (lds > 64 * 1024 && !ctx->lds_attr_linear_elim) {      // above the 64 KiB default dynamic-LDS cap
            ZK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(wit_linear_elim_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->lds_attr_linear_elim = true;
        }
        ScopedKernelTimer kt(ctx, "wit_linear_elim_kernel", (double)k * (double)n * (double)n * (double)n / 3);
        if (elim_lds) hipLaunchKernelGGL(wit_linear_elim_kernel<true>, dim3(blocks), dim3(LINEAR_ELIM_LANES), lds, ctx->stream, e);
        else hipLaunchKernelGGL(wit_linear_elim_kernel<false>, dim3(blocks), dim3(LINEAR_ELIM_LANES), lds, ctx->stream, e);
        ZK_HIP(hipGetLastError());
    } else {
        ScopedKernelTimer kt(ctx, "wit_linear_solve_kernel", (double)k * (double)n * (double)n / 2);
        hipLaunchKernelGGL(wit_linear_solve_kernel, dim3((unsigned)(k < cap ? k : cap)), dim3(LINEAR_LANES), n * sizeof(Fr), ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
    {
        const size_t bx = (k * vars + 255) / 256;
        ScopedKernelTimer kt(ctx, "wit_linear_fill_kernel", (double)k * (double)vars);
        hipLaunchKernelGGL(wit_linear_fill_kernel, dim3((unsigned)(bx < cap ? bx : cap)), dim3(256), 0, ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipMemcpyAsync(hs + x_off, ds + x_off, x_bytes + st_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipEventRecord(e1, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));      // the staging is free again, and the assignments are whole
    drain.ok = true;
    if (elim) {
        const uint32_t *st = reinterpret_cast<const uint32_t *>(hs + x_off + x_bytes);
        for (size_t i = 0; i < k; i++)
            if (st[i]) throw LinearSingular{i, (size_t)st[i] - 1};
    }
    float ms = 0;
    ZK_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (dev_ms) *dev_ms = ms;
    if (x) memcpy(x, hs + x_off, x_bytes);
    out = std::move(wits);
}

int witness_batch_register(zkg16_ctx *ctx, std::vector<std::shared_ptr<WitnessDev>> &wits, uint64_t *handles_out) {
    const size_t k = wits.size();
    const uint64_t first = ctx->next_handle.fetch_add(k);
    size_t put = 0;
    try {
        for (; put < k; put++) ctx->wits.put(first + put, std::move(wits[put]));
    } catch (const std::bad_alloc &) {          // all or nothing: what was registered is taken back
        for (size_t i = 0; i < put; i++) ctx->wits.erase(first + i);
        return ZKG16_ERR_OOM;
    }
    for (size_t i = 0; i < k; i++) handles_out[i] = first + i;
    return ZKG16_OK;
}

// The catch tail of the three zkg16_witness_*_batch entries below, called from their catch (...): the exception in flight -> its
// status, a HipError's text into ctx->last_error.  Anything else goes on as it would have.
static int witness_batch_status(zkg16_ctx *ctx) {
    try {
        throw;
    } catch (const HipError &e) {
        char buf[512];
        snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", e.what, hipGetErrorString(e.err), e.file, e.line);
        ctx->last_error = buf;
        (void)hipGetLastError();
        return e.err == hipErrorOutOfMemory ? ZKG16_ERR_OOM : ZKG16_ERR_HIP;
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
}

}  // namespace zk
#endif  // ZKG16_HOST_ONLY

extern "C" {

// Host-only half (no ctx, no GPU): the three native sponges of the matrix handler (matrix_proof.rs:110-115) with the state in
// front of every permutation.  states (nullable): 3 hashes x ceil(n^2 / 2) permutations x 3 Fr; hashes: hash_a, hash_b, hash_c.
int zkg16_matrix_sponge_states(size_t n, const uint64_t *a, const uint64_t *b, uint64_t *states, uint64_t hashes[12]) {
    if (!a || !b || !hashes || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    try {
        MatrixChains mc;
        mc.start(n, a, b, true);
        mc.join();
        for (int h = 0; h < 3; h++) {
            memcpy(hashes + 4 * h, mc.hash[h].l, 32);
            if (states) memcpy(states + (size_t)h * mc.perms * 12, mc.states[h].data(), mc.perms * 96);
        }
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

// The same for k requests of one size (a, b: k x n^2, request-major) on a pool of `threads` host threads (0 = 8; at most 16 and 3k):
// request i's states (nullable: k x 3 x perms x 3 Fr) and hashes (k x 3 Fr) are those of zkg16_matrix_sponge_states(n, a_i, b_i).
// On ZKG16_ERR_BAD_ARG nothing is written.
int zkg16_matrix_sponge_states_batch(size_t n, const uint64_t *a, const uint64_t *b, size_t k, int threads, uint64_t *states, uint64_t *hashes) {
    if (!a || !b || !hashes || k == 0 || n < 2 || n > 1024 || threads < 0) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / (3 * 96 * ((n * n + 1) / 2))) return ZKG16_ERR_BAD_ARG;       // the states of k requests have no size
    try {
        std::vector<Fr64> hs(3 * k);        // staged: an allocation failing half way leaves `hashes` alone
        matrix_chains_batch(n, a, b, k, threads, reinterpret_cast<Fr64 *>(states), hs.data());
        memcpy(hashes, hs.data(), 3 * k * sizeof(Fr64));
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

// k vectors of n Montgomery Fr each on the pool (no ctx, no GPU): out[i] is byte for byte zkg16_poseidon_hash(elems + 4 n i, n).
int zkg16_poseidon_hash_batch_host(const uint64_t *elems, size_t n, size_t k, int threads, uint64_t *out) {
    if (!elems || !out || n == 0 || k == 0 || threads < 0) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / 32 / n) return ZKG16_ERR_BAD_ARG;
    return hash_batch_host(false, elems, n, k, threads, out);
}
// k matrices of n^2 u64 (no ctx, no GPU): hashes[i] = hash_a of zkg16_matrix_sponge_states(n, m_i, .), what hash_matrix answers.
int zkg16_matrix_hash_batch_host(size_t n, const uint64_t *m, size_t k, int threads, uint64_t *hashes) {
    if (!m || !hashes || k == 0 || n < 2 || n > 1024 || threads < 0) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / 32 / (n * n)) return ZKG16_ERR_BAD_ARG;
    return hash_batch_host(true, m, n * n, k, threads, hashes);
}

#ifndef ZKG16_HOST_ONLY
// K MatrixCircuit assignments of one size in one upload, two launches and one synchronisation: handle i carries the bytes of
// zkg16_witness_matrix(n, a_i, b_i).  The chains run before the ctx is locked (option "matrix_batch_threads"); all or nothing: on
// any error no handle is registered and nothing is written.  timings_ms (nullable, 3): host chains (wall), device, whole call.
int zkg16_witness_matrix_batch(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, size_t k, uint64_t *witness_handles,
                               uint64_t *public_inputs, float *timings_ms) {
    if (!ctx || !a || !b || !witness_handles || k == 0 || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    const size_t total = MatrixWitnessLayout(n).total;
    if (total >= ((size_t)1 << 32)) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    if (k > SIZE_MAX / (total * sizeof(Fr))) return ZKG16_ERR_BAD_ARG;
    MatrixBatchChains mc;
    std::vector<uint64_t> hashes;
    try {
        hashes.resize(12 * k);
        if (sponge_chains_on_device(ctx, 3 * k)) matrix_batch_chains_device(mc, n, k, hashes.data());
        else matrix_batch_chains(mc, n, a, b, k, ctx->opt.matrix_batch_threads, hashes.data());
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    try {
        ZK_HIP(hipSetDevice(ctx->device));
        std::vector<std::shared_ptr<WitnessDev>> wits;
        float dev_ms = 0;
        matrix_batch_assign(ctx, mc, a, b, wits, &dev_ms);
        if (const int st = witness_batch_register(ctx, wits, witness_handles)) return st;
        if (public_inputs) memcpy(public_inputs, hashes.data(), 12 * k * sizeof(uint64_t));
        if (timings_ms) {
            timings_ms[0] = (float)mc.ms;
            timings_ms[1] = dev_ms;
            timings_ms[2] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        }
    } catch (...) {
        return witness_batch_status(ctx);
    }
    return ZKG16_OK;
}

// K FibonacciCircuit assignments of one round count in one upload, one launch and one synchronisation: handle i carries the bytes
// zkg16_circuit_export gives for (a[i], b[i], steps).  The two coefficients are formed before the ctx is locked; all or nothing: on
// any error no handle is registered and nothing is written.  timings_ms (nullable, 3): host coefficients, device, whole call.
int zkg16_witness_fibonacci_batch(zkg16_ctx *ctx, size_t steps, const uint64_t *a, const uint64_t *b, size_t k, uint64_t *witness_handles,
                                  uint64_t *public_inputs, float *timings_ms) {
    if (!ctx || !a || !b || !witness_handles || k == 0 || steps > ZKG16_FIBONACCI_STEPS_MAX) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / (FIBONACCI_VARS * sizeof(Fr))) return ZKG16_ERR_BAD_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    Fr ca, cb;
    fibonacci_coeffs(steps, ca, cb);
    const double coeff_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    std::lock_guard<std::mutex> lk(ctx->mu);
    try {
        ZK_HIP(hipSetDevice(ctx->device));
        std::vector<std::shared_ptr<WitnessDev>> wits;
        std::vector<uint64_t> pubs(12 * k);
        float dev_ms = 0;
        fibonacci_batch_assign(ctx, ca, cb, a, b, k, wits, pubs.data(), &dev_ms);
        if (const int st = witness_batch_register(ctx, wits, witness_handles)) return st;
        if (public_inputs) memcpy(public_inputs, pubs.data(), 12 * k * sizeof(uint64_t));
        if (timings_ms) {
            timings_ms[0] = (float)coeff_ms;
            timings_ms[1] = dev_ms;
            timings_ms[2] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        }
    } catch (...) {
        return witness_batch_status(ctx);
    }
    return ZKG16_OK;
}

// K linear-equation assignments of one size in one upload, two launches and one synchronisation: handle i carries the bytes
// zkg16_circuit_export gives for request i.  The diagonals are checked before the ctx is locked; all or nothing: on any error no
// handle is registered and nothing is written.  timings_ms (nullable, 3): host checks, device, whole call.
int zkg16_witness_linear_batch(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, size_t k, uint64_t *witness_handles,
                               uint64_t *x_out, float *timings_ms) {
    if (!ctx || !a || !b || !witness_handles || k == 0 || n == 0 || n > ZKG16_LINEAR_N_MAX) return ZKG16_ERR_BAD_ARG;
    if (k > SIZE_MAX / (LinearDims(n).vars() * sizeof(Fr))) return ZKG16_ERR_BAD_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    size_t bad_req = 0, bad_row = 0;
    const bool zero_diag = linear_zero_diagonal(n, a, k, &bad_req, &bad_row);
    const double check_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    std::lock_guard<std::mutex> lk(ctx->mu);
    try {
        if (zero_diag && ctx->opt.linear_solver == 0) {
            char buf[160];
            snprintf(buf, sizeof buf, "zkg16_witness_linear_batch: request %zu has a zero diagonal entry in row %zu", bad_req, bad_row);
            ctx->last_error = buf;
            return ZKG16_ERR_UNSUPPORTED;
        }
        ZK_HIP(hipSetDevice(ctx->device));
        std::vector<std::shared_ptr<WitnessDev>> wits;
        std::vector<uint64_t> xs(4 * k * n);
        float dev_ms = 0;
        linear_batch_assign(ctx, n, a, b, k, wits, xs.data(), &dev_ms);
        if (const int st = witness_batch_register(ctx, wits, witness_handles)) return st;
        if (x_out) memcpy(x_out, xs.data(), xs.size() * sizeof(uint64_t));
        if (timings_ms) {
            timings_ms[0] = (float)check_ms;
            timings_ms[1] = dev_ms;
            timings_ms[2] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        }
    } catch (const LinearSingular &e) {
        char buf[200];
        snprintf(buf, sizeof buf, "zkg16_witness_linear_batch: request %zu is singular: columns 0..%zu of a are linearly dependent (column %zu)", e.req, e.col, e.col);
        ctx->last_error = buf;
        return ZKG16_ERR_UNSUPPORTED;
    } catch (...) {
        return witness_batch_status(ctx);
    }
    return ZKG16_OK;
}

// The MatrixCircuit's full assignment for (a, b), built on the device: a witness handle as zkg16_witness_load would return for
// zkg16_circuit_matrix_witness's output.  public_inputs (nullable): hash_a, hash_b, hash_c (Montgomery), the handler's
// public inputs.  timings_ms (nullable, 3): host chains, upload + kernels (device time), whole call.
int zkg16_witness_matrix(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, uint64_t *witness_handle, uint64_t public_inputs[12],
                         float *timings_ms) {
    if (!a || !b || !witness_handle || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    if (!ctx) return ZKG16_ERR_BAD_ARG;
    const auto t_call = std::chrono::steady_clock::now();
    if (MatrixWitnessLayout(n).total >= ((size_t)1 << 32)) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    // the chains need neither the ctx nor the device: they run before the ctx is locked, so that other callers of this ctx are
    // not held up by the host arithmetic
    std::unique_ptr<MatrixWitnessStream, void (*)(MatrixWitnessStream *)> ms(nullptr, matrix_stream_free);
    try {
        ms.reset(matrix_stream_start(n, a, b, 1, 0, false));
        ms->mc.join();
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    try {
        ZK_HIP(hipSetDevice(ctx->device));
        auto w = std::make_unique<WitnessDev>();
        w->n = ms->L.total;
        w->z.alloc(ms->L.total * sizeof(Fr));
        hipEvent_t e0, e1;
        ZK_HIP(hipEventCreate(&e0));
        ZK_HIP(hipEventCreate(&e1));
        struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{e0, e1};
        ZK_HIP(hipEventRecord(e0, ctx->stream));
        const bool trace = getenv("ZKG16_TRACE_HOST") != nullptr;
        auto lap = [&](const char *what) {
            if (trace) fprintf(stderr, "witness_matrix: %s at %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count());
        };
        lap("locked, z allocated");
        matrix_stream_attach(ms.get(), ctx, w->z.as<Fr>(), 0);
        lap("attached");
        matrix_stream_produce(ms.get(), ctx, 0);
        lap("part 0 queued");
        matrix_stream_produce(ms.get(), ctx, 1);
        lap("part 1 queued");
        ZK_HIP(hipEventRecord(e1, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));      // the copies above read the stream object's host buffers
        float dev_ms = 0;
        ZK_HIP(hipEventElapsedTime(&dev_ms, e0, e1));
        if (public_inputs) matrix_stream_hashes(ms.get(), public_inputs);
        *witness_handle = ctx->next_handle++;
        ctx->wits.put(*witness_handle, std::move(w));
        if (timings_ms) {
            timings_ms[0] = (float)ms->mc.chain_ms;
            timings_ms[1] = dev_ms;
            timings_ms[2] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        }
    } catch (const HipError &e) {
        (void)hipStreamSynchronize(ctx->stream);
        char buf[512];
        snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", e.what, hipGetErrorString(e.err), e.file, e.line);
        ctx->last_error = buf;
        (void)hipGetLastError();
        return e.err == hipErrorOutOfMemory ? ZKG16_ERR_OOM : ZKG16_ERR_HIP;
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(ctx->stream);
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

// The slices zkg16_prove_matrix feeds the proof in at size n under options matrix_parts = parts_wanted and matrix_slice_min =
// slice_min: the choice matrix_stream_start makes (matrix_stream_slices), no ctx, no device.
int zkg16_matrix_stream_bounds(size_t n, int parts_wanted, int slice_min, uint32_t bounds_out[9], int *slices_out) {
    if (!bounds_out || !slices_out || n < 2 || n > 1024 || parts_wanted < 0 || parts_wanted > 8 || slice_min < 0 || slice_min > (1 << 20))
        return ZKG16_ERR_BAD_ARG;
    uint32_t bounds[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int k = matrix_stream_slices((n * n + POSEIDON_RATE - 1) / POSEIDON_RATE, parts_wanted, slice_min, bounds);
    memcpy(bounds_out, bounds, sizeof bounds);
    *slices_out = k;
    return ZKG16_OK;
}

// The streamed assignment alone, part by part, as zkg16_prove_matrix produces it (diagnostics for tests): the same start / attach /
// produce(k) calls under the ctx's matrix_parts and matrix_slice_min, on a buffer filled with 0xFF bytes first — an all-ones word is
// at least r, so no stored Fr equals the fill.  After every part the stream is drained and z read back: first_valid[i] = the first k
// after which entry i differs from the fill (255: never written).  Nothing runs but the production's own copies and kernels.
int zkg16_diag_matrix_stream(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, uint8_t *part_of_out, uint8_t *first_valid_out,
                             uint64_t *z_out, size_t n_assign, int *parts_out) {
    if (!ctx || !a || !b || !part_of_out || !first_valid_out || !z_out || !parts_out || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    const size_t total = MatrixWitnessLayout(n).total;
    if (n_assign != total) return ZKG16_ERR_BAD_ARG;
    if (total >= ((size_t)1 << 32)) return ZKG16_ERR_DOMAIN_TOO_LARGE;
    std::unique_ptr<MatrixWitnessStream, void (*)(MatrixWitnessStream *)> ms(nullptr, matrix_stream_free);
    std::vector<uint8_t> part_of, first;
    std::vector<Fr> z;
    int parts = 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    try {
        ms.reset(matrix_stream_start(n, a, b, ctx->opt.matrix_parts, ctx->opt.matrix_slice_min, ctx->opt.matrix_parts != 1));
        part_of.assign(total + 3, 0xFF);            // stays so when no map is built (matrix_parts = 1: the assignment first, then the proof)
        first.assign(total, 0xFF);
        z.resize(total);
        ZK_HIP(hipSetDevice(ctx->device));
        DevBuf d_z(total * sizeof(Fr));
        // the stream object's copies and kernels must not outlive it or d_z
        struct Drain { zkg16_ctx *c; ~Drain() { (void)hipStreamSynchronize(c->stream); } } drain{ctx};
        ZK_HIP(hipMemsetAsync(d_z.p, 0xFF, total * sizeof(Fr), ctx->stream));
        matrix_stream_attach(ms.get(), ctx, d_z.as<Fr>(), 3);
        parts = matrix_stream_parts(ms.get());
        for (int k = 0; k < parts; k++) {
            matrix_stream_produce(ms.get(), ctx, k);
            ZK_HIP(hipMemcpyAsync(z.data(), d_z.p, total * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
            ZK_HIP(hipStreamSynchronize(ctx->stream));
            for (size_t i = 0; i < total; i++) {
                if (first[i] != 0xFF) continue;
                bool fill = true;
                for (int l = 0; l < 8; l++) fill = fill && z[i].l[l] == 0xFFFFFFFFu;
                if (!fill) first[i] = (uint8_t)k;
            }
        }
        if (const uint8_t *d_part = matrix_stream_part_of(ms.get())) {
            ZK_HIP(hipMemcpyAsync(part_of.data(), d_part, total + 3, hipMemcpyDeviceToHost, ctx->stream));
            ZK_HIP(hipStreamSynchronize(ctx->stream));
        }
    } catch (const HipError &e) {
        char buf[512];
        snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", e.what, hipGetErrorString(e.err), e.file, e.line);
        ctx->last_error = buf;
        (void)hipGetLastError();
        return e.err == hipErrorOutOfMemory ? ZKG16_ERR_OOM : ZKG16_ERR_HIP;
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    memcpy(part_of_out, part_of.data(), total + 3);
    memcpy(first_valid_out, first.data(), total);
    memcpy(z_out, z.data(), total * sizeof(Fr));
    *parts_out = parts;
    return ZKG16_OK;
}
#endif  // ZKG16_HOST_ONLY

}  // extern "C"
