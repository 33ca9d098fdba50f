// Batched Groth16 verification: what verify.hip (host arithmetic), verify_batch.hip (kernels), api_verify.hip and api_rerandomize.hip
// (entry points on a lane of the ctx) share.  K proofs under one prepared key hold iff, for multipliers rho_k nobody could predict (error 2^-128),
//
//     FE( prod_k ML(rho_k A_k, B_k) * ML(sum_k rho_k X_k, -gamma) * ML(sum_k rho_k C_k, -delta) ) == e(alpha, beta)^(sum_k rho_k)
//
// with X_k = gamma_abc[0] + sum_i z_{k,i} gamma_abc[i].  Per proof: three membership tests, one scalar multiplication by 128 bits and
// one Miller loop on an unprepared G2 point (host threads or one GPU lane each).  Per batch: two Miller loops on the key's prepared
// coefficients, one exponentiation of e(alpha, beta) and ONE final exponentiation (host).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <system_error>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "ec.cuh"

namespace zk {

struct VbKey {
    const uint64_t *gamma_abc_g1;
    size_t num_instance;
    const uint64_t *alpha_beta, *gamma_neg_coeffs, *delta_neg_coeffs;
    size_t n_coeffs;
};
struct VbBatch {
    const uint64_t *public_inputs;      // k x (num_instance - 1) x 4, Montgomery
    const uint64_t *proofs;             // k x 48
    const uint8_t *inf;                 // k x 3
    const uint64_t *rho;                // k x 2
    size_t k;
};
// Where the public inputs of a batch come from: the kind, the host pointers of that kind, and the device copies the later stages
// read, filled in once they are uploaded.
//   Limbs: public_inputs as in VbBatch (nullable when num_instance == 1).
//   Prime: K requests of one trapdoor under the extended key of 260 points (zkg16_prime_vk_extend); xs, js [k], and d_dig the
//          digests the inputs kernel made of them.
//   U64:   a key of num_instance >= 2 whose inputs are plain 64-bit values; values k x (num_instance - 1), row-major.
enum class VbKind { Limbs, Prime, U64 };
struct VbForm {
    VbKind kind = VbKind::Limbs;
    const uint64_t *public_inputs = nullptr;
    const uint64_t *xs = nullptr, *js = nullptr;
    const uint64_t *values = nullptr;
    const uint64_t *d_xs = nullptr, *d_js = nullptr, *d_values = nullptr;
    const uint32_t *d_dig = nullptr;
};
inline VbForm vb_limbs(const uint64_t *public_inputs) { return VbForm{VbKind::Limbs, public_inputs}; }
inline VbForm vb_prime(const uint64_t *xs, const uint64_t *js) { return VbForm{VbKind::Prime, nullptr, xs, js}; }
inline VbForm vb_u64(const uint64_t *values) { return VbForm{VbKind::U64, nullptr, nullptr, nullptr, values}; }
// The argument checks every entry point makes before any work, each caller naming what it has: the key and the form's inputs for
// k proofs (k == 0, a key the form does not fit and k >= 2^32 where the kernels index by 32 bits are refused here) ...
int vb_check_batch(const VbKey &key, const VbForm &form, size_t k);
// ... and k multipliers, for the entry points that take them; vb_check_batch comes first (it bounds k)
int vb_check_rho(const uint64_t *rho, size_t k);
// The form's inputs as k x (num_instance - 1) x 4 Montgomery limbs: the caller's own for Limbs, else made in `made`.  digests
// (Prime, nullable): k x 8 words as the inputs kernel writes them; null: hashed here (zkg16_prime_ext_inputs)
const uint64_t *vb_form_expand(const VbKey &key, const VbForm &form, size_t k, const uint32_t *digests, std::vector<uint64_t> &made);

// fn(lo, hi) over [0, n) on up to `threads` host threads (0 = 8), at least min_per items each; a thread that cannot be started runs inline
template <class Fn>
void vb_parallel(size_t n, int threads, size_t min_per, Fn fn) {
    size_t nt = threads <= 0 ? 8 : (size_t)threads;
    if (min_per && n / min_per < nt) nt = n / min_per;
    if (nt <= 1) { if (n) fn((size_t)0, n); return; }
    struct Joiner {
        std::vector<std::thread> th;
        ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
    } tg;
    const size_t per = (n + nt - 1) / nt;
    for (size_t t = 0; t < nt; t++) {
        const size_t lo = t * per, hi = std::min(n, lo + per);
        if (lo >= hi) break;
        auto job = [lo, hi, &fn] { fn(lo, hi); };
        try {
            tg.th.emplace_back(job);
        } catch (const std::system_error &) {
            job();
        }
    }
}

// ---- verify.hip
// The batch's verdicts from its per-proof parts: member[k] != 0 iff A_k, B_k, C_k passed membership; prod (nullable, 72 u64): the
// product of the member proofs' Miller values ML(rho_k A_k, B_k) in ark's tower order; sum_c: sum over the member proofs of rho_k C_k
// (12 u64 affine; *sum_c_inf != 0: the point at infinity) or null = computed here.  fetch_miller() returns the K Miller values
// (k x 72 u64 by proof index; anything for proofs that failed membership: they are left out); it is called at most once, and only
// when prod is null or when the batch equation fails and ok_each wants the culprits (the device form downloads them then).
// *ok = 1 iff every proof holds; ok_each (nullable): each proof's own verdict, found by bisecting over index ranges.
// ms (nullable): ms[0] += coefficients + the batch equation, ms[1] += bisecting (the fetch included).
// each (nullable): where bisecting stops paying.  find_bad counts its range tests; when `after` of them have been made and bad
// proofs are still not all named, every proof of a range that is still open goes to decide() in ONE call — verdict[j] != 0 iff
// proof idx[j] holds by itself (what zkg16_verify_prepared says of it) — and no further range test is made.  decide empty: bisect
// to the end, as the host form does.  range_tests: how many find_bad made (out).
// count_whole (the u64 entries): the test of the whole batch counts as the first range test, so after = 1 hands every member proof
// of a failed batch to decide() with no range test of bisecting made.
struct VbEach {
    std::function<void(const uint32_t *idx, size_t n, uint8_t *verdict)> decide;
    size_t after = 0;
    size_t range_tests = 0;
    bool count_whole = false;
};
// Where the public inputs come from when b.public_inputs is null (the prime form; num_instance = 260).  sums (nullable): the
// num_instance multiplier sums s_i = sum_k rho_k z_{k,i} (z_{k,0} = 1) over the member proofs as plain integers below r, 4 u64 each
// (vb_prime_sums_launch): the whole-batch test takes them instead of walking K x 259 inputs; s_0 is also summed here, and when the
// two differ the sums are not used and sums_refused is set (out).  expand(): the k x (num_instance - 1) x 4 Montgomery inputs,
// called at most once and only when a range test needs them (bisecting, or no sums).
// sum_x (nullable; the u64 form, any num_instance): sum_i s_i gamma_abc[i] of those very sums, taken by the ctx's G1 MSM with the
// device sums as scalars (12 u64 affine; *sum_x_inf != 0: the point at infinity).  The range that covers every member proof then
// walks neither the inputs nor num_instance scalar multiplications; s_0 is cross-checked all the same, and a refusal drops sum_x too.
struct VbInputs {
    const uint64_t *sums = nullptr;
    std::function<const uint64_t *()> expand;
    bool sums_refused = false;
    const uint64_t *sum_x = nullptr;
    const uint8_t *sum_x_inf = nullptr;
};
void vb_decide(const VbKey &key, const VbBatch &b, const uint8_t *member, const std::function<const uint64_t *()> &fetch_miller, const uint64_t *prod,
               const uint64_t *sum_c, const uint8_t *sum_c_inf, int threads, int *ok, uint8_t *ok_each, float ms[2], VbEach *each = nullptr,
               VbInputs *inputs = nullptr);
// the prime form's inputs on the host: digests (k x 8 words as the inputs kernel writes them = k x 32 digest bytes) ->
// out (k x 259 x 4, Montgomery): x, the 256 digest bits, n = the digest mod 2^20, j
void vb_prime_expand(const uint64_t *xs, const uint64_t *js, const uint32_t *digests, size_t k, uint64_t *out);
// the u64 form's inputs on the host: n plain 64-bit values -> out (n x 4, Montgomery)
void vb_u64_expand(const uint64_t *values, size_t n, uint64_t *out);
// everything on host threads (zkg16_verify_batch_host).  dead (nullable, k bytes): proofs counted as failing membership whatever
// their limbs say (zkg16_verify_batch_wire: a proof with a point that did not decode; its zero limbs would read as infinity)
void vb_host(const VbKey &key, const VbBatch &b, int threads, int *ok, uint8_t *ok_each, const uint8_t *dead = nullptr);
// k x 192 proof bytes (A 48 | B 96 | C 48) decoded on up to `threads` host threads (0 = 8) by the host decoders' rules:
// proofs k x 48, inf k x 3, status k x 3 (A, B, C); validate != 0 adds the subgroup test (status 5)
void vb_wire_decode_host(const uint8_t *proof_bytes, size_t k, int validate, int threads, uint64_t *proofs, uint8_t *inf, uint8_t *status);
// the endomorphism constants the host calibrated at start-up, saturated limbs, for the membership kernel
struct VbEndo {
    Fq beta;
    Fq2 cx, cy;
    int fast_g1, fast_g2;
};
VbEndo vb_endo();
// the Frobenius constants gamma_i = xi^(i (q-1)/6), i = 1..5, of the final exponentiation (pf::frob_coeffs), saturated limbs
struct VbFrob {
    Fq2 g[5];
};
VbFrob vb_frob();
// public inputs as the per-proof kernels read them: n Montgomery Fr (4 u64 each) -> canonical limbs
void vb_scalars_canonical(const uint64_t *mont, size_t n, uint64_t *out);

// ---- verify_batch.hip: launches on `st` (a stream of the calling lane); nothing synchronises
// n points at pts + i * stride (u64 units; 12 / 24 u64 each), flag bytes at inf + i * inf_stride (null: none at infinity):
// ok[i * ok_stride] = what zkg16_point_check says of point i (infinity passes)
void vb_membership_launch(hipStream_t st, int group, const uint64_t *pts, size_t stride, const uint8_t *inf, size_t inf_stride, size_t n, const VbEndo &en,
                          uint8_t *ok, size_t ok_stride);
// out[i] (72 u64) = ML(rho_i P_i, Q_i); rho (2 u64 per pair) null = no scaling; a pair with P or Q at infinity gives one
void vb_miller_launch(hipStream_t st, const uint64_t *g1, size_t g1_stride, const uint8_t *g1_inf, const uint64_t *g2, size_t g2_stride, const uint8_t *g2_inf,
                      size_t inf_stride, const uint64_t *rho, size_t n, uint64_t *out);
// n compressed points of one group (1: 48 bytes, 2: 96 bytes) at bytes + i * byte_stride -> affine Montgomery limbs at
// out + i * stride (u64 units), the infinity flag at inf[i * inf_stride] and the status of zkg16_g1_decompress / zkg16_g2_decompress
// at status[i * status_stride] (0 ok ... 5 not in the subgroup, only with validate; limbs zero for statuses 1 to 4).  The strides let
// the three points of k x 192 proof bytes land in the k x 48 limb array the launches above read
void vb_decompress_launch(hipStream_t st, int group, const uint8_t *bytes, size_t byte_stride, size_t n, int validate, const VbEndo &en, uint64_t *out,
                          size_t stride, uint8_t *inf, size_t inf_stride, uint8_t *status, size_t status_stride);
// the product of f[0 .. n) by a tree (log2 n rounds); f is only read, and f[k] counts as one where live[k] == 0 (live nullable).
// tmp: room for 2 * ((n + 1) / 2) * 72 u64.  Returns where the product (72 u64) will lie, inside tmp
const uint64_t *vb_product_launch(hipStream_t st, const uint64_t *f, const uint8_t *live, size_t n, uint64_t *tmp);

// ---- each proof's own verdict (pairing_each_dev.cuh)
// out[i] (72 u64) = the verifier's final exponentiation of f[i], bit-equal to zkg16_final_exp; out may be f
void vb_final_exp_launch(hipStream_t st, const uint64_t *f, size_t n, uint64_t *out);
// A prepared key as the per-proof kernels read it, one block of u32 words made on the host once per call (vb_each_key_words) and
// uploaded: e(alpha, beta) as it came (144 words), the 2 x 68 line triples of -gamma and -delta in the U-form (2 x 68 x 84) and
// gamma_abc as affine U-form points (num_instance x 28)
size_t vb_each_key_count(size_t num_instance);
void vb_each_key_words(const VbKey &key, uint32_t *out);
// room for one launch of n proofs: X_k (affine, U-form) with its flag and the Miller values
size_t vb_each_scratch_bytes(size_t n);
// verdict[j] = what zkg16_verify_prepared says of proof idx[j] (idx null: proof j), j < n, for proofs that passed membership:
// FE( ML(A, B) ML(X, -gamma) ML(C, -delta) ) == e(alpha, beta), a pair with a point at infinity counting as one.  proofs
// (k x 48 limbs) and inf (k x 3 flags) are indexed by proof; z (n x (num_instance - 1) x 4 canonical limbs) by position j.
// Three kernels: X_k, the three-pair Miller loop (one squaring per bit), the final exponentiation with the comparison
void vb_each_launch(hipStream_t st, const uint32_t *key_words, size_t num_instance, const uint32_t *idx, size_t n, const uint64_t *proofs, const uint8_t *inf,
                    const uint64_t *z, void *scratch, uint8_t *verdict);
// the last two of those kernels alone, on X_k made elsewhere: xk (2 n U-form coordinates, 14 words each) and have (n flags) by
// position j, as each_x_kernel and vb_u64_x_launch write them; scratch: room for vb_each_scratch_bytes(n)
void vb_each_tail_launch(hipStream_t st, const uint32_t *key_words, const uint32_t *idx, size_t n, const uint64_t *proofs, const uint8_t *inf, const void *xk,
                         const uint8_t *have, void *scratch, uint8_t *verdict);
size_t vb_each_x_bytes(size_t n);       // room for xk of n proofs (their flags lie elsewhere)
// where gamma_abc lies in a key block (u32 words from its start)
size_t vb_each_key_points_at();

// ---- the prime form's front (prime_inputs_dev.cuh): K prime requests of one trapdoor under the extended key of 260 points
// (zkg16_prime_vk_extend), whose 259 public inputs x, bit_0 .. bit_255, n, j all follow from the 16 bytes (x, j).  Device pointers
// request i < n: dig[8 i .. 8 i + 7] = SHA-256(le32(x_i + j_i)) as little-endian words, n_out[i] (nullable) = the digest mod 2^20,
// pub (nullable) + 257 * 4 * i = zkg16_prime_public_inputs(x_i, j_i)
void vb_prime_inputs_launch(hipStream_t st, const uint64_t *xs, const uint64_t *js, size_t n, uint32_t *dig, uint32_t *n_out, uint64_t *pub);
// sums (260 x 4 u64, plain integers, unreduced) = sum_k rho_k (1, x_k, bit_0 .. bit_255, n_k, j_k) over the proofs with live[k] != 0
// (live null: all k of them); dig from the launch above; partial: room for vb_prime_sums_blocks(k) x 260 x 4 u64.  k < 2^32
size_t vb_prime_sums_blocks(size_t k);
void vb_prime_sums_launch(hipStream_t st, const uint64_t *xs, const uint64_t *js, const uint32_t *dig, const uint64_t *rho, const uint8_t *live, size_t k,
                          uint64_t *partial, uint64_t *sums);
// z (n x 259 x 4 canonical limbs, what vb_each_launch reads) of the requests idx[0 .. n) (idx null: requests 0 .. n - 1)
void vb_prime_z_launch(hipStream_t st, const uint32_t *idx, size_t n, const uint64_t *xs, const uint64_t *js, const uint32_t *dig, uint64_t *z);

// ---- the u64 form's front (u64_inputs_dev.cuh): a key of any num_instance >= 2 whose m = num_instance - 1 public inputs are
// plain 64-bit values, values = k x m u64 row-major on the device
// sums ((m + 1) x 4 u64, plain integers, unreduced) = sum_k rho_k (1, values[k][0], .., values[k][m - 1]) over the proofs with
// live[k] != 0 (live null: all k of them); partial: room for vb_u64_sums_partial_words(k, m) u64.  k < 2^32.  Two kernels: a
// 256-lane block per (256 columns, slice of proofs), then one lane per column adding the slices
size_t vb_u64_sums_partial_words(size_t k, size_t m);
void vb_u64_sums_launch(hipStream_t st, const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t k, uint64_t *partial, uint64_t *sums);
// X_k = gamma_abc[0] + sum_c values[idx[j]][c] gamma_abc[1 + c] of the proofs idx[0 .. n) (idx null: rows 0 .. n - 1), written
// as each_x_kernel writes it: xk[2 j], xk[2 j + 1] affine in the U-form, have[j] = 0 for the point at infinity.  gamma_abc:
// num_instance affine U-form points as they lie in a key block (vb_each_key_words).  A proof is spread over
// L = u6::group_lanes(m) lanes, 64 / L proofs per wave
// n affine points (12 u64 each, saturated Montgomery limbs; all-zero = the point at infinity) as the kernel reads them, without the
// rest of a key block: vb_points_count(n) words.  vb_point_limbs: one X as the kernel wrote it (two U-form coordinates) -> 12 limbs
size_t vb_points_count(size_t n);
void vb_points_words(const uint64_t *pts, size_t n, uint32_t *out);
void vb_point_limbs(const void *xk, uint64_t out[12]);
void vb_u64_x_launch(hipStream_t st, const uint32_t *gamma_abc_words, size_t num_instance, const uint64_t *values, const uint32_t *idx, size_t n, void *xk,
                     uint8_t *have);

// ---- re-randomising (rerandomize_dev.cuh): A' = r1^-1 A, B' = r1 B + (r1 r2) delta, C' = C + r2 A
// n proofs on the device (48 limbs and 3 flags each, the flags as vb_flags leaves them or as the decode kernel wrote them), r1 / r2
// n x 4 Montgomery limbs, delta 24 limbs: the G2 kernel on st_g2 and the G1 kernel on st_g1 -> out (n x 48), out_inf (n x 3).
// st3 / mem3 (nullable, n x 3 each): decode statuses and membership verdicts; a proof with a bad one is left out (zero outputs)
void vb_rerandomize_launch(hipStream_t st_g1, hipStream_t st_g2, const uint64_t *proofs, const uint8_t *inf, const uint64_t *delta, const uint64_t *r1,
                           const uint64_t *r2, const uint8_t *st3, const uint8_t *mem3, size_t n, uint64_t *out, uint8_t *out_inf);
// n affine points of one group at pts + i * stride (u64 units), flags at inf + i * inf_stride (null: none at infinity) -> the
// bytes of zkg16_points_compress at out + i * byte_stride.  st3 / mem3 (nullable): as above, point i belonging to proof i; a proof
// left out gets zero bytes
void vb_compress_launch(hipStream_t st, int group, const uint64_t *pts, size_t stride, const uint8_t *inf, size_t inf_stride, size_t n, const uint8_t *st3,
                        const uint8_t *mem3, uint8_t *out, size_t byte_stride);
// the proofs [lo, hi) on the calling host thread, by the kernels' own arithmetic (inf nullable: no flag set)
void vb_rerandomize_host_range(const uint64_t *proofs, const uint8_t *inf, const uint64_t *delta, const uint64_t *r1, const uint64_t *r2, size_t lo, size_t hi,
                               uint64_t *out, uint8_t *out_inf);

}  // namespace zk
