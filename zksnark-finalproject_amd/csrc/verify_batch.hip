// The per-proof part of batched Groth16 verification on the device (verify_batch.hpp; arithmetic: pairing_dev.cuh).  One GPU lane
// per pair / per point, blocks of one wave: the work is a long chain of dependent Fq products per lane with nothing to share
// between lanes, so 65,536 pairs are one round with one wave per SIMD.
//
//   membership_kernel     curve equation + endomorphism subgroup test of n points of one group
//   miller_batch_kernel   (rho_i P_i when multipliers are given, back to affine, then) the Miller loop of (P_i, Q_i): 72 u64 each
//   fq12_product_kernel   one round of the product tree over Fq12 values
//   decompress_kernel     n compressed points of one group (48 / 96 wire bytes each) to affine Montgomery limbs (decompress_dev.cuh)
//   each_x_kernel         the prepared public input X of each listed proof, to affine (pairing_each_dev.cuh, as the two below)
//   each_miller_kernel    ML(A, B) ML(X, -gamma) ML(C, -delta) of each listed proof: one squaring per bit for the three pairs
//   final_exp_kernel      the final exponentiation of n Fq12 values, and (for the per-proof pass) the comparison with e(alpha, beta)
//   prime_inputs_kernel   the prime form's front (prime_inputs_dev.cuh): SHA-256(x + j) of each request, one GPU lane each
//   prime_rho_sums_kernel the 260 multiplier sums of the batch equation under the extended key: one 256-lane block per 128 proofs,
//                         lane t owning digest bit t (rho and the digest word are the same address for a whole wave), then
//   prime_sums_reduce_kernel  the blocks' partial sums added up, one lane per column — integer sums, so any order gives the same
//   prime_z_expand_kernel the 259 canonical scalars of each listed request, for each_x_kernel
//   u64_rho_sums_kernel   the u64 form's front (u64_inputs_dev.cuh): the multiplier sums of a slice of proofs, a 256-lane block per
//                         (256 columns, slice), lane t owning a column (a row's values are contiguous across the wave), then
//   u64_sums_reduce_kernel    the slices' partial sums added up, one lane per column
//   u64_x_kernel          the prepared input X of each listed proof from its row of 64-bit values: a proof spread over L lanes,
//                         each walking one shared-doubling chain over its columns, the L partial sums met through LDS
//   rerandomize_g1_kernel A' = r1^-1 A and C' = C + r2 A of each proof (rerandomize_dev.cuh, as the two below): one doubling chain, two
//                         accumulators, one inversion for both results
//   rerandomize_g2_kernel B' = r1 B + (r1 r2) delta of each proof: one interleaved ladder over {B, delta, B + delta}
//   compress_kernel       n affine points of one group to their 48 / 96 wire bytes
//
// Registers: a Miller lane's state is f (12 Fq = 168 dwords), T (84), Q and P (84) and the operation at hand; every Fq product is a
// call (ffu.cuh: fqu_mul_call), so what is live across it sits in the callee-saved registers or in scratch: 4,272 B of scratch
// per Miller lane at one wave per SIMD (profiles/kernel_resource_usage_r8_verify.txt).  DESIGN 2.7.1 states the figures, what
// LDS / inlined placement would change, and why the spill was left in.
#include "verify_batch.hpp"

#include <string.h>

#include "common.hpp"
#include "decompress_dev.cuh"
#include "pairing_dev.cuh"
#include "pairing_each_dev.cuh"
#include "prime_inputs_dev.cuh"
#include "rerandomize_dev.cuh"
#include "u64_inputs_dev.cuh"

namespace zk {
namespace {

__global__ __launch_bounds__(64) void membership_kernel(int group, const uint64_t *pts, size_t stride, const uint8_t *inf, size_t inf_stride, size_t n, VbEndo en,
                                                        uint8_t *ok, size_t ok_stride) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    bool good = true;
    if (!(inf && inf[i * inf_stride])) {
        if (group == 1) {
            const G1Affine p = *reinterpret_cast<const G1Affine *>(pts + i * stride);
            good = pd::g1_valid(p, fqu_from_sat(en.beta), en.fast_g1 != 0);
        } else {
            const G2Affine p = *reinterpret_cast<const G2Affine *>(pts + i * stride);
            good = pd::g2_valid(p, fq2u_from_sat(en.cx), fq2u_from_sat(en.cy), en.fast_g2 != 0);
        }
    }
    ok[i * ok_stride] = good ? 1 : 0;
}

__global__ __launch_bounds__(64) void miller_batch_kernel(const uint64_t *g1, size_t g1_stride, const uint8_t *g1_inf, const uint64_t *g2, size_t g2_stride,
                                                          const uint8_t *g2_inf, size_t inf_stride, const uint64_t *rho, size_t n, uint64_t *out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    bool one = (g1_inf && g1_inf[i * inf_stride]) || (g2_inf && g2_inf[i * inf_stride]);
    pd::F12 f = pd::f12_one();
    if (!one) {
        const G1Affine p = *reinterpret_cast<const G1Affine *>(g1 + i * g1_stride);
        const G2Affine q = *reinterpret_cast<const G2Affine *>(g2 + i * g2_stride);
        FqU px = fqu_from_sat(p.x), py = fqu_from_sat(p.y);
        if (rho) {
            const uint32_t *r = reinterpret_cast<const uint32_t *>(rho + 2 * i);
            const uint32_t k[4] = {r[0], r[1], r[2], r[3]};
            one = !pd::g1_scale128(px, py, k, px, py);
        }
        if (!one) f = pd::miller_loop(px, py, fq2u_from_sat(q.x), fq2u_from_sat(q.y));
    }
    Fq2 s[6];
    pd::f12_to_sat(f, s);
    Fq2 *o = reinterpret_cast<Fq2 *>(out + 72 * i);
#pragma unroll
    for (int t = 0; t < 6; t++) o[t] = s[t];
}

// out[j] = in[2j] * in[2j + 1] (the last one alone when n_in is odd); live (nullable): in[k] counts as one where live[k] == 0
__global__ __launch_bounds__(64) void fq12_product_kernel(const uint64_t *in, const uint8_t *live, size_t n_in, uint64_t *out) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (2 * j >= n_in) return;
    const bool have_a = !live || live[2 * j], have_b = 2 * j + 1 < n_in && (!live || live[2 * j + 1]);
    pd::F12 f = pd::f12_one();
    if (have_a) f = pd::f12_from_sat(reinterpret_cast<const Fq2 *>(in + 72 * (2 * j)));
    if (have_b) {
        const pd::F12 g = pd::f12_from_sat(reinterpret_cast<const Fq2 *>(in + 72 * (2 * j + 1)));
        f = have_a ? pd::mul(f, g) : g;
    }
    Fq2 s[6];
    pd::f12_to_sat(f, s);
    Fq2 *o = reinterpret_cast<Fq2 *>(out + 72 * j);
#pragma unroll
    for (int t = 0; t < 6; t++) o[t] = s[t];
}

// point i: bytes + i * byte_stride -> out + i * stride (u64 units: 12 / 24 limbs), inf[i * inf_stride], status[i * status_stride]
__global__ __launch_bounds__(64) void decompress_kernel(int group, const uint8_t *bytes, size_t byte_stride, size_t n, int validate, VbEndo en, uint64_t *out,
                                                        size_t stride, uint8_t *inf, size_t inf_stride, uint8_t *status, size_t status_stride) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *b = bytes + i * byte_stride;
    uint8_t fl = 0;
    int st;
    if (group == 1) {
        G1Affine p;
        st = dc::g1_decompress(b, validate != 0, en.beta, en.fast_g1 != 0, p, fl);
        *reinterpret_cast<G1Affine *>(out + i * stride) = p;
    } else {
        G2Affine p;
        st = dc::g2_decompress(b, validate != 0, en.cx, en.cy, en.fast_g2 != 0, p, fl);
        *reinterpret_cast<G2Affine *>(out + i * stride) = p;
    }
    inf[i * inf_stride] = fl;
    status[i * status_stride] = (uint8_t)st;
}

// ---- each proof's own verdict: three kernels (DESIGN 2.7.3 has the resource figures the split was decided from)
const size_t EACH_AB_WORDS = 144, EACH_ELL_WORDS = 84, EACH_COEFF_WORDS = 2 * 68 * EACH_ELL_WORDS, EACH_POINT_WORDS = 28;
static_assert(sizeof(pd::Ell) == EACH_ELL_WORDS * 4 && sizeof(Affine<FqU>) == EACH_POINT_WORDS * 4, "the key block's layout");

ZK_HD pd::Frob frob_u(const VbFrob &fr) {
    pd::Frob r;
#pragma unroll
    for (int i = 0; i < 5; i++) r.g[i] = fq2u_from_sat(fr.g[i]);
    return r;
}

// X of the proof at list position j: xk[2j], xk[2j + 1] affine in the U-form, have[j] = 0 for the point at infinity
__global__ __launch_bounds__(64) void each_x_kernel(const Affine<FqU> *gamma_abc, size_t num_instance, const uint64_t *z, size_t n, FqU *xk, uint8_t *have) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    FqU x = FqU::zero(), y = FqU::zero();
    const bool h = pd::prepared_input(gamma_abc, num_instance, z + 4 * (num_instance - 1) * j, x, y);
    xk[2 * j] = x;
    xk[2 * j + 1] = y;
    have[j] = h ? 1 : 0;
}

// out[j] (72 u64) = ML(A, B) ML(X, -gamma) ML(C, -delta) of proof idx[j] (idx null: proof j)
__global__ __launch_bounds__(64) void each_miller_kernel(const uint32_t *idx, size_t n, const uint64_t *proofs, const uint8_t *inf, const FqU *xk, const uint8_t *have,
                                                         const pd::Ell *gamma_neg, const pd::Ell *delta_neg, uint64_t *out) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    const size_t i = idx ? idx[j] : j;
    const pd::EachKey key{gamma_neg, delta_neg, nullptr};
    const pd::F12 f = pd::miller_one(proofs + 48 * i, inf + 3 * i, have[j] != 0, xk[2 * j], xk[2 * j + 1], key);
    Fq2 s[6];
    pd::f12_to_sat(f, s);
    Fq2 *o = reinterpret_cast<Fq2 *>(out + 72 * j);
#pragma unroll
    for (int t = 0; t < 6; t++) o[t] = s[t];
}

// the final exponentiation of f[j]; out (nullable): the value, 72 u64; verdict (nullable): verdict[j] = the value == want (72 u64)
__global__ __launch_bounds__(64) void final_exp_kernel(const uint64_t *f, size_t n, VbFrob fr, uint64_t *out, const uint64_t *want, uint8_t *verdict) {
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    const pd::F12 r = pd::final_exp(pd::f12_from_sat(reinterpret_cast<const Fq2 *>(f + 72 * j)), frob_u(fr));
    Fq2 s[6];
    pd::f12_to_sat(r, s);
    if (out) {
        Fq2 *o = reinterpret_cast<Fq2 *>(out + 72 * j);
#pragma unroll
        for (int t = 0; t < 6; t++) o[t] = s[t];
    }
    if (verdict) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(want), *v = reinterpret_cast<const uint32_t *>(s);
        uint32_t diff = 0;
        for (int t = 0; t < 144; t++) diff |= w[t] ^ v[t];
        verdict[j] = diff == 0 ? 1 : 0;
    }
}

// ---- the prime form's front (prime_inputs_dev.cuh)
// request i: dig[8 i ..] = its digest words, n_out[i] (nullable) = the digest mod 2^20, pub (nullable) + 257 * 4 * i = its 257
// Montgomery public inputs (zkg16_prime_public_inputs)
__global__ __launch_bounds__(64) void prime_inputs_kernel(const uint64_t *xs, const uint64_t *js, size_t n, uint32_t *dig, uint32_t *n_out, uint64_t *pub) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8];
    pi::prime_digest(xs[i], js[i], d);
    uint4 *o = reinterpret_cast<uint4 *>(dig + 8 * i);
    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
    if (n_out) n_out[i] = pi::digest_n(d);
    if (pub) pi::public_inputs_mont(xs[i], d, reinterpret_cast<Fr *>(pub + 4 * 257 * i));
}

// block b: the sums of the proofs [b * SUM_SLICE, min(k, (b + 1) * SUM_SLICE)) -> partial + b * 260 * 4 (every column written)
__global__ __launch_bounds__(256) void prime_rho_sums_kernel(const uint64_t *xs, const uint64_t *js, const uint32_t *dig, const uint64_t *rho, const uint8_t *live,
                                                             size_t k, uint64_t *partial) {
    const size_t lo = (size_t)blockIdx.x * pi::SUM_SLICE, hi = lo + pi::SUM_SLICE < k ? lo + pi::SUM_SLICE : k;
    const unsigned t = threadIdx.x;
    uint64_t bit[4], extra[4];
    pi::column_sums(t, xs, js, dig, rho, live, lo, hi, bit, extra);
    uint64_t *o = partial + (size_t)blockIdx.x * pi::EXT_INSTANCE * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) o[4 * (2 + t) + i] = bit[i];
    if (t < 4) {
        const unsigned c = pi::extra_column(t);
#pragma unroll
        for (int i = 0; i < 4; i++) o[4 * c + i] = extra[i];
    }
}

// sums[c] = sum over the blocks of partial[b][c], c < 260
__global__ __launch_bounds__(64) void prime_sums_reduce_kernel(const uint64_t *partial, size_t blocks, uint64_t *sums) {
    const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= pi::EXT_INSTANCE) return;
    uint64_t acc[4] = {0, 0, 0, 0};
    for (size_t b = 0; b < blocks; b++) pi::add256(acc, partial + (b * pi::EXT_INSTANCE + c) * 4);
#pragma unroll
    for (int i = 0; i < 4; i++) sums[4 * c + i] = acc[i];
}

// z + 4 * (259 * j + c) = scalar c of request idx[j] (idx null: request j), j < n: one lane per scalar
__global__ __launch_bounds__(256) void prime_z_expand_kernel(const uint32_t *idx, size_t n, const uint64_t *xs, const uint64_t *js, const uint32_t *dig, uint64_t *z) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * pi::EXT_INPUTS) return;
    const size_t j = g / pi::EXT_INPUTS, i = idx ? idx[j] : j;
    const unsigned c = (unsigned)(g % pi::EXT_INPUTS);
    ulonglong4 *o = reinterpret_cast<ulonglong4 *>(z + 4 * g);
    *o = make_ulonglong4(pi::ext_scalar(c, xs[i], js[i], dig + 8 * i), 0, 0, 0);
}

// ---- the u64 form's front (u64_inputs_dev.cuh)
// block (x, y): the columns [256 x, 256 x + 256) (column 0: sum rho; the last tile may be partial) over the proofs of slice y,
// [y * per, min(k, (y + 1) * per)) -> partial + (y * (m + 1) + column) * 4; every column of every slice is written
__global__ __launch_bounds__(256) void u64_rho_sums_kernel(const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t k, size_t per,
                                                           uint64_t *partial) {
    const size_t col = (size_t)blockIdx.x * u6::SUM_LANES + threadIdx.x;
    if (col > m) return;
    const size_t start = (size_t)blockIdx.y * per, lo = start < k ? start : k, hi = lo + per < k ? lo + per : k;
    uint64_t acc[4];
    u6::column_sum(col, values, m, rho, live, lo, hi, acc);
    uint64_t *o = partial + ((size_t)blockIdx.y * (m + 1) + col) * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = acc[i];
}

// sums[c] = sum over the slices of partial[y][c], c <= m
__global__ __launch_bounds__(64) void u64_sums_reduce_kernel(const uint64_t *partial, size_t slices, size_t m, uint64_t *sums) {
    const size_t c = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (c > m) return;
    uint64_t acc[4] = {0, 0, 0, 0};
    for (size_t y = 0; y < slices; y++) pi::add256(acc, partial + (y * (m + 1) + c) * 4);
#pragma unroll
    for (int i = 0; i < 4; i++) sums[4 * c + i] = acc[i];
}

// X of the proof at list position j (row idx[j] of values; idx null: row j), written as each_x_kernel writes it.  One wave per
// block; L (a power of two <= 64) lanes share a proof, 64 / L proofs a wave.  Lanes past the list keep the point at infinity and
// take part in the rounds (the barriers are the block's)
const unsigned X_POINT_WORDS = 56;
static_assert(sizeof(XYZZ<FqU>) == X_POINT_WORDS * 4, "a partial sum in LDS");
__global__ __launch_bounds__(64) void u64_x_kernel(const Affine<FqU> *gamma_abc, size_t m, const uint64_t *values, const uint32_t *idx, size_t n, unsigned L, FqU *xk,
                                                   uint8_t *have) {
    __shared__ uint32_t part_words[64 * X_POINT_WORDS];
    XYZZ<FqU> *part = reinterpret_cast<XYZZ<FqU> *>(part_words);
    const unsigned t = threadIdx.x, lane = t & (L - 1), per = 64 / L;
    const size_t j = (size_t)blockIdx.x * per + t / L;
    const bool active = j < n;
    XYZZ<FqU> acc = XYZZ<FqU>::inf();
    if (active) acc = u6::ladder(gamma_abc, m, values + m * (idx ? (size_t)idx[j] : j), lane, L);
    for (unsigned s = L >> 1; s; s >>= 1) {
        if (lane >= s && lane < 2 * s) part[t] = acc;
        __syncthreads();
        if (lane < s) xyzz_add(acc, part[t + s]);
        __syncthreads();
    }
    if (active && lane == 0) {
        FqU x = FqU::zero(), y = FqU::zero();
        const bool h = u6::finish(acc, gamma_abc[0], x, y);
        xk[2 * j] = x;
        xk[2 * j + 1] = y;
        have[j] = h ? 1 : 0;
    }
}

// ---- re-randomising (rerandomize_dev.cuh).  st3 / mem3 (nullable, 3 bytes a proof: the decode statuses and membership verdicts of
// the wire form): a proof with a status that is not zero or a verdict that is zero is left out; its outputs are zero
ZK_HD bool rr_left_out(const uint8_t *st3, const uint8_t *mem3, size_t i) {
    bool out = false;
    if (st3) out = out || st3[3 * i] || st3[3 * i + 1] || st3[3 * i + 2];
    if (mem3) out = out || !mem3[3 * i] || !mem3[3 * i + 1] || !mem3[3 * i + 2];
    return out;
}
// proof i: A', C' -> out + 48 i (+ 0, + 36), their flags -> out_inf + 3 i (+ 0, + 2)
__global__ __launch_bounds__(64) void rerandomize_g1_kernel(const uint64_t *proofs, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2, const uint8_t *st3,
                                                            const uint8_t *mem3, size_t n, uint64_t *out, uint8_t *out_inf) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (rr_left_out(st3, mem3, i)) {
        for (int t = 0; t < 12; t++) out[48 * i + t] = out[48 * i + 36 + t] = 0;
        out_inf[3 * i] = out_inf[3 * i + 2] = 0;
        return;
    }
    rr::proof_g1(proofs + 48 * i, inf + 3 * i, r1 + 4 * i, r2 + 4 * i, out + 48 * i, out_inf + 3 * i);
}
// proof i: B' -> out + 48 i + 12, its flag -> out_inf + 3 i + 1; delta: 24 u64 on the device
__global__ __launch_bounds__(64) void rerandomize_g2_kernel(const uint64_t *proofs, const uint8_t *inf, const uint64_t *delta, const uint64_t *r1, const uint64_t *r2,
                                                            const uint8_t *st3, const uint8_t *mem3, size_t n, uint64_t *out, uint8_t *out_inf) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (rr_left_out(st3, mem3, i)) {
        for (int t = 0; t < 24; t++) out[48 * i + 12 + t] = 0;
        out_inf[3 * i + 1] = 0;
        return;
    }
    rr::proof_g2(proofs + 48 * i, inf + 3 * i, *reinterpret_cast<const G2Affine *>(delta), r1 + 4 * i, r2 + 4 * i, out + 48 * i, out_inf + 3 * i);
}
// point i: pts + i * stride (u64 units), inf[i * inf_stride] (inf null: none at infinity) -> out + i * byte_stride (48 / 96 bytes);
// with st3 / mem3, point i belongs to proof i and a proof left out gets zero bytes
__global__ __launch_bounds__(64) void compress_kernel(int group, const uint64_t *pts, size_t stride, const uint8_t *inf, size_t inf_stride, size_t n,
                                                      const uint8_t *st3, const uint8_t *mem3, uint8_t *out, size_t byte_stride) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint8_t b[96];
    const int nb = group == 1 ? 48 : 96;
    if (rr_left_out(st3, mem3, i)) {
        for (int t = 0; t < nb; t++) b[t] = 0;
    } else {
        const bool at_inf = inf && inf[i * inf_stride];
        if (group == 1) rr::g1_compress(pts + i * stride, at_inf, b);
        else rr::g2_compress(pts + i * stride, at_inf, b);
    }
    uint8_t *o = out + i * byte_stride;
    for (int t = 0; t < nb; t++) o[t] = b[t];
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 63) / 64); }

}  // namespace

void vb_final_exp_launch(hipStream_t st, const uint64_t *f, size_t n, uint64_t *out) {
    if (!n) return;
    hipLaunchKernelGGL(final_exp_kernel, dim3(blocks_of(n)), dim3(64), 0, st, f, n, vb_frob(), out, (const uint64_t *)nullptr, (uint8_t *)nullptr);
    ZK_HIP(hipGetLastError());
}

size_t vb_each_key_count(size_t num_instance) { return EACH_AB_WORDS + EACH_COEFF_WORDS + EACH_POINT_WORDS * num_instance; }

void vb_each_key_words(const VbKey &key, uint32_t *out) {
    memcpy(out, key.alpha_beta, EACH_AB_WORDS * 4);
    pd::Ell *ell = reinterpret_cast<pd::Ell *>(out + EACH_AB_WORDS);
    for (int which = 0; which < 2; which++) {
        const uint64_t *src = which ? key.delta_neg_coeffs : key.gamma_neg_coeffs;
        for (size_t i = 0; i < 68; i++) {
            Fq2 c[3];
            memcpy(c, src + 36 * i, sizeof c);
            ell[68 * which + i] = pd::Ell{fq2u_from_sat(c[0]), fq2u_from_sat(c[1]), fq2u_from_sat(c[2])};
        }
    }
    Affine<FqU> *pts = reinterpret_cast<Affine<FqU> *>(out + EACH_AB_WORDS + EACH_COEFF_WORDS);
    for (size_t i = 0; i < key.num_instance; i++) {
        G1Affine p;
        memcpy(&p, key.gamma_abc_g1 + 12 * i, sizeof p);
        pts[i] = Affine<FqU>{fqu_from_sat(p.x), fqu_from_sat(p.y)};      // exact zeros stay exact: the point at infinity
    }
}

size_t vb_each_scratch_bytes(size_t n) { return n * (576 + 2 * sizeof(FqU) + 1); }

void vb_each_launch(hipStream_t st, const uint32_t *key_words, size_t num_instance, const uint32_t *idx, size_t n, const uint64_t *proofs, const uint8_t *inf,
                    const uint64_t *z, void *scratch, uint8_t *verdict) {
    if (!n) return;
    uint64_t *f = static_cast<uint64_t *>(scratch);
    FqU *xk = reinterpret_cast<FqU *>(f + 72 * n);
    uint8_t *have = reinterpret_cast<uint8_t *>(xk + 2 * n);
    const pd::Ell *ell = reinterpret_cast<const pd::Ell *>(key_words + EACH_AB_WORDS);
    const Affine<FqU> *gamma_abc = reinterpret_cast<const Affine<FqU> *>(key_words + EACH_AB_WORDS + EACH_COEFF_WORDS);
    hipLaunchKernelGGL(each_x_kernel, dim3(blocks_of(n)), dim3(64), 0, st, gamma_abc, num_instance, z, n, xk, have);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(each_miller_kernel, dim3(blocks_of(n)), dim3(64), 0, st, idx, n, proofs, inf, (const FqU *)xk, (const uint8_t *)have, ell, ell + 68, f);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(final_exp_kernel, dim3(blocks_of(n)), dim3(64), 0, st, (const uint64_t *)f, n, vb_frob(), (uint64_t *)nullptr,
                       reinterpret_cast<const uint64_t *>(key_words), verdict);
    ZK_HIP(hipGetLastError());
}

size_t vb_each_x_bytes(size_t n) { return n * 2 * sizeof(FqU); }
size_t vb_each_key_points_at() { return EACH_AB_WORDS + EACH_COEFF_WORDS; }

void vb_each_tail_launch(hipStream_t st, const uint32_t *key_words, const uint32_t *idx, size_t n, const uint64_t *proofs, const uint8_t *inf, const void *xk,
                         const uint8_t *have, void *scratch, uint8_t *verdict) {
    if (!n) return;
    uint64_t *f = static_cast<uint64_t *>(scratch);
    const pd::Ell *ell = reinterpret_cast<const pd::Ell *>(key_words + EACH_AB_WORDS);
    hipLaunchKernelGGL(each_miller_kernel, dim3(blocks_of(n)), dim3(64), 0, st, idx, n, proofs, inf, static_cast<const FqU *>(xk), have, ell, ell + 68, f);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(final_exp_kernel, dim3(blocks_of(n)), dim3(64), 0, st, (const uint64_t *)f, n, vb_frob(), (uint64_t *)nullptr,
                       reinterpret_cast<const uint64_t *>(key_words), verdict);
    ZK_HIP(hipGetLastError());
}

size_t vb_points_count(size_t n) { return EACH_POINT_WORDS * n; }
void vb_points_words(const uint64_t *pts, size_t n, uint32_t *out) {
    Affine<FqU> *o = reinterpret_cast<Affine<FqU> *>(out);
    for (size_t i = 0; i < n; i++) {
        G1Affine p;
        memcpy(&p, pts + 12 * i, sizeof p);
        o[i] = Affine<FqU>{fqu_from_sat(p.x), fqu_from_sat(p.y)};       // exact zeros stay exact: the point at infinity
    }
}
void vb_point_limbs(const void *xk, uint64_t out[12]) {
    const FqU *c = static_cast<const FqU *>(xk);
    const G1Affine p{fqu_to_sat(c[0]), fqu_to_sat(c[1])};
    memcpy(out, &p, sizeof p);
}

size_t vb_u64_sums_partial_words(size_t k, size_t m) { return u6::sum_slices(k) * (m + 1) * 4; }

void vb_u64_sums_launch(hipStream_t st, const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t k, uint64_t *partial, uint64_t *sums) {
    const size_t slices = u6::sum_slices(k);
    if (slices) {
        const dim3 grid((unsigned)((m + 1 + u6::SUM_LANES - 1) / u6::SUM_LANES), (unsigned)slices);
        hipLaunchKernelGGL(u64_rho_sums_kernel, grid, dim3(u6::SUM_LANES), 0, st, values, m, rho, live, k, u6::slice_len(k), partial);
        ZK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(u64_sums_reduce_kernel, dim3(blocks_of(m + 1)), dim3(64), 0, st, (const uint64_t *)partial, slices, m, sums);
    ZK_HIP(hipGetLastError());
}

void vb_u64_x_launch(hipStream_t st, const uint32_t *gamma_abc_words, size_t num_instance, const uint64_t *values, const uint32_t *idx, size_t n, void *xk,
                     uint8_t *have) {
    if (!n) return;
    const size_t m = num_instance - 1;
    const unsigned L = u6::group_lanes(m), per = 64 / L;
    hipLaunchKernelGGL(u64_x_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(64), 0, st, reinterpret_cast<const Affine<FqU> *>(gamma_abc_words), m, values, idx, n, L,
                       static_cast<FqU *>(xk), have);
    ZK_HIP(hipGetLastError());
}

void vb_prime_inputs_launch(hipStream_t st, const uint64_t *xs, const uint64_t *js, size_t n, uint32_t *dig, uint32_t *n_out, uint64_t *pub) {
    if (!n) return;
    hipLaunchKernelGGL(prime_inputs_kernel, dim3(blocks_of(n)), dim3(64), 0, st, xs, js, n, dig, n_out, pub);
    ZK_HIP(hipGetLastError());
}

size_t vb_prime_sums_blocks(size_t k) { return (k + pi::SUM_SLICE - 1) / pi::SUM_SLICE; }

void vb_prime_sums_launch(hipStream_t st, const uint64_t *xs, const uint64_t *js, const uint32_t *dig, const uint64_t *rho, const uint8_t *live, size_t k,
                          uint64_t *partial, uint64_t *sums) {
    const size_t blocks = vb_prime_sums_blocks(k);
    if (blocks) {
        hipLaunchKernelGGL(prime_rho_sums_kernel, dim3((unsigned)blocks), dim3(pi::SUM_LANES), 0, st, xs, js, dig, rho, live, k, partial);
        ZK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(prime_sums_reduce_kernel, dim3(blocks_of(pi::EXT_INSTANCE)), dim3(64), 0, st, (const uint64_t *)partial, blocks, sums);
    ZK_HIP(hipGetLastError());
}

void vb_prime_z_launch(hipStream_t st, const uint32_t *idx, size_t n, const uint64_t *xs, const uint64_t *js, const uint32_t *dig, uint64_t *z) {
    if (!n) return;
    hipLaunchKernelGGL(prime_z_expand_kernel, dim3((unsigned)((n * pi::EXT_INPUTS + 255) / 256)), dim3(256), 0, st, idx, n, xs, js, dig, z);
    ZK_HIP(hipGetLastError());
}

void vb_membership_launch(hipStream_t st, int group, const uint64_t *pts, size_t stride, const uint8_t *inf, size_t inf_stride, size_t n, const VbEndo &en,
                          uint8_t *ok, size_t ok_stride) {
    if (!n) return;
    hipLaunchKernelGGL(membership_kernel, dim3(blocks_of(n)), dim3(64), 0, st, group, pts, stride, inf, inf_stride, n, en, ok, ok_stride);
    ZK_HIP(hipGetLastError());
}

void vb_miller_launch(hipStream_t st, const uint64_t *g1, size_t g1_stride, const uint8_t *g1_inf, const uint64_t *g2, size_t g2_stride, const uint8_t *g2_inf,
                      size_t inf_stride, const uint64_t *rho, size_t n, uint64_t *out) {
    if (!n) return;
    hipLaunchKernelGGL(miller_batch_kernel, dim3(blocks_of(n)), dim3(64), 0, st, g1, g1_stride, g1_inf, g2, g2_stride, g2_inf, inf_stride, rho, n, out);
    ZK_HIP(hipGetLastError());
}

void vb_decompress_launch(hipStream_t st, int group, const uint8_t *bytes, size_t byte_stride, size_t n, int validate, const VbEndo &en, uint64_t *out,
                          size_t stride, uint8_t *inf, size_t inf_stride, uint8_t *status, size_t status_stride) {
    if (!n) return;
    hipLaunchKernelGGL(decompress_kernel, dim3(blocks_of(n)), dim3(64), 0, st, group, bytes, byte_stride, n, validate, en, out, stride, inf, inf_stride, status,
                       status_stride);
    ZK_HIP(hipGetLastError());
}

void vb_rerandomize_launch(hipStream_t st_g1, hipStream_t st_g2, const uint64_t *proofs, const uint8_t *inf, const uint64_t *delta, const uint64_t *r1,
                           const uint64_t *r2, const uint8_t *st3, const uint8_t *mem3, size_t n, uint64_t *out, uint8_t *out_inf) {
    if (!n) return;
    // the long kernel first
    hipLaunchKernelGGL(rerandomize_g2_kernel, dim3(blocks_of(n)), dim3(64), 0, st_g2, proofs, inf, delta, r1, r2, st3, mem3, n, out, out_inf);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(rerandomize_g1_kernel, dim3(blocks_of(n)), dim3(64), 0, st_g1, proofs, inf, r1, r2, st3, mem3, n, out, out_inf);
    ZK_HIP(hipGetLastError());
}

void vb_compress_launch(hipStream_t st, int group, const uint64_t *pts, size_t stride, const uint8_t *inf, size_t inf_stride, size_t n, const uint8_t *st3,
                        const uint8_t *mem3, uint8_t *out, size_t byte_stride) {
    if (!n) return;
    hipLaunchKernelGGL(compress_kernel, dim3(blocks_of(n)), dim3(64), 0, st, group, pts, stride, inf, inf_stride, n, st3, mem3, out, byte_stride);
    ZK_HIP(hipGetLastError());
}

void vb_rerandomize_host_range(const uint64_t *proofs, const uint8_t *inf, const uint64_t *delta, const uint64_t *r1, const uint64_t *r2, size_t lo, size_t hi,
                               uint64_t *out, uint8_t *out_inf) {
    G2Affine d;
    memcpy(&d, delta, sizeof d);
    for (size_t i = lo; i < hi; i++) {
        rr::proof_g1(proofs + 48 * i, inf ? inf + 3 * i : nullptr, r1 + 4 * i, r2 + 4 * i, out + 48 * i, out_inf + 3 * i);
        rr::proof_g2(proofs + 48 * i, inf ? inf + 3 * i : nullptr, d, r1 + 4 * i, r2 + 4 * i, out + 48 * i, out_inf + 3 * i);
    }
}

const uint64_t *vb_product_launch(hipStream_t st, const uint64_t *f, const uint8_t *live, size_t n, uint64_t *tmp) {
    const size_t half = (n + 1) / 2;
    uint64_t *buf[2] = {tmp, tmp + 72 * half};
    const uint64_t *in = f;
    int w = 0;
    // one round at least, also for n == 1: it is the round that replaces the factors of dead proofs by one
    do {
        const size_t n_out = (n + 1) / 2;
        hipLaunchKernelGGL(fq12_product_kernel, dim3(blocks_of(n_out)), dim3(64), 0, st, in, live, n, buf[w]);
        ZK_HIP(hipGetLastError());
        in = buf[w];
        live = nullptr;
        w ^= 1;
        n = n_out;
    } while (n > 1);
    return in;
}

}  // namespace zk
