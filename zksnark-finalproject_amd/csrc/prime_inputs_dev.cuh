// The front of batched prime verification (verify_batch.hpp: the prime form): everything that differs between two prime requests
// of one trapdoor is a function of (x, j), so under the extended key (the template's 258 gamma_abc_g1 points, then V_n, then -V_j)
// request k has the 259 short public inputs  x_k, bit_0 .. bit_255 of SHA-256(x_k + j_k), n_k = the digest mod 2^20, j_k.
// Here: the lane functions of the three kernels of verify_batch.hip that make those inputs and their multiplier sums on the device
// from 16 bytes per request.  All of it is integer arithmetic on u32 / u64, ZK_HD, so tests/csrc/prime_inputs_host_shim.hip runs the
// same functions on the host.
//
//   prime_digest     x + j (at most 65 bits) as 32 little-endian bytes, one SHA-256 compression of that single padded block
//   column_sums      what one lane of a 256-lane block adds up over a slice of proofs: sum rho_k over the proofs whose digest bit t
//                    is set, and for t < 4 one of sum rho_k, sum rho_k x_k, sum rho_k n_k, sum rho_k j_k — plain integers in 4 u64:
//                    rho < 2^128, x and j < 2^64, K < 2^32, so every sum stays below 2^224 and nothing is reduced on the device
//   ext_scalar       the c-th of a request's 259 scalars as the per-proof kernels read them (canonical, all below 2^64)
#pragma once
#include <stddef.h>

#include "ff.cuh"

namespace zk {
namespace pi {

constexpr size_t EXT_INPUTS = 259, EXT_INSTANCE = 260, SUM_SLICE = 128;
constexpr unsigned SUM_LANES = 256;

ZK_HD uint32_t rotr(uint32_t v, int s) { return (v >> s) | (v << (32 - s)); }
ZK_HD uint32_t bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
ZK_HD constexpr uint32_t sha_k(int i) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K[i];
}

// d[i] = bytes 4i .. 4i + 3 of SHA-256(le32(x + j)) as a little-endian word: bit t of the digest (bit t & 7 of byte t >> 3, the order
// of the circuit's public inputs) is bit t & 31 of d[t >> 5], and the digest mod 2^20 is d[0] & 0xFFFFF
ZK_HD void prime_digest(uint64_t x, uint64_t j, uint32_t d[8]) {
    const uint64_t lo = x + j;
    const uint32_t carry = lo < x ? 1u : 0u;
    // the one block: 32 message bytes (the sum's nine low bytes, then zeros), 0x80, zeros, the bit length 256 — as big-endian words
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
    w[0] = bswap((uint32_t)lo);
    w[1] = bswap((uint32_t)(lo >> 32));
    w[2] = carry << 24;
    w[8] = 0x80000000u;
    w[15] = 256;
    const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint32_t a = iv[0], b = iv[1], c = iv[2], dd = iv[3], e = iv[4], f = iv[5], g = iv[6], h = iv[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + sha_k(i) + w[i & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = dd + t1; dd = c; c = b; b = a; a = t1 + t2;
    }
    d[0] = bswap(iv[0] + a); d[1] = bswap(iv[1] + b); d[2] = bswap(iv[2] + c); d[3] = bswap(iv[3] + dd);
    d[4] = bswap(iv[4] + e); d[5] = bswap(iv[5] + f); d[6] = bswap(iv[6] + g); d[7] = bswap(iv[7] + h);
}
ZK_HD uint32_t digest_n(const uint32_t d[8]) { return d[0] & 0xFFFFFu; }
ZK_HD uint32_t digest_bit(const uint32_t *d, unsigned t) { return (d[t >> 5] >> (t & 31)) & 1u; }

// zkg16_prime_public_inputs on the lane: x, then the 256 digest bits, Montgomery
ZK_HD void public_inputs_mont(uint64_t x, const uint32_t d[8], Fr *out) {
    Fr c = Fr::zero();
    c.l[0] = (uint32_t)x;
    c.l[1] = (uint32_t)(x >> 32);
    out[0] = fp_to_mont(c);
    const Fr one = Fr::one(), zero = Fr::zero();
    for (unsigned t = 0; t < 256; t++) out[1 + t] = digest_bit(d, t) ? one : zero;
}

// ---- 256-bit plain integers in 4 u64 (no modulus: the bounds above keep every sum inside them)
// acc += a (4 u64)
ZK_HD void add256(uint64_t acc[4], const uint64_t a[4]) {
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t s = acc[i] + a[i], t = s + carry;
        carry = (uint64_t)(s < a[i]) + (uint64_t)(t < s);
        acc[i] = t;
    }
}
// a * b = hi : lo, by 32-bit halves (the same code for the host and the device)
ZK_HD void mul64(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    lo = (mid << 32) | (uint32_t)p00;
    hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
// acc += (rho_hi : rho_lo) * m
ZK_HD void add_mul(uint64_t acc[4], uint64_t rho_lo, uint64_t rho_hi, uint64_t m) {
    uint64_t l0, h0, l1, h1;
    mul64(rho_lo, m, l0, h0);
    mul64(rho_hi, m, l1, h1);
    const uint64_t mid = h0 + l1;
    const uint64_t p[4] = {l0, mid, h1 + (uint64_t)(mid < h0), 0};      // h1 <= 2^64 - 2: the carry fits
    add256(acc, p);
}

// which of the 260 sums lane t's second accumulator is (t < 4): s_0 = sum rho, s_1 = sum rho x, s_258 = sum rho n, s_259 = sum rho j
ZK_HD unsigned extra_column(unsigned t) { return t == 0 ? 0u : t == 1 ? 1u : 256u + t; }

// Lane t (< 256) of the block that owns the proofs [lo, hi): bit = sum of rho_k over the live proofs whose digest bit t is set
// (column 2 + t); extra = column extra_column(t) for t < 4 (untouched zeros otherwise).  dig: 8 words per proof (prime_digest);
// rho: 2 u64 per proof; live (nullable): proofs with live[k] == 0 are left out
ZK_HD void column_sums(unsigned t, const uint64_t *xs, const uint64_t *js, const uint32_t *dig, const uint64_t *rho, const uint8_t *live, size_t lo, size_t hi,
                       uint64_t bit[4], uint64_t extra[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) bit[i] = extra[i] = 0;
    for (size_t k = lo; k < hi; k++) {
        if (live && !live[k]) continue;
        const uint64_t r[4] = {rho[2 * k], rho[2 * k + 1], 0, 0};
        const uint32_t *d = dig + 8 * k;
        if (digest_bit(d, t)) add256(bit, r);
        if (t < 4) {
            const uint64_t m = t == 0 ? 1 : t == 1 ? xs[k] : t == 2 ? (uint64_t)digest_n(d) : js[k];
            add_mul(extra, r[0], r[1], m);
        }
    }
}

// the c-th (c < 259) scalar of a request under the extended key: x, bit_0 .. bit_255, n, j
ZK_HD uint64_t ext_scalar(unsigned c, uint64_t x, uint64_t j, const uint32_t *d) {
    return c == 0 ? x : c <= 256 ? (uint64_t)digest_bit(d, c - 1) : c == 257 ? (uint64_t)digest_n(d) : j;
}

}  // namespace pi
}  // namespace zk
