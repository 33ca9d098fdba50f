// TEST-ONLY: csrc/prime_inputs_dev.cuh (the lane functions of prime_inputs_kernel, prime_rho_sums_kernel, prime_sums_reduce_kernel
// and prime_z_expand_kernel) compiled for the host, so that digests, sums and scalars can be compared with hashlib and Python
// integers on a machine without a GPU.  Built by tests/prime_verify_cases.py with `hipcc --offload-host-only`.
#include "prime_inputs_dev.cuh"

#include <string.h>

#include <vector>
using namespace zk;

extern "C" {

// the inputs kernel's lane: digest (32 bytes) and n of one request
void pi_digest(uint64_t x, uint64_t j, uint8_t digest[32], uint32_t *n) {
    uint32_t d[8];
    pi::prime_digest(x, j, d);
    memcpy(digest, d, 32);
    *n = pi::digest_n(d);
}

// ... with the 257 Montgomery public inputs (257 x 4 u64)
void pi_public_inputs(uint64_t x, uint64_t j, uint64_t *out) {
    uint32_t d[8];
    pi::prime_digest(x, j, d);
    pi::public_inputs_mont(x, d, reinterpret_cast<Fr *>(out));
}

// The two sums kernels as they are launched: one block of SUM_LANES lanes per SUM_SLICE proofs writing every column of its partial,
// then one lane per column adding the partials up.  sums: 260 x 4 u64
void pi_rho_sums(const uint64_t *xs, const uint64_t *js, const uint64_t *rho, const uint8_t *live, size_t k, uint64_t *sums) {
    std::vector<uint32_t> dig(8 * k + 8);
    for (size_t i = 0; i < k; i++) pi::prime_digest(xs[i], js[i], dig.data() + 8 * i);
    const size_t blocks = (k + pi::SUM_SLICE - 1) / pi::SUM_SLICE;
    std::vector<uint64_t> partial(blocks * pi::EXT_INSTANCE * 4 + 4, 0xA5A5A5A5A5A5A5A5ull);      // as unwritten device memory: not zero
    for (size_t b = 0; b < blocks; b++) {
        const size_t lo = b * pi::SUM_SLICE, hi = lo + pi::SUM_SLICE < k ? lo + pi::SUM_SLICE : k;
        uint64_t *o = partial.data() + b * pi::EXT_INSTANCE * 4;
        for (unsigned t = 0; t < pi::SUM_LANES; t++) {
            uint64_t bit[4], extra[4];
            pi::column_sums(t, xs, js, dig.data(), rho, live, lo, hi, bit, extra);
            memcpy(o + 4 * (2 + t), bit, 32);
            if (t < 4) memcpy(o + 4 * pi::extra_column(t), extra, 32);
        }
    }
    for (size_t c = 0; c < pi::EXT_INSTANCE; c++) {
        uint64_t acc[4] = {0, 0, 0, 0};
        for (size_t b = 0; b < blocks; b++) pi::add256(acc, partial.data() + (b * pi::EXT_INSTANCE + c) * 4);
        memcpy(sums + 4 * c, acc, 32);
    }
}

// the expand kernel's lane: scalar c (< 259) of one request
uint64_t pi_ext_scalar(unsigned c, uint64_t x, uint64_t j) {
    uint32_t d[8];
    pi::prime_digest(x, j, d);
    return pi::ext_scalar(c, x, j, d);
}

}  // extern "C"
