// TEST-ONLY: csrc/r1cs_check_dev.cuh (the lane function and the block reduction of r1cs_check_kernel) compiled for the host, so that
// verdicts can be compared with Python integers on a machine without a GPU.  Built by tests/r1cs_check_cases.py with
// `hipcc --offload-host-only`.
#include "r1cs_check_dev.cuh"

#include <string.h>

#include <vector>
using namespace zk;

extern "C" {

// the kernel's lane: a, b, c as 4 u64 limbs each -> 1 when the row fails
int rck_row_fails(const uint64_t *a, const uint64_t *b, const uint64_t *c) {
    Fr x, y, z;
    memcpy(&x, a, 32);
    memcpy(&y, b, 32);
    memcpy(&z, c, 32);
    return rck::row_fails(x, y, z) ? 1 : 0;
}

// The two kernels as they are launched on nvec vectors of `stride` elements: the init lanes over result words that start as
// unwritten memory, then one block of rck::BLOCK lanes per rck::BLOCK rows and vector — lanes at or beyond nc vote "fine" without
// loading — each folding its four ballots and merging only when a row failed.  order 0: blocks in launch order, 1: last block
// first (the atomics make the words independent of it).  res: n_bad[nvec] | first_bad[nvec]
void rck_walk(const uint64_t *a, const uint64_t *b, const uint64_t *c, size_t stride, size_t nc, unsigned nvec, int order, uint64_t *res) {
    std::vector<uint64_t> words(2 * (size_t)nvec + 2, 0xA5A5A5A5A5A5A5A5ull);      // as unwritten device memory: not zero
    const unsigned init_lanes = (2 * nvec + 255) / 256 * 256;
    for (unsigned t = 0; t < init_lanes; t++)
        if (t < 2 * nvec) words[t] = rck::result_init(t, nvec);
    const size_t blocks = (nc + rck::BLOCK - 1) / rck::BLOCK;
    for (unsigned v = 0; v < nvec; v++)
        for (size_t q = 0; q < blocks; q++) {
            const size_t blk = order ? blocks - 1 - q : q, row0 = blk * rck::BLOCK;
            uint64_t ballots[rck::WAVES];
            for (unsigned w = 0; w < rck::WAVES; w++) ballots[w] = 0;
            for (unsigned t = 0; t < rck::BLOCK; t++) {
                const size_t i = row0 + t;
                bool bad = false;
                if (i < nc) {
                    const size_t at = (size_t)v * stride + i;
                    bad = rck_row_fails(a + 4 * at, b + 4 * at, c + 4 * at) != 0;
                }
                if (bad) ballots[t >> 6] |= (uint64_t)1 << (t & 63u);
            }
            uint64_t count, first;
            if (rck::block_fold(ballots, row0, count, first)) rck::result_merge(words[v], words[nvec + v], count, first);
        }
    memcpy(res, words.data(), 2 * (size_t)nvec * sizeof(uint64_t));
}

}  // extern "C"
