// TEST-ONLY: csrc/trapdoor_dev.cuh (what trapdoor_dot_kernel runs: the lane body and the fold step) compiled for the host, so that a
// block's schedule can be driven lane by lane on a machine without a GPU and compared with Python sums.  Built by
// tests/trapdoor_cases.py with `hipcc --offload-host-only`.  Values cross in Montgomery u64 limbs (ark's order).
#include "ff.cuh"
#include <string.h>
#include <vector>
using namespace zk;

namespace {
#include "trapdoor_dev.cuh"
}  // namespace

extern "C" {

unsigned td_block(void) { return TD_BLOCK; }
unsigned td_chunk(void) { return TD_CHUNK; }

// The kernel's grid for one request on TD_BLOCK simulated lanes per block: every lane's four sums, the LDS tree (step = TD_BLOCK / 2,
// .., 1: lane t takes lane t + step in), lane 0's four values to partial_out[chunk][4], then the sum over the chunks to sums_out[4].
// Returns the number of chunks.
size_t td_dot_lanes(size_t nv, size_t ni, const uint64_t *z, const uint64_t *u, const uint64_t *v, const uint64_t *w, const uint64_t *lg,
                    uint64_t *partial_out, uint64_t *sums_out) {
    const Fr *zf = reinterpret_cast<const Fr *>(z), *uf = reinterpret_cast<const Fr *>(u), *vf = reinterpret_cast<const Fr *>(v),
             *wf = reinterpret_cast<const Fr *>(w), *lf = reinterpret_cast<const Fr *>(lg);
    const size_t chunks = (nv + TD_CHUNK - 1) / TD_CHUNK;
    Fr total[4] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
    std::vector<TdSums> lane(TD_BLOCK);
    for (size_t c = 0; c < chunks; c++) {
        for (unsigned t = 0; t < TD_BLOCK; t++) lane[t] = td_lane_sums(zf, uf, vf, wf, lf, nv, ni, c, t);
        for (int j = 0; j < 4; j++) {
            std::vector<Fr> part(TD_BLOCK);
            for (unsigned t = 0; t < TD_BLOCK; t++) part[t] = lane[t].s[j];
            for (unsigned step = TD_BLOCK / 2; step >= 1; step >>= 1)
                for (unsigned t = 0; t < step; t++) part[t] = td_fold_step(part[t], part[t + step]);
            memcpy(partial_out + (c * 4 + j) * 4, &part[0], sizeof(Fr));
            total[j] = fp_add(total[j], part[0]);
        }
    }
    memcpy(sums_out, total, sizeof total);
    return chunks;
}

}  // extern "C"
