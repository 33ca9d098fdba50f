// TEST-ONLY: csrc/rerandomize_dev.cuh (the lane functions of rerandomize_g1_kernel, rerandomize_g2_kernel and compress_kernel) compiled
// for the host, so that every case of tests/rerandomize_cases.py can be compared with the points its logs say, and the compress lane
// with the host encoder, on a machine without a GPU.  Built by tests/rerandomize_cases.py with `hipcc --offload-host-only`;
// ZK_PD_CHECK turns on the value-bound assertions of the device pairing header.  Points cross this interface in saturated
// Montgomery limbs (u64, ark's order), scalars as 4 u64.
#define ZK_PD_CHECK 1
#include "rerandomize_dev.cuh"

#include <string.h>
using namespace zk;

extern "C" {

// the four canonical scalars of one proof: r1^-1, r2 (the G1 lane's) and r1, r1 r2 (the G2 lane's), 4 u64 each
void rr_scalars(const uint64_t *r1, const uint64_t *r2, uint64_t *out) {
    uint32_t k[4][8];
    rr::g1_scalars(rr::fr_load(r1), rr::fr_load(r2), k[0], k[1]);
    rr::g2_scalars(rr::fr_load(r1), rr::fr_load(r2), k[2], k[3]);
    memcpy(out, k, sizeof k);
}
// the G1 lane and the G2 lane of one proof as the kernels call them: proof 48 limbs, inf 3 flags -> out 48 limbs, out_inf 3 flags
void rr_g1_lane(const uint64_t *proof, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2, uint64_t *out, uint8_t *out_inf) {
    rr::proof_g1(proof, inf, r1, r2, out, out_inf);
}
void rr_g2_lane(const uint64_t *proof, const uint8_t *inf, const uint64_t *delta, const uint64_t *r1, const uint64_t *r2, uint64_t *out, uint8_t *out_inf) {
    G2Affine d;
    memcpy(&d, delta, sizeof d);
    rr::proof_g2(proof, inf, d, r1, r2, out, out_inf);
}
// the compress lane over n points: group 1 (12 limbs -> 48 bytes) or 2 (24 limbs -> 96 bytes); inf nullable
void rr_compress(int group, const uint64_t *points, const uint8_t *inf, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        if (group == 1) rr::g1_compress(points + 12 * i, inf && inf[i], out + 48 * i);
        else rr::g2_compress(points + 24 * i, inf && inf[i], out + 96 * i);
    }
}

}  // extern "C"
