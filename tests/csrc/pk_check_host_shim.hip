// TEST-ONLY: csrc/pk_check_dev.cuh (the lane functions of pk_check_g1_kernel and pk_check_g2_kernel) compiled for the host, so that
// every case of tests/pk_check_cases.py can be compared with zkg16_point_check on a machine without a GPU.  Built by
// tests/pk_check_cases.py with `hipcc --offload-host-only`; ZK_FQU_CHECK turns on the operand-bound assertions of ffu.cuh, which
// every product and subtraction of the header goes through.  Points cross this interface in saturated Montgomery limbs (u64, ark's
// order); the shim lays them out as a resident query: U-form entries at a byte stride, the padding behind an entry filled with a
// byte of the caller's choice.
#define ZK_FQU_CHECK 1
#define ZK_PKC_LANES_ONLY 1
#include "ff.cuh"
#include "ec.cuh"
#include "pk_check_dev.cuh"
#include "hostff.hpp"
#include <string.h>
#include <vector>
using namespace zk;

namespace {
#include "final_exp.inc"
const uint64_t Z_ABS = 0xd201000000010000ULL;
struct Fq12 { Fq2 c[6]; };
#include "pairing_fast.inc"
}  // namespace

extern "C" {

// whether the start-up calibration gave the endomorphism constants of the group (1 / 2): the fast route can be tested
int pkc_fast_available(int group) {
    const pf::Endo &en = pf::endo();
    return (group == 1 ? en.fast_g1 : en.fast_g2) ? 1 : 0;
}
// good[i] = the lane verdict of point i of n points of one group (12 / 24 u64 each; inf nullable: a flagged point is stored as
// (0, 0), as upload_points does), laid out at `stride` bytes (>= 112 / 224) with `filler` in every byte behind an entry's two
// coordinates.  fast != 0: the endomorphism test with the host's calibrated constants; 0: the ladder by r.  Returns 0, or -1 for
// arguments the layout cannot hold
int pkc_lanes(int group, const uint64_t *points, const uint8_t *inf, size_t n, size_t stride, int fast, int filler, uint8_t *good) {
    const size_t entry = group == 1 ? sizeof(G1AffineU) : sizeof(G2AffineU);
    if ((group != 1 && group != 2) || stride < entry || stride % 4) return -1;
    const pf::Endo &en = pf::endo();
    std::vector<unsigned char> mem(n * stride + 16, (unsigned char)filler);
    for (size_t i = 0; i < n; i++) {
        if (group == 1) {
            G1Affine p;
            memcpy(&p, points + 12 * i, sizeof p);
            const G1AffineU u = (inf && inf[i]) ? G1AffineU::inf() : G1AffineU{to_u(p.x), to_u(p.y)};
            memcpy(mem.data() + i * stride, &u, sizeof u);
        } else {
            G2Affine p;
            memcpy(&p, points + 24 * i, sizeof p);
            const G2AffineU u = (inf && inf[i]) ? G2AffineU::inf() : G2AffineU{to_u(p.x), to_u(p.y)};
            memcpy(mem.data() + i * stride, &u, sizeof u);
        }
    }
    if (group == 1) {
        const pkc::ParamsG1 prm = pkc::params_g1(en.beta.to(), fast != 0);
        for (size_t i = 0; i < n; i++) good[i] = pkc::g1_lane(mem.data(), stride, i, prm) ? 1 : 0;
    } else {
        const pkc::ParamsG2 prm = pkc::params_g2(pf::to_sat(en.cx), pf::to_sat(en.cy), fast != 0);
        for (size_t i = 0; i < n; i++) good[i] = pkc::g2_lane(mem.data(), stride, i, prm) ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
