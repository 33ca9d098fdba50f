// The launches of pk_check_dev.cuh: membership of the points of a resident array, one lane per point, the verdicts of an array
// folded into a two-word result slot (api_keys.hip: zkg16_pk_check, zkg16_points_check_bulk, option "pk_validate").
//
// Launch bounds (profiles/kernel_resource_usage_pk_check.txt).  A lane is a chain of ~1,300 dependent Fq products (G1) or ~1,650
// (G2) behind one load of 112 / 224 bytes: the kernels are bound by VALU issue, and a second wave on the SIMD fills the slots a
// single chain leaves between dependent multiply-adds.  G1 (one ladder, the affine addend: 84 registers of state and a product's
// working set) compiles to 212 registers: two waves per SIMD, nothing spilled.  G2 holds twice the state per point (an Fq2
// accumulator is 112 registers, the mixed addition's temporaries as much again): 442 registers, one wave per SIMD, no scratch.
// Compiled for two waves it spills 904 B per lane and measured 3 % faster (same file): not taken.
#include "pk_check_dev.cuh"

#include "common.hpp"
#include "verify_batch.hpp"

namespace zk {

void pk_check_init_launch(hipStream_t st, uint64_t *res, int slots) {
    hipLaunchKernelGGL(pkc::pk_check_init_kernel, dim3((slots + 63) / 64), dim3(64), 0, st, reinterpret_cast<unsigned long long *>(res), slots);
    ZK_HIP(hipGetLastError());
}

void pk_check_launch(hipStream_t st, int group, const void *base, size_t stride, size_t n, const VbEndo &en, uint64_t *res) {
    if (!n) return;
    const size_t blocks = (n + 63) / 64;
    const unsigned char *b = static_cast<const unsigned char *>(base);
    unsigned long long *r = reinterpret_cast<unsigned long long *>(res);
    if (group == 1) hipLaunchKernelGGL(pkc::pk_check_g1_kernel, dim3((unsigned)blocks), dim3(64), 0, st, b, stride, n, pkc::params_g1(en.beta, en.fast_g1 != 0), r);
    else hipLaunchKernelGGL(pkc::pk_check_g2_kernel, dim3((unsigned)blocks), dim3(64), 0, st, b, stride, n, pkc::params_g2(en.cx, en.cy, en.fast_g2 != 0), r);
    ZK_HIP(hipGetLastError());
}

}  // namespace zk
