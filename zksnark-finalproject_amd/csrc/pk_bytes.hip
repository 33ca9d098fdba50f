// The launches of pk_bytes_dev.cuh: a key's points between arkworks' compressed bytes and the resident U-form, one lane per point
// (api_keys.hip: zkg16_pk_load_bytes, zkg16_pk_save, zkg16_pk_read).  Nothing here synchronises.
//
// Launch bounds (profiles/kernel_resource_usage_pk_bytes.txt).  A decode lane is a chain of dependent Fq products (~500 in G1,
// ~1,000 in G2) behind 48 / 96 bytes in and 112 / 224 out: bound by VALU issue, so both kernels are compiled for two waves per
// SIMD, where a second wave fills the slots one chain leaves between dependent multiply-adds.  The power loops' window table (16
// entries of 14 words) is indexed by a digit of the exponent and lies in scratch; the figures are in that file.  The encode and
// read kernels are three to six products a point between two memory streams and run 256 lanes a block.
#include "pk_bytes_dev.cuh"

#include "common.hpp"
#include "api_internal.hpp"

namespace zk {

void pk_bytes_init_launch(hipStream_t st, uint64_t *res, int slots) {
    hipLaunchKernelGGL(pkb::pkb_init_kernel, dim3((slots + 63) / 64), dim3(64), 0, st, reinterpret_cast<unsigned long long *>(res), slots);
    ZK_HIP(hipGetLastError());
}

void pk_bytes_decode_launch(hipStream_t st, int group, const uint8_t *bytes, size_t n, void *out, size_t stride, size_t first, uint64_t *res) {
    if (!n) return;
    const unsigned blocks = (unsigned)((n + 63) / 64);
    unsigned char *o = static_cast<unsigned char *>(out);
    unsigned long long *r = reinterpret_cast<unsigned long long *>(res);
    if (group == 1) hipLaunchKernelGGL(pkb::pkb_decode_g1_kernel, dim3(blocks), dim3(64), 0, st, bytes, n, o, stride, first, r);
    else hipLaunchKernelGGL(pkb::pkb_decode_g2_kernel, dim3(blocks), dim3(64), 0, st, bytes, n, o, stride, first, r);
    ZK_HIP(hipGetLastError());
}

void pk_bytes_encode_launch(hipStream_t st, int group, const void *base, size_t stride, size_t n, uint8_t *out) {
    if (!n) return;
    hipLaunchKernelGGL(pkb::pkb_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, group, static_cast<const unsigned char *>(base), stride, n, out);
    ZK_HIP(hipGetLastError());
}

void pk_bytes_read_launch(hipStream_t st, int group, const void *base, size_t stride, size_t n, uint64_t *limbs, uint8_t *inf) {
    if (!n) return;
    hipLaunchKernelGGL(pkb::pkb_read_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, group, static_cast<const unsigned char *>(base), stride, n, limbs, inf);
    ZK_HIP(hipGetLastError());
}

}  // namespace zk
