// The dot products of the trapdoor route (api_trapdoor.hip): for request q and the QAP column values u, v, w, lg at tau
//   S_u = sum_k z_k u_k    S_v = sum_k z_k v_k    S_w = sum_k z_k w_k    S_l = sum_{k >= num_instance} z_k lg_k
// One kernel, grid (chunks, requests): block (c, q) covers the variables [c TD_CHUNK, (c + 1) TD_CHUNK) of assignment q, lane t the
// variables c TD_CHUNK + t, + TD_BLOCK, ...; z_k is loaded once and enters the four products; the four accumulators are fully
// reduced Montgomery values (fp_mul and fp_add both return values < r), the block folds them through LDS as
// setup_col_sum_heavy_kernel does, and lane 0 writes partial[q][c][0..4).  No atomics: the sums over the chunks are made by whoever
// reads the partials (the host, after the call's one read-back).  Field addition is exact and commutative, so the result does not
// depend on TD_CHUNK, on the lane a variable falls to or on the order of the fold.
// The lane body and the fold step are ZK_HD and take the lane as an argument, so tests/csrc/trapdoor_host_shim.hip runs the same
// functions on the host with TD_BLOCK simulated lanes.  Included inside a namespace, after ff.cuh.
#pragma once

constexpr unsigned TD_BLOCK = 256;                 // lanes of a block
constexpr unsigned TD_CHUNK = 4 * TD_BLOCK;        // variables of a block: four per lane

struct TdSums { Fr s[4]; };                        // S_u, S_v, S_w, S_l

ZK_HD Fr td_ld(const Fr *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *q = reinterpret_cast<const uint4 *>(p);      // Fr vectors are 32-byte aligned (allocation base + 32 k)
    const uint4 a = q[0], b = q[1];
    Fr v;
    v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w; v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
    return v;
#else
    return *p;
#endif
}

// what lane `lane` of the block of chunk `chunk` accumulates; nv variables, the first ni of them the instance
ZK_HD TdSums td_lane_sums(const Fr *z, const Fr *u, const Fr *v, const Fr *w, const Fr *lg, size_t nv, size_t ni, size_t chunk, unsigned lane) {
    TdSums a;
    for (int j = 0; j < 4; j++) a.s[j] = Fr::zero();
    const size_t lo = chunk * TD_CHUNK, end = lo + TD_CHUNK < nv ? lo + TD_CHUNK : nv;
    for (size_t k = lo + lane; k < end; k += TD_BLOCK) {
        const Fr zk = td_ld(z + k);
        a.s[0] = fp_add(a.s[0], fp_mul(zk, td_ld(u + k)));
        a.s[1] = fp_add(a.s[1], fp_mul(zk, td_ld(v + k)));
        a.s[2] = fp_add(a.s[2], fp_mul(zk, td_ld(w + k)));
        if (k >= ni) a.s[3] = fp_add(a.s[3], fp_mul(zk, td_ld(lg + k)));
    }
    return a;
}
// one step of the fold: lane t takes lane t + step's value in
ZK_HD Fr td_fold_step(const Fr &mine, const Fr &other) { return fp_add(mine, other); }

#if defined(__HIPCC__)
struct TdArgs {
    const Fr *const *zs;          // device-visible table of the pass's assignments
    const Fr *u, *v, *w, *lg;
    size_t nv, ni;
    Fr *partial;                  // [gridDim.y][gridDim.x][4]
};
__global__ void __launch_bounds__(TD_BLOCK) trapdoor_dot_kernel(TdArgs k) {
    __shared__ uint32_t part[8][TD_BLOCK];
    const unsigned t = threadIdx.x;
    const TdSums mine = td_lane_sums(k.zs[blockIdx.y], k.u, k.v, k.w, k.lg, k.nv, k.ni, blockIdx.x, t);
    Fr *out = k.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
    for (int j = 0; j < 4; j++) {
        Fr acc = mine.s[j];
        for (int i = 0; i < 8; i++) part[i][t] = acc.l[i];
        __syncthreads();
        for (unsigned step = TD_BLOCK / 2; step >= 1; step >>= 1) {
            if (t < step) {
                Fr o;
                for (int i = 0; i < 8; i++) o.l[i] = part[i][t + step];
                acc = td_fold_step(acc, o);
                for (int i = 0; i < 8; i++) part[i][t] = acc.l[i];
            }
            __syncthreads();
        }
        if (t == 0) out[j] = acc;
        __syncthreads();
    }
}
#endif
