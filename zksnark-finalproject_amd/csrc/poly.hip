// R1CS -> QAP witness map on device (everything of ark-groth16 0.4 `LibsnarkReduction::witness_map_from_matrices`
// — src/r1cs_to_qap.rs, SURVEY.md A.4 — that is not an NTT): the three CSR SpMVs <A_i,z>, <B_i,z>, <C_i,z>,
// the pointwise (a*b - c) / Z on the coset, and the Montgomery -> canonical conversion that feeds the MSMs.
// Called from /root/reference/src/arkworks/backend/matrix_proof.rs:139-140 via Groth16::prove.
// All kernels are HBM-streaming (32 B per Fr, 16-B vector loads); SpMV gathers z through L2/MALL.
#include "common.hpp"
#include "r1cs_check_dev.cuh"

namespace zk {

__device__ __forceinline__ Fr gld_fr(const Fr *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 a = q[0], b = q[1];
    Fr v;
    v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w;
    v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
    return v;
}
__device__ __forceinline__ void gst_fr(Fr *p, const Fr &v) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

struct SpmvArgs {
    const uint64_t *rp[3];
    const uint32_t *col[3];
    const uint32_t *perm[3];      // row order of the lanes (null: natural order)
    const Fr *cf[3];
    Fr *out[3];
    const Fr *z;
    size_t nc, num_instance, n;   // n = domain size (outputs are zero-padded to n)
    const uint32_t *rows[3];      // null, or lane t takes row rows[m][t], t < nrows[m] (a rank's rows, split witness map)
    size_t nrows[3];
    const Fr *const *zs;          // a batch (zkg16_prove_batch): blockIdx.z = vector v reads zs[v] and writes out[m] + v * out_stride
    size_t out_stride;
};
// the row of lane `t` of matrix m: from the rank's row list, else from the length-class order (rows < nc), else t itself
template <class Args>
__device__ __forceinline__ bool spmv_row(const Args &a, int m, size_t &row) {
    if (a.rows[m]) {
        if (row >= a.nrows[m]) return false;
        row = a.rows[m][row];
        return row < a.n;
    }
    if (row >= a.n) return false;
    if (row < a.nc && a.perm[m]) {
        row = a.perm[m][row];
        if (row >= a.nc) return false;          // never: the order is a permutation of the rows (row_perm_build)
    }
    return true;
}

// One thread per (matrix, row): the reference's circuits have short rows (matmul rows: 1 nnz per side;
// Poseidon rows: a few tens), so a row per lane keeps all 64 lanes busy.  Rows >= nc are the padding:
// a[nc + i] = z[i] for i < num_instance (the "input consistency" rows of LibsnarkReduction), else 0.
__global__ void __launch_bounds__(256) spmv_kernel(SpmvArgs a) {
    size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (!spmv_row(a, m, row)) return;
    const Fr *z = a.zs ? a.zs[blockIdx.z] : a.z;
    Fr acc = Fr::zero();
    if (row < a.nc) {
        const uint64_t lo = a.rp[m][row], hi = a.rp[m][row + 1];
        for (uint64_t k = lo; k < hi; k++) {
            Fr c = gld_fr(a.cf[m] + k);
            Fr v = gld_fr(z + a.col[m][k]);
            acc = fp_add(acc, fp_mul(c, v));
        }
    } else if (m == 0 && row < a.nc + a.num_instance) {
        acc = gld_fr(z + (row - a.nc));
    }
    gst_fr(a.out[m] + (size_t)blockIdx.z * a.out_stride + row, acc);
}

// ab[i] = (a[i]*b[i] - c[i]) * zinv; c null (six transforms: b carries 1/Z, C is subtracted after the last transform): a[i]*b[i]
__global__ void __launch_bounds__(256) pointwise_h_kernel(Fr *a, const Fr *b, const Fr *c, Fr zinv, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr x = fp_mul(gld_fr(a + i), gld_fr(b + i));
    if (c) x = fp_mul(fp_sub(x, gld_fr(c + i)), zinv);
    gst_fr(a + i, x);
}

__global__ void __launch_bounds__(256) fr_from_mont_kernel(const Fr *in, Fr *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gst_fr(out + i, fp_from_mont(gld_fr(in + i)));
}

// ------------------------------------------------------------------------------------------------ coefficient dictionary
// The coefficients of an R1CS are a small set of field elements (1, -1, the Poseidon MDS entries and round constants, small
// integers).  One pass over the three coefficient arrays puts the distinct values into an open-addressing table (claimed with
// one compare-and-swap per NEW value), a one-block pass numbers the used slots densely, a third rewrites the slot numbers: from
// then on the SpMV reads 2 bytes per non-zero and takes the coefficient from LDS.  More than DICT_MAX distinct values: the
// handle keeps the plain kernel.
static constexpr uint32_t DICT_CAP = 4096, DICT_MAX = 1024;
struct DictArgs {
    const Fr *cf;
    size_t nnz;
    uint16_t *idx;
    uint32_t *keys;          // [DICT_CAP][8]
    uint32_t *state;         // [DICT_CAP]: 0 free, 1 being written, 2 ready
    uint32_t *count;         // [0] values inserted, [1] overflow flag, [2] dense count
};
// slot of `c` in the global table (inserted if new); 0xffff after an overflow
__device__ __forceinline__ uint32_t dict_global_slot(const DictArgs &a, const Fr &c, uint32_t h) {
    uint32_t p = h & (DICT_CAP - 1);
    // every path through the body ends the lane's turn for this iteration: a lane that finds a slot "being written" simply looks
    // again on the next trip, so the lane that owns the slot (possibly in the same wave) is never waited for inside a branch
    for (uint32_t trips = 0; trips < 64u * DICT_CAP; trips++) {
        if (__hip_atomic_load(a.count + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0xffffu;
        const uint32_t s = __hip_atomic_load(a.state + p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (s == 2) {
            bool same = true;
#pragma unroll
            for (int k = 0; k < 8; k++) same = same && __hip_atomic_load(a.keys + 8 * p + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c.l[k];
            if (same) return p;
            p = (p + 1) & (DICT_CAP - 1);
        } else if (s == 0) {
            if (atomicCAS(a.state + p, 0u, 1u) == 0u) {
                if (atomicAdd(a.count, 1u) >= DICT_MAX) break;
#pragma unroll
                for (int k = 0; k < 8; k++) __hip_atomic_store(a.keys + 8 * p + k, c.l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.state + p, 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return p;
            }
        }
    }
    __hip_atomic_store(a.count + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // table full (or never settled): give up for this handle
    return 0xffffu;
}
// A workgroup walks DICT_CHUNK consecutive non-zeros and remembers the slots it has looked up in a write-once LDS table (512
// entries, direct-mapped on other hash bits), so the global table — a few hundred hot addresses for the whole device — is
// consulted once per distinct value per workgroup instead of once per non-zero.
static constexpr uint32_t DICT_CHUNK = 16384, DICT_LOCAL = 512;
__global__ void __launch_bounds__(256) coef_dict_kernel(DictArgs a) {
    __shared__ uint32_t l_slot[DICT_LOCAL];              // 0 free, 0xffffffff being written, else slot + 1
    __shared__ uint32_t l_key[DICT_LOCAL * 8];
    for (uint32_t e = threadIdx.x; e < DICT_LOCAL; e += blockDim.x) l_slot[e] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * DICT_CHUNK;
    for (uint32_t j = threadIdx.x; j < DICT_CHUNK; j += blockDim.x) {
        const size_t i = base + j;
        if (i >= a.nnz) break;
        const Fr c = gld_fr(a.cf + i);
        uint32_t h = c.l[0] * 0x9E3779B1u ^ c.l[1] * 0x85EBCA77u ^ c.l[2] * 0xC2B2AE3Du ^ c.l[5] * 0x27D4EB2Fu ^ c.l[7];
        h ^= h >> 15;
        const uint32_t lp = (h >> 16) & (DICT_LOCAL - 1);
        uint32_t found = 0xffffffffu;
        const uint32_t ls = __hip_atomic_load(l_slot + lp, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (ls != 0u && ls != 0xffffffffu) {
            bool same = true;
#pragma unroll
            for (int k = 0; k < 8; k++) same = same && l_key[lp * 8 + k] == c.l[k];
            if (same) found = ls - 1u;
        }
        if (found == 0xffffffffu) {
            found = dict_global_slot(a, c, h);
            if (ls == 0u && found != 0xffffu && atomicCAS(l_slot + lp, 0u, 0xffffffffu) == 0u) {      // this lane fills the free local entry
#pragma unroll
                for (int k = 0; k < 8; k++) l_key[lp * 8 + k] = c.l[k];
                __hip_atomic_store(l_slot + lp, found + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        a.idx[i] = (uint16_t)found;
    }
}
// one block: dense numbers for the used slots (slot order), the dense value table, and slot -> dense in state[]
__global__ void __launch_bounds__(1024) coef_dict_compact_kernel(uint32_t *keys, uint32_t *state, uint32_t *count, Fr *dict) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    constexpr uint32_t PER = DICT_CAP / 1024;
    uint32_t used[PER], mine = 0;
    for (uint32_t j = 0; j < PER; j++) {
        used[j] = state[t * PER + j] == 2u ? 1u : 0u;
        mine += used[j];
    }
    part[t] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t next = part[t] - mine;
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t p = t * PER + j;
        if (used[j]) {
            Fr v;
            for (int k = 0; k < 8; k++) v.l[k] = keys[8 * p + k];
            if (next < DICT_MAX) gst_fr(dict + next, v);
            state[p] = next++;
        }
    }
    if (t == 1023) count[2] = part[1023];
}
__global__ void __launch_bounds__(256) coef_dict_remap_kernel(uint16_t *idx, size_t nnz, const uint32_t *dense) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nnz) idx[i] = (uint16_t)dense[idx[i] & (DICT_CAP - 1)];
}

struct SpmvDictArgs {
    const uint64_t *rp[3];
    const uint32_t *col[3];
    const uint32_t *perm[3];
    const uint16_t *ci[3];
    Fr *out[3];
    const Fr *z, *dict;
    uint32_t ndict;
    size_t nc, num_instance, n;
    const uint32_t *rows[3];
    size_t nrows[3];
    const Fr *const *zs;
    size_t out_stride;
};
// the same row-per-lane product with the coefficient taken from the dictionary in LDS ([8][ndict] words: neighbouring lanes
// reading different entries spread over the banks); a coefficient equal to one (40 % of the MatrixCircuit's, all of its C
// matrix) costs no product
__global__ void __launch_bounds__(256) spmv_dict_kernel(SpmvDictArgs a) {
    extern __shared__ uint32_t s_dict[];                 // [8][ndict] limbs, then ndict flag bytes
    uint8_t *s_one = reinterpret_cast<uint8_t *>(s_dict + 8 * a.ndict);
    for (uint32_t e = threadIdx.x; e < a.ndict; e += blockDim.x) {
        const Fr v = gld_fr(a.dict + e);
#pragma unroll
        for (int k = 0; k < 8; k++) s_dict[k * a.ndict + e] = v.l[k];
        s_one[e] = v == Fr::one() ? 1 : 0;
    }
    __syncthreads();
    size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (!spmv_row(a, m, row)) return;
    const Fr *z = a.zs ? a.zs[blockIdx.z] : a.z;
    Fr acc = Fr::zero();
    if (row < a.nc) {
        const uint64_t lo = a.rp[m][row], hi = a.rp[m][row + 1];
        for (uint64_t k = lo; k < hi; k++) {
            const uint32_t e = a.ci[m][k];
            const Fr v = gld_fr(z + a.col[m][k]);
            if (s_one[e]) {
                acc = fp_add(acc, v);
            } else {
                Fr c;
#pragma unroll
                for (int q = 0; q < 8; q++) c.l[q] = s_dict[q * a.ndict + e];
                acc = fp_add(acc, fp_mul(c, v));
            }
        }
    } else if (m == 0 && row < a.nc + a.num_instance) {
        acc = gld_fr(z + (row - a.nc));
    }
    gst_fr(a.out[m] + (size_t)blockIdx.z * a.out_stride + row, acc);
}

// ------------------------------------------------------------------------------------------------ rows by length
// The reference's matrices mix rows of 1 non-zero (88 % of them) with rows of 4 .. 133 (the Poseidon rounds' linear layers), in
// runs of every length: with a row per lane in natural order a wave runs as long as its longest row while most lanes idle —
// the SpMV of the 128x128 circuit took 6.3 ms, 4 of them the multiplier at ~8 % lane utilisation.  The rows are therefore
// ordered once per handle by length class = bit length of the row's non-zero count (0, 1, 2-3, 4-7, ... : lanes of a wave
// differ by less than 2x), longest class first, and in natural order inside a class: neighbouring rows read neighbouring
// variables, and an order that shuffled them (exact-length classes filled through atomics) tripled the kernel's HBM reads.
// Stable counting sort: per-workgroup class counts, a scan over the workgroups per class, ballot ranks inside the workgroup.
static constexpr int ROW_CLASSES = 18;
__device__ __forceinline__ uint32_t row_class(const uint64_t *rp, size_t row) {
    const uint64_t len = rp[row + 1] - rp[row];
    const uint32_t c = len ? 64u - (uint32_t)__builtin_clzll(len) : 0u;
    return c < ROW_CLASSES ? c : ROW_CLASSES - 1;
}
__global__ void __launch_bounds__(256) row_class_count_kernel(const uint64_t *rp, size_t nc, uint32_t *counts /*[class][block]*/) {
    __shared__ uint32_t h[ROW_CLASSES];
    if (threadIdx.x < ROW_CLASSES) h[threadIdx.x] = 0;
    __syncthreads();
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row < nc) atomicAdd(&h[row_class(rp, row)], 1u);
    __syncthreads();
    if (threadIdx.x < ROW_CLASSES) counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}
// one workgroup per class: counts[class][0 .. nblk) -> exclusive prefix; total -> tot[class]
__global__ void __launch_bounds__(1024) row_class_scan_kernel(uint32_t *counts, uint32_t nblk, uint32_t *tot) {
    __shared__ uint32_t wave_tot[16];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    uint32_t *row = counts + (size_t)blockIdx.x * nblk;
    const uint32_t per = ((nblk + nwv - 1) / nwv + 63u) & ~63u;
    const uint32_t lo = wv * per, hi = lo + per < nblk ? lo + per : nblk;
    uint32_t carry = 0;
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        uint32_t v = i < hi ? row[i] : 0u;
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        carry += v;
    }
    if (lane == 0) wave_tot[wv] = carry;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t x = 0; x < nwv; x++) {
        const uint32_t t = wave_tot[x];
        if (x < wv) before += t;
        total += t;
    }
    carry = before;
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        const uint32_t v = i < hi ? row[i] : 0u;
        uint32_t inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += up;
        }
        if (i < hi) row[i] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) row_perm_kernel(const uint64_t *rp, size_t nc, const uint32_t *counts, const uint32_t *tot, uint32_t *perm) {
    __shared__ uint32_t wcount[4][ROW_CLASSES], cbase[ROW_CLASSES];
    const uint32_t wv = threadIdx.x >> 6;
    if (threadIdx.x < ROW_CLASSES) {          // longest class first: everything of a larger class comes before this one
        uint32_t b = 0;
        for (int c = ROW_CLASSES - 1; c > (int)threadIdx.x; c--) b += tot[c];
        cbase[threadIdx.x] = b + counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
    }
    for (uint32_t e = threadIdx.x; e < 4 * ROW_CLASSES; e += blockDim.x) (&wcount[0][0])[e] = 0;
    __syncthreads();
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = row < nc;
    const uint32_t cls = valid ? row_class(rp, row) : 0u;
    uint64_t peers = __ballot(valid);          // the lanes of this wave with the same class
    for (int b = 0; b < 5; b++) {
        const bool bit = (cls >> b) & 1u;
        const uint64_t mk = __ballot(valid && bit);
        peers &= bit ? mk : ~mk;
    }
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
    if (valid && below == 0) wcount[wv][cls] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
        uint32_t rank = below;
        for (uint32_t x = 0; x < wv; x++) rank += wcount[x][cls];
        const uint32_t pos = cbase[cls] + rank;
        if (pos < nc) perm[pos] = (uint32_t)row;
    }
}
static void row_perm_build(zkg16_ctx *ctx, R1csDev &m) {
    const size_t nc = m.num_constraints;
    if (nc < 4096 || nc >= ((size_t)1 << 32)) return;
    const unsigned grid = (unsigned)((nc + 255) / 256);
    DevBuf counts(((size_t)ROW_CLASSES * grid + ROW_CLASSES) * sizeof(uint32_t));
    uint32_t *cnt = counts.as<uint32_t>(), *tot = cnt + (size_t)ROW_CLASSES * grid;
    for (int i = 0; i < 3; i++) {
        m.perm[i].ensure(nc * sizeof(uint32_t));
        hipLaunchKernelGGL(row_class_count_kernel, dim3(grid), dim3(256), 0, ctx->stream, m.rp[i].as<uint64_t>(), nc, cnt);
        hipLaunchKernelGGL(row_class_scan_kernel, dim3(ROW_CLASSES), dim3(1024), 0, ctx->stream, cnt, grid, tot);
        hipLaunchKernelGGL(row_perm_kernel, dim3(grid), dim3(256), 0, ctx->stream, m.rp[i].as<uint64_t>(), nc, cnt, tot, m.perm[i].as<uint32_t>());
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(ctx->stream));               // `counts` goes out of scope
    m.perm_ok = true;
}

static void coef_dict_build(zkg16_ctx *ctx, R1csDev &m) {
    m.dict_state = 2;
    row_perm_build(ctx, m);
    const size_t total = m.nnz[0] + m.nnz[1] + m.nnz[2];
    if (total < 4096) return;        // tiny systems: not worth three launches and a sync
    DevBuf scratch((DICT_CAP * 9 + 4) * sizeof(uint32_t));
    uint32_t *keys = scratch.as<uint32_t>(), *state = keys + 8 * DICT_CAP, *count = state + DICT_CAP;
    ZK_HIP(hipMemsetAsync(scratch.p, 0, (DICT_CAP * 9 + 4) * sizeof(uint32_t), ctx->stream));
    m.dict.ensure(DICT_MAX * sizeof(Fr));
    for (int i = 0; i < 3; i++) {
        m.ci[i].ensure((m.nnz[i] ? m.nnz[i] : 1) * sizeof(uint16_t));
        if (!m.nnz[i]) continue;
        const DictArgs d{m.cf[i].as<Fr>(), m.nnz[i], m.ci[i].as<uint16_t>(), keys, state, count};
        hipLaunchKernelGGL(coef_dict_kernel, dim3((unsigned)((m.nnz[i] + DICT_CHUNK - 1) / DICT_CHUNK)), dim3(256), 0, ctx->stream, d);
    }
    hipLaunchKernelGGL(coef_dict_compact_kernel, dim3(1), dim3(1024), 0, ctx->stream, keys, state, count, m.dict.as<Fr>());
    for (int i = 0; i < 3; i++)
        if (m.nnz[i])
            hipLaunchKernelGGL(coef_dict_remap_kernel, dim3((unsigned)((m.nnz[i] + 255) / 256)), dim3(256), 0, ctx->stream, m.ci[i].as<uint16_t>(),
                               m.nnz[i], state);
    ZK_HIP(hipGetLastError());
    uint32_t res[3] = {0, 0, 0};
    ZK_HIP(hipMemcpyAsync(res, count, sizeof res, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    if (res[1] || res[2] == 0 || res[2] > DICT_MAX) {            // too many distinct values: this handle keeps the plain kernel
        for (int i = 0; i < 3; i++) m.ci[i].release();
        m.dict.release();
        return;
    }
    m.ndict = res[2];
    m.dict_state = 1;
}

// zs / nvec (a batch): vector v's assignment at zs[v] (device-visible pointer table), its a / b / c at a / b / c + v * N
void spmv_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, Fr *a, Fr *b, Fr *c, const SpmvRows *rows, const Fr *const *zs, unsigned nvec) {
    // both structures are built the SECOND time a handle is used: the reference's request flow uses its matrices once (the
    // three passes of the build cost more than they save there: Fermat-prime request 8.1 -> 9.7 ms), a resident system pays once
    {
        std::lock_guard<std::mutex> lazy(m.lazy_mu);       // lanes share the handle: one of them builds (and synchronises its stream), the others wait
        if (m.dict_state == 0 && ctx->opt.spmv_dict != 2 && ++m.spmv_uses >= 2) coef_dict_build(ctx, m);
    }
    const size_t n = (size_t)1 << m.log_n;
    size_t lanes = n;
    if (rows) lanes = std::max(rows->n[0], std::max(rows->n[1], rows->n[2]));
    if (!lanes) return;
    const unsigned grid = (unsigned)((lanes + 255) / 256);
    if (nvec < 1 || nvec > 65535 || (nvec > 1 && (rows || !zs))) throw HipError{hipErrorInvalidValue, "spmv: bad batch", __FILE__, __LINE__};
    ScopedKernelTimer kt(ctx, "spmv_kernel", (double)(m.nnz[0] + m.nnz[1] + m.nnz[2]) * nvec);
    if (m.dict_state == 1 && ctx->opt.spmv_dict != 2) {
        SpmvDictArgs s;
        for (int i = 0; i < 3; i++) {
            s.rp[i] = m.rp[i].as<uint64_t>();
            s.col[i] = m.col[i].as<uint32_t>();
            s.ci[i] = m.ci[i].as<uint16_t>();
            s.perm[i] = m.perm_ok ? m.perm[i].as<uint32_t>() : nullptr;
        }
        s.out[0] = a; s.out[1] = b; s.out[2] = c;
        s.z = z;
        s.zs = nvec > 1 ? zs : nullptr;
        s.out_stride = nvec > 1 ? n : 0;
        s.dict = m.dict.as<Fr>();
        s.ndict = m.ndict;
        s.nc = m.num_constraints;
        s.num_instance = m.num_instance;
        s.n = n;
        for (int i = 0; i < 3; i++) {
            s.rows[i] = rows ? rows->list[i] : nullptr;
            s.nrows[i] = rows ? rows->n[i] : 0;
        }
        hipLaunchKernelGGL(spmv_dict_kernel, dim3(grid, 3, nvec), dim3(256), m.ndict * 33 + 16, ctx->stream, s);
    } else {
        SpmvArgs s;
        for (int i = 0; i < 3; i++) {
            s.rp[i] = m.rp[i].as<uint64_t>();
            s.col[i] = m.col[i].as<uint32_t>();
            s.cf[i] = m.cf[i].as<Fr>();
            s.perm[i] = (m.perm_ok && ctx->opt.spmv_dict != 2) ? m.perm[i].as<uint32_t>() : nullptr;
        }
        s.out[0] = a; s.out[1] = b; s.out[2] = c;
        s.z = z;
        s.zs = nvec > 1 ? zs : nullptr;
        s.out_stride = nvec > 1 ? n : 0;
        s.nc = m.num_constraints;
        s.num_instance = m.num_instance;
        s.n = n;
        for (int i = 0; i < 3; i++) {
            s.rows[i] = rows ? rows->list[i] : nullptr;
            s.nrows[i] = rows ? rows->n[i] : 0;
        }
        hipLaunchKernelGGL(spmv_kernel, dim3(grid, 3, nvec), dim3(256), 0, ctx->stream, s);
    }
    ZK_HIP(hipGetLastError());
}

void pointwise_h_run(zkg16_ctx *ctx, Fr *ab_a, const Fr *b, const Fr *c, const Fr &zinv, size_t n) {
    ScopedKernelTimer kt(ctx, "pointwise_h_kernel", (double)n);
    hipLaunchKernelGGL(pointwise_h_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ab_a, b, c, zinv, n);
    ZK_HIP(hipGetLastError());
}

void fr_from_mont_run(zkg16_ctx *ctx, const Fr *in, Fr *out, size_t n) {
    if (n == 0) return;
    ScopedKernelTimer kt(ctx, "fr_from_mont_kernel", (double)n);
    hipLaunchKernelGGL(fr_from_mont_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, in, out, n);
    ZK_HIP(hipGetLastError());
}

// Proofs on the PrimeCircuit's template (WmPatch): the request's four column-0 coefficients are not in the matrices, and z[0] = 1, so
// their products are added to the SpMV's results here — add[2 v] to a[rows[0..2]], add[2 v + 1] to c[rows[3]] of vector v.  Four
// lanes per vector, one element each (distinct constraint rows, checked at the launch); before any transform, so
// both sequences of wm_transforms see the request's A z and C z.
__global__ void __launch_bounds__(256) wm_patch_kernel(Fr *a, Fr *c, size_t stride, WmPatch p, unsigned nvec) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned v = t >> 2, k = t & 3u;
    if (v >= nvec) return;
    Fr *dst = (k < 3 ? a : c) + (size_t)v * stride + p.rows[k];
    gst_fr(dst, fp_add(gld_fr(dst), gld_fr(p.add + 2 * (size_t)v + (k < 3 ? 0 : 1))));
}
static void wm_patch_run(zkg16_ctx *ctx, const R1csDev &m, Fr *a, Fr *c, const WmPatch &p, unsigned nvec) {
    const size_t n = (size_t)1 << m.log_n;
    for (int k = 0; k < 4; k++)
        if (p.rows[k] >= m.num_constraints) throw HipError{hipErrorInvalidValue, "witness map: patch row outside the constraints", __FILE__, __LINE__};
    if (p.rows[0] == p.rows[1] || p.rows[0] == p.rows[2] || p.rows[1] == p.rows[2]) throw HipError{hipErrorInvalidValue, "witness map: patch rows repeat", __FILE__, __LINE__};
    ScopedKernelTimer kt(ctx, "wm_patch_kernel", 4.0 * nvec);
    hipLaunchKernelGGL(wm_patch_kernel, dim3((4 * nvec + 255) / 256), dim3(256), 0, ctx->stream, a, c, n, p, nvec);
    ZK_HIP(hipGetLastError());
}

// The transforms of the witness map on the SpMV's a, b, c (nvec vectors of N side by side, tmp the scratch) -> h (= tmp).  They
// ping-pong between each vector and the one scratch buffer (ifft: x -> tmp, coset fft: tmp -> x), and the point-wise stage rides
// on the load of the last transform: no device-to-device copy and no separate point-wise pass (round 1 had both).
//   6 (default): h = coset_ifft(A_cos * B_cos / Z) - ifft(c) / Z, X_cos = coset_fft(ifft x).  coset_ifft is linear and undoes
//     coset_fft, so this is arkworks' h below exactly, for any assignment: C needs only its inverse transform.  1/Z (and the U-form
//     2^5) is folded into the last-store constant of B's coset fft, so the fused load is ONE product; 1/Z into that of c's ifft, and
//     the last transform's store subtracts the ifft(c)/Z it finds in tmp (the thread that overwrites a position read it).
//   7 (option wm_transforms = 7): ark-groth16's coset_ifft((A_cos * B_cos - C_cos) / Z).
static Fr *wm_transforms(zkg16_ctx *ctx, int log_n, Fr *a, Fr *b, Fr *c, Fr *tmp, unsigned nvec) {
    const size_t n = (size_t)1 << log_n;
    auto run = [&](Fr *src, Fr *dst, bool inverse, bool coset, const NttPointwise *pw = nullptr, const NttLast *last = nullptr) {
        return ntt_run_batch(ctx, src, dst, log_n, inverse, coset, pw, nvec, n, last);
    };
    NttTables *t = ntt_get_tables(ctx, log_n);
    const bool fuse = ctx->opt.fuse_pointwise != 0;
    run(a, tmp, true, false);
    run(tmp, a, false, true);
    if (ctx->opt.wm_transforms == 7) {
        run(b, tmp, true, false);
        run(tmp, b, false, true);
        run(c, tmp, true, false);
        run(tmp, c, false, true);
        const NttPointwise pw{b, c, t->zinv};
        if (fuse) return run(a, tmp, true, true, &pw);
        pointwise_h_run(ctx, a, b, c, t->zinv, (size_t)nvec * n);      // element-wise: the K vectors are one array
        return run(a, tmp, true, true);
    }
    const NttLast to_b{&t->zinv, fuse, false}, to_c{&t->zinv, false, false}, sub{nullptr, false, true};
    run(b, tmp, true, false);
    run(tmp, b, false, true, nullptr, &to_b);          // b <- B_cos / Z (x 2^5 in U-form when the product rides on a load)
    run(c, tmp, true, false, nullptr, &to_c);          // tmp <- ifft(c) / Z
    const NttPointwise pw{b, nullptr, t->zinv};
    if (fuse) return run(a, tmp, true, true, &pw, &sub);
    pointwise_h_run(ctx, a, b, nullptr, t->zinv, (size_t)nvec * n);
    return run(a, tmp, true, true, nullptr, &sub);
}

// ------------------------------------------------------------------------------------------------ satisfaction
// (A z)_i (B z)_i == (C z)_i on the rows the SpMV (and the patch) has just written, in natural order whatever order its lanes took:
// lane i < nc of vector blockIdx.z reads a, b, c at v * stride + i (r1cs_check_dev.cuh: row_fails), a wave's verdicts are one ballot,
// lane 0 of the block folds the four and — only when a row failed — adds to n_bad[v] and lowers first_bad[v].  Rows from nc on (the
// instance rows, the padding) are not rows of the system.  12 KB read per block, one product per lane: bound by the three streams.
struct R1csCheckArgs {
    const Fr *a, *b, *c;
    size_t stride, nc;
    uint64_t *res;                // n_bad[nvec] | first_bad[nvec], filled by r1cs_check_init_kernel
    unsigned nvec;
};
__global__ void __launch_bounds__(256) r1cs_check_init_kernel(uint64_t *res, unsigned nvec) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * nvec) res[t] = rck::result_init(t, nvec);
}
__global__ void __launch_bounds__(256) r1cs_check_kernel(R1csCheckArgs k) {
    __shared__ uint64_t s_ballot[rck::WAVES];
    const size_t row0 = (size_t)blockIdx.x * rck::BLOCK, i = row0 + threadIdx.x;
    const unsigned v = blockIdx.z;
    bool bad = false;
    if (i < k.nc) {
        const size_t at = (size_t)v * k.stride + i;
        bad = rck::row_fails(gld_fr(k.a + at), gld_fr(k.b + at), gld_fr(k.c + at));
    }
    const uint64_t m = __ballot(bad);
    if ((threadIdx.x & 63u) == 0) s_ballot[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t ballots[rck::WAVES], count, first;
    for (unsigned w = 0; w < rck::WAVES; w++) ballots[w] = s_ballot[w];
    if (!rck::block_fold(ballots, row0, count, first)) return;
    atomicAdd(reinterpret_cast<unsigned long long *>(k.res + v), (unsigned long long)count);
    atomicMin(reinterpret_cast<unsigned long long *>(k.res + k.nvec + v), (unsigned long long)first);
}
void r1cs_check_run(zkg16_ctx *ctx, size_t nc, const Fr *a, const Fr *b, const Fr *c, size_t stride, unsigned nvec, uint64_t *res) {
    if (nvec < 1 || nvec > 65535 || nc > stride || nc >= ((size_t)1 << 32)) throw HipError{hipErrorInvalidValue, "r1cs check: bad shape", __FILE__, __LINE__};
    ScopedKernelTimer kt(ctx, "r1cs_check_kernel", (double)nc * nvec);
    hipLaunchKernelGGL(r1cs_check_init_kernel, dim3((2 * nvec + 255) / 256), dim3(256), 0, ctx->stream, res, nvec);
    if (nc) {
        const R1csCheckArgs k{a, b, c, stride, nc, res, nvec};
        hipLaunchKernelGGL(r1cs_check_kernel, dim3((unsigned)((nc + rck::BLOCK - 1) / rck::BLOCK), 1, nvec), dim3(rck::BLOCK), 0, ctx->stream, k);
    }
    ZK_HIP(hipGetLastError());
}
void r1cs_check_spmv_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, const Fr *const *zs, unsigned nvec, const WmPatch *patch, uint64_t *res) {
    const size_t n = (size_t)1 << m.log_n;
    for (int i = 0; i < 3; i++) ctx->poly[i].ensure((size_t)nvec * n * sizeof(Fr));
    Fr *a = ctx->poly[0].as<Fr>(), *b = ctx->poly[1].as<Fr>(), *c = ctx->poly[2].as<Fr>();
    if (nvec == 1 && !zs) spmv_run(ctx, m, z, a, b, c);
    else spmv_run(ctx, m, nullptr, a, b, c, nullptr, zs, nvec);
    if (patch) wm_patch_run(ctx, m, a, c, *patch, nvec);
    r1cs_check_run(ctx, m.num_constraints, a, b, c, n, nvec, res);
}

// h of one assignment, N Montgomery coefficients.  Result pointer = ctx->poly[3].
void witness_map_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, Fr **h_out, const WmPatch *patch, uint64_t *check) {
    const size_t n = (size_t)1 << m.log_n;
    for (int i = 0; i < 4; i++) ctx->poly[i].ensure(n * sizeof(Fr));
    Fr *a = ctx->poly[0].as<Fr>(), *b = ctx->poly[1].as<Fr>(), *c = ctx->poly[2].as<Fr>(), *tmp = ctx->poly[3].as<Fr>();
    spmv_run(ctx, m, z, a, b, c);
    if (patch) wm_patch_run(ctx, m, a, c, *patch, 1);
    if (check) r1cs_check_run(ctx, m.num_constraints, a, b, c, n, 1, check);
    *h_out = wm_transforms(ctx, m.log_n, a, b, c, tmp, 1);
}

// The witness map of a batch: the K assignments at zs[0 .. K) (device-visible pointer table), every launch of witness_map_run
// once over the K vectors — one SpMV, the transform passes with grid.z = K (shared tables, the fused point-wise stage per
// vector).  a, b, c and the scratch hold K vectors of N side by side; *h_out = K h vectors of N, vector v at (*h_out) + v * N.
void witness_map_run_batch(zkg16_ctx *ctx, R1csDev &m, const Fr *const *zs, unsigned nvec, Fr **h_out, const WmPatch *patch, uint64_t *check) {
    const size_t n = (size_t)1 << m.log_n;
    for (int i = 0; i < 4; i++) ctx->poly[i].ensure((size_t)nvec * n * sizeof(Fr));
    Fr *a = ctx->poly[0].as<Fr>(), *b = ctx->poly[1].as<Fr>(), *c = ctx->poly[2].as<Fr>(), *tmp = ctx->poly[3].as<Fr>();
    spmv_run(ctx, m, nullptr, a, b, c, nullptr, zs, nvec);
    if (patch) wm_patch_run(ctx, m, a, c, *patch, nvec);
    if (check) r1cs_check_run(ctx, m.num_constraints, a, b, c, n, nvec, check);
    *h_out = wm_transforms(ctx, m.log_n, a, b, c, tmp, nvec);
}

}  // namespace zk
