// The PrimeCircuit's R1CS and assignment written ON THE DEVICE for candidate (x, j) (prime_program.hpp).
//
// Per prime request the host path synthesises 338,296 constraints and 320,945 variables (seven threads) and uploads ~65 MB of CSR
// arrays and assignment.  The circuit's structure is the same for every candidate, so here:
//   - R1CS: the ctx keeps the recorded template resident; a request is a device-to-device copy plus four coefficients (n three
//     times in A, -j once in C; at j = 0 C's term is dropped and the j = 0 row pointers are used).  32-byte uploads only.
//   - assignment: the host computes the program's inputs natively (909 field-valued slots, the 258 instance entries included, and
//     the 124 values that to_bits_le decomposes: 33 KB); prime_witness_eval_kernel runs the recorded bit program, one workgroup per
//     part (head, three bases, three Fermat parts: they share no bits), bits in LDS, one barrier per dependency level;
//     prime_witness_expand_kernel writes z in Montgomery form (0 / one / slot values), 16 B per thread.
// The recorded program (ZKG16_TRACE_HOST=1 prints it):
//   part        witnesses   instructions   levels
//   head           39,686         29,549      318     (one SHA-256 compression)
//   base k         73,098         54,389      639     (x 3; two compressions each: the largest LDS footprint, 73 KB)
//   Fermat k       20,569         20,360       49     (x 3; 40 unchecked comparisons = 40 x to_bits_le)
// (an addmany is ONE instruction for all its result bits, so a part has fewer instructions than witnesses; its slots have none)
// K requests in one pass (prime_witness_batch_on_device): the K x (slots | sources) go up in ONE copy out of pinned staging,
// prime_witness_eval_batch_kernel runs the program on a (part, request) grid — the 639 barrier levels of a base part are latency, not
// work, and K requests fill the device where one fills seven CUs — and prime_witness_expand_batch_kernel writes the K assignments,
// which share one allocation, through a table of their addresses.
#include "common.hpp"
#include "prime_program.hpp"

using namespace zk;

namespace zk {

void mbatch_staging_ensure(zkg16_ctx *ctx, size_t bytes);      // witness.hip: the ctx's pinned staging block and its device copy

struct PrimeDev {
    std::shared_ptr<const PrimeProgram> prog;
    DevBuf rp[3], col[3], cf[3], rp_c_j0;      // the R1CS template (j >= 1 form) and C's row pointers at j = 0
    DevBuf ins, lvl, terms, code;              // the witness program
};

}  // namespace zk

namespace {

struct EvalArgs {
    const PrimeInstr *ins;
    const uint32_t *lvl, *terms;
    const Fr *src;                             // canonical
    uint8_t *bits;                             // [num_witness]
    uint32_t lvl_base[PRIME_PROGRAM_PARTS + 1], wit_base[PRIME_PROGRAM_PARTS + 1];
};

// one workgroup per part: its bits live in LDS (dynamic, max_part bytes); level by level, a barrier between levels.  Every index
// was checked when the program was recorded (operands and destinations inside the part, sources and terms inside their arrays).
__global__ void __launch_bounds__(1024) prime_witness_eval_kernel(EvalArgs g) {
    extern __shared__ uint8_t sb[];
    const int p = blockIdx.x;
    const uint32_t lo = g.wit_base[p], n = g.wit_base[p + 1] - lo;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) sb[i] = 0;
    __syncthreads();
    for (uint32_t L = g.lvl_base[p]; L < g.lvl_base[p + 1]; L++) {
        const uint32_t e = g.lvl[L + 1];
        for (uint32_t i = g.lvl[L] + threadIdx.x; i < e; i += blockDim.x) prime_exec(g.ins[i], sb, g.terms, g.src);
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) g.bits[lo + i] = sb[i];
}

// z[v] = slot, one or zero by code[v]; thread t writes half t & 1 of entry t >> 1 (16-byte stores, coalesced)
__global__ void __launch_bounds__(256) prime_witness_expand_kernel(const uint32_t *code, const uint8_t *bits, const Fr *slots, uint4 *z, uint64_t halves) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= halves) return;
    const uint32_t c = code[t >> 1], h = (uint32_t)t & 1u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (c & PRIME_SLOT) {
        v = reinterpret_cast<const uint4 *>(slots + (c & ~PRIME_SLOT))[h];
    } else if (bits[c]) {
        const Fr one = Fr::one();
        v = make_uint4(one.l[4 * h], one.l[4 * h + 1], one.l[4 * h + 2], one.l[4 * h + 3]);
    }
    z[t] = v;
}

// The same on a (part, request) grid: request r reads its sources at in + r * in_stride + n_slots and writes its bits at
// bits + r * num_witness.  grid.y is capped (option "matrix_batch_grid", else 65,535): a workgroup then takes requests blockIdx.y,
// blockIdx.y + gridDim.y, ... one after another — every lane of it the same number, so the barriers stay uniform.
struct EvalBatchArgs {
    EvalArgs e;                                // src / bits: request 0's
    size_t in_stride, num_witness, k;
};
__global__ void __launch_bounds__(1024) prime_witness_eval_batch_kernel(EvalBatchArgs g) {
    extern __shared__ uint8_t sb[];
    const int p = blockIdx.x;
    const uint32_t lo = g.e.wit_base[p], n = g.e.wit_base[p + 1] - lo;
    for (size_t r = blockIdx.y; r < g.k; r += gridDim.y) {
        const Fr *src = g.e.src + r * g.in_stride;
        uint8_t *bits = g.e.bits + r * g.num_witness;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) sb[i] = 0;
        __syncthreads();
        for (uint32_t L = g.e.lvl_base[p]; L < g.e.lvl_base[p + 1]; L++) {
            const uint32_t e = g.e.lvl[L + 1];
            for (uint32_t i = g.e.lvl[L] + threadIdx.x; i < e; i += blockDim.x) prime_exec(g.e.ins[i], sb, g.e.terms, src);
            __syncthreads();
        }
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) bits[lo + i] = sb[i];
        __syncthreads();                       // the next request clears the bits this one is still writing out
    }
}

// prime_witness_expand_kernel for K requests: z[r] is request r's assignment (a table of addresses into one allocation); both grid
// dimensions are capped as above and loop beyond
__global__ void __launch_bounds__(256) prime_witness_expand_batch_kernel(const uint32_t *code, const uint8_t *bits, const Fr *in, Fr *const *z,
                                                                         uint64_t halves, size_t k, size_t in_stride, size_t num_witness) {
    const Fr one = Fr::one();
    for (size_t r = blockIdx.y; r < k; r += gridDim.y) {
        const uint8_t *rb = bits + r * num_witness;
        const Fr *slots = in + r * in_stride;
        uint4 *zr = reinterpret_cast<uint4 *>(z[r]);
        for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < halves; t += (uint64_t)gridDim.x * blockDim.x) {
            const uint32_t c = code[t >> 1], h = (uint32_t)t & 1u;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (c & PRIME_SLOT) v = reinterpret_cast<const uint4 *>(slots + (c & ~PRIME_SLOT))[h];
            else if (rb[c]) v = make_uint4(one.l[4 * h], one.l[4 * h + 1], one.l[4 * h + 2], one.l[4 * h + 3]);
            zr[t] = v;
        }
    }
}

template <class T>
void upload(zkg16_ctx *ctx, DevBuf &b, const std::vector<T> &v) {
    b.alloc(v.size() * sizeof(T));
    if (!v.empty()) ZK_HIP(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
}

// the root ctx's resident copy, uploaded on first use (callers hold ctx->mu)
std::shared_ptr<PrimeDev> prime_dev_get(zkg16_ctx *ctx, int *status) {
    zkg16_ctx *root = ctx->root ? ctx->root : ctx;
    if (root->prime_dev) return root->prime_dev;
    std::shared_ptr<const PrimeProgram> P;
    if ((*status = prime_program(P)) != ZKG16_OK) return nullptr;
    auto d = std::make_shared<PrimeDev>();
    d->prog = P;
    for (int m = 0; m < 3; m++) {
        upload(ctx, d->rp[m], P->rp[m]);
        upload(ctx, d->col[m], P->col[m]);
        upload(ctx, d->cf[m], P->cf[m]);
    }
    upload(ctx, d->rp_c_j0, P->rp_c_j0);
    upload(ctx, d->ins, P->ins);
    upload(ctx, d->lvl, P->lvl);
    upload(ctx, d->terms, P->terms);
    upload(ctx, d->code, P->code);
    ZK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(prime_witness_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P->max_part));
    ZK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(prime_witness_eval_batch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P->max_part));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    root->prime_dev = d;
    return d;
}

Fr fr_mont_u64(uint64_t v) {
    Fr c = Fr::zero();
    c.l[0] = (uint32_t)v;
    c.l[1] = (uint32_t)(v >> 32);
    return fp_to_mont(c);
}

}  // namespace

namespace zk {

std::shared_ptr<R1csDev> prime_r1cs_on_device(zkg16_ctx *ctx, uint64_t x, uint64_t j, int *status) {
    *status = ZKG16_OK;
    std::shared_ptr<PrimeDev> D = prime_dev_get(ctx, status);
    if (!D) return nullptr;
    const PrimeProgram &P = *D->prog;
    std::vector<Fr> slots, src;
    uint32_t n = 0;
    if ((*status = prime_inputs(P, x, j, slots, src, &n)) != ZKG16_OK) return nullptr;
    const size_t nc = P.num_constraints;
    int log_n = 0;
    while (((size_t)1 << log_n) < nc + P.num_instance) log_n++;
    auto r = std::make_shared<R1csDev>();
    r->num_instance = P.num_instance;
    r->num_constraints = nc;
    r->num_variables = P.num_instance + P.num_witness;
    r->log_n = log_n;
    const auto d2d = [&](void *dst, const void *s, size_t bytes) {
        if (bytes) ZK_HIP(hipMemcpyAsync(dst, s, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    };
    for (int m = 0; m < 3; m++) {
        const size_t nnz = P.col[m].size(), drop = (m == 2 && j == 0) ? 1 : 0;
        r->nnz[m] = nnz - drop;
        r->rp[m].alloc((nc + 1) * sizeof(uint64_t));
        r->col[m].alloc(r->nnz[m] * sizeof(uint32_t));
        r->cf[m].alloc(r->nnz[m] * sizeof(Fr));
        d2d(r->rp[m].p, (drop ? D->rp_c_j0 : D->rp[m]).p, (nc + 1) * sizeof(uint64_t));
        if (!drop) {
            d2d(r->col[m].p, D->col[m].p, nnz * sizeof(uint32_t));
            d2d(r->cf[m].p, D->cf[m].p, nnz * sizeof(Fr));
        } else {                 // C without its column-0 term in the packing row of x + j
            const size_t k = P.c_pos;
            d2d(r->col[m].p, D->col[m].p, k * sizeof(uint32_t));
            d2d(r->col[m].as<uint32_t>() + k, D->col[m].as<uint32_t>() + k + 1, (nnz - k - 1) * sizeof(uint32_t));
            d2d(r->cf[m].p, D->cf[m].p, k * sizeof(Fr));
            d2d(r->cf[m].as<Fr>() + k, D->cf[m].as<Fr>() + k + 1, (nnz - k - 1) * sizeof(Fr));
        }
    }
    const Fr fn = fr_mont_u64(n), mj = fp_neg(fr_mont_u64(j));
    for (int k = 0; k < 3; k++) ZK_HIP(hipMemcpyAsync(r->cf[0].as<Fr>() + P.a_pos[k], &fn, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    if (j != 0) ZK_HIP(hipMemcpyAsync(r->cf[2].as<Fr>() + P.c_pos, &mj, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));      // fn / mj are read by the copies above
    return r;
}

std::shared_ptr<R1csDev> prime_r1cs_template_on_device(zkg16_ctx *ctx, int *status) {
    *status = ZKG16_OK;
    std::shared_ptr<PrimeDev> D = prime_dev_get(ctx, status);
    if (!D) return nullptr;
    const PrimeProgram &P = *D->prog;
    const size_t nc = P.num_constraints;
    int log_n = 0;
    while (((size_t)1 << log_n) < nc + P.num_instance) log_n++;
    auto r = std::make_shared<R1csDev>();
    r->num_instance = P.num_instance;
    r->num_constraints = nc;
    r->num_variables = P.num_instance + P.num_witness;
    r->log_n = log_n;
    r->prime_template = true;
    for (int k = 0; k < 4; k++) r->patch_rows[k] = P.patch_rows[k];
    for (int m = 0; m < 3; m++) {
        const size_t nnz = P.col[m].size();
        r->nnz[m] = nnz;
        r->rp[m].alloc((nc + 1) * sizeof(uint64_t));
        r->col[m].alloc(nnz * sizeof(uint32_t));
        r->cf[m].alloc(nnz * sizeof(Fr));
        ZK_HIP(hipMemcpyAsync(r->rp[m].p, D->rp[m].p, (nc + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        ZK_HIP(hipMemcpyAsync(r->col[m].p, D->col[m].p, nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        ZK_HIP(hipMemcpyAsync(r->cf[m].p, D->cf[m].p, nnz * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    }
    for (int k = 0; k < 3; k++) ZK_HIP(hipMemsetAsync(r->cf[0].as<Fr>() + P.a_pos[k], 0, sizeof(Fr), ctx->stream));
    ZK_HIP(hipMemsetAsync(r->cf[2].as<Fr>() + P.c_pos, 0, sizeof(Fr), ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    return r;
}

int prime_batch_inputs(const uint64_t *xs, const uint64_t *js, size_t k, std::vector<Fr> &in, uint32_t *ns, size_t *stride) {
    std::shared_ptr<const PrimeProgram> Pp;
    if (const int st = prime_program(Pp)) return st;
    const PrimeProgram &P = *Pp;
    const size_t in_stride = P.n_slots + P.n_sources;
    if (k == 0 || k > SIZE_MAX / ((P.num_instance + P.num_witness) * sizeof(Fr))) return ZKG16_ERR_BAD_ARG;
    std::vector<Fr> all(k * in_stride), slots, src;
    std::vector<uint32_t> n(k);
    for (size_t i = 0; i < k; i++) {
        if (const int st = prime_inputs(P, xs[i], js[i], slots, src, &n[i])) return st;
        memcpy(all.data() + i * in_stride, slots.data(), P.n_slots * sizeof(Fr));
        memcpy(all.data() + i * in_stride + P.n_slots, src.data(), P.n_sources * sizeof(Fr));
    }
    in.swap(all);
    if (ns) memcpy(ns, n.data(), k * sizeof(uint32_t));
    if (stride) *stride = in_stride;
    return ZKG16_OK;
}

void prime_witness_batch_assign(zkg16_ctx *ctx, const Fr *in, size_t k, std::vector<std::shared_ptr<WitnessDev>> &out, float *dev_ms) {
    zkg16_ctx *root = ctx->root ? ctx->root : ctx;
    int status = ZKG16_OK;
    // a lane gets here only with the template's handle in hand, which was made from the resident copy: it exists
    std::shared_ptr<PrimeDev> D = ctx == root ? prime_dev_get(ctx, &status) : root->prime_dev;
    if (!D) throw HipError{hipErrorInvalidValue, "prime batch: no resident program", __FILE__, __LINE__};
    const PrimeProgram &P = *D->prog;
    const size_t in_stride = P.n_slots + P.n_sources, total = P.num_instance + P.num_witness;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t in_bytes = up(k * in_stride * sizeof(Fr)), bytes = in_bytes + up(k * sizeof(Fr *));
    const size_t cap = ctx->opt.matrix_batch_grid > 0 ? (size_t)ctx->opt.matrix_batch_grid : 65535;
    mbatch_staging_ensure(ctx, bytes);
    auto backing = std::make_shared<DevBuf>(k * total * sizeof(Fr));
    std::vector<std::shared_ptr<WitnessDev>> wits(k);
    for (size_t i = 0; i < k; i++) {
        wits[i] = std::make_shared<WitnessDev>();
        wits[i]->n = total;
        wits[i]->backing = backing;
        wits[i]->z.p = backing->as<Fr>() + i * total;
        wits[i]->z.bytes = total * sizeof(Fr);
    }
    DevBuf d_bits(k * P.num_witness);
    uint8_t *hs = static_cast<uint8_t *>(ctx->mbatch_host), *ds = ctx->mbatch_dev.as<uint8_t>();
    memcpy(hs, in, k * in_stride * sizeof(Fr));
    Fr **h_tab = reinterpret_cast<Fr **>(hs + in_bytes);
    for (size_t i = 0; i < k; i++) h_tab[i] = wits[i]->z.as<Fr>();

    hipEvent_t e0, e1;
    ZK_HIP(hipEventCreate(&e0));
    struct EvGuard { hipEvent_t e; ~EvGuard() { (void)hipEventDestroy(e); } } g0{e0};
    ZK_HIP(hipEventCreate(&e1));
    EvGuard g1{e1};
    struct Drain { zkg16_ctx *c; bool ok = false; ~Drain() { if (!ok) (void)hipStreamSynchronize(c->stream); } } drain{ctx};
    ZK_HIP(hipEventRecord(e0, ctx->stream));
    ZK_HIP(hipMemcpyAsync(ds, hs, in_bytes + k * sizeof(Fr *), hipMemcpyHostToDevice, ctx->stream));      // the one upload: inputs | z table
    const Fr *d_in = reinterpret_cast<const Fr *>(ds);
    {
        EvalBatchArgs g;
        memset(&g, 0, sizeof g);
        g.e.ins = D->ins.as<PrimeInstr>();
        g.e.lvl = D->lvl.as<uint32_t>();
        g.e.terms = D->terms.as<uint32_t>();
        g.e.src = d_in + P.n_slots;
        g.e.bits = d_bits.as<uint8_t>();
        for (int p = 0; p <= PRIME_PROGRAM_PARTS; p++) {
            g.e.lvl_base[p] = P.lvl_base[p];
            g.e.wit_base[p] = P.wit_base[p];
        }
        g.in_stride = in_stride;
        g.num_witness = P.num_witness;
        g.k = k;
        ScopedKernelTimer kt(ctx, "prime_witness_eval_batch_kernel", (double)P.ins.size() * (double)k);
        hipLaunchKernelGGL(prime_witness_eval_batch_kernel, dim3(PRIME_PROGRAM_PARTS, (unsigned)(k < cap ? k : cap)), dim3(1024), P.max_part, ctx->stream, g);
        ZK_HIP(hipGetLastError());
    }
    {
        const uint64_t halves = 2 * (uint64_t)total;
        const size_t bx = (size_t)((halves + 255) / 256);
        ScopedKernelTimer kt(ctx, "prime_witness_expand_batch_kernel", (double)total * (double)k);
        hipLaunchKernelGGL(prime_witness_expand_batch_kernel, dim3((unsigned)(bx < cap ? bx : cap), (unsigned)(k < cap ? k : cap)), dim3(256), 0, ctx->stream,
                           D->code.as<uint32_t>(), d_bits.as<uint8_t>(), d_in, reinterpret_cast<Fr *const *>(ds + in_bytes), halves, k, in_stride,
                           (size_t)P.num_witness);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipEventRecord(e1, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));      // the staging is free again, and the assignments are whole
    drain.ok = true;
    if (dev_ms) ZK_HIP(hipEventElapsedTime(dev_ms, e0, e1));
    out = std::move(wits);
}

std::shared_ptr<WitnessDev> prime_witness_on_device(zkg16_ctx *ctx, uint64_t x, uint64_t j, int *status) {
    *status = ZKG16_OK;
    std::shared_ptr<PrimeDev> D = prime_dev_get(ctx, status);
    if (!D) return nullptr;
    const PrimeProgram &P = *D->prog;
    std::vector<Fr> in, src;
    if ((*status = prime_inputs(P, x, j, in, src, nullptr)) != ZKG16_OK) return nullptr;
    in.insert(in.end(), src.begin(), src.end());           // one upload: slots | sources
    DevBuf d_in(in.size() * sizeof(Fr)), d_bits(P.num_witness);
    ZK_HIP(hipMemcpyAsync(d_in.p, in.data(), in.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    auto w = std::make_shared<WitnessDev>();
    w->n = P.num_instance + P.num_witness;
    w->z.alloc(w->n * sizeof(Fr));
    EvalArgs g;
    memset(&g, 0, sizeof g);
    g.ins = D->ins.as<PrimeInstr>();
    g.lvl = D->lvl.as<uint32_t>();
    g.terms = D->terms.as<uint32_t>();
    g.src = d_in.as<Fr>() + P.n_slots;
    g.bits = d_bits.as<uint8_t>();
    for (int p = 0; p <= PRIME_PROGRAM_PARTS; p++) {
        g.lvl_base[p] = P.lvl_base[p];
        g.wit_base[p] = P.wit_base[p];
    }
    {
        ScopedKernelTimer kt(ctx, "prime_witness_eval_kernel", (double)P.ins.size());
        hipLaunchKernelGGL(prime_witness_eval_kernel, dim3(PRIME_PROGRAM_PARTS), dim3(1024), P.max_part, ctx->stream, g);
    }
    {
        const uint64_t halves = 2 * (uint64_t)w->n;
        ScopedKernelTimer kt(ctx, "prime_witness_expand_kernel", (double)w->n);
        hipLaunchKernelGGL(prime_witness_expand_kernel, dim3((unsigned)((halves + 255) / 256)), dim3(256), 0, ctx->stream, D->code.as<uint32_t>(),
                           d_bits.as<uint8_t>(), d_in.as<Fr>(), w->z.as<uint4>(), halves);
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(ctx->stream));      // `in` and the scratch buffers are read by the copies and kernels above
    return w;
}

}  // namespace zk
