// libzkg16 C ABI, part 2 of 8 (api.hip): residency — proving keys and their shards (load, slice, shard plans, window tables), R1CS
// matrices, synthesized circuits and assignments; the host -> device upload helpers the other parts share; a key to and from arkworks'
// ProvingKey bytes (at the end of the file).
#include "api_internal.hpp"

using namespace zk;

namespace {
inline void convert_bases(zkg16_ctx *ctx, const G1Affine *in, G1AffineU *out, size_t n) { convert_g1_bases(ctx, in, out, n); }
inline void convert_bases(zkg16_ctx *ctx, const G2Affine *in, G2AffineU *out, size_t n) { convert_g2_bases(ctx, in, out, n); }

}  // namespace

namespace zk {
template <class A>
void upload_points(zkg16_ctx *ctx, typename UOf<A>::T *dst, const uint64_t *src, const uint8_t *inf, size_t lo, size_t hi) {
    if (hi <= lo) return;
    const size_t n = hi - lo;
    const A *s = reinterpret_cast<const A *>(src) + lo;
    DevBuf stage(n * sizeof(A));
    if (!inf) {
        ZK_HIP(hipMemcpyAsync(stage.p, s, n * sizeof(A), hipMemcpyHostToDevice, ctx->stream));
    } else {
        std::vector<A> tmp(s, s + n);
        for (size_t i = 0; i < n; i++)
            if (inf[lo + i]) tmp[i] = A::inf();
        ZK_HIP(hipMemcpyAsync(stage.p, tmp.data(), n * sizeof(A), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));      // tmp is freed at scope exit
    }
    convert_bases(ctx, stage.as<A>(), dst, n);
    ZK_HIP(hipStreamSynchronize(ctx->stream));
}

template <class A>
void upload_one(zkg16_ctx *ctx, typename UOf<A>::T *dst, const A &p) {
    const typename UOf<A>::T u{to_u(p.x), to_u(p.y)};     // host-side conversion (same templates)
    ZK_HIP(hipMemcpyAsync(dst, &u, sizeof(u), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
}
template void upload_points<G1Affine>(zkg16_ctx *, G1AffineU *, const uint64_t *, const uint8_t *, size_t, size_t);
template void upload_points<G2Affine>(zkg16_ctx *, G2AffineU *, const uint64_t *, const uint8_t *, size_t, size_t);
template void upload_one<G1Affine>(zkg16_ctx *, G1AffineU *, const G1Affine &);
template void upload_one<G2Affine>(zkg16_ctx *, G2AffineU *, const G2Affine &);

// validate + allocate (nothing is copied yet)
int r1cs_create(const uint64_t *const rp[3], const uint32_t *const col[3], const uint64_t *const cf[3], size_t num_instance,
                size_t num_constraints, size_t num_variables, std::unique_ptr<R1csDev> &out) {
    if (num_instance == 0) return ZKG16_ERR_BAD_ARG;
    for (int i = 0; i < 3; i++)
        if (!rp[i] || (rp[i][num_constraints] && (!col[i] || !cf[i]))) return ZKG16_ERR_BAD_ARG;
    const size_t dom = num_constraints + num_instance;
    int log_n = 0;
    while (((size_t)1 << log_n) < dom) log_n++;
    if (log_n > 32) return ZKG16_ERR_DOMAIN_TOO_LARGE;      // ark: SynthesisError::PolynomialDegreeTooLarge
    if (log_n > 28) return ZKG16_ERR_DOMAIN_TOO_LARGE;      // build limit (three-pass NTT covers 2^31; 32-bit entry indices cap the MSMs)
    auto r = std::make_unique<R1csDev>();
    r->num_instance = num_instance;
    r->num_constraints = num_constraints;
    r->num_variables = num_variables;
    r->log_n = log_n;
    for (int i = 0; i < 3; i++) {
        const size_t nnz = rp[i][num_constraints];
        // row pointers: start at 0, never decrease, end at nnz — spmv_kernel walks [rp[row], rp[row+1]) unchecked on the device
        if (rp[i][0] != 0) return ZKG16_ERR_BAD_ARG;
        // both scans in slices on a few host threads (86.6 M column indices in the 128x128 circuit: ~0.1 s on one)
        const int T = (nnz + num_constraints) >= ((size_t)1 << 22) ? 8 : 1;
        std::vector<int> bad(T, 0);
        auto scan = [&](int t) {
            const size_t r0 = num_constraints * t / T, r1 = num_constraints * (t + 1) / T;
            for (size_t row = r0; row < r1; row++)
                if (rp[i][row] > rp[i][row + 1]) { bad[t] = 1; return; }
            const size_t k0 = nnz * t / T, k1 = nnz * (t + 1) / T;
            uint32_t top = 0;
            for (size_t k = k0; k < k1; k++) top = col[i][k] > top ? col[i][k] : top;
            if (k1 > k0 && top >= num_variables) bad[t] = 1;
        };
        {
            ThreadGroup tg;
            for (int t = 1; t < T; t++) tg.run([&scan, t]() { scan(t); });
            scan(0);
        }
        for (int t = 0; t < T; t++)
            if (bad[t]) return ZKG16_ERR_BAD_ARG;
        r->nnz[i] = nnz;
        r->rp[i].alloc((num_constraints + 1) * sizeof(uint64_t));
        r->col[i].alloc(nnz * sizeof(uint32_t));
        r->cf[i].alloc(nnz * sizeof(Fr));
    }
    out = std::move(r);
    return ZKG16_OK;
}
// Host -> device copy of a large pageable buffer, queued on ctx->stream.  hipMemcpyAsync from pageable memory goes through
// the runtime's own single-threaded staging (~9 GB/s measured: the 3.5 GB of a 128x128 R1CS took 0.38 s of the 0.55 s
// host-pointer proof); here four host threads fill one half of a pinned ring while the DMA engine drains the other.
static constexpr size_t STAGE_BYTES = (size_t)64 << 20;
void upload_h2d(zkg16_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes < ((size_t)8 << 20)) {
        ZK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return;
    }
    for (int i = 0; i < 2; i++)
        if (!ctx->stage_host[i]) {
            ZK_HIP(hipHostMalloc(&ctx->stage_host[i], STAGE_BYTES, hipHostMallocDefault));
            ZK_HIP(hipEventCreateWithFlags(&ctx->stage_done[i], hipEventDisableTiming));
        }
    const unsigned char *s = static_cast<const unsigned char *>(src);
    unsigned char *d = static_cast<unsigned char *>(dst);
    int slot = 0;
    for (size_t off = 0; off < bytes; off += STAGE_BYTES, slot ^= 1) {
        const size_t len = bytes - off < STAGE_BYTES ? bytes - off : STAGE_BYTES;
        ZK_HIP(hipEventSynchronize(ctx->stage_done[slot]));         // the copy that last used this half has left it (a fresh event is complete)
        unsigned char *stage = static_cast<unsigned char *>(ctx->stage_host[slot]);
        constexpr int T = 4;
        const size_t part = (len / T + 4095) & ~(size_t)4095;
        {
            ThreadGroup tg;
            for (int t = 1; t < T; t++) {
                const size_t lo = part * t < len ? part * t : len, hi = part * (t + 1) < len ? part * (t + 1) : len;
                tg.run([=]() { if (hi > lo) memcpy(stage + lo, s + off + lo, hi - lo); });
            }
            memcpy(stage, s + off, part < len ? part : len);
        }
        ZK_HIP(hipMemcpyAsync(d + off, stage, len, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipEventRecord(ctx->stage_done[slot], ctx->stream));
    }
}
// host -> device copies of the three matrices, queued on ctx->stream (the call returns when the last piece is staged)
void r1cs_copy(zkg16_ctx *ctx, R1csDev &r, const uint64_t *const rp[3], const uint32_t *const col[3], const uint64_t *const cf[3]) {
    for (int i = 0; i < 3; i++) {
        upload_h2d(ctx, r.rp[i].p, rp[i], (r.num_constraints + 1) * sizeof(uint64_t));
        if (r.nnz[i]) {
            upload_h2d(ctx, r.col[i].p, col[i], r.nnz[i] * sizeof(uint32_t));
            upload_h2d(ctx, r.cf[i].p, cf[i], r.nnz[i] * sizeof(Fr));
        }
    }
}

// ---- zkg16_pk_check: every point of a resident key or shard against zkg16_point_check's rule, where the key lies
static const char *const PK_QUERY_NAMES[5] = {"a_query", "b_g1_query", "b_g2_query", "h_query", "l_query"};
static const char *const PK_SINGLE_NAMES[5] = {"alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2"};
template <class A>
static bool single_good(const A &p, int group) {
    if (p.is_inf()) return false;      // a key's single points are generators' multiples by non-zero trapdoors: infinity is a broken key
    uint64_t limbs[sizeof(A) / 8];
    memcpy(limbs, &p, sizeof p);
    int ok = 0;
    return zkg16_point_check(group, limbs, &ok) == ZKG16_OK && ok;
}
void pk_check_run(zkg16_ctx *ctx, const PkDev &pk, PkCheckResult &out) {
    const size_t nz = pk.z_hi - pk.z_lo, nh = pk.h_hi - pk.h_lo;
    // level 0 of a window table is the query itself, at the table's entry stride; the three trailing blinding slots are copies of
    // delta (checked below from the host copies) and are left out
    const size_t s1z = pk.pad_z_g1 ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G1 : sizeof(G1AffineU), s2z = pk.pad_z_g2 ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G2 : sizeof(G2AffineU);
    const size_t s1h = pk.pad_h ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G1 : sizeof(G1AffineU);
    // l_query[j] lies at the index of z[num_instance + j]; the entries below it are infinity by construction
    const size_t l_lo = pk.z_lo > pk.num_instance ? pk.z_lo : pk.num_instance, nl = pk.z_hi > l_lo ? pk.z_hi - l_lo : 0;
    struct Arr { int group; const void *base; size_t stride, n, first; hipStream_t st; };
    const Arr arr[5] = {
        {1, pk.a.p, s1z, nz, pk.z_lo, ctx->slots[1].stream},
        {1, pk.b1.p, s1z, nz, pk.z_lo, ctx->slots[2].stream},
        {2, pk.b2.p, s2z, nz, pk.z_lo, ctx->slots[0].stream},
        {1, pk.h.p, s1h, nh, pk.h_lo, ctx->stream},
        {1, static_cast<const unsigned char *>(pk.l.p) + (l_lo - pk.z_lo) * s1z, s1z, nl, l_lo - pk.num_instance, ctx->slots[3].stream},
    };
    const VbEndo en = vb_endo();
    DevBuf res(10 * sizeof(uint64_t));
    VbEvents ev;           // [0] the fork; [1 + 2q], [2 + 2q] around the kernel of query q
    const double t0 = now_ms();
    // the slot is written on the main stream; the four small queries run beside h_query on streams of their own and are joined again
    pk_check_init_launch(ctx->stream, res.as<uint64_t>(), 5);
    ZK_HIP(hipEventRecord(ev.ev[0], ctx->stream));
    for (int q = 0; q < 5; q++) {
        if (arr[q].st != ctx->stream) ZK_HIP(hipStreamWaitEvent(arr[q].st, ev.ev[0], 0));
        ZK_HIP(hipEventRecord(ev.ev[1 + 2 * q], arr[q].st));
        pk_check_launch(arr[q].st, arr[q].group, arr[q].base, arr[q].stride, arr[q].n, en, res.as<uint64_t>() + 2 * q);
        ZK_HIP(hipEventRecord(ev.ev[2 + 2 * q], arr[q].st));
    }
    for (int q = 0; q < 5; q++)
        if (arr[q].st != ctx->stream) ZK_HIP(hipStreamWaitEvent(ctx->stream, ev.ev[2 + 2 * q], 0));
    uint64_t host[10];
    ZK_HIP(hipMemcpyAsync(host, res.p, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
    // the single points on the host meanwhile, from the key's own copies
    out.single_mask = (single_good(pk.alpha_g1, 1) ? 0u : 1u) | (single_good(pk.beta_g1, 1) ? 0u : 2u) | (single_good(pk.beta_g2, 2) ? 0u : 4u) |
                      (single_good(pk.delta_g1, 1) ? 0u : 8u) | (single_good(pk.delta_g2, 2) ? 0u : 16u);
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < 5; q++) {
        out.n_bad[q] = host[2 * q];
        out.first_bad[q] = host[2 * q] ? host[2 * q + 1] + arr[q].first : UINT64_MAX;      // the whole key's numbering
        ctx->pkc_timings[K_A + q] = arr[q].n ? vb_elapsed(ev.ev[1 + 2 * q], ev.ev[2 + 2 * q]) : 0.0f;
    }
    ctx->pkc_timings[K_TOTAL] = (float)(now_ms() - t0);
}
// option "pk_validate": the text zkg16_last_error gives for a key zkg16_pk_load refused
static std::string pk_check_text(const PkCheckResult &r) {
    std::string s = "pk_validate: not a point of the group:";
    for (int q = 0; q < 5; q++)
        if (r.n_bad[q]) s += std::string(" ") + PK_QUERY_NAMES[q] + "[" + std::to_string(r.first_bad[q]) + "] (" + std::to_string(r.n_bad[q]) + " in all)";
    for (int b = 0; b < 5; b++)
        if (r.single_mask & (1u << b)) s += std::string(" ") + PK_SINGLE_NAMES[b];
    return s;
}
}  // namespace zk

namespace {
int load_r1cs(zkg16_ctx *ctx, const uint64_t *const rp[3], const uint32_t *const col[3], const uint64_t *const cf[3],
              size_t num_instance, size_t num_constraints, size_t num_variables, uint64_t *handle) {
    if (!handle) return ZKG16_ERR_BAD_ARG;
    std::unique_ptr<R1csDev> r;
    const int rc = r1cs_create(rp, col, cf, num_instance, num_constraints, num_variables, r);
    if (rc) return rc;
    r1cs_copy(ctx, *r, rp, col, cf);
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    *handle = ctx->next_handle++;
    ctx->r1cs.put(*handle, std::move(r));
    return ZKG16_OK;
}
}  // namespace

extern "C" {

int zkg16_pk_load_range(zkg16_ctx *ctx,
                        const uint64_t *a_query, const uint8_t *a_inf, size_t n_a,
                        const uint64_t *b_g1_query, const uint8_t *b_g1_inf, size_t n_b1,
                        const uint64_t *b_g2_query, const uint8_t *b_g2_inf, size_t n_b2,
                        const uint64_t *h_query, const uint8_t *h_inf, size_t n_h,
                        const uint64_t *l_query, const uint8_t *l_inf, size_t n_l,
                        const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                        const uint64_t delta_g1[12], const uint64_t delta_g2[24],
                        size_t num_instance, size_t z_lo, size_t z_hi, size_t h_lo, size_t h_hi, int blinding, uint64_t *pk_handle) {
    if (!pk_handle || !a_query || !b_g1_query || !b_g2_query || (!h_query && n_h) || (!l_query && n_l) || !alpha_g1 || !beta_g1 ||
        !beta_g2 || !delta_g1 || !delta_g2)
        return ZKG16_ERR_BAD_ARG;
    if (n_a == 0 || n_a != n_b1 || n_a != n_b2 || num_instance == 0 || num_instance > n_a || n_l != n_a - num_instance) return ZKG16_ERR_BAD_ARG;
    if (z_lo > z_hi || z_hi > n_a || h_lo > h_hi || h_hi > n_h) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto pk = std::make_unique<PkDev>();
    pk->num_instance = num_instance;
    pk->m_total = n_a;
    pk->n_h_total = n_h;
    pk->z_lo = z_lo; pk->z_hi = z_hi; pk->h_lo = h_lo; pk->h_hi = h_hi;
    pk->blinding = blinding != 0;
    pk->full = z_lo == 0 && z_hi == n_a && h_lo == 0 && h_hi == n_h && pk->blinding;
    const size_t nz = pk->z_hi - pk->z_lo, nh = pk->h_hi - pk->h_lo;
    pk->a.alloc((nz + 3) * sizeof(G1AffineU));
    pk->b1.alloc((nz + 3) * sizeof(G1AffineU));
    pk->l.alloc((nz + 3) * sizeof(G1AffineU));
    pk->b2.alloc((nz + 3) * sizeof(G2AffineU));
    pk->h.alloc((nh ? nh : 1) * sizeof(G1AffineU));
    ZK_HIP(hipMemsetAsync(pk->a.p, 0, pk->a.bytes, ctx->stream));      // (0,0) = infinity everywhere by default
    ZK_HIP(hipMemsetAsync(pk->b1.p, 0, pk->b1.bytes, ctx->stream));
    ZK_HIP(hipMemsetAsync(pk->l.p, 0, pk->l.bytes, ctx->stream));
    ZK_HIP(hipMemsetAsync(pk->b2.p, 0, pk->b2.bytes, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    upload_points<G1Affine>(ctx, pk->a.as<G1AffineU>(), a_query, a_inf, pk->z_lo, pk->z_hi);
    upload_points<G1Affine>(ctx, pk->b1.as<G1AffineU>(), b_g1_query, b_g1_inf, pk->z_lo, pk->z_hi);
    upload_points<G2Affine>(ctx, pk->b2.as<G2AffineU>(), b_g2_query, b_g2_inf, pk->z_lo, pk->z_hi);
    upload_points<G1Affine>(ctx, pk->h.as<G1AffineU>(), h_query, h_inf, pk->h_lo, pk->h_hi);
    // l_query[j] pairs with z[num_instance + j]: place it at the same index as its scalar in this shard's z slice
    {
        const size_t lo = pk->z_lo > num_instance ? pk->z_lo : num_instance, hi = pk->z_hi;
        if (hi > lo)
            upload_points<G1Affine>(ctx, pk->l.as<G1AffineU>() + (lo - pk->z_lo), l_query, l_inf, lo - num_instance, hi - num_instance);
    }
    pk->alpha_g1 = g1_from_abi(alpha_g1, 0);
    pk->beta_g1 = g1_from_abi(beta_g1, 0);
    pk->delta_g1 = g1_from_abi(delta_g1, 0);
    pk->beta_g2 = g2_from_abi(beta_g2, 0);
    pk->delta_g2 = g2_from_abi(delta_g2, 0);
    // extra slots (scalars r, s, -rs):  a += r*delta1 ; b1 += s*delta1 ; b2 += s*delta2 ; l += (-rs)*delta1
    upload_one<G1Affine>(ctx, pk->a.as<G1AffineU>() + nz + 0, pk->delta_g1);
    upload_one<G1Affine>(ctx, pk->b1.as<G1AffineU>() + nz + 1, pk->delta_g1);
    upload_one<G2Affine>(ctx, pk->b2.as<G2AffineU>() + nz + 1, pk->delta_g2);
    upload_one<G1Affine>(ctx, pk->l.as<G1AffineU>() + nz + 2, pk->delta_g1);
    pk->b_mask.alloc(nz + 3);
    pk->b_skipped = b_density_mask_run(ctx, pk->b1.as<G1AffineU>(), pk->b2.as<G2AffineU>(), nz + 3, pk->b_mask.as<uint8_t>());
    if (ctx->opt.pk_validate) {      // before the handle exists: a refused key leaves nothing behind (its buffers go with `pk`)
        PkCheckResult chk;
        pk_check_run(ctx, *pk, chk);
        if (!chk.ok()) {
            ctx->last_error = pk_check_text(chk);
            return ZKG16_ERR_BAD_ARG;
        }
    }
    *pk_handle = ctx->next_handle++;
    ctx->pks.put(*pk_handle, std::move(pk));
    ZK_API_END(ctx)
}

int zkg16_pk_load(zkg16_ctx *ctx,
                  const uint64_t *a_query, const uint8_t *a_inf, size_t n_a,
                  const uint64_t *b_g1_query, const uint8_t *b_g1_inf, size_t n_b1,
                  const uint64_t *b_g2_query, const uint8_t *b_g2_inf, size_t n_b2,
                  const uint64_t *h_query, const uint8_t *h_inf, size_t n_h,
                  const uint64_t *l_query, const uint8_t *l_inf, size_t n_l,
                  const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                  const uint64_t delta_g1[12], const uint64_t delta_g2[24],
                  size_t num_instance, int shard_index, int shard_count, uint64_t *pk_handle) {
    if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return ZKG16_ERR_BAD_ARG;
    return zkg16_pk_load_range(ctx, a_query, a_inf, n_a, b_g1_query, b_g1_inf, n_b1, b_g2_query, b_g2_inf, n_b2, h_query, h_inf, n_h, l_query,
                               l_inf, n_l, alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, num_instance,
                               n_a * (size_t)shard_index / shard_count, n_a * (size_t)(shard_index + 1) / shard_count,
                               n_h * (size_t)shard_index / shard_count, n_h * (size_t)(shard_index + 1) / shard_count, shard_index == 0,
                               pk_handle);
}

// A shard of a key that is already resident (zkg16_setup_resident / an un-sharded zkg16_pk_load): device-to-device copies of
// the index ranges, nothing crosses PCIe.
int zkg16_pk_slice(zkg16_ctx *ctx, uint64_t src_handle, size_t z_lo, size_t z_hi, size_t h_lo, size_t h_hi, int blinding,
                   uint64_t *pk_handle) {
    if (!pk_handle) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto src_ref = ctx->pks.get(src_handle); PkDev *src = src_ref.get();
    if (!src) return ZKG16_ERR_BAD_HANDLE;
    if (!src->full) return ZKG16_ERR_BAD_ARG;
    if (z_lo > z_hi || z_hi > src->m_total || h_lo > h_hi || h_hi > src->n_h_total) return ZKG16_ERR_BAD_ARG;
    auto pk = std::make_unique<PkDev>();
    pk->num_instance = src->num_instance;
    pk->m_total = src->m_total;
    pk->n_h_total = src->n_h_total;
    pk->z_lo = z_lo; pk->z_hi = z_hi; pk->h_lo = h_lo; pk->h_hi = h_hi;
    pk->blinding = blinding != 0;
    pk->full = z_lo == 0 && z_hi == src->m_total && h_lo == 0 && h_hi == src->n_h_total && pk->blinding;
    const size_t nz = z_hi - z_lo, nh = h_hi - h_lo, sm = src->m_total;
    pk->a.alloc((nz + 3) * sizeof(G1AffineU));
    pk->b1.alloc((nz + 3) * sizeof(G1AffineU));
    pk->l.alloc((nz + 3) * sizeof(G1AffineU));
    pk->b2.alloc((nz + 3) * sizeof(G2AffineU));
    pk->h.alloc((nh ? nh : 1) * sizeof(G1AffineU));
    // the shard is a plain key: level 0 of the source (the query itself), packed again when the source's table holds padded entries
    auto cp_range = [&](void *dst, const DevBuf &from, size_t lo, size_t cnt, size_t elem, bool padded) {
        if (!cnt) return;
        const size_t stride = padded ? (elem == sizeof(G2AffineU) ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G2 : (size_t)ZKG16_TABLE_STRIDE_PADDED_G1) : elem;
        const unsigned char *s = static_cast<const unsigned char *>(from.p) + lo * stride;
        if (padded) msm_bases_restride(ctx, s, stride, dst, elem, elem, cnt);
        else ZK_HIP(hipMemcpyAsync(dst, s, cnt * elem, hipMemcpyDeviceToDevice, ctx->stream));
    };
    auto cp = [&](DevBuf &dst, const DevBuf &from, size_t elem, bool padded) {
        cp_range(dst.p, from, z_lo, nz, elem, padded);
        cp_range(static_cast<unsigned char *>(dst.p) + nz * elem, from, sm, 3, elem, padded);      // the three trailing delta slots
    };
    cp(pk->a, src->a, sizeof(G1AffineU), src->pad_z_g1);
    cp(pk->b1, src->b1, sizeof(G1AffineU), src->pad_z_g1);
    cp(pk->l, src->l, sizeof(G1AffineU), src->pad_z_g1);
    cp(pk->b2, src->b2, sizeof(G2AffineU), src->pad_z_g2);
    cp_range(pk->h.p, src->h, h_lo, nh, sizeof(G1AffineU), src->pad_h);
    pk->alpha_g1 = src->alpha_g1; pk->beta_g1 = src->beta_g1; pk->delta_g1 = src->delta_g1;
    pk->beta_g2 = src->beta_g2; pk->delta_g2 = src->delta_g2;
    pk->b_mask.alloc(nz + 3);
    pk->b_skipped = b_density_mask_run(ctx, pk->b1.as<G1AffineU>(), pk->b2.as<G2AffineU>(), nz + 3, pk->b_mask.as<uint8_t>());
    *pk_handle = ctx->next_handle++;
    ctx->pks.put(*pk_handle, std::move(pk));
    ZK_API_END(ctx)
}

// Rank roles for one proof over n_ranks GPUs (host-only, no ctx).  Work is counted in G1 mixed additions: a z-side term
// costs W_z * (2 + density * (1 + kappa)) (L, A, and the B1 / B2 terms that are not infinity; kappa = G2 : G1 addition cost),
// an h term W_h, the witness map omega per domain element.  The first k ranks run the witness map and share h_query; every
// rank takes a share of the z ranges proportional to the time it has left, so that all finish together at
//   T(k) = max( (Z + H + k * WM) / n_ranks,  WM + H / k ),
// and k is the one that minimises T (k = n_ranks is the homogeneous split of round 1: every rank repeats the witness map).
static int default_window_bits(size_t n) {
    if (n >= ((size_t)1 << 23)) return 17;
    if (n >= ((size_t)1 << 20)) return 16;
    if (n >= ((size_t)1 << 17)) return 15;
    if (n >= ((size_t)1 << 14)) return 13;
    int lg = 0;
    while (((size_t)2 << lg) <= n) lg++;
    return lg - 3 < 4 ? 4 : lg - 3;
}
int zkg16_shard_plan(int n_ranks, size_t m_total, size_t n_h, double b_density, int h_ranks, const float *z_cost, uint64_t *ranges,
                     uint8_t *blinding, int *h_ranks_out) {
    return zkg16_shard_plan_tables(n_ranks, m_total, n_h, b_density, h_ranks, z_cost, 0, ranges, blinding, h_ranks_out);
}
int zkg16_shard_plan_tables(int n_ranks, size_t m_total, size_t n_h, double b_density, int h_ranks, const float *z_cost, int window_tables,
                            uint64_t *ranges, uint8_t *blinding, int *h_ranks_out) {
    if (n_ranks < 1 || m_total == 0 || !ranges || !blinding || h_ranks < 0 || h_ranks > n_ranks) return ZKG16_ERR_BAD_ARG;
    if (!(b_density > 0.0) || b_density > 1.0) b_density = 0.8;
    // calibrated on one MI355X playing every rank in turn (tools/shard_calibrate.py, profiles/shard_calibration_r2.txt, 128x128):
    // a z-only shard takes 3.6 ms + 108 ms x its fraction of the z cost (97 ms with window tables on the shard), an h-only shard
    // 23.8 ms (the witness map) + 1.2 ms + 46.0 ms x its fraction of h_query (41.2 ms with tables).  In additions at 6.2 G/s:
    // z side 1.33x (1.19x) its additions, h side 1.13x (1.015x), witness map 8.8 per domain element.
    constexpr double KAPPA = 2.8, OMEGA = 8.8;
    const double Z_OVERHEAD = window_tables ? 1.19 : 1.33, H_OVERHEAD = window_tables ? 0.965 : 1.13;
    const int G = n_ranks;
    const double Wz = 254 / default_window_bits(m_total + 3) + 1, Wh = n_h ? 254 / default_window_bits(n_h) + 1 : 0;
    // z-side work: uniform model, or the caller's per-index costs (in G1 mixed additions: entries of the scalar times the
    // queries in which its base is not the point at infinity, the G2 one counted KAPPA times) — the witness of a real circuit
    // is not uniform (runs of 0 / 1 values, variables absent from B), so equal index ranges are not equal work
    double Z = (double)m_total * Wz * (2.0 + b_density * (1.0 + KAPPA));
    if (z_cost) {
        Z = 0;
        for (size_t i = 0; i < m_total; i++) Z += z_cost[i] > 0 ? (double)z_cost[i] : 0.0;
        if (!(Z > 0)) Z = 1.0;
    }
    Z *= Z_OVERHEAD;
    const double H = H_OVERHEAD * (double)n_h * Wh, WM = n_h ? OMEGA * (double)(n_h + 1) : 0.0;
    // fixed cost of taking part at all (latency chains that do not shrink with the share: the scatter passes and the four / one
    // bucket reductions): ~1.9 ms for the z side, ~0.5 ms for the h side, in additions at 6.2 G/s.  With them a rank whose time
    // is used up by the witness map and its h share takes no z work at all, and small circuits use fewer witness-map ranks.
    // (round 3, profiles/shard_calibration_r3.txt: with the bit-sliced reductions a z-only shard takes 1.9 ms + 96.8 ms x its fraction,
    // an h-only one 24.26 ms (the witness map + 0.46 ms) + 39.1 ms x its fraction: round 2's 3.5 / 1.15 ms became 1.9 / 0.46, and the
    // h-side factor with tables 0.965 — with 1.5 ms / 1.015 the model preferred five witness-map ranks of eight, measured 36.0 against 34.5 ms)
    constexpr double F_Z = 11.8e6, F_H = 2.9e6;
    // time of the plan with k witness-map ranks: smallest T with  sum_i max(0, T - busy_i - F_Z) >= Z,  busy_i = WM + F_H + H/k (i < k)
    auto busy_of = [&](int k, int i) { return i < k ? WM + (n_h ? F_H : 0.0) + H / k : 0.0; };
    auto T_of = [&](int k) {
        double lo = busy_of(k, 0), hi = lo + F_Z + Z + 1.0;
        for (int it = 0; it < 80; it++) {
            const double T = 0.5 * (lo + hi);
            double c = 0;
            for (int i = 0; i < G; i++) { const double x = T - busy_of(k, i) - F_Z; if (x > 0) c += x; }
            if (c >= Z) hi = T; else lo = T;
        }
        return hi;
    };
    int k = h_ranks;
    if (k == 0) {
        k = 1;
        for (int c = 2; c <= G; c++)
            if (T_of(c) < T_of(k) * (1.0 - 1e-9)) k = c;
    }
    const double T = T_of(k);
    std::vector<double> cap(G);
    double cap_sum = 0;
    for (int i = 0; i < G; i++) {
        cap[i] = T - busy_of(k, i) - F_Z;
        if (cap[i] < 0) cap[i] = 0;
        cap_sum += cap[i];
    }
    if (!(cap_sum > 0)) { cap.assign(G, 1.0); cap_sum = G; }
    double acc = 0, run = 0;
    size_t prev = 0, pos = 0;
    bool blind_given = false;
    for (int i = 0; i < G; i++) {
        acc += cap[i];
        size_t hi;
        if (i == G - 1) {
            hi = m_total;
        } else if (!z_cost) {
            hi = (size_t)((double)m_total * (acc / cap_sum) + 0.5);
        } else {                                              // advance until this rank's share of the total cost is reached
            const double target = Z * (acc / cap_sum);
            while (pos < m_total && run < target) { run += Z_OVERHEAD * (z_cost[pos] > 0 ? (double)z_cost[pos] : 0.0); pos++; }
            hi = pos;
        }
        if (hi < prev) hi = prev;
        if (hi > m_total) hi = m_total;
        ranges[4 * i + 0] = prev;
        ranges[4 * i + 1] = hi;
        ranges[4 * i + 2] = i < k ? n_h * (size_t)i / k : 0;
        ranges[4 * i + 3] = i < k ? n_h * (size_t)(i + 1) / k : 0;
        blinding[i] = (!blind_given && hi > prev) ? 1 : 0;
        blind_given = blind_given || blinding[i];
        prev = hi;
    }
    if (h_ranks_out) *h_ranks_out = k;
    return ZKG16_OK;
}

// Window tables for a resident key or shard (msm.hip, "window tables").  window_bits_* = 0: chosen from the query length;
// < 0: leave that side as it is.  All four z-side queries share one width (A and L share a sorted term list, so do B1 and B2).
// Width chosen by a cost model in mixed additions: one per (scalar, window) term plus ~7 per bucket (its two additions of
// the reduction, the lost first slot of its run, its share of the fix-ups), over the widths that end on a window boundary
// (15, 14, 13, 12 windows).  Measured (ms per proof, plain key -> table): 32x32 13.4 -> 12.05 at 17 bits (13.15 at 19, 14.0 at
// 20); 46x46 22.6 -> 19.65 at 17 (21.7 at 19); 128x128 181 -> 171.0 at 20 / 22 for z / h (172.0 at 20 / 20, 172.4 at 22 / 22,
// 176.4 at 19 / 22).  Below 17 bits a bucket run spans more than the four lanes the short fix-up path handles (one resident round
// of accumulation waves is 2^17 lanes) and everything goes through the long path: 46x46 at 16 bits 27.8 ms, at 15 bits 40 ms.
// Every query gets a table by default: with the bit-sliced bucket reduction one bucket set of 2^15 / 2^16 buckets is reduced in ~20
// dependent additions, so even small keys gain (profiles/table_sweep_r3.txt: 4x4 3.5 -> 2.45 ms and 8x8 3.9 -> 3.1 ms at 16 bits, 16x16
// 5.6 -> 4.7 ms and the PrimeCircuit 5.9 -> 4.9 ms at 17; narrower tables lose: few buckets, each a long dependent chain).  Round 2
// left queries under 3 * 2^17 terms plain because the reduction of 2^16 buckets then cost a G2 MSM 6 ms.
static int default_table_bits(size_t n) {
    if (n < ((size_t)1 << 16)) return 16;
    int best = 17;
    double best_cost = 0;
    for (int c : {17, 19, 20, 22}) {
        const double cost = (double)n * (254 / c + 1) + 7.0 * (double)((size_t)1 << (c - 1));
        if (c == 17 || cost < best_cost) { best = c; best_cost = cost; }
    }
    return best;
}
// Entry layout of a window table; the one rule zkg16_pk_precompute and its fit check go by (host-only)
int zkg16_table_layout(int kind, size_t n, int digits, int stride_mode, size_t *entry_stride, uint64_t *bytes) {
    if ((kind != 1 && kind != 2) || digits < 1 || stride_mode < 0 || stride_mode > 2) return ZKG16_ERR_BAD_ARG;
    const uint64_t packed = kind == 1 ? ZKG16_TABLE_STRIDE_PACKED_G1 : ZKG16_TABLE_STRIDE_PACKED_G2;
    const uint64_t padded = kind == 1 ? ZKG16_TABLE_STRIDE_PADDED_G1 : ZKG16_TABLE_STRIDE_PADDED_G2;
    if (n && padded * (uint64_t)digits > UINT64_MAX / (uint64_t)n) return ZKG16_ERR_BAD_ARG;      // (stride x digits < 2^40)
    if (stride_mode == 0) {
        const bool large = packed * (uint64_t)digits * (uint64_t)n >= (uint64_t)ZKG16_TABLE_STRIDE_PAD_MIN_BYTES;
        stride_mode = !large ? 1 : kind == 1 ? ZKG16_TABLE_STRIDE_DEFAULT_G1 : ZKG16_TABLE_STRIDE_DEFAULT_G2;
    }
    const uint64_t stride = stride_mode == 2 ? padded : packed;
    if (entry_stride) *entry_stride = (size_t)stride;
    if (bytes) *bytes = stride * (uint64_t)digits * (uint64_t)n;
    return ZKG16_OK;
}
int zkg16_pk_precompute(zkg16_ctx *ctx, uint64_t pk_handle, int window_bits_z, int window_bits_h, uint64_t *table_bytes) {
    if (window_bits_z > 24 || window_bits_h > 24 || (window_bits_z > 0 && window_bits_z < 4) || (window_bits_h > 0 && window_bits_h < 4))
        return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    std::unique_lock<std::shared_mutex> keys(ctx->key_rw);      // the key's buffers are replaced: no proof on any lane meanwhile
    auto pk_ref = ctx->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    if ((window_bits_z >= 0 && pk->tab_c_z) || (window_bits_h >= 0 && pk->tab_c_h)) return ZKG16_ERR_BAD_ARG;      // already built
    const size_t nz = pk->z_hi - pk->z_lo, nzs = nz + 3, nh = pk->h_hi - pk->h_lo;
    const int cz = window_bits_z < 0 || (nz == 0 && !pk->blinding) ? 0 : window_bits_z ? window_bits_z : default_table_bits(nzs);
    const int ch = window_bits_h < 0 || nh == 0 ? 0 : window_bits_h ? window_bits_h : default_table_bits(nh);
    if ((cz && nzs * (size_t)(254 / cz + 1) >= ((size_t)1 << 31)) || (ch && nh * (size_t)(254 / ch + 1) >= ((size_t)1 << 31))) return ZKG16_ERR_BAD_ARG;
    // the three kinds of table this call may build (z side: three G1 and one G2; h side: one G1), each laid out by zkg16_table_layout
    struct Lay { size_t stride = 0; uint64_t bytes = 0; bool padded = false; } g1z, g2z, g1h;
    auto lay_all = [&](int mode) {
        auto one = [mode](int kind, size_t n, int c) {
            Lay l;
            if (c) (void)zkg16_table_layout(kind, n, 254 / c + 1, mode, &l.stride, &l.bytes);
            l.padded = l.stride == (kind == 1 ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G1 : (size_t)ZKG16_TABLE_STRIDE_PADDED_G2);
            return l;
        };
        g1z = one(1, nzs, cz); g2z = one(2, nzs, cz); g1h = one(1, nh, ch);
        return 3 * g1z.bytes + g2z.bytes + g1h.bytes;
    };
    const uint64_t packed = lay_all(1), want = lay_all(ctx->opt.table_stride);
    if (want > packed) {
        // Padded entries add one seventh.  Where only the packed tables fit what is free now (several ranks rehearsed on one GPU, a
        // key next to other tenants), build those: same proofs.  Free = what the driver reports + the allocation cache's parked
        // blocks (given back on demand); needed on top of the tables: the largest level's XYZZ points and prefix products, while the
        // plain queries are still resident.
        size_t free_b = 0, total_b = 0;
        ZK_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t avail = (uint64_t)free_b + dev_cached_bytes();
        const uint64_t scratch = (uint64_t)std::max(cz ? nzs : (size_t)0, ch ? nh : (size_t)0) * (sizeof(XYZZ<Fq2U>) + sizeof(Fq2U)) + ((uint64_t)64 << 20);
        if (want + scratch > avail) (void)lay_all(1);
    }
    uint64_t added = 0;
    if (cz) {
        DevBuf a = msm_tables_build_g1(ctx, pk->a, nzs, cz, g1z.padded);
        DevBuf l = msm_tables_build_g1(ctx, pk->l, nzs, cz, g1z.padded);
        DevBuf b1 = msm_tables_build_g1(ctx, pk->b1, nzs, cz, g1z.padded);
        DevBuf b2 = msm_tables_build_g2(ctx, pk->b2, nzs, cz, g2z.padded);
        pk->a = std::move(a); pk->l = std::move(l); pk->b1 = std::move(b1); pk->b2 = std::move(b2);      // all four or none
        pk->tab_c_z = cz;
        pk->pad_z_g1 = g1z.padded; pk->pad_z_g2 = g2z.padded;
        added += 3 * g1z.bytes + g2z.bytes - (uint64_t)nzs * (3 * sizeof(G1AffineU) + sizeof(G2AffineU));      // the plain queries are released
    }
    if (ch) {
        pk->h = msm_tables_build_g1(ctx, pk->h, nh, ch, g1h.padded);
        pk->tab_c_h = ch;
        pk->pad_h = g1h.padded;
        added += g1h.bytes - (uint64_t)nh * sizeof(G1AffineU);
    }
    if (table_bytes) *table_bytes = added;
    ZK_API_END(ctx)
}

int zkg16_pk_table_bits(zkg16_ctx *ctx, uint64_t pk_handle, int *window_bits_z, int *window_bits_h) {
    ZK_API_BEGIN(ctx)
    auto pk_ref = ctx->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    if (window_bits_z) *window_bits_z = pk->tab_c_z;
    if (window_bits_h) *window_bits_h = pk->tab_c_h;
    ZK_API_END(ctx)
}

// Is every element of a resident key a point of its group (ark: ProvingKey::deserialize_compressed with Validate::Yes)?  Any handle:
// a whole key or a shard, with or without window tables.  A bad key is an answer, not an error.
int zkg16_pk_check(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t n_bad[5], uint64_t first_bad[5], uint32_t *single_mask, int *ok) {
    if (!n_bad || !first_bad || !single_mask || !ok) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    std::shared_lock<std::shared_mutex> keys(ctx->key_rw);      // zkg16_pk_precompute replaces the buffers under the exclusive lock
    auto pk_ref = ctx->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    PkCheckResult r;
    pk_check_run(ctx, *pk, r);
    memcpy(n_bad, r.n_bad, sizeof r.n_bad);
    memcpy(first_bad, r.first_bad, sizeof r.first_bad);
    *single_mask = r.single_mask;
    *ok = r.ok() ? 1 : 0;
    ZK_API_END(ctx)
}

// The stage entry of the same kernels: n host points in the limbs of zkg16_point_check_batch, uploaded and converted as a key's
// queries are.  No points (n == 0) is accepted, as there: nothing runs, and the answer is that of an array without a bad point.
int zkg16_points_check_bulk(zkg16_ctx *ctx, int group, const uint64_t *points, const uint8_t *inf, size_t n, uint64_t *n_bad, uint64_t *first_bad) {
    if (!ctx || (group != 1 && group != 2) || (!points && n) || !n_bad || !first_bad || n >= ((size_t)1 << 36)) return ZKG16_ERR_BAD_ARG;
    *n_bad = 0;
    *first_bad = UINT64_MAX;
    if (!n) return ZKG16_OK;
    ZK_API_BEGIN(ctx)
    DevBuf pts(n * (group == 1 ? sizeof(G1AffineU) : sizeof(G2AffineU))), res(2 * sizeof(uint64_t));
    EventSet ev;
    const double t0 = now_ms();
    if (group == 1) upload_points<G1Affine>(ctx, pts.as<G1AffineU>(), points, inf, 0, n);
    else upload_points<G2Affine>(ctx, pts.as<G2AffineU>(), points, inf, 0, n);
    const double t1 = now_ms();
    pk_check_init_launch(ctx->stream, res.as<uint64_t>(), 1);
    ZK_HIP(hipEventRecord(ev.ev[0], ctx->stream));
    pk_check_launch(ctx->stream, group, pts.p, group == 1 ? sizeof(G1AffineU) : sizeof(G2AffineU), n, vb_endo(), res.as<uint64_t>());
    ZK_HIP(hipEventRecord(ev.ev[1], ctx->stream));
    uint64_t host[2];
    ZK_HIP(hipMemcpyAsync(host, res.p, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->pkc_timings[K_BULK_KERNEL] = vb_elapsed(ev.ev[0], ev.ev[1]);
    ctx->pkc_timings[K_BULK_UPLOAD] = (float)(t1 - t0);
    *n_bad = host[0];
    *first_bad = host[0] ? host[1] : UINT64_MAX;
    ZK_API_END(ctx)
}

int zkg16_pk_check_timings(zkg16_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms || cap < 0) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int n = cap < K_COUNT ? cap : K_COUNT;
    memcpy(ms, ctx->pkc_timings, n * sizeof(float));
    return n;
}

void zkg16_pk_free(zkg16_ctx *ctx, uint64_t h) {
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    ctx->pks.erase(h);
}

int zkg16_r1cs_load(zkg16_ctx *ctx,
                    const uint64_t *a_row_ptr, const uint32_t *a_col, const uint64_t *a_coeff,
                    const uint64_t *b_row_ptr, const uint32_t *b_col, const uint64_t *b_coeff,
                    const uint64_t *c_row_ptr, const uint32_t *c_col, const uint64_t *c_coeff,
                    size_t num_instance, size_t num_constraints, size_t num_variables, uint64_t *r1cs_handle) {
    ZK_API_BEGIN(ctx)
    const uint64_t *rp[3] = {a_row_ptr, b_row_ptr, c_row_ptr};
    const uint32_t *col[3] = {a_col, b_col, c_col};
    const uint64_t *cf[3] = {a_coeff, b_coeff, c_coeff};
    int rc = load_r1cs(ctx, rp, col, cf, num_instance, num_constraints, num_variables, r1cs_handle);
    if (rc) return rc;
    ZK_API_END(ctx)
}

// A synthesized circuit (zkg16_circuit_*) loaded straight onto the device: the handles zkg16_r1cs_load / zkg16_witness_load would
// return for zkg16_circuit_export's arrays, without those arrays crossing the ABI.  The arrays are written into pinned staging memory
// the ctx keeps (grown on demand): a caller that exported into fresh buffers per request paid for 65 MB of allocation, page faults
// and unmapping around every PrimeCircuit request — and the unmapping slowed the NEXT synthesis from 18 to 45-60 ms on the GPU box.
int zkg16_circuit_load(zkg16_ctx *ctx, const zkg16_circuit *c, uint64_t *r1cs_handle, uint64_t *witness_handle) {
    if (!c || !r1cs_handle || !witness_handle) return ZKG16_ERR_BAD_ARG;
    size_t ni = 0, nw = 0, nc = 0, nnz[3] = {0, 0, 0};
    if (zkg16_circuit_dims(c, &ni, &nw, &nc, nnz) != ZKG16_OK) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    zkg16_ctx *root = ctx->root ? ctx->root : ctx;
    // layout of the staging block: 3 row-pointer arrays, 3 column arrays, 3 coefficient arrays, the assignment; 64-byte aligned
    size_t off[10], total = 0;
    auto place = [&](int i, size_t bytes) { off[i] = total; total += (bytes + 63) & ~(size_t)63; };
    for (int m = 0; m < 3; m++) place(m, (nc + 1) * sizeof(uint64_t));
    for (int m = 0; m < 3; m++) place(3 + m, (nnz[m] ? nnz[m] : 1) * sizeof(uint32_t));
    for (int m = 0; m < 3; m++) place(6 + m, (nnz[m] ? nnz[m] : 1) * sizeof(Fr));
    place(9, (ni + nw) * sizeof(Fr));
    if (root->circuit_stage_bytes < total) {
        if (root->circuit_stage) (void)hipHostFree(root->circuit_stage);
        root->circuit_stage = nullptr;
        root->circuit_stage_bytes = 0;
        ZK_HIP(hipHostMalloc(&root->circuit_stage, total + total / 8, hipHostMallocDefault));
        root->circuit_stage_bytes = total + total / 8;
    }
    uint8_t *base = static_cast<uint8_t *>(root->circuit_stage);
    uint64_t *rp[3], *cf[3], *z = reinterpret_cast<uint64_t *>(base + off[9]);
    uint32_t *col[3];
    for (int m = 0; m < 3; m++) {
        rp[m] = reinterpret_cast<uint64_t *>(base + off[m]);
        col[m] = reinterpret_cast<uint32_t *>(base + off[3 + m]);
        cf[m] = reinterpret_cast<uint64_t *>(base + off[6 + m]);
    }
    if (zkg16_circuit_export(c, rp, col, cf, z) != ZKG16_OK) return ZKG16_ERR_BAD_ARG;
    const uint64_t *crp[3] = {rp[0], rp[1], rp[2]}, *ccf[3] = {cf[0], cf[1], cf[2]};
    const uint32_t *ccol[3] = {col[0], col[1], col[2]};
    auto w = std::make_unique<WitnessDev>();
    w->n = ni + nw;
    w->z.alloc(w->n * sizeof(Fr));
    ZK_HIP(hipMemcpyAsync(w->z.p, z, w->n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    const int rc = load_r1cs(ctx, crp, ccol, ccf, ni, nc, ni + nw, r1cs_handle);      // synchronises the stream: the staging block is free again
    if (rc) return rc;
    *witness_handle = ctx->next_handle++;
    ctx->wits.put(*witness_handle, std::move(w));
    ZK_API_END(ctx)
}

// The MatrixCircuit's R1CS of size n written on the device (matrix_r1cs.hip): a handle as zkg16_r1cs_load would return for the
// arrays of zkg16_circuit_matrix + zkg16_circuit_export, without synthesising or uploading them.
int zkg16_r1cs_matrix(zkg16_ctx *ctx, size_t n, uint64_t *r1cs_handle) {
    if (!r1cs_handle || n < 2 || n > 1024) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    int st = ZKG16_OK;
    std::shared_ptr<R1csDev> r = matrix_r1cs_on_device(ctx, n, &st);
    if (!r) return st;
    *r1cs_handle = ctx->next_handle++;
    ctx->r1cs.put(*r1cs_handle, std::move(r));
    ZK_API_END(ctx)
}

// The FibonacciCircuit's R1CS of `steps` rounds with no request in hand: the matrices do not depend on (a, b), so the host mirror is
// synthesized for (0, 0) and its arrays loaded as zkg16_r1cs_load would — steps + 1 rows of at most three terms, a few hundred KB at
// the largest round counts in use, written once per round count: nothing a kernel would be faster at.
int zkg16_r1cs_fibonacci(zkg16_ctx *ctx, size_t steps, uint64_t *r1cs_handle) {
    if (!ctx || !r1cs_handle || steps > ZKG16_FIBONACCI_STEPS_MAX) return ZKG16_ERR_BAD_ARG;
    zkg16_circuit *raw = nullptr;
    try {                               // the synthesis needs neither the ctx nor the device
        if (const int st = zkg16_circuit_fibonacci(0, 0, steps, &raw)) return st;
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    std::unique_ptr<zkg16_circuit, void (*)(zkg16_circuit *)> c(raw, zkg16_circuit_free);
    size_t ni = 0, nw = 0, nc = 0, nnz[3] = {0, 0, 0};
    if (zkg16_circuit_dims(c.get(), &ni, &nw, &nc, nnz) != ZKG16_OK) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    std::vector<uint64_t> rp[3], cf[3], z((ni + nw) * 4);
    std::vector<uint32_t> col[3];
    uint64_t *prp[3], *pcf[3];
    uint32_t *pcol[3];
    for (int m = 0; m < 3; m++) {
        rp[m].resize(nc + 1);
        col[m].resize(nnz[m] ? nnz[m] : 1);
        cf[m].resize(4 * (nnz[m] ? nnz[m] : 1));
        prp[m] = rp[m].data(); pcol[m] = col[m].data(); pcf[m] = cf[m].data();
    }
    if (zkg16_circuit_export(c.get(), prp, pcol, pcf, z.data()) != ZKG16_OK) return ZKG16_ERR_BAD_ARG;
    const uint64_t *crp[3] = {prp[0], prp[1], prp[2]}, *ccf[3] = {pcf[0], pcf[1], pcf[2]};
    const uint32_t *ccol[3] = {pcol[0], pcol[1], pcol[2]};
    const int rc = load_r1cs(ctx, crp, ccol, ccf, ni, nc, ni + nw, r1cs_handle);      // synchronises the stream: the vectors may go
    if (rc) return rc;
    ZK_API_END(ctx)
}

// The linear-equations circuit's R1CS of size n with no request in hand: the matrices do not depend on (a, b) and have a closed form
// (linear_r1cs_build, circuits.hip), written on the host and loaded as zkg16_r1cs_load would — once per n, in front of a setup that
// costs orders of magnitude more.
int zkg16_r1cs_linear(zkg16_ctx *ctx, size_t n, uint64_t *r1cs_handle) {
    if (!ctx || !r1cs_handle || n == 0 || n > ZKG16_LINEAR_N_MAX) return ZKG16_ERR_BAD_ARG;
    const LinearDims d(n);
    ZK_API_BEGIN(ctx)
    std::vector<uint64_t> rp[3];
    std::vector<uint32_t> col[3];
    std::vector<Fr> cf[3];
    uint64_t *prp[3];
    uint32_t *pcol[3];
    Fr *pcf[3];
    for (int m = 0; m < 3; m++) {
        rp[m].resize(d.nc + 1);
        col[m].resize(d.nnz[m]);
        cf[m].resize(d.nnz[m]);
        prp[m] = rp[m].data(); pcol[m] = col[m].data(); pcf[m] = cf[m].data();
    }
    linear_r1cs_build(n, prp, pcol, pcf);
    const uint64_t *crp[3] = {prp[0], prp[1], prp[2]};
    const uint64_t *ccf[3] = {reinterpret_cast<const uint64_t *>(pcf[0]), reinterpret_cast<const uint64_t *>(pcf[1]),
                              reinterpret_cast<const uint64_t *>(pcf[2])};
    const uint32_t *ccol[3] = {pcol[0], pcol[1], pcol[2]};
    const int rc = load_r1cs(ctx, crp, ccol, ccf, d.ni, d.nc, d.vars(), r1cs_handle);      // synchronises the stream: the vectors may go
    if (rc) return rc;
    ZK_API_END(ctx)
}

// The PrimeCircuit of candidate (x, j) on the device (prime_device.hip): handles as zkg16_r1cs_load / zkg16_witness_load would return
// for the arrays of zkg16_circuit_prime + zkg16_circuit_export, without synthesising or uploading them.  The template is uploaded on
// the first call under ctx->mu (held by every entry here) and stays resident until zkg16_destroy.
int zkg16_r1cs_prime(zkg16_ctx *ctx, uint64_t x, uint64_t j, uint64_t *r1cs_handle) {
    if (!r1cs_handle) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    int st = ZKG16_OK;
    std::shared_ptr<R1csDev> r = prime_r1cs_on_device(ctx, x, j, &st);
    if (!r) return st;
    *r1cs_handle = ctx->next_handle++;
    ctx->r1cs.put(*r1cs_handle, std::move(r));
    ZK_API_END(ctx)
}
int zkg16_witness_prime(zkg16_ctx *ctx, uint64_t x, uint64_t j, uint64_t *witness_handle) {
    if (!witness_handle) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    int st = ZKG16_OK;
    std::shared_ptr<WitnessDev> w = prime_witness_on_device(ctx, x, j, &st);
    if (!w) return st;
    *witness_handle = ctx->next_handle++;
    ctx->wits.put(*witness_handle, std::move(w));
    ZK_API_END(ctx)
}

// The template of every candidate's R1CS as a handle (marked: zkg16_prove_prime_batch takes no other), and k assignments in one pass —
// all or nothing, as zkg16_witness_matrix_batch.
int zkg16_r1cs_prime_template(zkg16_ctx *ctx, uint64_t *r1cs_handle) {
    if (!r1cs_handle) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    int st = ZKG16_OK;
    std::shared_ptr<R1csDev> r = prime_r1cs_template_on_device(ctx, &st);
    if (!r) return st;
    *r1cs_handle = ctx->next_handle++;
    ctx->r1cs.put(*r1cs_handle, std::move(r));
    ZK_API_END(ctx)
}
int zkg16_witness_prime_batch(zkg16_ctx *ctx, const uint64_t *xs, const uint64_t *js, size_t k, uint64_t *witness_handles) {
    if (!ctx || !xs || !js || !witness_handles || k == 0) return ZKG16_ERR_BAD_ARG;
    std::vector<Fr> in;      // the host inputs need neither the ctx nor the device
    try {
        if (const int st = prime_batch_inputs(xs, js, k, in, nullptr, nullptr)) return st;
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    ZK_API_BEGIN(ctx)
    std::vector<std::shared_ptr<WitnessDev>> wits;
    prime_witness_batch_assign(ctx, in.data(), k, wits, nullptr);
    if (const int st = witness_batch_register(ctx, wits, witness_handles)) return st;
    ZK_API_END(ctx)
}

// The arrays behind an r1cs handle, copied back (tests compare the device-written MatrixCircuit with the host synthesis).  Each
// pointer may be null; sizes as at load (num_constraints + 1 row pointers, nnz columns / coefficients per matrix).
int zkg16_r1cs_read(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t *const row_ptr[3], uint32_t *const col[3], uint64_t *const coeff[3],
                    size_t *num_instance, size_t *num_constraints, size_t *num_variables, size_t nnz[3]) {
    ZK_API_BEGIN(ctx)
    auto rc_ref = ctx->r1cs.get(r1cs_handle); R1csDev *rc = rc_ref.get();
    if (!rc) return ZKG16_ERR_BAD_HANDLE;
    if (num_instance) *num_instance = rc->num_instance;
    if (num_constraints) *num_constraints = rc->num_constraints;
    if (num_variables) *num_variables = rc->num_variables;
    for (int m = 0; m < 3; m++) {
        if (nnz) nnz[m] = rc->nnz[m];
        if (row_ptr && row_ptr[m]) ZK_HIP(hipMemcpyAsync(row_ptr[m], rc->rp[m].p, (rc->num_constraints + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (col && col[m] && rc->nnz[m]) ZK_HIP(hipMemcpyAsync(col[m], rc->col[m].p, rc->nnz[m] * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (coeff && coeff[m] && rc->nnz[m]) ZK_HIP(hipMemcpyAsync(coeff[m], rc->cf[m].p, rc->nnz[m] * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_API_END(ctx)
}

void zkg16_r1cs_free(zkg16_ctx *ctx, uint64_t h) {
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    ctx->r1cs.erase(h);
}

int zkg16_witness_load(zkg16_ctx *ctx, const uint64_t *full_assignment, size_t n_assign, uint64_t *witness_handle) {
    if (!full_assignment || !witness_handle || n_assign == 0) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto w = std::make_unique<WitnessDev>();
    w->n = n_assign;
    w->z.alloc(n_assign * sizeof(Fr));
    ZK_HIP(hipMemcpyAsync(w->z.p, full_assignment, n_assign * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    *witness_handle = ctx->next_handle++;
    ctx->wits.put(*witness_handle, std::move(w));
    ZK_API_END(ctx)
}

// The assignment behind a witness handle, copied back to the host (tests compare the device-built MatrixCircuit assignment of
// zkg16_witness_matrix with the host builder's byte for byte).
int zkg16_witness_read(zkg16_ctx *ctx, uint64_t witness_handle, uint64_t *out, size_t n_assign) {
    if (!out) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto w_ref = ctx->wits.get(witness_handle); WitnessDev *w = w_ref.get();
    if (!w) return ZKG16_ERR_BAD_HANDLE;
    if (w->n != n_assign) return ZKG16_ERR_BAD_ARG;
    ZK_HIP(hipMemcpyAsync(out, w->z.p, n_assign * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ZK_API_END(ctx)
}

void zkg16_witness_free(zkg16_ctx *ctx, uint64_t h) {
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    ctx->wits.erase(h);
}

}  // extern "C"

// ---- a proving key as the bytes of ark-groth16 0.4's ProvingKey<Bls12_381>::serialize_compressed (include/zkg16.h has the layout):
// zkg16_pk_bytes_dims / _size and the host forms (no ctx), zkg16_pk_read / _save / _load_bytes on the device where the key lies
namespace {
constexpr size_t PKB_HEAD = 48 + 3 * 96;      // alpha_g1 | beta_g2 | gamma_g2 | delta_g2
constexpr size_t PKB_QSIZE[5] = {48, 48, 96, 48, 48};
constexpr int PKB_QGROUP[5] = {1, 1, 2, 1, 1};
constexpr size_t PKB_PIECE_DEFAULT = (size_t)1 << 19;      // 48 MiB of G2 bytes: one half of the staging ring holds a piece
struct PkbLayout {
    size_t ni = 0, m = 0, n_h = 0, n_l = 0;
    size_t at_abc = 0, at_beta_g1 = 0, at_delta_g1 = 0, at_q[5] = {0, 0, 0, 0, 0};
    size_t n_q(int q) const { return q == 3 ? n_h : q == 4 ? n_l : m; }
};
uint64_t le64(const uint8_t *b) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)b[i] << (8 * i);
    return v;
}
void put_le64(uint8_t *b, uint64_t v) {
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
}
// The five length prefixes and nothing else.  A count is compared with the bytes that remain BEFORE it is multiplied: no product of
// a hostile prefix is ever formed.  false: err names the field
bool pkb_walk(const uint8_t *b, size_t len, PkbLayout &L, std::string &err) {
    size_t pos = 0;
    auto need = [&](size_t k, const char *what) {
        if (len - pos >= k) return true;
        err = std::string("pk bytes: truncated in ") + what;
        return false;
    };
    auto count = [&](size_t item, const char *what, size_t &out) {
        if (!need(8, what)) return false;
        const uint64_t c = le64(b + pos);
        pos += 8;
        if (c > (uint64_t)((len - pos) / item)) {
            err = std::string("pk bytes: ") + what + ": count " + std::to_string(c) + " exceeds the bytes that remain";
            return false;
        }
        out = (size_t)c;
        return true;
    };
    if (!need(PKB_HEAD, "vk")) return false;
    pos = PKB_HEAD;
    if (!count(48, "gamma_abc_g1", L.ni)) return false;
    L.at_abc = pos;
    pos += 48 * L.ni;
    if (!need(96, "beta_g1 / delta_g1")) return false;
    L.at_beta_g1 = pos;
    L.at_delta_g1 = pos + 48;
    pos += 96;
    size_t cnt[5];
    for (int q = 0; q < 5; q++) {
        if (!count(PKB_QSIZE[q], PK_QUERY_NAMES[q], cnt[q])) return false;
        L.at_q[q] = pos;
        pos += PKB_QSIZE[q] * cnt[q];
    }
    if (pos != len) { err = "pk bytes: " + std::to_string(len - pos) + " trailing bytes"; return false; }
    L.m = cnt[0]; L.n_h = cnt[3]; L.n_l = cnt[4];
    if (L.ni == 0 || L.ni > L.m) { err = "pk bytes: gamma_abc_g1: count " + std::to_string(L.ni) + " is not in 1 .. a_query's " + std::to_string(L.m); return false; }
    for (int q = 1; q < 3; q++)
        if (cnt[q] != L.m) { err = std::string("pk bytes: ") + PK_QUERY_NAMES[q] + ": count " + std::to_string(cnt[q]) + " differs from a_query's " + std::to_string(L.m); return false; }
    if (L.n_l != L.m - L.ni) { err = "pk bytes: l_query: count " + std::to_string(L.n_l) + " is not a_query's less gamma_abc_g1's"; return false; }
    return true;
}
bool pkb_size(size_t ni, size_t m, size_t n_h, size_t &bytes) {
    if (ni == 0 || ni > m) return false;
    unsigned __int128 t = PKB_HEAD + 8 + 96 + 5 * 8;
    t += (unsigned __int128)48 * ni + (unsigned __int128)(48 + 48 + 96) * m + (unsigned __int128)48 * n_h + (unsigned __int128)48 * (m - ni);
    if (t > (unsigned __int128)SIZE_MAX) return false;
    bytes = (size_t)t;
    return true;
}
// n points of one group through the host decoders on up to `threads` threads: the smallest index with a status and that status
// (0: none).  out / inf: n x 12 | 24 limbs and n flags
int pkb_decode_host(int group, const uint8_t *src, size_t n, int validate, int threads, uint64_t *out, uint8_t *inf, size_t &bad_at) {
    const size_t sz = group == 1 ? 48 : 96, w = group == 1 ? 12 : 24;
    std::vector<int> st(n ? n : 1, 0);
    vb_parallel(n, threads, 64, [&](size_t lo, size_t hi) {
        if (group == 1) (void)zkg16_g1_decompress(src + sz * lo, hi - lo, out + w * lo, inf + lo, validate, st.data() + lo);
        else (void)zkg16_g2_decompress(src + sz * lo, hi - lo, out + w * lo, inf + lo, validate, st.data() + lo);
    });
    for (size_t i = 0; i < n; i++)
        if (st[i]) { bad_at = i; return st[i]; }
    return 0;
}
void pkb_compress_host(int group, const uint64_t *pts, const uint8_t *inf, size_t n, int threads, uint8_t *out) {
    const size_t sz = group == 1 ? 48 : 96, w = group == 1 ? 12 : 24;
    vb_parallel(n, threads, 256, [&](size_t lo, size_t hi) { (void)zkg16_points_compress(group, pts + w * lo, inf ? inf + lo : nullptr, hi - lo, out + sz * lo); });
}
// the six single points in file order: name, group, offset, whether the key (PkDev) holds it
struct PkbSingle { const char *name; int group; size_t at; };
void pkb_singles(const PkbLayout &L, PkbSingle s[6]) {
    s[0] = {"alpha_g1", 1, 0}; s[1] = {"beta_g2", 2, 48}; s[2] = {"gamma_g2", 2, 144}; s[3] = {"delta_g2", 2, 240};
    s[4] = {"beta_g1", 1, L.at_beta_g1}; s[5] = {"delta_g1", 1, L.at_delta_g1};
}
std::string pkb_status_text(const char *name, bool indexed, size_t i, int status) {
    return std::string(name) + (indexed ? "[" + std::to_string(i) + "]" : std::string()) + ": status " + std::to_string(status);
}
// one single point by the host decoder; a point at infinity is refused as zkg16_pk_check refuses it.  "" = good
std::string pkb_single_host(const PkbSingle &sp, const uint8_t *bytes, int validate, uint64_t out[24]) {
    uint8_t inf = 0;
    int st = 0;
    if (sp.group == 1) (void)zkg16_g1_decompress(bytes + sp.at, 1, out, &inf, validate, &st);
    else (void)zkg16_g2_decompress(bytes + sp.at, 1, out, &inf, validate, &st);
    if (st) return pkb_status_text(sp.name, false, 0, st);
    if (inf) return std::string(sp.name) + ": the point at infinity";
    return std::string();
}
void par_memcpy(void *dst, const void *src, size_t len) {
    if (len < ((size_t)8 << 20)) { memcpy(dst, src, len); return; }
    constexpr int T = 4;
    const size_t part = (len / T + 4095) & ~(size_t)4095;
    unsigned char *d = static_cast<unsigned char *>(dst);
    const unsigned char *s = static_cast<const unsigned char *>(src);
    ThreadGroup tg;
    for (int t = 1; t < T; t++) {
        const size_t lo = part * t < len ? part * t : len, hi = part * (t + 1) < len ? part * (t + 1) : len;
        tg.run([=]() { if (hi > lo) memcpy(d + lo, s + lo, hi - lo); });
    }
    memcpy(d, s, part < len ? part : len);
}
// Pieces between host memory and the kernels through the ctx's pinned ring (two halves of STAGE_BYTES) and two device buffers:
// copies run on the ctx's second stream, kernels on its first, so the copy of piece i + 1 overlaps the kernel of piece i.
// stage_done[s]: the last transfer through pinned half s; krn[s]: the last kernel on device buffer s.
struct PkbPipe {
    zkg16_ctx *ctx;
    hipStream_t copy;
    DevBuf dev[2];
    VbEvents ev;            // [2q], [2q + 1]: around the kernels of query q (q < 5); [10 + s]: krn[s]
    size_t turn = 0;
    double host_ms = 0;
    struct Pending { void *dst = nullptr; size_t bytes = 0; } pending[2];
    PkbPipe(zkg16_ctx *c, size_t dev_bytes) : ctx(c), copy(c->wm_stream) {
        for (int i = 0; i < 2; i++) {
            dev[i].alloc(dev_bytes);
            if (!ctx->stage_host[i]) {
                ZK_HIP(hipHostMalloc(&ctx->stage_host[i], STAGE_BYTES, hipHostMallocDefault));
                ZK_HIP(hipEventCreateWithFlags(&ctx->stage_done[i], hipEventDisableTiming));
            }
        }
    }
    unsigned char *pinned(int s) const { return static_cast<unsigned char *>(ctx->stage_host[s]); }
    // host bytes -> device buffer of the next slot, queued; the caller launches its kernel on ctx->stream and calls kernel_done
    int upload(const void *src, size_t bytes) {
        const int s = (int)(turn++ & 1);
        const double t0 = now_ms();
        ZK_HIP(hipEventSynchronize(ctx->stage_done[s]));            // the transfer that last read this half has left it (a fresh event is complete)
        par_memcpy(pinned(s), src, bytes);
        host_ms += now_ms() - t0;
        ZK_HIP(hipStreamWaitEvent(copy, ev.ev[10 + s], 0));         // the kernel that last read this device buffer is done
        ZK_HIP(hipMemcpyAsync(dev[s].p, pinned(s), bytes, hipMemcpyHostToDevice, copy));
        ZK_HIP(hipEventRecord(ctx->stage_done[s], copy));
        ZK_HIP(hipStreamWaitEvent(ctx->stream, ctx->stage_done[s], 0));
        return s;
    }
    void kernel_done(int s) { ZK_HIP(hipEventRecord(ev.ev[10 + s], ctx->stream)); }
    // the next slot for a kernel that writes dev[s]; what the slot still holds for the host is delivered first
    int claim() {
        const int s = (int)(turn++ & 1);
        flush(s);
        return s;
    }
    // device buffer s (written by the kernel just launched on ctx->stream) -> dst on the host, delivered by a later flush
    void download(int s, void *dst, size_t bytes) {
        kernel_done(s);
        ZK_HIP(hipStreamWaitEvent(copy, ev.ev[10 + s], 0));
        ZK_HIP(hipMemcpyAsync(pinned(s), dev[s].p, bytes, hipMemcpyDeviceToHost, copy));
        ZK_HIP(hipEventRecord(ctx->stage_done[s], copy));
        pending[s].dst = dst;
        pending[s].bytes = bytes;
    }
    void flush(int s) {
        if (!pending[s].bytes) return;
        const double t0 = now_ms();
        ZK_HIP(hipEventSynchronize(ctx->stage_done[s]));
        par_memcpy(pending[s].dst, pinned(s), pending[s].bytes);
        host_ms += now_ms() - t0;
        pending[s].bytes = 0;
    }
    void flush_all() { flush((int)(turn & 1)); flush((int)((turn + 1) & 1)); }      // the older piece first
};
size_t pkb_piece(const zkg16_ctx *ctx, size_t per_point) {
    size_t p = ctx->opt.pk_bytes_piece > 0 ? (size_t)ctx->opt.pk_bytes_piece : PKB_PIECE_DEFAULT;
    if (p * per_point > STAGE_BYTES) p = STAGE_BYTES / per_point;
    return p;
}
// level 0 of a whole key's five queries where they lie: base, entry stride, length (l_query in its own numbering)
struct PkbArr { int group; const unsigned char *base; size_t stride, n; };
void pkb_arrays(const PkDev &pk, PkbArr arr[5]) {
    const size_t s1z = pk.pad_z_g1 ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G1 : sizeof(G1AffineU), s2z = pk.pad_z_g2 ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G2 : sizeof(G2AffineU);
    const size_t s1h = pk.pad_h ? (size_t)ZKG16_TABLE_STRIDE_PADDED_G1 : sizeof(G1AffineU);
    arr[0] = {1, pk.a.as<unsigned char>(), s1z, pk.m_total};
    arr[1] = {1, pk.b1.as<unsigned char>(), s1z, pk.m_total};
    arr[2] = {2, pk.b2.as<unsigned char>(), s2z, pk.m_total};
    arr[3] = {1, pk.h.as<unsigned char>(), s1h, pk.n_h_total};
    arr[4] = {1, pk.l.as<unsigned char>() + pk.num_instance * s1z, s1z, pk.m_total - pk.num_instance};
}
void pkb_query_times(zkg16_ctx *ctx, PkbPipe &pipe, const size_t n[5]) {
    for (int q = 0; q < 5; q++) ctx->pkb_timings[B_A + q] = n[q] ? vb_elapsed(pipe.ev.ev[2 * q], pipe.ev.ev[2 * q + 1]) : 0.0f;
}
}  // namespace

extern "C" {

int zkg16_pk_bytes_dims(const uint8_t *bytes, size_t len, size_t *num_instance, size_t *m, size_t *n_h, size_t *n_l) {
    if (!bytes || !num_instance || !m || !n_h || !n_l) { host_last_error() = "zkg16_pk_bytes_dims: null pointer"; return ZKG16_ERR_BAD_ARG; }
    PkbLayout L;
    std::string err;
    try {
        if (!pkb_walk(bytes, len, L, err)) { host_last_error() = err; return ZKG16_ERR_BAD_ARG; }
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    *num_instance = L.ni; *m = L.m; *n_h = L.n_h; *n_l = L.n_l;
    return ZKG16_OK;
}

int zkg16_pk_bytes_size(size_t num_instance, size_t m, size_t n_h, size_t *bytes) {
    size_t b = 0;
    if (!bytes || !pkb_size(num_instance, m, n_h, b)) { host_last_error() = "zkg16_pk_bytes_size: null pointer, num_instance outside 1 .. m, or a size beyond size_t"; return ZKG16_ERR_BAD_ARG; }
    *bytes = b;
    return ZKG16_OK;
}

int zkg16_pk_serialize_host(const uint64_t *a_query, const uint8_t *a_inf, const uint64_t *b_g1_query, const uint8_t *b_g1_inf, const uint64_t *b_g2_query,
                            const uint8_t *b_g2_inf, const uint64_t *h_query, const uint8_t *h_inf, const uint64_t *l_query, const uint8_t *l_inf,
                            const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24], const uint64_t delta_g1[12],
                            const uint64_t delta_g2[24], const uint64_t gamma_g2[24], const uint64_t *gamma_abc_g1, size_t num_instance, size_t m, size_t n_h,
                            int threads, uint8_t *out, size_t cap, size_t *written) {
    size_t total = 0;
    if (!a_query || !b_g1_query || !b_g2_query || (!h_query && n_h) || (!l_query && m != num_instance) || !alpha_g1 || !beta_g1 || !beta_g2 || !delta_g1 ||
        !delta_g2 || !gamma_g2 || !gamma_abc_g1 || !out || !written || threads < 0 || !pkb_size(num_instance, m, n_h, total) || cap < total) {
        host_last_error() = "zkg16_pk_serialize_host: null pointer, num_instance outside 1 .. m, or cap below zkg16_pk_bytes_size";
        return ZKG16_ERR_BAD_ARG;
    }
    try {
        uint8_t *p = out;
        (void)zkg16_points_compress(1, alpha_g1, nullptr, 1, p); p += 48;
        (void)zkg16_points_compress(2, beta_g2, nullptr, 1, p); p += 96;
        (void)zkg16_points_compress(2, gamma_g2, nullptr, 1, p); p += 96;
        (void)zkg16_points_compress(2, delta_g2, nullptr, 1, p); p += 96;
        put_le64(p, num_instance); p += 8;
        pkb_compress_host(1, gamma_abc_g1, nullptr, num_instance, threads, p); p += 48 * num_instance;
        (void)zkg16_points_compress(1, beta_g1, nullptr, 1, p); p += 48;
        (void)zkg16_points_compress(1, delta_g1, nullptr, 1, p); p += 48;
        const uint64_t *pts[5] = {a_query, b_g1_query, b_g2_query, h_query, l_query};
        const uint8_t *inf[5] = {a_inf, b_g1_inf, b_g2_inf, h_inf, l_inf};
        const size_t n[5] = {m, m, m, n_h, m - num_instance};
        for (int q = 0; q < 5; q++) {
            put_le64(p, n[q]); p += 8;
            pkb_compress_host(PKB_QGROUP[q], pts[q], inf[q], n[q], threads, p); p += PKB_QSIZE[q] * n[q];
        }
        *written = (size_t)(p - out);
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

int zkg16_pk_deserialize_host(const uint8_t *bytes, size_t len, int validate, int threads, uint64_t *a_query, uint8_t *a_inf, uint64_t *b_g1_query, uint8_t *b_g1_inf,
                              uint64_t *b_g2_query, uint8_t *b_g2_inf, uint64_t *h_query, uint8_t *h_inf, uint64_t *l_query, uint8_t *l_inf, uint64_t alpha_g1[12],
                              uint64_t beta_g1[12], uint64_t beta_g2[24], uint64_t delta_g1[12], uint64_t delta_g2[24], uint64_t gamma_g2[24],
                              uint64_t *gamma_abc_g1) {
    if (!bytes || !a_query || !a_inf || !b_g1_query || !b_g1_inf || !b_g2_query || !b_g2_inf || !alpha_g1 || !beta_g1 || !beta_g2 || !delta_g1 || !delta_g2 ||
        !gamma_g2 || !gamma_abc_g1 || threads < 0) {
        host_last_error() = "zkg16_pk_deserialize_host: null pointer";
        return ZKG16_ERR_BAD_ARG;
    }
    try {
        PkbLayout L;
        std::string err;
        if (!pkb_walk(bytes, len, L, err)) { host_last_error() = err; return ZKG16_ERR_BAD_ARG; }
        if ((L.n_h && (!h_query || !h_inf)) || (L.n_l && (!l_query || !l_inf))) { host_last_error() = "zkg16_pk_deserialize_host: null pointer"; return ZKG16_ERR_BAD_ARG; }
        // everything into buffers of the call first: a refusal writes no output
        PkbSingle sp[6];
        pkb_singles(L, sp);
        uint64_t single[6][24];
        std::vector<uint64_t> abc(12 * L.ni), qv[5];
        std::vector<uint8_t> abc_inf(L.ni), qi[5];
        auto refuse = [&](const std::string &text) { host_last_error() = text; return ZKG16_ERR_BAD_ARG; };
        auto abc_run = [&]() {
            size_t at = 0;
            const int st = pkb_decode_host(1, bytes + L.at_abc, L.ni, validate, threads, abc.data(), abc_inf.data(), at);
            return st ? pkb_status_text("gamma_abc_g1", true, at, st) : std::string();
        };
        for (int i = 0; i < 6; i++) {
            if (i == 4) { const std::string t = abc_run(); if (!t.empty()) return refuse(t); }       // file order
            const std::string t = pkb_single_host(sp[i], bytes, validate, single[i]);
            if (!t.empty()) return refuse(t);
        }
        for (int q = 0; q < 5; q++) {
            const size_t n = L.n_q(q);
            qv[q].resize((PKB_QGROUP[q] == 1 ? 12 : 24) * (n ? n : 1));
            qi[q].resize(n ? n : 1);
            size_t at = 0;
            const int st = pkb_decode_host(PKB_QGROUP[q], bytes + L.at_q[q], n, validate, threads, qv[q].data(), qi[q].data(), at);
            if (st) return refuse(pkb_status_text(PK_QUERY_NAMES[q], true, at, st));
        }
        uint64_t *single_out[6] = {alpha_g1, beta_g2, gamma_g2, delta_g2, beta_g1, delta_g1};
        for (int i = 0; i < 6; i++) memcpy(single_out[i], single[i], (sp[i].group == 1 ? 12 : 24) * sizeof(uint64_t));
        memcpy(gamma_abc_g1, abc.data(), 12 * L.ni * sizeof(uint64_t));
        uint64_t *q_out[5] = {a_query, b_g1_query, b_g2_query, h_query, l_query};
        uint8_t *i_out[5] = {a_inf, b_g1_inf, b_g2_inf, h_inf, l_inf};
        for (int q = 0; q < 5; q++) {
            const size_t n = L.n_q(q);
            if (!n) continue;
            memcpy(q_out[q], qv[q].data(), (PKB_QGROUP[q] == 1 ? 12 : 24) * n * sizeof(uint64_t));
            memcpy(i_out[q], qi[q].data(), n);
        }
    } catch (const std::bad_alloc &) {
        return ZKG16_ERR_OOM;
    }
    return ZKG16_OK;
}

// A whole resident key back as zkg16_pk_load's arrays: level 0 of each query where it lies (a window table's first level at the
// table's entry stride), without the three blinding slots, l_query in its own numbering.  Null arrays: the dimensions alone.
int zkg16_pk_read(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t *a_query, uint8_t *a_inf, uint64_t *b_g1_query, uint8_t *b_g1_inf, uint64_t *b_g2_query,
                  uint8_t *b_g2_inf, uint64_t *h_query, uint8_t *h_inf, uint64_t *l_query, uint8_t *l_inf, uint64_t alpha_g1[12], uint64_t beta_g1[12],
                  uint64_t beta_g2[24], uint64_t delta_g1[12], uint64_t delta_g2[24], size_t *num_instance, size_t *m, size_t *n_h) {
    ZK_API_BEGIN(ctx)
    std::shared_lock<std::shared_mutex> keys(ctx->key_rw);
    auto pk_ref = ctx->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    if (!pk->full) return ZKG16_ERR_UNSUPPORTED;
    if (num_instance) *num_instance = pk->num_instance;
    if (m) *m = pk->m_total;
    if (n_h) *n_h = pk->n_h_total;
    uint64_t *q_out[5] = {a_query, b_g1_query, b_g2_query, h_query, l_query};
    uint8_t *i_out[5] = {a_inf, b_g1_inf, b_g2_inf, h_inf, l_inf};
    PkbArr arr[5];
    pkb_arrays(*pk, arr);
    bool any = false, all = true;
    for (int q = 0; q < 5; q++) {
        const bool have = q_out[q] && i_out[q];
        any = any || q_out[q] || i_out[q];
        all = all && (have || !arr[q].n);
    }
    if (!any && !alpha_g1 && !beta_g1 && !beta_g2 && !delta_g1 && !delta_g2) return ZKG16_OK;      // the dimensions alone
    if (!all || !alpha_g1 || !beta_g1 || !beta_g2 || !delta_g1 || !delta_g2) return ZKG16_ERR_BAD_ARG;
    const double t0 = now_ms();
    memset(ctx->pkb_timings, 0, sizeof ctx->pkb_timings);
    const size_t piece = pkb_piece(ctx, sizeof(G2Affine) + 1);
    PkbPipe pipe(ctx, piece * (sizeof(G2Affine) + 1));
    size_t n5[5];
    // a piece travels as its limbs followed by its flags; the host puts the two where they belong
    struct Split { uint64_t *limbs; uint8_t *inf; size_t cnt, w; };
    std::vector<unsigned char> bounce[2];
    Split split[2] = {};
    auto deliver = [&](int s) {
        pipe.flush(s);
        if (!split[s].cnt) return;
        memcpy(split[s].limbs, bounce[s].data(), split[s].cnt * split[s].w);
        memcpy(split[s].inf, bounce[s].data() + split[s].cnt * split[s].w, split[s].cnt);
        split[s].cnt = 0;
    };
    for (int q = 0; q < 5; q++) {
        n5[q] = arr[q].n;
        const size_t w = arr[q].group == 1 ? sizeof(G1Affine) : sizeof(G2Affine);
        for (size_t off = 0; off < arr[q].n; off += piece) {
            const size_t cnt = arr[q].n - off < piece ? arr[q].n - off : piece;
            const int s = (int)(pipe.turn & 1);
            deliver(s);
            (void)pipe.claim();
            if (off == 0) ZK_HIP(hipEventRecord(pipe.ev.ev[2 * q], ctx->stream));
            pk_bytes_read_launch(ctx->stream, arr[q].group, arr[q].base + off * arr[q].stride, arr[q].stride, cnt, pipe.dev[s].as<uint64_t>(),
                                 pipe.dev[s].as<uint8_t>() + cnt * w);
            bounce[s].resize(piece * (sizeof(G2Affine) + 1));
            pipe.download(s, bounce[s].data(), cnt * (w + 1));
            split[s] = Split{q_out[q] + off * (w / 8), i_out[q] + off, cnt, w};
        }
        if (arr[q].n) ZK_HIP(hipEventRecord(pipe.ev.ev[2 * q + 1], ctx->stream));
    }
    deliver((int)(pipe.turn & 1));
    deliver((int)((pipe.turn + 1) & 1));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    point_to_abi(pk->alpha_g1, alpha_g1, nullptr);
    point_to_abi(pk->beta_g1, beta_g1, nullptr);
    point_to_abi(pk->beta_g2, beta_g2, nullptr);
    point_to_abi(pk->delta_g1, delta_g1, nullptr);
    point_to_abi(pk->delta_g2, delta_g2, nullptr);
    pkb_query_times(ctx, pipe, n5);
    ctx->pkb_timings[B_COPY] = (float)pipe.host_ms;
    ctx->pkb_timings[B_TOTAL] = (float)(now_ms() - t0);
    ZK_API_END(ctx)
}

// The bytes of zkg16_pk_serialize_host for zkg16_pk_read's arrays, encoded on the device where the key lies and brought back in
// pieces through the pinned ring.  The handle holds neither gamma_g2 nor gamma_abc_g1: the caller passes them.
int zkg16_pk_save(zkg16_ctx *ctx, uint64_t pk_handle, const uint64_t gamma_g2[24], const uint64_t *gamma_abc_g1, uint8_t *out, size_t cap, size_t *written) {
    if (!gamma_g2 || !gamma_abc_g1 || !out || !written) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    std::shared_lock<std::shared_mutex> keys(ctx->key_rw);
    auto pk_ref = ctx->pks.get(pk_handle); PkDev *pk = pk_ref.get();
    if (!pk) return ZKG16_ERR_BAD_HANDLE;
    if (!pk->full) return ZKG16_ERR_UNSUPPORTED;
    size_t total = 0;
    if (!pkb_size(pk->num_instance, pk->m_total, pk->n_h_total, total) || cap < total) {
        ctx->last_error = "zkg16_pk_save: cap " + std::to_string(cap) + " is below the key's " + std::to_string(total) + " bytes";
        return ZKG16_ERR_BAD_ARG;
    }
    const double t0 = now_ms();
    memset(ctx->pkb_timings, 0, sizeof ctx->pkb_timings);
    const size_t piece = pkb_piece(ctx, 96);
    PkbPipe pipe(ctx, piece * 96);
    PkbArr arr[5];
    pkb_arrays(*pk, arr);
    // where each section goes
    uint8_t *p = out + PKB_HEAD + 8 + 48 * pk->num_instance + 96;
    uint8_t *q_at[5];
    size_t n5[5];
    for (int q = 0; q < 5; q++) {
        n5[q] = arr[q].n;
        q_at[q] = p + 8;
        p += 8 + PKB_QSIZE[q] * arr[q].n;
    }
    for (int q = 0; q < 5; q++) {
        for (size_t off = 0; off < arr[q].n; off += piece) {
            const size_t cnt = arr[q].n - off < piece ? arr[q].n - off : piece;
            const int s = pipe.claim();
            if (off == 0) ZK_HIP(hipEventRecord(pipe.ev.ev[2 * q], ctx->stream));
            pk_bytes_encode_launch(ctx->stream, arr[q].group, arr[q].base + off * arr[q].stride, arr[q].stride, cnt, pipe.dev[s].as<uint8_t>());
            pipe.download(s, q_at[q] + off * PKB_QSIZE[q], cnt * PKB_QSIZE[q]);
        }
        if (arr[q].n) ZK_HIP(hipEventRecord(pipe.ev.ev[2 * q + 1], ctx->stream));
    }
    // the verifying key and the single points on the host meanwhile
    const double tv = now_ms();
    {
        uint64_t limbs[24];
        uint8_t *v = out;
        point_to_abi(pk->alpha_g1, limbs, nullptr); (void)zkg16_points_compress(1, limbs, nullptr, 1, v); v += 48;
        point_to_abi(pk->beta_g2, limbs, nullptr); (void)zkg16_points_compress(2, limbs, nullptr, 1, v); v += 96;
        (void)zkg16_points_compress(2, gamma_g2, nullptr, 1, v); v += 96;
        point_to_abi(pk->delta_g2, limbs, nullptr); (void)zkg16_points_compress(2, limbs, nullptr, 1, v); v += 96;
        put_le64(v, pk->num_instance); v += 8;
        pkb_compress_host(1, gamma_abc_g1, nullptr, pk->num_instance, 0, v); v += 48 * pk->num_instance;
        point_to_abi(pk->beta_g1, limbs, nullptr); (void)zkg16_points_compress(1, limbs, nullptr, 1, v); v += 48;
        point_to_abi(pk->delta_g1, limbs, nullptr); (void)zkg16_points_compress(1, limbs, nullptr, 1, v);
        for (int q = 0; q < 5; q++) put_le64(q_at[q] - 8, arr[q].n);
    }
    ctx->pkb_timings[B_VK] = (float)(now_ms() - tv);
    pipe.flush_all();
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    *written = total;
    pkb_query_times(ctx, pipe, n5);
    ctx->pkb_timings[B_COPY] = (float)pipe.host_ms;
    ctx->pkb_timings[B_TOTAL] = (float)(now_ms() - t0);
    ZK_API_END(ctx)
}

// A whole key from its bytes, decoded on the device straight into the key's arrays: the handle zkg16_pk_load makes from
// zkg16_pk_deserialize_host's arrays.  All or nothing.
int zkg16_pk_load_bytes(zkg16_ctx *ctx, const uint8_t *bytes, size_t len, int validate, uint64_t *pk_handle, uint64_t alpha_g1[12], uint64_t beta_g2[24],
                        uint64_t gamma_g2[24], uint64_t delta_g2[24], uint64_t *gamma_abc_g1, size_t cap_abc) {
    if (!bytes || !pk_handle || !alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1) return ZKG16_ERR_BAD_ARG;
    ZK_API_BEGIN(ctx)
    auto refuse = [&](const std::string &text) { ctx->last_error = text; return ZKG16_ERR_BAD_ARG; };
    PkbLayout L;
    {
        std::string err;
        if (!pkb_walk(bytes, len, L, err)) return refuse(err);
    }
    if (cap_abc < L.ni) return refuse("zkg16_pk_load_bytes: cap_abc " + std::to_string(cap_abc) + " is below num_instance " + std::to_string(L.ni));
    if (L.m + 3 >= ((size_t)1 << 32) || L.n_h >= ((size_t)1 << 32)) return refuse("zkg16_pk_load_bytes: a query of 2^32 points or more");
    const double t0 = now_ms();
    memset(ctx->pkb_timings, 0, sizeof ctx->pkb_timings);
    // the six single points on the host, in file order; gamma_abc_g1 lies between the fourth and the fifth, so a failure of the
    // last two is reported only when gamma_abc_g1 (decoded on the host for that rare answer) has none
    PkbSingle sp[6];
    pkb_singles(L, sp);
    uint64_t single[6][24];
    for (int i = 0; i < 6; i++) {
        const std::string t = pkb_single_host(sp[i], bytes, 0, single[i]);
        if (t.empty()) continue;
        if (i >= 4) {
            std::vector<uint64_t> abc(12 * L.ni);
            std::vector<uint8_t> abc_inf(L.ni);
            size_t at = 0;
            if (const int st = pkb_decode_host(1, bytes + L.at_abc, L.ni, 0, 0, abc.data(), abc_inf.data(), at)) return refuse(pkb_status_text("gamma_abc_g1", true, at, st));
        }
        return refuse(t);
    }
    auto pk = std::make_unique<PkDev>();
    pk->num_instance = L.ni;
    pk->m_total = L.m;
    pk->n_h_total = L.n_h;
    pk->z_lo = 0; pk->z_hi = L.m; pk->h_lo = 0; pk->h_hi = L.n_h;
    pk->blinding = true;
    pk->full = true;
    const size_t nz = L.m;
    pk->a.alloc((nz + 3) * sizeof(G1AffineU));
    pk->b1.alloc((nz + 3) * sizeof(G1AffineU));
    pk->l.alloc((nz + 3) * sizeof(G1AffineU));
    pk->b2.alloc((nz + 3) * sizeof(G2AffineU));
    pk->h.alloc((L.n_h ? L.n_h : 1) * sizeof(G1AffineU));
    ZK_HIP(hipMemsetAsync(pk->a.p, 0, pk->a.bytes, ctx->stream));      // (0,0) = infinity everywhere by default
    ZK_HIP(hipMemsetAsync(pk->b1.p, 0, pk->b1.bytes, ctx->stream));
    ZK_HIP(hipMemsetAsync(pk->l.p, 0, pk->l.bytes, ctx->stream));
    ZK_HIP(hipMemsetAsync(pk->b2.p, 0, pk->b2.bytes, ctx->stream));
    const size_t piece = pkb_piece(ctx, 96);
    PkbPipe pipe(ctx, piece * 96);
    DevBuf res(12 * sizeof(uint64_t)), abc_u(L.ni * sizeof(G1AffineU)), abc_sat(L.ni * (sizeof(G1Affine) + 1));
    pk_bytes_init_launch(ctx->stream, res.as<uint64_t>(), 6);
    struct Dst { int group; unsigned char *base; size_t stride, n; const uint8_t *src; };
    const Dst dst[6] = {
        {1, pk->a.as<unsigned char>(), sizeof(G1AffineU), L.m, bytes + L.at_q[0]},
        {1, pk->b1.as<unsigned char>(), sizeof(G1AffineU), L.m, bytes + L.at_q[1]},
        {2, pk->b2.as<unsigned char>(), sizeof(G2AffineU), L.m, bytes + L.at_q[2]},
        {1, pk->h.as<unsigned char>(), sizeof(G1AffineU), L.n_h, bytes + L.at_q[3]},
        {1, pk->l.as<unsigned char>() + L.ni * sizeof(G1AffineU), sizeof(G1AffineU), L.n_l, bytes + L.at_q[4]},      // l_query[j] at the index of its scalar
        {1, abc_u.as<unsigned char>(), sizeof(G1AffineU), L.ni, bytes + L.at_abc},
    };
    const double tv = now_ms();
    for (int qq = 0; qq < 6; qq++) {
        const int q = (qq + 5) % 6;      // gamma_abc_g1 first, then the queries in file order
        const size_t sz = dst[q].group == 1 ? 48 : 96;
        for (size_t off = 0; off < dst[q].n; off += piece) {
            const size_t cnt = dst[q].n - off < piece ? dst[q].n - off : piece;
            const int s = pipe.upload(dst[q].src + off * sz, cnt * sz);
            if (off == 0 && q < 5) ZK_HIP(hipEventRecord(pipe.ev.ev[2 * q], ctx->stream));
            pk_bytes_decode_launch(ctx->stream, dst[q].group, pipe.dev[s].as<uint8_t>(), cnt, dst[q].base + off * dst[q].stride, dst[q].stride, off, res.as<uint64_t>() + 2 * q);
            pipe.kernel_done(s);
        }
        if (dst[q].n && q < 5) ZK_HIP(hipEventRecord(pipe.ev.ev[2 * q + 1], ctx->stream));
        if (q == 5) {      // gamma_abc_g1 back as limbs
            pk_bytes_read_launch(ctx->stream, 1, abc_u.p, sizeof(G1AffineU), L.ni, abc_sat.as<uint64_t>(), abc_sat.as<uint8_t>() + L.ni * sizeof(G1Affine));
            ctx->pkb_timings[B_VK] = (float)(now_ms() - tv);
        }
    }
    uint64_t host[12];
    std::vector<uint64_t> abc(12 * L.ni);
    ZK_HIP(hipMemcpyAsync(host, res.p, sizeof host, hipMemcpyDeviceToHost, ctx->stream));      // the failures of the whole call, once
    ZK_HIP(hipMemcpyAsync(abc.data(), abc_sat.p, L.ni * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    for (int qq = 0; qq < 6; qq++) {
        const int q = (qq + 5) % 6;
        if (host[2 * q]) return refuse(pkb_status_text(q == 5 ? "gamma_abc_g1" : PK_QUERY_NAMES[q], true, (size_t)(host[2 * q + 1] >> 3), (int)(host[2 * q + 1] & 7)));
    }
    pk->alpha_g1 = g1_from_abi(single[0], 0);
    pk->beta_g2 = g2_from_abi(single[1], 0);
    pk->delta_g2 = g2_from_abi(single[3], 0);
    pk->beta_g1 = g1_from_abi(single[4], 0);
    pk->delta_g1 = g1_from_abi(single[5], 0);
    // the blinding slots and the B-side mask, as zkg16_pk_load_range
    upload_one<G1Affine>(ctx, pk->a.as<G1AffineU>() + nz + 0, pk->delta_g1);
    upload_one<G1Affine>(ctx, pk->b1.as<G1AffineU>() + nz + 1, pk->delta_g1);
    upload_one<G2Affine>(ctx, pk->b2.as<G2AffineU>() + nz + 1, pk->delta_g2);
    upload_one<G1Affine>(ctx, pk->l.as<G1AffineU>() + nz + 2, pk->delta_g1);
    pk->b_mask.alloc(nz + 3);
    pk->b_skipped = b_density_mask_run(ctx, pk->b1.as<G1AffineU>(), pk->b2.as<G2AffineU>(), nz + 3, pk->b_mask.as<uint8_t>());
    if (validate || ctx->opt.pk_validate) {      // before the handle exists, as zkg16_pk_load_range; the verifying key's own points on the host
        PkCheckResult chk;
        pk_check_run(ctx, *pk, chk);
        ctx->pkb_timings[B_CHECK] = ctx->pkc_timings[K_TOTAL];
        if (!chk.ok()) return refuse(pk_check_text(chk));
        int ok = 0;
        if (zkg16_point_check(2, single[2], &ok) != ZKG16_OK || !ok) return refuse("pk_validate: not a point of the group: gamma_g2");
        for (size_t i = 0; i < L.ni; i++) {
            bool zero = true;
            for (int k = 0; k < 12; k++) zero = zero && abc[12 * i + k] == 0;
            if (zero) continue;      // the point at infinity passes, as in the queries
            if (zkg16_point_check(1, abc.data() + 12 * i, &ok) != ZKG16_OK || !ok) return refuse("pk_validate: not a point of the group: gamma_abc_g1[" + std::to_string(i) + "]");
        }
    }
    size_t n5[5];
    for (int q = 0; q < 5; q++) n5[q] = dst[q].n;
    pkb_query_times(ctx, pipe, n5);
    ctx->pkb_timings[B_COPY] = (float)pipe.host_ms;
    memcpy(alpha_g1, single[0], 12 * sizeof(uint64_t));
    memcpy(beta_g2, single[1], 24 * sizeof(uint64_t));
    memcpy(gamma_g2, single[2], 24 * sizeof(uint64_t));
    memcpy(delta_g2, single[3], 24 * sizeof(uint64_t));
    memcpy(gamma_abc_g1, abc.data(), 12 * L.ni * sizeof(uint64_t));
    *pk_handle = ctx->next_handle++;
    ctx->pks.put(*pk_handle, std::move(pk));
    ctx->pkb_timings[B_TOTAL] = (float)(now_ms() - t0);
    ZK_API_END(ctx)
}

int zkg16_pk_bytes_timings(zkg16_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms || cap < 0) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int n = cap < B_COUNT ? cap : B_COUNT;
    memcpy(ms, ctx->pkb_timings, n * sizeof(float));
    return n;
}

}  // extern "C"
