// Split witness map over the ranks of a device group: layout (host), exchange kernel and one rank's share of the witness
// map's transforms.  See group.hpp for the layout; the group object and its entry points are in api_group.hip.
#include <chrono>

#include "group.hpp"

namespace zk {

// ------------------------------------------------------------------------------------------------ layout (host only)
bool group_layout(int log_n, int k, int ntt_mode, GroupLayout &L) {
    L = GroupLayout();
    L.log_n = log_n;
    L.k = k;
    if (k < 1 || k > GROUP_LAYOUT_MAX_K || log_n < 0 || log_n > 31) return false;
    if (!ntt_two_pass_shape(log_n, ntt_mode, &L.log_n1, &L.log_n2, &L.tile_log)) return true;      // single / three passes
    L.n1 = (uint64_t)1 << L.log_n1;
    L.n2 = (uint64_t)1 << L.log_n2;
    L.m = std::min(L.n1, L.n2);
    const uint64_t cols_per_tile = (uint64_t)1 << (L.tile_log - L.log_n1), rows_per_tile = (uint64_t)1 << (L.tile_log - L.log_n2);
    L.unit = std::max(cols_per_tile, rows_per_tile);
    const uint64_t units = L.m / L.unit;
    if ((uint64_t)k > units) return true;                                 // more ranks than the tiles can be split into
    for (int g = 0; g < k; g++) {
        L.lo.push_back((uint64_t)g * units / (uint64_t)k * L.unit);
        L.hi.push_back((uint64_t)(g + 1) * units / (uint64_t)k * L.unit);
    }
    L.applies = true;
    return true;
}

std::vector<GroupRect> group_exchange_rects(const GroupLayout &L) {
    std::vector<GroupRect> out;
    if (!L.applies) return out;
    for (int g = 0; g < L.k; g++)
        for (int h = 0; h < L.k; h++) {
            if (h == g) continue;
            for (uint64_t jr = 0; jr < L.n1 / L.m; jr++)
                for (uint64_t jc = 0; jc < L.n2 / L.m; jc++)
                    out.push_back(GroupRect{h, g, jr * L.m + L.lo[g], jr * L.m + L.hi[g], jc * L.m + L.lo[h], jc * L.m + L.hi[h], L.n2});
        }
    return out;
}

std::vector<GroupRect> group_h_rects(const GroupLayout &L, const uint64_t *h_lo, const uint64_t *h_hi) {
    std::vector<GroupRect> out;
    if (!L.applies) return out;
    const uint64_t m = L.m;
    for (int g = 0; g < L.k; g++) {
        if (h_hi[g] <= h_lo[g]) continue;
        const uint64_t q0 = h_lo[g] / m, q1 = (h_hi[g] - 1) / m;        // first and last row of n = q * m + r
        for (int p = 0; p < L.k; p++) {
            if (p == g) continue;
            auto row_cols = [&](uint64_t q, uint64_t &c0, uint64_t &c1) {
                const uint64_t a = q * m, lo = std::max(L.lo[p], h_lo[g] > a ? h_lo[g] - a : 0), hi = std::min(L.hi[p], h_hi[g] - a);
                c0 = lo;
                c1 = hi;
                return hi > lo;
            };
            uint64_t c0, c1;
            if (row_cols(q0, c0, c1)) out.push_back(GroupRect{p, g, q0, q0 + 1, c0, c1, m});
            if (q1 > q0 + 1) out.push_back(GroupRect{p, g, q0 + 1, q1, L.lo[p], L.hi[p], m});
            if (q1 > q0 && row_cols(q1, c0, c1)) out.push_back(GroupRect{p, g, q1, q1 + 1, c0, c1, m});
        }
    }
    return out;
}

void group_share_tiles(const GroupLayout &L, int g, unsigned cols[4], unsigned rows[4]) {
    const uint64_t cpt = (uint64_t)1 << (L.tile_log - L.log_n1), rpt = (uint64_t)1 << (L.tile_log - L.log_n2);
    auto fill = [&](unsigned t[4], uint64_t reps, uint64_t per_tile) {
        t[0] = (unsigned)(L.lo[g] / per_tile);
        t[1] = (unsigned)((L.hi[g] - L.lo[g]) / per_tile);
        t[2] = reps > 1 ? (unsigned)((L.m + L.lo[g]) / per_tile) : 0u;
        t[3] = reps > 1 ? t[1] : 0u;
    };
    fill(cols, L.n2 / L.m, cpt);
    fill(rows, L.n1 / L.m, rpt);
}

// ------------------------------------------------------------------------------------------------ barrier
void GroupBarrier::wait() {
    std::unique_lock<std::mutex> lk(mu_);
    if (broken_) throw HipError{hipErrorLaunchFailure, "group: a peer rank failed", __FILE__, __LINE__};
    const unsigned gen = gen_;
    if (++count_ == n_) {
        count_ = 0;
        gen_++;
        cv_.notify_all();
        return;
    }
    cv_.wait(lk, [&] { return gen_ != gen || broken_; });
    if (gen_ == gen) throw HipError{hipErrorLaunchFailure, "group: a peer rank failed", __FILE__, __LINE__};
}
void GroupBarrier::brk() {
    std::lock_guard<std::mutex> lk(mu_);
    broken_ = true;
    cv_.notify_all();
}

GroupSync::~GroupSync() {
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (size_t g = 0; g < ev.size(); g++) {
        (void)hipSetDevice(device[g]);
        for (auto &e : ev[g])
            if (e) (void)hipEventDestroy(e);
        for (auto &p : tev[g])
            for (auto &e : p)
                if (e) (void)hipEventDestroy(e);
    }
    (void)hipSetDevice(cur);
}

// ------------------------------------------------------------------------------------------------ device
static constexpr int GATHER_MAX = 32;       // rectangles of one exchange: (k - 1) x 2 for the row pass, (k - 1) x 3 for h, k <= 8
struct GatherArgs {
    const uint4 *src[GATHER_MAX];           // the peer's buffer (same layout as dst)
    uint64_t base[GATHER_MAX];              // position of the rectangle's first element
    uint64_t stride[GATHER_MAX];            // positions between its rows
    uint32_t width[GATHER_MAX];             // 16-byte words per row (2 per element)
    uint32_t nrows[GATHER_MAX];
    uint4 *dst;
};
// one launch per exchange: blockIdx.y = rectangle; each thread moves 16-byte words of it from the peer's buffer into the same
// positions of this rank's buffer
__global__ void __launch_bounds__(256) group_gather_kernel(GatherArgs a) {
    const int r = blockIdx.y;
    const uint32_t w = a.width[r];
    const uint32_t total = w * a.nrows[r];                 // < 2^26: two-pass domains are at most 2^24 elements
    const uint4 *src = a.src[r];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint32_t row = i / w, off = i - row * w;
        const uint64_t p = (a.base[r] + (uint64_t)row * a.stride[r]) * 2 + off;
        a.dst[p] = src[p];
    }
}

// (ab - c) / Z on the positions n with n mod m in [lo, hi) only (option fuse_pointwise 0); c null (six transforms): ab only
__global__ void __launch_bounds__(256) group_pointwise_kernel(Fr *a, const Fr *b, const Fr *c, Fr zinv, uint64_t m, uint64_t lo,
                                                              uint64_t w, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t q = i / w, p = q * m + lo + (i - q * w);
    auto ld = [](const Fr *x) {
        const uint4 *u = reinterpret_cast<const uint4 *>(x);
        const uint4 s = u[0], t = u[1];
        Fr v;
        v.l[0] = s.x; v.l[1] = s.y; v.l[2] = s.z; v.l[3] = s.w; v.l[4] = t.x; v.l[5] = t.y; v.l[6] = t.z; v.l[7] = t.w;
        return v;
    };
    Fr x = fp_mul(ld(a + p), ld(b + p));
    if (c) x = fp_mul(fp_sub(x, ld(c + p)), zinv);
    uint4 *o = reinterpret_cast<uint4 *>(a + p);
    o[0] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
    o[1] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
}

// rank g's gather of `rects` (those with dst == g) from its peers' buffer of role `role` into its own; -> bytes moved
static uint64_t group_gather(zkg16_ctx *ctx, GroupSync &S, int g, int role, const std::vector<GroupRect> &rects, uint64_t n) {
    GatherArgs a;
    memset(&a, 0, sizeof a);
    a.dst = reinterpret_cast<uint4 *>(S.bufs[g][role]);
    int nr = 0;
    uint64_t bytes = 0, widest = 0;
    for (const GroupRect &r : rects) {
        if (r.dst != g) continue;
        if (nr == GATHER_MAX) throw HipError{hipErrorInvalidValue, "group: too many rectangles in one exchange", __FILE__, __LINE__};
        // bounds: every position the rectangle names lies inside both N-element buffers
        if (r.src == g || r.src < 0 || r.src >= S.L.k || r.r1 <= r.r0 || r.c1 <= r.c0 || (r.r1 - 1) * r.stride + r.c1 > n ||
            r.c1 > r.stride || !S.bufs[r.src][role])
            throw HipError{hipErrorInvalidValue, "group: exchange rectangle out of bounds", __FILE__, __LINE__};
        a.src[nr] = reinterpret_cast<const uint4 *>(S.bufs[r.src][role]);
        a.base[nr] = r.r0 * r.stride + r.c0;
        a.stride[nr] = r.stride;
        a.width[nr] = (uint32_t)(2 * (r.c1 - r.c0));
        a.nrows[nr] = (uint32_t)(r.r1 - r.r0);
        const uint64_t words = (uint64_t)a.width[nr] * a.nrows[nr];
        widest = std::max(widest, words);
        bytes += words * 16;
        nr++;
    }
    if (!nr) return 0;
    const unsigned gx = (unsigned)std::min<uint64_t>((widest + 255) / 256, 2048);
    ScopedKernelTimer kt(ctx, "group_gather_kernel", (double)bytes);
    hipLaunchKernelGGL(group_gather_kernel, dim3(gx, (unsigned)nr), dim3(256), 0, ctx->stream, a);
    ZK_HIP(hipGetLastError());
    return bytes;
}

// rank g's rows of the SpMV: the rows i < N with i mod m in [lo, hi), in the handle's length-class order when it has one.  Built
// once per (handle, share) with a host round trip (a resident handle pays it once), then cached on the handle.
static std::shared_ptr<R1csDev::RowShare> group_rows(zkg16_ctx *ctx, R1csDev &m, const GroupLayout &L, int g) {
    std::lock_guard<std::mutex> lk(m.lazy_mu);
    const bool from_perm = m.perm_ok;
    for (auto &rs : m.row_shares)
        if (rs->m == L.m && rs->lo == L.lo[g] && rs->hi == L.hi[g] && rs->from_perm == from_perm) return rs;
    auto rs = std::make_shared<R1csDev::RowShare>();
    rs->m = L.m; rs->lo = L.lo[g]; rs->hi = L.hi[g]; rs->from_perm = from_perm;
    const uint64_t n = (uint64_t)1 << m.log_n, nc = m.num_constraints;
    auto owned = [&](uint64_t i) { const uint64_t r = i % L.m; return r >= L.lo[g] && r < L.hi[g]; };
    std::vector<uint32_t> perm(from_perm ? nc : 0), list;
    for (int i = 0; i < 3; i++) {
        list.clear();
        if (from_perm) {
            ZK_HIP(hipMemcpyAsync(perm.data(), m.perm[i].p, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            ZK_HIP(hipStreamSynchronize(ctx->stream));
            for (uint64_t t = 0; t < nc; t++)
                if (owned(perm[t])) list.push_back(perm[t]);
            for (uint64_t r = nc; r < n; r++)
                if (owned(r)) list.push_back((uint32_t)r);
        } else {
            for (uint64_t r = 0; r < n; r++)
                if (owned(r)) list.push_back((uint32_t)r);
        }
        rs->n[i] = list.size();
        rs->list[i].alloc(list.size() * sizeof(uint32_t));
        ZK_HIP(hipMemcpyAsync(rs->list[i].p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));          // `list` is reused
    }
    m.row_shares.push_back(rs);
    return rs;
}

// Rank g's share of h, the same transforms and the same ping-pong between a, b, c and tmp as witness_map_run (poly.hip:
// wm_transforms): six by default, h = coset_ifft(A_cos B_cos / Z) - ifft(c) / Z with the subtraction on the last row pass's store;
// seven with option wm_transforms = 7.  T = the number of transforms.  Ordering across ranks, per exchange t (one in front of each
// row pass, t < T; the redistribution of h is t = T):
//   - rank g records ev[g][t] on its stream after the writes the peers will read (its column pass; for t = T its last row pass);
//   - a host barrier across the rank threads follows, so no wait below is enqueued before the event it names was recorded;
//   - g's gather waits on ev[h][t] of every peer h.
// The same events cover write after read.  Exchange t reads the peers' buffer src_t (the column pass's); a peer's first later
// write into src_t is either its row pass of t + 1 (src_t = dst_{t+1}) or a pass of t + 2 or later, and every one of those is
// queued behind that peer's own gather of t + 1, which waits on ev[g][t + 1], which g records after its gather of t.  The only
// peer write not behind that wait is its column pass of t + 1, and it runs in place on src_{t+1} != src_t (consecutive
// transforms use different buffers: sources a tmp b tmp c a with six, a tmp b tmp c tmp a with seven).  With six, the last row
// pass reads the rank's own tmp at exactly the positions the same rank's row pass of c wrote (a rank's row tiles are the same in
// every transform): same stream, and gathers write only the gathering rank's own buffers.  No peer reads tmp in between: the
// exchanges there read the source of the last transform, a, and the redistribution's event follows the last row pass.  The
// redistribution (t = T) reads the peers' tmp; no later write to tmp happens in this call, and the next group call's first write to
// tmp (its first row pass) again waits on every rank's next column-pass event, queued after that rank's redistribution.  Nothing
// else here synchronises with the host (the row order of the SpMV is built once per handle and share).
void group_witness_map_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, Fr **h_out, GroupRank &r) {
    GroupSync &S = *r.sync;
    const int g = r.idx;
    const GroupLayout &L = S.L;
    const uint64_t n = (uint64_t)1 << m.log_n;
    if (!L.applies || L.log_n != m.log_n) throw HipError{hipErrorInvalidValue, "group: layout does not match the domain", __FILE__, __LINE__};
    for (int i = 0; i < 4; i++) ctx->poly[i].ensure(n * sizeof(Fr));
    Fr *v[4] = {ctx->poly[0].as<Fr>(), ctx->poly[1].as<Fr>(), ctx->poly[2].as<Fr>(), ctx->poly[3].as<Fr>()};
    S.bufs[g] = {v[0], v[1], v[2], v[3]};
    S.device[g] = ctx->device;
    for (auto &e : S.ev[g])
        if (!e) ZK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const auto rows = group_rows(ctx, m, L, g);
    const SpmvRows sp{{rows->list[0].as<uint32_t>(), rows->list[1].as<uint32_t>(), rows->list[2].as<uint32_t>()}, {rows->n[0], rows->n[1], rows->n[2]}};
    NttTables *tab = ntt_get_tables(ctx, m.log_n);

    // device time of this rank's steps: one event pair per step (between two barriers); with group_serial each step runs alone
    // (the serial mutex is held from its first launch until its stream has drained)
    std::unique_lock<std::mutex> turn(S.serial_mu, std::defer_lock);
    auto step_begin = [&] {
        if (S.serial) turn.lock();
        std::array<hipEvent_t, 2> p{nullptr, nullptr};
        S.tev[g].push_back(p);
        for (auto &e : S.tev[g].back()) ZK_HIP(hipEventCreate(&e));
        ZK_HIP(hipEventRecord(S.tev[g].back()[0], ctx->stream));
    };
    auto step_end = [&] {
        ZK_HIP(hipEventRecord(S.tev[g].back()[1], ctx->stream));
        if (S.serial) {
            ZK_HIP(hipStreamSynchronize(ctx->stream));
            turn.unlock();
        }
    };
    auto exchange = [&](int t, int role, const std::vector<GroupRect> &rects) {
        step_end();
        ZK_HIP(hipEventRecord(S.ev[g][t], ctx->stream));
        S.bar.wait();
        step_begin();
        for (int h = 0; h < L.k; h++)
            if (h != g) ZK_HIP(hipStreamWaitEvent(ctx->stream, S.ev[h][t], 0));
        return group_gather(ctx, S, g, role, rects, n);
    };

    struct Step { int src, dst; bool inverse, coset; const NttLast *last; };
    const bool six = ctx->opt.wm_transforms != 7;
    const bool fuse = ctx->opt.fuse_pointwise != 0;
    const NttLast to_b{&tab->zinv, fuse, false}, to_c{&tab->zinv, false, false}, sub{nullptr, false, true};
    const Step seq7[7] = {{0, 3, true, false, nullptr}, {3, 0, false, true, nullptr}, {1, 3, true, false, nullptr}, {3, 1, false, true, nullptr},
                          {2, 3, true, false, nullptr}, {3, 2, false, true, nullptr}, {0, 3, true, true, nullptr}};
    const Step seq6[6] = {{0, 3, true, false, nullptr}, {3, 0, false, true, nullptr}, {1, 3, true, false, nullptr}, {3, 1, false, true, &to_b},
                          {2, 3, true, false, &to_c}, {0, 3, true, true, &sub}};
    const Step *seq = six ? seq6 : seq7;
    const int T = six ? 6 : 7;
    static_assert(GroupSync::EXCHANGES >= 8, "an event per exchange of the seven-transform map and the redistribution");
    step_begin();
    spmv_run(ctx, m, z, v[0], v[1], v[2], &sp);
    for (int t = 0; t < T; t++) {
        NttShare sh;
        group_share_tiles(L, g, sh.cols, sh.rows);
        const int role = seq[t].src;
        sh.between = [&, t, role] { S.ex_bytes[g] = exchange(t, role, S.ex_rects); };
        const NttPointwise pw{v[1], six ? nullptr : v[2], tab->zinv};
        const bool fused = t == T - 1 && fuse;
        if (t == T - 1 && !fused) {
            const uint64_t w = L.hi[g] - L.lo[g], count = n / L.m * w;
            hipLaunchKernelGGL(group_pointwise_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, v[0], v[1],
                               six ? nullptr : v[2], tab->zinv, L.m, L.lo[g], w, count);
            ZK_HIP(hipGetLastError());
        }
        ntt_run_share(ctx, v[seq[t].src], v[seq[t].dst], m.log_n, seq[t].inverse, seq[t].coset, fused ? &pw : nullptr, sh, seq[t].last);
    }
    S.h_bytes[g] = exchange(T, 3, S.h_rects);
    step_end();
    *h_out = v[3];
}

double GroupSync::rank_ms(int g) {
    double t = 0;
    for (auto &p : tev[g]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p[0], p[1]) == hipSuccess) t += ms;
        else (void)hipGetLastError();
    }
    return t;
}

}  // namespace zk

// ------------------------------------------------------------------------------------------------ host-only ABI
using namespace zk;

namespace {
int rects_out(const std::vector<GroupRect> &v, uint64_t *rects, size_t cap, size_t *n_rects) {
    *n_rects = v.size();
    if (v.size() > cap || (v.size() && !rects)) return ZKG16_ERR_BAD_ARG;
    for (size_t i = 0; i < v.size(); i++) {
        uint64_t *o = rects + 7 * i;
        o[0] = (uint64_t)v[i].src; o[1] = (uint64_t)v[i].dst;
        o[2] = v[i].r0; o[3] = v[i].r1; o[4] = v[i].c0; o[5] = v[i].c1; o[6] = v[i].stride;
    }
    return ZKG16_OK;
}
}  // namespace

extern "C" {

int zkg16_group_layout(int log_n, int k, int ntt_mode, int *applies, uint64_t shape[4], uint64_t *residues, uint64_t *rects, size_t cap,
                       size_t *n_rects) {
    if (!applies || !shape || !n_rects || (ntt_mode != 0 && ntt_mode != 1 && ntt_mode != 3)) return ZKG16_ERR_BAD_ARG;
    GroupLayout L;
    if (!group_layout(log_n, k, ntt_mode, L)) return ZKG16_ERR_BAD_ARG;
    *applies = L.applies ? 1 : 0;
    shape[0] = L.n1; shape[1] = L.n2; shape[2] = L.m; shape[3] = L.unit;
    if (residues)
        for (int g = 0; g < k; g++) {
            residues[2 * g] = L.applies ? L.lo[g] : 0;
            residues[2 * g + 1] = L.applies ? L.hi[g] : 0;
        }
    return rects_out(group_exchange_rects(L), rects, cap, n_rects);
}

int zkg16_group_h_layout(int log_n, int k, int ntt_mode, const uint64_t *h_ranges, uint64_t *rects, size_t cap, size_t *n_rects) {
    if (!h_ranges || !n_rects || (ntt_mode != 0 && ntt_mode != 1 && ntt_mode != 3)) return ZKG16_ERR_BAD_ARG;
    GroupLayout L;
    if (!group_layout(log_n, k, ntt_mode, L)) return ZKG16_ERR_BAD_ARG;
    if (!L.applies) return ZKG16_ERR_UNSUPPORTED;
    const uint64_t n = (uint64_t)1 << log_n;
    std::vector<uint64_t> lo(k), hi(k);
    for (int g = 0; g < k; g++) {
        lo[g] = h_ranges[2 * g];
        hi[g] = h_ranges[2 * g + 1];
        if (lo[g] > hi[g] || hi[g] > n) return ZKG16_ERR_BAD_ARG;
        for (int p = 0; p < g; p++)
            if (lo[g] < hi[g] && lo[p] < hi[p] && lo[g] < hi[p] && lo[p] < hi[g]) return ZKG16_ERR_BAD_ARG;     // overlapping ranges
    }
    return rects_out(group_h_rects(L, lo.data(), hi.data()), rects, cap, n_rects);
}

}  // extern "C"
