// libzkg16 C ABI, part 5 of 8 (api.hip): device groups.
#include "api_internal.hpp"
#include "group.hpp"

using namespace zk;

// ------------------------------------------------------------------------------------------------ device groups
// Several ctxs of one process (one per GPU, or several on one GPU) that prove one proof together: one host thread per rank, each
// on a leased lane of its ctx.  The ranks whose key shard has an h range form the witness-map set; when the split layout applies
// (group.hpp) they split the seven NTTs between them, else each runs the whole witness map as zkg16_prove_partial does.
struct zkg16_group {
    std::vector<zkg16_ctx *> ctxs;
    std::mutex mu;                                  // one group call at a time
    int serial = 0;                                 // option group_serial
    int last_k_dist = 0;
    std::vector<std::array<double, 4>> last_stats;  // per rank: witness-map device ms, bytes per row-pass exchange, bytes of h, wall ms
    std::string last_error;
};

namespace {

// one thread per rank runs fn(rank, leased lane); a rank that fails breaks `bar` (if any) so that no peer waits for it.  Every
// rank drains its streams and then waits for all the others before its lease ends: no lane is handed to another caller while a
// peer's gather may still read its buffers.  -> the first failure's status (its text in grp->last_error)
int group_run(zkg16_group *grp, GroupBarrier *bar, const std::function<void(int, zkg16_ctx *)> &fn) {
    const int n = (int)grp->ctxs.size();
    std::vector<int> status(n, ZKG16_OK);
    std::vector<std::string> text(n);
    std::mutex done_mu;
    std::condition_variable done_cv;
    int done = 0;
    auto arrive = [&](bool wait) {
        std::unique_lock<std::mutex> lk(done_mu);
        if (++done == n) done_cv.notify_all();
        else if (wait) done_cv.wait(lk, [&] { return done == n; });
    };
    auto rank = [&](int i) {
        zkg16_ctx *root = grp->ctxs[i];
        auto failed = [&](int rc, zkg16_ctx *c) {
            status[i] = rc;
            text[i] = c ? c->last_error : std::string();
            if (bar) bar->brk();
        };
        try {
            LaneLease lease(root);
            zkg16_ctx *lane = lease.lane;
            struct Arrive {
                std::function<void()> f;
                ~Arrive() { f(); }
            } at_end{[&] { arrive(true); }};
            try {
                ZK_HIP(hipSetDevice(lane->device));
                fn(i, lane);
            } catch (const HipError &e) {
                failed(fail(lane, e), lane);
            } catch (const std::bad_alloc &) {
                failed(ZKG16_ERR_OOM, nullptr);
            } catch (...) {
                failed(ZKG16_ERR_HIP, nullptr);
            }
            (void)hipStreamSynchronize(lane->stream);
            (void)hipStreamSynchronize(lane->wm_stream);
        } catch (const HipError &e) {           // the lease itself failed: nothing was started on this rank
            failed(fail(root, e), root);
            arrive(true);
        } catch (...) {
            failed(ZKG16_ERR_OOM, nullptr);
            arrive(true);
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n; i++) {
        try {
            th.emplace_back([&rank, i] { rank(i); });
        } catch (const std::system_error &) {      // a rank that never starts counts as failed (and as arrived)
            status[i] = ZKG16_ERR_OOM;
            text[i] = "no thread for this rank";
            if (bar) bar->brk();
            arrive(false);
        }
    }
    rank(0);
    for (auto &t : th) t.join();
    for (int i = 0; i < n; i++)
        if (status[i] != ZKG16_OK) {
            grp->last_error = "rank " + std::to_string(i) + ": " + text[i];
            return status[i];
        }
    grp->last_error.clear();
    return ZKG16_OK;
}

// the split witness map of a group call, or null when the replicated one runs (k < 2, the layout does not apply, or the
// witness-map ranks do not agree on the NTT plan or on the number of transforms: their exchanges would not pair up)
std::unique_ptr<GroupSync> group_sync_for(zkg16_group *grp, const std::vector<int> &wm_ranks, int log_n, const std::vector<uint64_t> &h_lo,
                                          const std::vector<uint64_t> &h_hi) {
    const int k = (int)wm_ranks.size();
    if (k < 2) return nullptr;
    const int mode = grp->ctxs[wm_ranks[0]]->opt.ntt_mode, transforms = grp->ctxs[wm_ranks[0]]->opt.wm_transforms;
    for (int r : wm_ranks)
        if (grp->ctxs[r]->opt.ntt_mode != mode || grp->ctxs[r]->opt.wm_transforms != transforms) return nullptr;
    GroupLayout L;
    if (!group_layout(log_n, k, mode, L) || !L.applies) return nullptr;
    auto S = std::make_unique<GroupSync>(k);
    S->L = L;
    S->ex_rects = group_exchange_rects(L);
    S->h_rects = group_h_rects(L, h_lo.data(), h_hi.data());
    S->serial = grp->serial != 0;
    return S;
}

// the ranges [lo, hi) of all ranks cover [0, total) exactly once (empty ranges allowed)
bool ranges_tile(std::vector<std::pair<uint64_t, uint64_t>> r, uint64_t total) {
    std::sort(r.begin(), r.end());
    uint64_t at = 0;
    for (auto &x : r) {
        if (x.second < x.first) return false;
        if (x.second == x.first) continue;
        if (x.first != at) return false;
        at = x.second;
    }
    return at == total;
}

}  // namespace

extern "C" {

int zkg16_group_create(zkg16_ctx *const *ctxs, int n, zkg16_group **out) {
    if (!out) return ZKG16_ERR_BAD_ARG;
    *out = nullptr;
    if (!ctxs || n < 1 || n > GROUP_MAX) return ZKG16_ERR_BAD_ARG;
    for (int i = 0; i < n; i++) {
        if (!ctxs[i] || ctxs[i]->root) return ZKG16_ERR_BAD_ARG;
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return ZKG16_ERR_BAD_ARG;                  // one ctx twice
    }
    // ranks on different GPUs read each other's buffers: peer access both ways, or no group
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const int a = ctxs[i]->device, b = ctxs[j]->device;
            if (a == b) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) {
                (void)hipGetLastError();
                return ZKG16_ERR_UNSUPPORTED;
            }
            if (hipSetDevice(a) != hipSuccess) { (void)hipGetLastError(); return ZKG16_ERR_HIP; }
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                (void)hipGetLastError();
                return ZKG16_ERR_UNSUPPORTED;
            }
            (void)hipGetLastError();
        }
    auto *g = new (std::nothrow) zkg16_group();
    if (!g) return ZKG16_ERR_OOM;
    g->ctxs.assign(ctxs, ctxs + n);
    *out = g;
    return ZKG16_OK;
}

void zkg16_group_destroy(zkg16_group *group) {
    if (!group) return;
    { std::lock_guard<std::mutex> lk(group->mu); }      // a group call still running finishes first
    delete group;
}

const char *zkg16_group_last_error(zkg16_group *group) { return group ? group->last_error.c_str() : ""; }

int zkg16_group_set_option(zkg16_group *group, const char *name, int64_t value) {
    if (!group || !name) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(group->mu);
    if (!strcmp(name, "group_serial")) {
        group->serial = value ? 1 : 0;
        return ZKG16_OK;
    }
    return ZKG16_ERR_UNSUPPORTED;
}

int zkg16_group_last_wm(zkg16_group *group, int *k_dist) {
    if (!group || !k_dist) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(group->mu);
    *k_dist = group->last_k_dist;
    return ZKG16_OK;
}

int zkg16_group_rank_stats(zkg16_group *group, double *out, int cap_ranks) {
    if (!group || !out) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(group->mu);
    const int n = (int)group->last_stats.size();
    if (cap_ranks < n) return ZKG16_ERR_BAD_ARG;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = group->last_stats[i][j];
    return n;
}

int zkg16_witness_map_group(zkg16_group *group, const uint64_t *r1cs_handles, const uint64_t *witness_handles, uint64_t *h_out,
                            size_t *log_n_out) {
    if (!group || !r1cs_handles || !witness_handles || !h_out) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(group->mu);
    const int n = (int)group->ctxs.size();
    std::vector<std::shared_ptr<R1csDev>> rc(n);
    std::vector<std::shared_ptr<WitnessDev>> wit(n);
    for (int i = 0; i < n; i++) {
        rc[i] = group->ctxs[i]->r1cs.get(r1cs_handles[i]);
        wit[i] = group->ctxs[i]->wits.get(witness_handles[i]);
        if (!rc[i] || !wit[i]) return ZKG16_ERR_BAD_HANDLE;
    }
    for (int i = 0; i < n; i++)
        if (wit[i]->n != rc[i]->num_variables || rc[i]->log_n != rc[0]->log_n || rc[i]->num_variables != rc[0]->num_variables ||
            rc[i]->num_constraints != rc[0]->num_constraints || rc[i]->num_instance != rc[0]->num_instance ||
            rc[i]->nnz[0] != rc[0]->nnz[0] || rc[i]->nnz[1] != rc[0]->nnz[1] || rc[i]->nnz[2] != rc[0]->nnz[2])
            return ZKG16_ERR_BAD_ARG;
    const uint64_t N = (uint64_t)1 << rc[0]->log_n;
    // every rank is a witness-map rank here; rank i brings the equal share [i N / n, (i + 1) N / n) of h back to the host
    std::vector<int> wm(n);
    std::vector<uint64_t> lo(n), hi(n);
    for (int i = 0; i < n; i++) {
        wm[i] = i;
        lo[i] = N * (uint64_t)i / (uint64_t)n;
        hi[i] = N * (uint64_t)(i + 1) / (uint64_t)n;
    }
    std::unique_ptr<GroupSync> S = group_sync_for(group, wm, rc[0]->log_n, lo, hi);
    std::vector<double> wall(n, 0);
    const int st = group_run(group, S ? &S->bar : nullptr, [&](int i, zkg16_ctx *ctx) {
        const double t0 = now_ms();
        Fr *h = nullptr;
        GroupRank gr{S.get(), i};
        if (S) group_witness_map_run(ctx, *rc[i], wit[i]->z.as<Fr>(), &h, gr);
        else witness_map_run(ctx, *rc[i], wit[i]->z.as<Fr>(), &h);
        if (hi[i] > lo[i])
            ZK_HIP(hipMemcpyAsync(h_out + 4 * lo[i], h + lo[i], (hi[i] - lo[i]) * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        wall[i] = now_ms() - t0;
    });
    group->last_k_dist = st == ZKG16_OK && S ? S->L.k : 0;
    group->last_stats.assign(n, std::array<double, 4>{0, 0, 0, 0});
    for (int i = 0; i < n; i++) {
        auto &x = group->last_stats[i];
        if (S && st == ZKG16_OK) {
            (void)hipSetDevice(group->ctxs[i]->device);
            x[0] = S->rank_ms(i);
            x[1] = (double)S->ex_bytes[i];
            x[2] = (double)S->h_bytes[i];
        }
        x[3] = wall[i];
    }
    if (st == ZKG16_OK && log_n_out) *log_n_out = (size_t)rc[0]->log_n;
    return st;
}

int zkg16_prove_group(zkg16_group *group, const uint64_t *pk_handles, const uint64_t *r1cs_handles, const uint64_t *witness_handles,
                      const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3]) {
    if (!group || !pk_handles || !r1cs_handles || !witness_handles || !r || !s || !proof_out || !inf_out) return ZKG16_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(group->mu);
    const int n = (int)group->ctxs.size();
    std::vector<std::shared_ptr<PkDev>> pk(n);
    std::vector<std::shared_ptr<R1csDev>> rc(n);
    std::vector<std::shared_ptr<WitnessDev>> wit(n);
    for (int i = 0; i < n; i++) {
        pk[i] = group->ctxs[i]->pks.get(pk_handles[i]);
        rc[i] = group->ctxs[i]->r1cs.get(r1cs_handles[i]);
        wit[i] = group->ctxs[i]->wits.get(witness_handles[i]);
        if (!pk[i] || !rc[i] || !wit[i]) return ZKG16_ERR_BAD_HANDLE;
    }
    // every handle and dimension on every rank, before any work: one system, one key, shards that tile it, one blinding rank
    const uint64_t N = (uint64_t)1 << rc[0]->log_n, m_total = rc[0]->num_variables;
    std::vector<std::pair<uint64_t, uint64_t>> zr, hr;
    int blinding = -1, nblind = 0;
    for (int i = 0; i < n; i++) {
        const R1csDev &c = *rc[i];
        const PkDev &p = *pk[i];
        if (wit[i]->n != c.num_variables || p.m_total != c.num_variables || p.num_instance != c.num_instance || p.n_h_total != N - 1 ||
            c.log_n != rc[0]->log_n || c.num_variables != m_total || c.num_constraints != rc[0]->num_constraints ||
            c.num_instance != rc[0]->num_instance || c.nnz[0] != rc[0]->nnz[0] || c.nnz[1] != rc[0]->nnz[1] || c.nnz[2] != rc[0]->nnz[2])
            return ZKG16_ERR_BAD_ARG;
        zr.emplace_back(p.z_lo, p.z_hi);
        hr.emplace_back(p.h_lo, p.h_hi);
        if (p.blinding) { blinding = i; nblind++; }
    }
    if (nblind != 1 || !ranges_tile(zr, m_total) || !ranges_tile(hr, N - 1)) return ZKG16_ERR_BAD_ARG;
    std::vector<int> wm, wm_of(n, -1);
    std::vector<uint64_t> lo, hi;
    for (int i = 0; i < n; i++)
        if (pk[i]->h_hi > pk[i]->h_lo) {
            wm_of[i] = (int)wm.size();
            wm.push_back(i);
            lo.push_back(pk[i]->h_lo);
            hi.push_back(pk[i]->h_hi);
        }
    std::unique_ptr<GroupSync> S = group_sync_for(group, wm, rc[0]->log_n, lo, hi);
    const Fr rr = fr_from_abi(r), ss = fr_from_abi(s);
    std::vector<Partials> parts(n);
    std::vector<double> wall(n, 0);
    const int st = group_run(group, S ? &S->bar : nullptr, [&](int i, zkg16_ctx *ctx) {
        GroupRank gr{S.get(), wm_of[i]};
        prove_device(ctx, *pk[i], *rc[i], *wit[i], rr, ss, parts[i], nullptr, nullptr, (S && wm_of[i] >= 0) ? &gr : nullptr, false);
        wall[i] = ctx->timings[T_TOTAL];
    });
    group->last_k_dist = st == ZKG16_OK && S ? S->L.k : 0;
    group->last_stats.assign(n, std::array<double, 4>{0, 0, 0, 0});
    for (int i = 0; i < n; i++) {
        auto &x = group->last_stats[i];
        if (S && st == ZKG16_OK && wm_of[i] >= 0) {
            (void)hipSetDevice(group->ctxs[i]->device);
            x[0] = S->rank_ms(wm_of[i]);
            x[1] = (double)S->ex_bytes[wm_of[i]];
            x[2] = (double)S->h_bytes[wm_of[i]];
        }
        x[3] = wall[i];
    }
    if (st != ZKG16_OK) return st;
    // the partials combined exactly as zkg16_prove_finish combines the records of zkg16_prove_partial
    std::vector<uint64_t> rec((size_t)n * 72);
    std::vector<uint8_t> rinf((size_t)n * 5);
    for (int i = 0; i < n; i++) partials_to_abi(parts[i], rec.data() + 72 * (size_t)i, rinf.data() + 5 * (size_t)i);
    Partials sum;
    sum_partials(sum, rec.data(), rinf.data(), n);
    prove_tail(*pk[blinding], rr, ss, sum, proof_out, inf_out);
    return ZKG16_OK;
}

}  // extern "C"
