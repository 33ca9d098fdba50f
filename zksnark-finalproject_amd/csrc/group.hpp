// Split witness map over the ranks of a device group (group.hip; entry points in api_group.hip).
//
// The two-pass NTT plans view N = N1 * N2 as a matrix x[N2 * i1 + i2]: the column pass transforms the columns i2 in place,
// the row pass reads the rows k1 and writes X[k1 + N1 * k2].  With m = min(N1, N2), rank g of k owns the residues
// [lo_g, hi_g) mod m: its column pass runs the columns with i2 mod m in range, its row pass the rows with k1 mod m in range,
// and every position n with n mod m in range is its own.  The row pass leaves the rank owning exactly what the next
// transform's column pass needs, so the only exchange of a transform is the one in front of its row pass (rank g copies
// g's rows x h's columns from every peer h), plus one redistribution of h at the end (rank g gathers its key shard's
// [h_lo, h_hi)).  Every buffer stays full-size on every rank; only owned positions are valid.
#pragma once
#include <array>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "common.hpp"

namespace zk {

static constexpr int GROUP_MAX = 8;              // ranks of a device group (zkg16_group_create)
static constexpr int GROUP_LAYOUT_MAX_K = 64;    // ranks the host-only layout function accepts

// a rectangle of positions row * stride + col, rows [r0, r1), columns [c0, c1), that rank dst copies from rank src
struct GroupRect {
    int src, dst;
    uint64_t r0, r1, c0, c1, stride;
};

struct GroupLayout {
    bool applies = false;            // false: the replicated witness map runs (not two-pass, or k above the granularity)
    int log_n = 0, k = 0;
    int log_n1 = 0, log_n2 = 0, tile_log = 0;
    uint64_t n1 = 0, n2 = 0, m = 0;  // m = min(N1, N2)
    uint64_t unit = 0;               // residues per unit of the split: the larger of a column tile's columns and a row tile's rows
    std::vector<uint64_t> lo, hi;    // rank g owns the residues [lo[g], hi[g]) mod m
};
// false (and L.applies == false) for arguments that are refused: k < 1 or above GROUP_LAYOUT_MAX_K, log_n outside 0 .. 31
bool group_layout(int log_n, int k, int ntt_mode, GroupLayout &L);
// the row-pass exchange: for every rank g, g's rows x every peer's columns (positions k1 * N2 + i2)
std::vector<GroupRect> group_exchange_rects(const GroupLayout &L);
// the redistribution of h: rank g receives [h_lo[g], h_hi[g]) from the ranks that own those positions (positions q * m + r)
std::vector<GroupRect> group_h_rects(const GroupLayout &L, const uint64_t *h_lo, const uint64_t *h_hi);
// column / row tile ranges {lo0, n0, lo1, n1} of rank g's share of a transform
void group_share_tiles(const GroupLayout &L, int g, unsigned cols[4], unsigned rows[4]);

// A barrier over the rank threads of one group call that a failing rank breaks: every rank then leaves wait() by an exception,
// so nobody hangs on a peer that is gone.
class GroupBarrier {
    std::mutex mu_;
    std::condition_variable cv_;
    int n_ = 0, count_ = 0;
    unsigned gen_ = 0;
    bool broken_ = false;
  public:
    explicit GroupBarrier(int n) : n_(n) {}
    void wait();
    void brk();
};

// One split witness map across the k witness-map ranks of a group call, shared by their threads.
struct GroupSync {
    static constexpr int EXCHANGES = 8;          // one per transform (six, or seven with wm_transforms = 7) + the redistribution of h
    GroupLayout L;
    std::vector<GroupRect> ex_rects, h_rects;
    std::vector<int> device;                     // per rank
    std::vector<std::array<Fr *, 4>> bufs;       // per rank: its a, b, c, tmp vectors (published before the first barrier)
    std::vector<std::array<hipEvent_t, EXCHANGES>> ev;
    GroupBarrier bar;
    bool serial = false;                         // option group_serial: ranks run each step one at a time (per-rank timing)
    std::mutex serial_mu;
    // per rank: device time of its witness-map steps (with serial: alone on the device), bytes gathered per exchange and in the
    // redistribution
    std::vector<std::vector<std::array<hipEvent_t, 2>>> tev;   // per rank: an event pair per step
    std::vector<uint64_t> ex_bytes, h_bytes;
    explicit GroupSync(int k) : device(k, 0), bufs(k), ev(k), bar(k), tev(k), ex_bytes(k, 0), h_bytes(k, 0) {
        for (auto &e : ev) e.fill(nullptr);
        for (auto &b : bufs) b.fill(nullptr);
    }
    double rank_ms(int g);                       // after the rank's stream has drained: its steps' device time
    ~GroupSync();
    GroupSync(const GroupSync &) = delete;
    GroupSync &operator=(const GroupSync &) = delete;
};
struct GroupRank {
    GroupSync *sync;
    int idx;                                     // rank within the witness-map set
};
// rank `r.idx`'s share of the witness map on ctx->stream; *h_out = the vector whose redistributed range [h_lo, h_hi) of this
// rank is valid.  Events for the exchanges are created on first use.
void group_witness_map_run(zkg16_ctx *ctx, R1csDev &m, const Fr *z, Fr **h_out, GroupRank &r);

}  // namespace zk
