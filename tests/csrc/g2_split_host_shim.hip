// TEST-ONLY: the pair-split G2 mixed addition (csrc/g2split.cuh: h2_madd over the lane model) on RAW limbs, with the lane pair
// emulated on the host (H2Pair: both halves in a two-element array), so that the text the split accumulation kernel runs
// (csrc/msm.hip: msm_accumulate_split_kernel) executes on the CPU with every operand assertion of csrc/ffu.cuh live:
//   hipcc --offload-host-only -DZK_FQU_CHECK   value bounds, the limb bound of every operand that skipped its carry pass, and every
//                                              product column accumulated a second time in 128 bits (no 64-bit column may wrap).
// Records are those of tests/csrc/madd_lazy_shim.hip's G2 operations (tests/madd_lazy_cases.py builds and checks them):
//   an addition: accumulator (X, Y, ZZ, ZZZ), base (X, Y, two unused coordinates), neg flag -> the sum
//   a chain:     accumulator, two bases, seed -> the point after each of 32 additions, + or - either base by the lane's generator
// and the VS operations run the one-lane addition (csrc/ec.cuh: xyzz_madd_lazy / xyzz_madd_lazy_lc) beside the split one on the same
// chain and report, per step, which coordinates differ as residues (0 = none).  Host build only; nothing from libzkg16.so.
#if !defined(ZK_FQU_CHECK)
#error "host build with -DZK_FQU_CHECK only"
#endif
#include <string.h>
#include "ff.cuh"
#include "ffu.cuh"
#include "ec.cuh"
#include "g2split.cuh"
using namespace zk;

namespace {

template <class T> T ld(const uint32_t *p) { T r; memcpy(&r, p, sizeof(T)); return r; }
template <class T> void st(uint32_t *p, const T &v) { memcpy(p, &v, sizeof(T)); }

// operation numbers (tests/g2_split_cases.py holds the same table); odd = the form without the spare carry passes
enum { MADD = 0, MADD_LC = 1, CHAIN = 2, CHAIN_LC = 3, VS = 4, VS_LC = 5, NOPS = 6 };
constexpr int CHAIN_STEPS = 32;
constexpr int W = 28;      // words of one Fq2U coordinate
constexpr int in_words(int) { return 8 * W + 1; }
constexpr int out_words(int op) { return op <= MADD_LC ? 4 * W : op <= CHAIN_LC ? CHAIN_STEPS * 4 * W : CHAIN_STEPS; }

H2PairV split(const Fq2U &a) { return H2PairV{{a.c0, a.c1}}; }
Fq2U join(const H2PairV &a) { return Fq2U{a.c[0], a.c[1]}; }
H2XYZZ<H2Pair> split(const XYZZ<Fq2U> &p) { return H2XYZZ<H2Pair>{split(p.x), split(p.y), split(p.zz), split(p.zzz)}; }
H2Affine<H2Pair> split(const Affine<Fq2U> &p) { return H2Affine<H2Pair>{split(p.x), split(p.y)}; }
XYZZ<Fq2U> join(const H2XYZZ<H2Pair> &p) { return XYZZ<Fq2U>{join(p.x), join(p.y), join(p.zz), join(p.zzz)}; }

template <bool LC> void madd_op(const uint32_t *in, uint32_t *out) {
    H2XYZZ<H2Pair> acc = split(ld<XYZZ<Fq2U>>(in));
    const H2Affine<H2Pair> base = split(ld<Affine<Fq2U>>(in + 4 * W));
    h2_madd<LC>(H2Pair{}, acc, base, in[8 * W] != 0);
    st(out, join(acc));
}

bool same_residue(const Fq2U &a, const Fq2U &b) {
    const Fq2 x = to_sat(a), y = to_sat(b);
    return memcmp(&x, &y, sizeof x) == 0;
}

// CHAIN_STEPS additions, each chosen by the lane's own generator (tests/madd_lazy_cases.py: chain_choices repeats it)
template <bool LC, bool VERSUS> void chain_op(const uint32_t *in, uint32_t *out) {
    const XYZZ<Fq2U> start = ld<XYZZ<Fq2U>>(in);
    const Affine<Fq2U> b1 = ld<Affine<Fq2U>>(in + 4 * W), b2 = ld<Affine<Fq2U>>(in + 6 * W);
    H2XYZZ<H2Pair> acc = split(start);
    XYZZ<Fq2U> one_lane = start;
    uint32_t s = in[8 * W];
    for (int step = 0; step < CHAIN_STEPS; step++) {
        s = s * 1664525u + 1013904223u;
        const uint32_t c = s >> 29;
        const Affine<Fq2U> &b = c < 5 ? b1 : b2;
        const bool neg = c == 3 || c == 4 || c == 7;
        h2_madd<LC>(H2Pair{}, acc, split(b), neg);
        if (VERSUS) {
            if (LC) xyzz_madd_lazy_lc(one_lane, b, neg);
            else xyzz_madd_lazy(one_lane, b, neg);
            const XYZZ<Fq2U> got = join(acc);
            uint32_t diff = 0;
            if (got.is_inf() != one_lane.is_inf()) diff |= 16u;
            if (!same_residue(got.x, one_lane.x)) diff |= 1u;
            if (!same_residue(got.y, one_lane.y)) diff |= 2u;
            if (!same_residue(got.zz, one_lane.zz)) diff |= 4u;
            if (!same_residue(got.zzz, one_lane.zzz)) diff |= 8u;
            out[step] = diff;
        } else {
            st(out + step * 4 * W, join(acc));
        }
    }
}

template <int OP> int run_cases(int n, const uint32_t *in, uint32_t *out) {
    for (int i = 0; i < n; i++) {
        const uint32_t *ip = in + (size_t)i * in_words(OP);
        uint32_t *op = out + (size_t)i * out_words(OP);
        if constexpr (OP == MADD || OP == MADD_LC) madd_op<OP == MADD_LC>(ip, op);
        else if constexpr (OP == CHAIN || OP == CHAIN_LC) chain_op<OP == CHAIN_LC, false>(ip, op);
        else chain_op<OP == VS_LC, true>(ip, op);
    }
    return 0;
}

}  // namespace

#define G2S_VISIBLE extern "C" __attribute__((visibility("default")))
#define G2S_OPS(X) X(0) X(1) X(2) X(3) X(4) X(5)

// 0 = done; -1: unknown operation
G2S_VISIBLE int g2_split_run(int op, int n, const uint32_t *in, uint32_t *out) {
    switch (op) {
#define X(OP) case OP: return run_cases<OP>(n, in, out);
        G2S_OPS(X)
#undef X
    }
    return -1;
}
G2S_VISIBLE int g2_split_words(int op, int output) {
    if (op < 0 || op >= NOPS) return -1;
    return output ? out_words(op) : in_words(op);
}
G2S_VISIBLE int g2_split_check_active(void) { return 1; }
