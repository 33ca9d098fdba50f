// TEST-ONLY: csrc/sponge_chain_dev.cuh (what wit_chain_batch_kernel runs, one GPU lane per sponge chain) compiled for the host, so
// that a chain walked in segments can be compared with the host chains and with the host assignment builder on a machine without a
// GPU.  Built by tests/sponge_chain_cases.py with `hipcc --offload-host-only`.  Values cross in Montgomery u64 limbs (ark's order).
#include "ff.cuh"
#include <string.h>
using namespace zk;

namespace {
#include "poseidon_params.inc"
constexpr int P_ROUNDS = POSEIDON_FULL + POSEIDON_PARTIAL, P_HALF = POSEIDON_FULL / 2;
constexpr size_t PERM_WITNESSES = 265, FIRST_PERM_SKIPPED = 5;
#include "sponge_chain_dev.cuh"

struct Params { Fr mds[3][3], ark[P_ROUNDS][3]; };
const Params &params() {
    static const Params p = [] {
        Params q;
        auto mont = [](const uint64_t l[4]) {
            Fr c;
            memcpy(c.l, l, 32);
            return fp_to_mont(c);
        };
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) q.mds[i][j] = mont(POSEIDON_MDS[i][j]);
        for (int r = 0; r < P_ROUNDS; r++)
            for (int j = 0; j < 3; j++) q.ark[r][j] = mont(POSEIDON_ARK[r][j]);
        return q;
    }();
    return p;
}
template <class L>
Fr walk(const L &ld, size_t count, size_t p_lo, size_t p_hi, Fr st[3], Fr *out) {
    return out ? sponge_chain_walk<true>(params(), ld, count, p_lo, p_hi, st, out) : sponge_chain_walk<false>(params(), ld, count, p_lo, p_hi, st, out);
}
}  // namespace

extern "C" {

// Permutations [p_lo, p_hi) of one chain of `count` elements from the carried state st (3 Fr, updated in place).  kind 0: p = count
// Montgomery Fr; 1: p = count u64; 2: the entries of a b (n x n u64 each, count = n^2).  any != 0: through ChainLoadAny, the kernel's
// loader.  out (nullable): the first value of the chain's gadget — the S-box values are stored when it is given.  hash: st[1] at p_hi.
void sc_walk(int kind, int any, const void *p, const uint64_t *a, const uint64_t *b, size_t n, size_t count, size_t p_lo, size_t p_hi,
             uint64_t *st, uint64_t *out, uint64_t *hash) {
    Fr s[3];
    memcpy(s, st, sizeof s);
    Fr *o = reinterpret_cast<Fr *>(out);
    Fr h;
    if (any) h = walk(ChainLoadAny{kind, p, a, b, n}, count, p_lo, p_hi, s, o);
    else if (kind == 0) h = walk(ChainLoadMont{static_cast<const Fr *>(p)}, count, p_lo, p_hi, s, o);
    else if (kind == 1) h = walk(ChainLoadU64{static_cast<const uint64_t *>(p)}, count, p_lo, p_hi, s, o);
    else h = walk(ChainLoadProduct{a, b, n}, count, p_lo, p_hi, s, o);
    memcpy(st, s, sizeof s);
    memcpy(hash, h.l, 32);
}

}  // extern "C"
