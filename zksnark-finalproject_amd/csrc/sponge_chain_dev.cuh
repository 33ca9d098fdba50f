// One Poseidon sponge chain walked by ONE lane (witness.hip: wit_chain_batch_kernel, a lane per chain of a batch), written
// __host__ __device__ so that tests/csrc/sponge_chain_host_shim.hip can run the same code on a machine without a GPU.
//
// A chain is sequential: permutation p + 1 needs the state permutation p leaves.  The host walks the chains of small batches
// (poseidon_h64.inc: sponge_chain) and a kernel then recomputes every permutation from its entering state to write the S-box values;
// here the lane that walks the chain writes them as it goes, so every permutation is computed once.  The values, their order and
// their offsets are wit_sponge_batch_kernel's: per permutation, round by round, S-box lane 0..2 (lane 0 only in a partial round),
// x^2, x^4, x^8, x^16, x^17 — 265 values, 260 for permutation 0, whose capacity lane is a constant in round 0.
//
// Include inside a namespace after poseidon_params.inc, with P_ROUNDS, P_HALF, PERM_WITNESSES and FIRST_PERM_SKIPPED defined
// (as poseidon_h64.inc is).  Params: any struct with Fr mds[3][3] and Fr ark[P_ROUNDS][3] in Montgomery form.
#pragma once

// ---- where a chain's elements come from.  operator()(i) = element i as Montgomery Fr.
struct ChainLoadMont {          // Fr in Montgomery form
    const Fr *e;
    ZK_HD Fr operator()(size_t i) const { return e[i]; }
};
ZK_HD Fr chain_u64_to_mont(uint64_t lo, uint64_t mid, uint64_t hi) {
    Fr v = Fr::zero();
    v.l[0] = (uint32_t)lo; v.l[1] = (uint32_t)(lo >> 32);
    v.l[2] = (uint32_t)mid; v.l[3] = (uint32_t)(mid >> 32);
    v.l[4] = (uint32_t)hi; v.l[5] = (uint32_t)(hi >> 32);
    return fp_to_mont(v);
}
struct ChainLoadU64 {           // a u64 taken to Montgomery form
    const uint64_t *e;
    ZK_HD Fr operator()(size_t i) const { return chain_u64_to_mont(e[i], 0, 0); }
};
// entry (i / n, i % n) of a b over the integers, as matmul_u64 forms it: n products of u64 summed in three limbs (below n 2^128 < r),
// then to Montgomery form.  n multiply-adds beside the ~600 field products of the permutation that absorbs the entry.
struct ChainLoadProduct {
    const uint64_t *a, *b;
    size_t n;
    ZK_HD Fr operator()(size_t e) const {
        const uint64_t *ar = a + (e / n) * n, *bc = b + e % n;
        uint64_t s0 = 0, s1 = 0, s2 = 0;
        for (size_t k = 0; k < n; k++) {
            const uint64_t x = ar[k], y = bc[k * n];
            const uint64_t lo = x * y;
#if defined(__HIP_DEVICE_COMPILE__)
            const uint64_t hi = __umul64hi(x, y);
#else
            const uint64_t hi = (uint64_t)(((unsigned __int128)x * y) >> 64);
#endif
            s0 += lo;
            const uint64_t c0 = s0 < lo ? 1 : 0;
            s1 += hi;
            const uint64_t c1 = s1 < hi ? 1 : 0;       // hi <= 2^64 - 2, so hi + c0 cannot wrap on its own
            s1 += c0;
            s2 += c1 + (s1 < c0 ? 1 : 0);
        }
        return chain_u64_to_mont(s0, s1, s2);
    }
};
// the three behind one run-time switch: what a kernel whose waves each hold one kind of chain is compiled with (one copy of the
// permutation instead of three)
struct ChainLoadAny {
    int kind;                   // 0 = Montgomery Fr at p, 1 = u64 at p, 2 = entries of a b
    const void *p;
    const uint64_t *a, *b;
    size_t n;
    ZK_HD Fr operator()(size_t i) const {
        if (kind == 0) return ChainLoadMont{static_cast<const Fr *>(p)}(i);
        if (kind == 1) return ChainLoadU64{static_cast<const uint64_t *>(p)}(i);
        return ChainLoadProduct{a, b, n}(i);
    }
};

ZK_HD void chain_store(Fr *p, const Fr &v) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *q = reinterpret_cast<uint4 *>(p);            // every destination is a 32-byte element of an allocation
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
#else
    *p = v;
#endif
}

// Permutations [p_lo, p_hi) of one chain of `count` elements.  st: the carried state — all zero in front of permutation 0, else what
// the call that ended at p_lo left.  Per permutation: absorb its (up to POSEIDON_RATE) elements, then permute.  STORE: the S-box values
// go to out + (p == 0 ? 0 : p * PERM_WITNESSES - FIRST_PERM_SKIPPED), out = the first value of the chain's gadget.  Returns
// st[POSEIDON_CAP]: the hash once p_hi is the chain's last permutation (hasher.rs:17-27: absorb all, squeeze one).
template <bool STORE, class Params, class Loader>
ZK_HD Fr sponge_chain_walk(const Params &pp, const Loader &elem, size_t count, size_t p_lo, size_t p_hi, Fr st[3], Fr *out) {
    for (size_t p = p_lo; p < p_hi; p++) {
        for (size_t pos = 0; pos < (size_t)POSEIDON_RATE && p * POSEIDON_RATE + pos < count; pos++)
            st[POSEIDON_CAP + pos] = fp_add(st[POSEIDON_CAP + pos], elem(p * POSEIDON_RATE + pos));
        Fr *o = STORE ? out + (p == 0 ? 0 : p * PERM_WITNESSES - FIRST_PERM_SKIPPED) : nullptr;
        for (int r = 0; r < P_ROUNDS; r++) {
            const bool full = r < P_HALF || r >= P_HALF + POSEIDON_PARTIAL;
            for (int i = 0; i < 3; i++) st[i] = fp_add(st[i], pp.ark[r][i]);
            for (int i = 0; i < (full ? 3 : 1); i++) {
                const Fr x = st[i];
                const Fr x2 = fp_sqr(x), x4 = fp_sqr(x2), x8 = fp_sqr(x4), x16 = fp_sqr(x8), x17 = fp_mul(x16, x);
                if (STORE && !(p == 0 && r == 0 && i == 0)) {       // the capacity lane of a fresh sponge is a constant: no witnesses
                    chain_store(o, x2); chain_store(o + 1, x4); chain_store(o + 2, x8); chain_store(o + 3, x16); chain_store(o + 4, x17);
                    o += 5;
                }
                st[i] = x17;
            }
            Fr nst[3];
            for (int i = 0; i < 3; i++) {
                Fr acc = fp_mul(st[0], pp.mds[i][0]);
                acc = fp_add(acc, fp_mul(st[1], pp.mds[i][1]));
                nst[i] = fp_add(acc, fp_mul(st[2], pp.mds[i][2]));
            }
            for (int i = 0; i < 3; i++) st[i] = nst[i];
        }
    }
    return st[POSEIDON_CAP];
}
