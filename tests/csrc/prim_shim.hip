// TEST-ONLY: the field and curve primitives of csrc/ff.cuh, ffu.cuh, fru.cuh and ec.cuh (and pd::tidy of pairing_dev.cuh) one
// operation at a time on RAW limbs - no to_u / to_sat round trip, so a test can put every operand at the top of its stated
// bound.  One source, two builds (tests/prim_cases.py):
//   host build   hipcc --offload-host-only -DPRIM_HOST_BUILD -DZK_FQU_CHECK: `prim_run` loops over the cases on the CPU, with
//                the operand assertions of ffu.cuh live;
//   device build the product's flags: `prim_run` launches prim_kernel<OP>, one lane per case, 64 lanes per block (one wave: the
//                LDS operand slots of fq2u_mul_lazy are indexed by the lane), and copies the results back.
// Every operation body is written once (run_op<OP>); the operation is a template parameter, so each kernel holds one variant.
// Operations that exist only in a device pass (fq2u_mul_lazy, xyzz_madd_lazy, xyzz_madd_inline) are refused by the host build.
// The shim needs nothing from libzkg16.so.
#include "ff.cuh"
#include "ffu.cuh"
#include "fru.cuh"
#include "ec.cuh"
#include "pairing_dev.cuh"
using namespace zk;

namespace {

template <class T> ZK_HD T ld(const uint32_t *p) { T r; __builtin_memcpy(&r, p, sizeof(T)); return r; }
template <class T> ZK_HD void st(uint32_t *p, const T &v) { __builtin_memcpy(p, &v, sizeof(T)); }

// operation numbers (tests/prim_cases.py holds the same table and checks the record sizes against prim_words)
enum {
    SAT_FR = 0, SAT_FQ = 10,      // + 0 add, 1 sub, 2 neg, 3 dbl, 4 fp_mul, 5 fp_mul_inline, 6 sqr, 7 to_mont, 8 from_mont, 9 inv
    U_MUL = 20, U_SQR, U_MUL_IMPL, U_SQR_IMPL, U_MUL2, U_ADD, U_DBL, U_SUB8, U_SUB32, U_SUB64, U_SUB128, U_NEG, U_IS_ZERO_MOD,
    U_TIDY, U_FROM_SAT, U_TO_SAT, U_INV, U_CONSTANTS,
    Q2_MUL = 40, Q2_MUL_INLINE, Q2_MUL_LAZY, Q2_SQR, Q2_SUB, Q2_SUB2, Q2_NEG, Q2_INV,
    FRU = 50,                     // + the eleven operations of ht_fru_op (tests/csrc/ff_host_shim.hip)
    G1 = 70, G2 = 80,             // + 0 madd, 1 madd_front + madd_finish, 2 madd_inline (G1) / madd_lazy (G2), 3 add, 4 dbl, 5 dbl_affine, 6 chain
};
constexpr int CHAIN_STEPS = 32;

constexpr bool device_only(int op) { return op == Q2_MUL_LAZY || op == G1 + 2 || op == G2 + 2; }
// words (u32) of one case's input / output record
constexpr int in_words(int op) {
    return op < 10 ? 16 : op < 20 ? 24 : op < 50 ? 56 : op < 70 ? 16
         : op == G1 + 6 ? 10 * 14 + 1 : op < 80 ? 8 * 14 + 1 : op == G2 + 6 ? 10 * 28 + 1 : 8 * 28 + 1;
}
constexpr int out_words(int op) {
    return op < 10 ? 8 : op < 20 ? 12 : op == U_CONSTANTS ? 8 * 14 : op < 40 ? 14 : op < 50 ? 28 : op < 70 ? 8
         : op == G1 + 6 ? CHAIN_STEPS * 4 * 14 : op < 80 ? 4 * 14 : op == G2 + 6 ? CHAIN_STEPS * 4 * 28 : 4 * 28;
}

template <class P, int K> ZK_HD void sat_op(const uint32_t *in, uint32_t *out) {
    using F = Fp<P>;
    const F a = ld<F>(in), b = ld<F>(in + P::N);
    F r;
    if constexpr (K == 0) r = fp_add(a, b);
    else if constexpr (K == 1) r = fp_sub(a, b);
    else if constexpr (K == 2) r = fp_neg(a);
    else if constexpr (K == 3) r = fp_dbl(a);
    else if constexpr (K == 4) r = fp_mul(a, b);              // device: fq_mul_call for Fq; host: fp_mul_host64
    else if constexpr (K == 5) r = fp_mul_inline(a, b);       // the 32-bit-limb CIOS itself, in both builds
    else if constexpr (K == 6) r = fp_sqr(a);
    else if constexpr (K == 7) r = fp_to_mont(a);
    else if constexpr (K == 8) r = fp_from_mont(a);
    else r = fp_inv(a);
    st(out, r);
}

template <int OP> ZK_HD void fqu_op(const uint32_t *in, uint32_t *out) {
    const FqU a = ld<FqU>(in), b = ld<FqU>(in + 14);
    FqU r = FqU::zero();
    if constexpr (OP == U_MUL) r = fqu_mul(a, b);             // device: fqu_mul_call
    else if constexpr (OP == U_SQR) r = fqu_sqr(a);           // device: fqu_sqr_call
    else if constexpr (OP == U_MUL_IMPL) r = fqu_mul_impl<false>(a, b);
    else if constexpr (OP == U_SQR_IMPL) r = fqu_mul_impl<true>(a, a);
    else if constexpr (OP == U_MUL2) r = fqu_mul2(a, b, ld<FqU>(in + 28), ld<FqU>(in + 42));
    else if constexpr (OP == U_ADD) r = fqu_add(a, b);
    else if constexpr (OP == U_DBL) r = fqu_dbl(a);
    else if constexpr (OP == U_SUB8) r = fqu_sub<8>(a, b);
    else if constexpr (OP == U_SUB32) r = fqu_sub<32>(a, b);
    else if constexpr (OP == U_SUB64) r = fqu_sub<64>(a, b);
    else if constexpr (OP == U_SUB128) r = fqu_sub<128>(a, b);
    else if constexpr (OP == U_NEG) r = fqu_neg(a);
    else if constexpr (OP == U_IS_ZERO_MOD) r.l[0] = fqu_is_zero_mod(a) ? 1u : 0u;
    else if constexpr (OP == U_TIDY) r = pd::tidy(a);
    else if constexpr (OP == U_FROM_SAT) r = fqu_from_sat(ld<Fq>(in));
    else if constexpr (OP == U_TO_SAT) st(r.l, fqu_to_sat(a));      // 12 words, the last two stay zero
    else if constexpr (OP == U_INV) r = fqu_inv(a);
    st(out, r);
}

ZK_HD void fqu_constants(uint32_t *out) {
    for (int i = 0; i < 14; i++) {
        out[i] = FqUP::m8(i);
        out[14 + i] = FqUP::m32(i);
        out[28 + i] = FqUP::m64(i);
        out[42 + i] = FqUP::m128(i);
        out[56 + i] = FqUP::c_in(i);
        out[70 + i] = FqUP::d_out(i);
        out[84 + i] = FqUP::one(i);
        out[98 + i] = FqUP::mod(i);
    }
}

template <int OP> ZK_HD void fq2u_op(const uint32_t *in, uint32_t *out) {
    const Fq2U a = ld<Fq2U>(in), b = ld<Fq2U>(in + 28);
    Fq2U r = Fq2U::zero();
    if constexpr (OP == Q2_MUL) r = f_mul(a, b);
    else if constexpr (OP == Q2_MUL_INLINE) r = fq2u_mul_inline(a, b);
    else if constexpr (OP == Q2_MUL_LAZY) {
#if defined(__HIP_DEVICE_COMPILE__)
        r = fq2u_mul_lazy(a, b);
#endif
    }
    else if constexpr (OP == Q2_SQR) r = f_sqr(a);
    else if constexpr (OP == Q2_SUB) r = f_sub(a, b);
    else if constexpr (OP == Q2_SUB2) r = f_sub2(a, b);
    else if constexpr (OP == Q2_NEG) r = f_neg(a);
    else if constexpr (OP == Q2_INV) r = f_inv(a);
    st(out, r);
}

ZK_HD Fr two10_mont() {
    Fr c = Fr::zero();
    c.l[0] = 1u << 10;
    return fp_to_mont(c);
}
// the operations of ht_fru_op (tests/csrc/ff_host_shim.hip), unchanged: saturated in, saturated out, the NTT's arithmetic between
template <int K> ZK_HD void fru_op(const uint32_t *in, uint32_t *out) {
    const Fr sa = ld<Fr>(in), sb = ld<Fr>(in + 8);
    const FrU x = fru_from_sat(sa), y = fru_from_sat(sb);
    FrU r = x;
    if constexpr (K == 0) r = fru_cond_sub<true>(fru_add(x, y));
    else if constexpr (K == 1) r = fru_cond_sub<true>(fru_sub_2r(x, y));
    else if constexpr (K == 2) r = fru_mul(x, y);
    else if constexpr (K == 3) r = fru_mul(fru_sub_2r(x, y), y);
    else if constexpr (K == 4) { st(out, fru_mul_to_sat(x, fru_repack(sb))); return; }
    else if constexpr (K == 5) r = fru_mul(fru_repack(sa), fru_repack(fp_mul(sb, two10_mont())));
    else if constexpr (K == 6) {
        const FrU zc = fru_repack(fp_mul(sa, two10_mont()));
        const FrU xb = fru_mul(fru_repack(sa), fru_repack(sb));
        const FrU c = fru_mul(fru_repack(sb), fru_one_sat());
        r = fru_mul(fru_sub_2r(xb, c), zc);
    }
    else if constexpr (K == 7) r = fru_repack(sa);
    else if constexpr (K == 8) {
        for (int i = 0; i < 12; i++) r = fru_add_lazy(r, y);
    }
    else if constexpr (K == 9) r = fru_mul(fru_sub_4r_raw(x, fru_add_lazy(fru_add_lazy(x, y), y)), y);
    else if constexpr (K == 10) {
        FrU s2 = x;
        for (int i = 0; i < 11; i++) s2 = fru_add_lazy(s2, x);
        st(out, fru_mul_to_sat(fru_sub_4r_raw(s2, y), fru_one_sat()));
        return;
    }
    st(out, fru_mul_to_sat(r, fru_one_sat()));
}

// the device-only mixed additions: xyzz_madd_inline exists for G1, xyzz_madd_lazy for G2
ZK_HD void madd_device_only(XYZZ<FqU> &acc, const Affine<FqU> &q, bool neg) {
#if defined(__HIP_DEVICE_COMPILE__)
    xyzz_madd_inline(acc, q, neg);
#endif
}
ZK_HD void madd_device_only(XYZZ<Fq2U> &acc, const Affine<Fq2U> &q, bool neg) {
#if defined(__HIP_DEVICE_COMPILE__)
    xyzz_madd_lazy(acc, q, neg);
#endif
}

// record: accumulator (X, Y, ZZ, ZZZ), second operand (X, Y, ZZ, ZZZ; a base uses X, Y only), neg flag
template <class F, int K> ZK_HD void curve_op(const uint32_t *in, uint32_t *out) {
    constexpr int W = sizeof(F) / 4;
    XYZZ<F> acc = ld<XYZZ<F>>(in);
    const XYZZ<F> q = ld<XYZZ<F>>(in + 4 * W);
    const Affine<F> base{q.x, q.y};
    const bool neg = in[8 * W] != 0;
    if constexpr (K == 0) xyzz_madd(acc, base, neg);
    else if constexpr (K == 1) {
        MaddTail<F> t;
        const bool normal = xyzz_madd_front(acc, base, neg, t);
        xyzz_madd_finish(acc, t, normal);
    }
    else if constexpr (K == 2) madd_device_only(acc, base, neg);
    else if constexpr (K == 3) xyzz_add(acc, q);
    else if constexpr (K == 4) acc = xyzz_dbl(acc);
    else acc = xyzz_dbl_affine(base);
    st(out, acc);
}

// record: accumulator, base (X, Y), addend (X, Y, ZZ, ZZZ), seed.  CHAIN_STEPS steps, each chosen by the lane's own generator
// (tests/prim_cases.py: chain_choices repeats it): acc += base, acc -= base, acc += addend or acc = 2 acc; the point after
// EVERY step is written out, so closure of the stored bounds is checked on each of them.
template <class F> ZK_HD void chain_op(const uint32_t *in, uint32_t *out) {
    constexpr int W = sizeof(F) / 4;
    XYZZ<F> acc = ld<XYZZ<F>>(in);
    const Affine<F> base = ld<Affine<F>>(in + 4 * W);
    const XYZZ<F> addend = ld<XYZZ<F>>(in + 6 * W);
    uint32_t s = in[10 * W];
#pragma unroll 1
    for (int step = 0; step < CHAIN_STEPS; step++) {
        s = s * 1664525u + 1013904223u;
        const uint32_t c = s >> 29;
        if (c < 3) xyzz_madd(acc, base, false);
        else if (c == 3) xyzz_madd(acc, base, true);
        else if (c < 6) xyzz_add(acc, addend);
        else acc = xyzz_dbl(acc);
        st(out + step * 4 * W, acc);
    }
}

template <int OP> ZK_HD void run_op(const uint32_t *in, uint32_t *out) {
    if constexpr (OP < 10) sat_op<FrP, OP>(in, out);
    else if constexpr (OP < 20) sat_op<FqP, OP - 10>(in, out);
    else if constexpr (OP == U_CONSTANTS) fqu_constants(out);
    else if constexpr (OP < 40) fqu_op<OP>(in, out);
    else if constexpr (OP < 50) fq2u_op<OP>(in, out);
    else if constexpr (OP < 70) fru_op<OP - FRU>(in, out);
    else if constexpr (OP == G1 + 6) chain_op<FqU>(in, out);
    else if constexpr (OP < 80) curve_op<FqU, OP - G1>(in, out);
    else if constexpr (OP == G2 + 6) chain_op<Fq2U>(in, out);
    else curve_op<Fq2U, OP - G2>(in, out);
}

#define PRIM_OPS(X) \
    X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) \
    X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35) X(36) X(37) \
    X(40) X(41) X(42) X(43) X(44) X(45) X(46) X(47) \
    X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58) X(59) X(60) \
    X(70) X(71) X(72) X(73) X(74) X(75) X(76) X(80) X(81) X(82) X(83) X(84) X(85) X(86)

#ifdef PRIM_HOST_BUILD
template <int OP> int run_cases(int n, const uint32_t *in, uint32_t *out) {
    if (device_only(OP)) return -2;
    for (int i = 0; i < n; i++) run_op<OP>(in + (size_t)i * in_words(OP), out + (size_t)i * out_words(OP));
    return 0;
}
#else
template <int OP> __global__ void __launch_bounds__(64) prim_kernel(int n, const uint32_t *in, uint32_t *out) {
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= n) return;
    run_op<OP>(in + (size_t)i * in_words(OP), out + (size_t)i * out_words(OP));
}
template <int OP> int run_cases(int n, const uint32_t *in, uint32_t *out) {
    if (n <= 0) return 0;
    const size_t ib = (size_t)n * in_words(OP) * 4, ob = (size_t)n * out_words(OP) * 4;
    uint32_t *din = nullptr, *dout = nullptr;
    int rc = 0;
    if (hipMalloc(&din, ib) != hipSuccess) return 1;
    if (hipMalloc(&dout, ob) != hipSuccess) { (void)hipFree(din); return 1; }
    if (hipMemcpy(din, in, ib, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
    if (!rc && hipMemset(dout, 0, ob) != hipSuccess) rc = 2;
    if (!rc) {
        prim_kernel<OP><<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(n, din, dout);
        if (hipGetLastError() != hipSuccess) rc = 3;
    }
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = 4;
    if (!rc && hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    if (hipFree(din) != hipSuccess && !rc) rc = 6;
    if (hipFree(dout) != hipSuccess && !rc) rc = 6;
    return rc;
}
#endif

}  // namespace

#define PRIM_VISIBLE extern "C" __attribute__((visibility("default")))

// 0 = done; negative: unknown operation (-1) or one that only a device pass has (-2); positive: a HIP call failed
PRIM_VISIBLE int prim_run(int op, int n, const uint32_t *in, uint32_t *out) {
    switch (op) {
#define X(OP) case OP: return run_cases<OP>(n, in, out);
        PRIM_OPS(X)
#undef X
    }
    return -1;
}
PRIM_VISIBLE int prim_words(int op, int output) {
    switch (op) {
#define X(OP) case OP: return output ? out_words(OP) : in_words(OP);
        PRIM_OPS(X)
#undef X
    }
    return -1;
}
PRIM_VISIBLE int prim_is_device_build(void) {
#ifdef PRIM_HOST_BUILD
    return 0;
#else
    return 1;
#endif
}
PRIM_VISIBLE int prim_fqu_check_active(void) {
#ifdef ZK_FQU_CHECK
    return 1;
#else
    return 0;
#endif
}
