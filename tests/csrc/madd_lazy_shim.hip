// TEST-ONLY: the bucket accumulations' mixed additions without their spare carry passes (csrc/ec.cuh: xyzz_madd_inline_lc for G1,
// xyzz_madd_lazy_lc for G2; csrc/ffu.cuh, "Skipped carry passes") on RAW limbs, one addition or one 32-step chain per case.  One
// source, two builds (tests/madd_lazy_cases.py), as tests/csrc/prim_shim.hip:
//   host build   hipcc --offload-host-only -DMADD_HOST_BUILD -DZK_FQU_CHECK: the cases run on the CPU with every operand assertion
//                of ffu.cuh live - value bounds, the limb bound of every lazy operand, and every product column accumulated a
//                second time in 128 bits;
//   device build the product's flags: one lane per case, 64 lanes per block (one wave: the LDS operand slots of fqu_mul2_lds are
//                indexed by the lane).
// Two operations exist only in the host build: products fed operands the limb rule forbids, which must abort (run in a child process).
// The shim needs nothing from libzkg16.so.
#include "ff.cuh"
#include "ffu.cuh"
#include "ec.cuh"
using namespace zk;

namespace {

template <class T> ZK_HD T ld(const uint32_t *p) { T r; __builtin_memcpy(&r, p, sizeof(T)); return r; }
template <class T> ZK_HD void st(uint32_t *p, const T &v) { __builtin_memcpy(p, &v, sizeof(T)); }

// operation numbers (tests/madd_lazy_cases.py holds the same table)
enum { G1_MADD = 0, G2_MADD = 1, G1_CHAIN = 2, G2_CHAIN = 3, BAD_TWO_LAZY = 4, BAD_COLUMN = 5 };
constexpr int CHAIN_STEPS = 32;

constexpr bool host_only(int op) { return op == BAD_TWO_LAZY || op == BAD_COLUMN; }
constexpr int words(int op) { return op == G1_MADD || op == G1_CHAIN ? 14 : 28; }      // of one coordinate
// record of an addition: accumulator (X, Y, ZZ, ZZZ), base (X, Y, two unused coordinates), neg flag
// record of a chain: accumulator, two bases (X, Y each), seed
constexpr int in_words(int op) { return host_only(op) ? 28 : 8 * words(op) + 1; }
constexpr int out_words(int op) { return host_only(op) ? 14 : op >= G1_CHAIN ? CHAIN_STEPS * 4 * words(op) : 4 * words(op); }

ZK_HD void madd_lc(XYZZ<FqU> &acc, const Affine<FqU> &q, bool neg) { xyzz_madd_inline_lc(acc, q, neg); }
ZK_HD void madd_lc(XYZZ<Fq2U> &acc, const Affine<Fq2U> &q, bool neg) { xyzz_madd_lazy_lc(acc, q, neg); }

template <class F> ZK_HD void madd_op(const uint32_t *in, uint32_t *out) {
    constexpr int W = sizeof(F) / 4;
    XYZZ<F> acc = ld<XYZZ<F>>(in);
    const Affine<F> base = ld<Affine<F>>(in + 4 * W);
    madd_lc(acc, base, in[8 * W] != 0);
    st(out, acc);
}

// CHAIN_STEPS additions, each chosen by the lane's own generator (tests/madd_lazy_cases.py: chain_choices repeats it): + or - the
// first or the second base; the point after EVERY step is written out.
template <class F> ZK_HD void chain_op(const uint32_t *in, uint32_t *out) {
    constexpr int W = sizeof(F) / 4;
    XYZZ<F> acc = ld<XYZZ<F>>(in);
    const Affine<F> b1 = ld<Affine<F>>(in + 4 * W), b2 = ld<Affine<F>>(in + 6 * W);
    uint32_t s = in[8 * W];
#pragma unroll 1
    for (int step = 0; step < CHAIN_STEPS; step++) {
        s = s * 1664525u + 1013904223u;
        const uint32_t c = s >> 29;
        madd_lc(acc, c < 5 ? b1 : b2, c == 3 || c == 4 || c == 7);
        st(out + step * 4 * W, acc);
    }
}

#ifdef MADD_HOST_BUILD
// what the limb rule forbids (ffu.cuh): both operands un-normalised.  BAD_TWO_LAZY declares nothing, so the operand check fires;
// BAD_COLUMN declares the limbs as they are (which only this test may do: the rule's static_assert is the product's own
// instantiation guard, bypassed here by a local copy of the column loop), so the 128-bit column check is what fires.
void bad_two_lazy(const uint32_t *in, uint32_t *out) { st(out, fqu_mul_impl<false>(ld<FqU>(in), ld<FqU>(in + 14))); }
void bad_column(const uint32_t *in, uint32_t *out) {
    const FqU a = ld<FqU>(in), b = ld<FqU>(in + 14);
    uint64_t acc = 0;
    FqU r = FqU::zero();
    for (int k = 0; k < 14; k++) {      // the operand rows of fqu_mul_impl's first columns, with its column check
        ZK_FQU_COL_DECL(col);
        acc = 0;
        for (int i = 0; i <= k; i++) { acc += (uint64_t)a.l[i] * b.l[k - i]; ZK_FQU_COL_MAC(col, a.l[i], b.l[k - i]); }
        ZK_FQU_COL_END(col, acc, "bad_column", k);
        r.l[k] = (uint32_t)acc;
    }
    st(out, r);
}
#endif

template <int OP> ZK_HD void run_op(const uint32_t *in, uint32_t *out) {
    if constexpr (OP == G1_MADD) madd_op<FqU>(in, out);
    else if constexpr (OP == G2_MADD) madd_op<Fq2U>(in, out);
    else if constexpr (OP == G1_CHAIN) chain_op<FqU>(in, out);
    else if constexpr (OP == G2_CHAIN) chain_op<Fq2U>(in, out);
}

#ifdef MADD_HOST_BUILD
template <int OP> int run_cases(int n, const uint32_t *in, uint32_t *out) {
    for (int i = 0; i < n; i++) {
        if constexpr (OP == BAD_TWO_LAZY) bad_two_lazy(in + (size_t)i * in_words(OP), out + (size_t)i * out_words(OP));
        else if constexpr (OP == BAD_COLUMN) bad_column(in + (size_t)i * in_words(OP), out + (size_t)i * out_words(OP));
        else run_op<OP>(in + (size_t)i * in_words(OP), out + (size_t)i * out_words(OP));
    }
    return 0;
}
#else
template <int OP> __global__ void __launch_bounds__(64) madd_lazy_kernel(int n, const uint32_t *in, uint32_t *out) {
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= n) return;
    run_op<OP>(in + (size_t)i * in_words(OP), out + (size_t)i * out_words(OP));
}
template <int OP> int run_cases(int n, const uint32_t *in, uint32_t *out) {
    if (host_only(OP)) return -2;
    if (n <= 0) return 0;
    const size_t ib = (size_t)n * in_words(OP) * 4, ob = (size_t)n * out_words(OP) * 4;
    uint32_t *din = nullptr, *dout = nullptr;
    int rc = 0;
    if (hipMalloc(&din, ib) != hipSuccess) return 1;
    if (hipMalloc(&dout, ob) != hipSuccess) { (void)hipFree(din); return 1; }
    if (hipMemcpy(din, in, ib, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
    if (!rc && hipMemset(dout, 0, ob) != hipSuccess) rc = 2;
    if (!rc) {
        madd_lazy_kernel<OP><<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(n, din, dout);
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

#define MADD_VISIBLE extern "C" __attribute__((visibility("default")))
#define MADD_OPS(X) X(0) X(1) X(2) X(3) X(4) X(5)

// 0 = done; negative: unknown operation (-1) or one that only the host build has (-2); positive: a HIP call failed
MADD_VISIBLE int madd_lazy_run(int op, int n, const uint32_t *in, uint32_t *out) {
    switch (op) {
#define X(OP) case OP: return run_cases<OP>(n, in, out);
        MADD_OPS(X)
#undef X
    }
    return -1;
}
MADD_VISIBLE int madd_lazy_words(int op, int output) {
    switch (op) {
#define X(OP) case OP: return output ? out_words(OP) : in_words(OP);
        MADD_OPS(X)
#undef X
    }
    return -1;
}
MADD_VISIBLE int madd_lazy_is_device_build(void) {
#ifdef MADD_HOST_BUILD
    return 0;
#else
    return 1;
#endif
}
MADD_VISIBLE int madd_lazy_check_active(void) {
#ifdef ZK_FQU_CHECK
    return 1;
#else
    return 0;
#endif
}
