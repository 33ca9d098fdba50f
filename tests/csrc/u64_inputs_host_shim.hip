// TEST-ONLY: csrc/u64_inputs_dev.cuh (the lane functions of u64_rho_sums_kernel, u64_sums_reduce_kernel and u64_x_kernel) compiled for
// the host, so that the multiplier sums can be compared with Python integers and the grouped ladder's X with the oracle's points on a
// machine without a GPU.  Built by tests/u64_verify_cases.py with `hipcc --offload-host-only`; ZK_PD_CHECK turns on the value-bound
// assertions of the device pairing header.  Points cross this interface in saturated Montgomery limbs (u64, ark's order).
#define ZK_PD_CHECK 1
#include "u64_inputs_dev.cuh"

#include <string.h>

#include <vector>
using namespace zk;

extern "C" {

size_t u6_sum_slices(size_t k) { return u6::sum_slices(k); }
size_t u6_slice_len(size_t k) { return u6::slice_len(k); }
unsigned u6_group_lanes(size_t m) { return u6::group_lanes(m); }

// The two sums kernels as they are launched: a block of SUM_LANES lanes per (column tile, slice) writing its columns of the slice's
// partial, then one lane per column adding the slices.  sums: (m + 1) x 4 u64
void u6_rho_sums(const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t k, uint64_t *sums) {
    const size_t slices = u6::sum_slices(k), per = u6::slice_len(k), tiles = (m + 1 + u6::SUM_LANES - 1) / u6::SUM_LANES;
    std::vector<uint64_t> partial(slices * (m + 1) * 4 + 4, 0xA5A5A5A5A5A5A5A5ull);      // as unwritten device memory: not zero
    for (size_t y = 0; y < slices; y++)
        for (size_t x = 0; x < tiles; x++)
            for (unsigned t = 0; t < u6::SUM_LANES; t++) {
                const size_t col = x * u6::SUM_LANES + t;
                if (col > m) continue;
                const size_t start = y * per, lo = start < k ? start : k, hi = lo + per < k ? lo + per : k;
                u6::column_sum(col, values, m, rho, live, lo, hi, partial.data() + (y * (m + 1) + col) * 4);
            }
    for (size_t c = 0; c <= m; c++) {
        uint64_t acc[4] = {0, 0, 0, 0};
        for (size_t y = 0; y < slices; y++) pi::add256(acc, partial.data() + (y * (m + 1) + c) * 4);
        memcpy(sums + 4 * c, acc, 32);
    }
}

// u64_x_kernel's work for one proof over L simulated lanes (L = 0: group_lanes(m)): each lane's ladder, the rounds s = L / 2 .. 1
// in which lane l takes lane l + s's partial sum, and lane 0's finish.  gamma_abc: (1 + m) x 12 limbs (all-zero: the point at
// infinity); row: the m values.  Returns have (0: the point at infinity, out zeroed); out: 12 limbs
int u6_prepared_input(const uint64_t *gamma_abc, size_t m, const uint64_t *row, unsigned L, uint64_t *out) {
    std::vector<Affine<FqU>> g(m + 1);
    for (size_t i = 0; i <= m; i++) {
        G1Affine p;
        memcpy(&p, gamma_abc + 12 * i, sizeof p);
        g[i] = Affine<FqU>{fqu_from_sat(p.x), fqu_from_sat(p.y)};
    }
    if (!L) L = u6::group_lanes(m);
    std::vector<XYZZ<FqU>> part(L);
    for (unsigned l = 0; l < L; l++) part[l] = u6::ladder(g.data(), m, row, l, L);
    for (unsigned s = L >> 1; s; s >>= 1)
        for (unsigned l = 0; l < s; l++) xyzz_add(part[l], part[l + s]);
    FqU x = FqU::zero(), y = FqU::zero();
    const bool have = u6::finish(part[0], g[0], x, y);
    memset(out, 0, 96);
    if (have) {
        const G1Affine p{fqu_to_sat(x), fqu_to_sat(y)};
        memcpy(out, &p, sizeof p);
    }
    return have ? 1 : 0;
}

}  // extern "C"
