// TEST-ONLY: csrc/linear_dev.cuh (what wit_linear_solve_kernel runs, one 64-lane wave per request, and what wit_linear_fill_kernel runs,
// one lane per element) compiled for the host, so that the wave's schedule can be driven lane by lane and compared with the Python
// model on a machine without a GPU.  Built by tests/linear_cases.py with `hipcc --offload-host-only`.  Values cross in Montgomery u64
// limbs (ark's order).
#include "ff.cuh"
#include <string.h>
#include <vector>
using namespace zk;

namespace {
#include "linear_dev.cuh"
}  // namespace

extern "C" {

// The solve kernel's schedule for one request on 64 simulated lanes: the inverses (lane l the rows l, l + 64, ...), then row by row
// every lane's partial sum, the butterfly (partner = lane ^ 32, 16, .., 1) and lane 0's finish.  x_out: n x 4 limbs.  Returns the
// number of (row, lane) pairs whose folded sum differs from lane 0's — the butterfly leaves the sum in every lane, so 0.
int lin_solve_lanes(size_t n, const uint64_t *a, const uint64_t *b, uint64_t *x_out) {
    std::vector<Fr> y(n), x(n);
    for (int lane = 0; lane < LINEAR_LANES; lane++)
        for (size_t i = (size_t)lane; i < n; i += LINEAR_LANES) y[i] = linear_diag_inv(a[i * n + i]);
    int differ = 0;
    for (size_t i = 0; i < n; i++) {
        Fr v[LINEAR_LANES], nv[LINEAR_LANES];
        for (int lane = 0; lane < LINEAR_LANES; lane++) v[lane] = linear_partial(a + i * n, y.data(), i, lane);
        for (int off = LINEAR_LANES / 2; off; off >>= 1) {
            for (int lane = 0; lane < LINEAR_LANES; lane++) nv[lane] = linear_fold_step(v[lane], v[lane ^ off]);
            for (int lane = 0; lane < LINEAR_LANES; lane++) v[lane] = nv[lane];
        }
        for (int lane = 1; lane < LINEAR_LANES; lane++) differ += v[lane] != v[0];
        x[i] = linear_finish(b[i], v[0], y[i]);
        y[i] = linear_keep(x[i]);
    }
    memcpy(x_out, x.data(), n * sizeof(Fr));
    return differ;
}

// The fill kernel's element function for every t of one request: z_out = (3 n^2 + 2 n + 1) x 4 limbs; x = n x 4 limbs (Montgomery).
void lin_fill(size_t n, const uint64_t *a, const uint64_t *b, const uint64_t *x, uint64_t *z_out) {
    const size_t vars = 3 * n * n + 2 * n + 1;
    const Fr *xs = reinterpret_cast<const Fr *>(x);
    Fr *z = reinterpret_cast<Fr *>(z_out);
    for (size_t t = 0; t < vars; t++) z[t] = linear_fill_value(n, a, b, xs, t);
}

}  // extern "C"
