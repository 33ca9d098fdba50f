// TEST-ONLY: csrc/linear_elim_dev.cuh (the phases wit_linear_elim_kernel runs, one workgroup per request) compiled for the host, so that
// the workgroup's schedule can be driven lane by lane, phase by phase, and compared with the Python model on a machine without a GPU.
// Built by tests/linear_general_cases.py with `hipcc --offload-host-only`.  Values cross in Montgomery u64 limbs (ark's order).
#include "ff.cuh"
#include <string.h>
#include <vector>
using namespace zk;

namespace {
#include "linear_dev.cuh"
#include "linear_elim_dev.cuh"
}  // namespace

extern "C" {

// The kernel's schedule for one request on `lanes` simulated lanes.  Each phase runs for every lane before the next begins — where the
// kernel has a barrier —, the offers meet in their minimum as they do in the kernel's LDS word, and a request without a pivot in some
// column skips the arithmetic from there on and gets x = 0.  x_out: n x 4 limbs.  disagree (nullable): the number of (column, lane)
// pairs of the back substitution whose x_c differs from lane 0's — every lane forms it from the same two values, so 0.
// -> the status word: 0, or 1 + the first column without a pivot.
uint32_t lin_elim_lanes(size_t n, const uint64_t *a, const uint64_t *b, int lanes, uint64_t *x_out, int *disagree) {
    std::vector<Fr> M(n * (n + 1)), inv(n), x(n, Fr::zero());
    std::vector<uint32_t> order(n);
    uint32_t status = 0;
    int differ = 0;
    for (int lane = 0; lane < lanes; lane++) linear_elim_load(n, a, b, M.data(), order.data(), lane, lanes);
    for (size_t c = 0; c < n; c++) {
        uint32_t pick = (uint32_t)n;
        for (int lane = 0; lane < lanes; lane++) {
            const uint32_t offer = linear_elim_offer(n, M.data(), order.data(), c, lane, lanes);
            if (offer < pick) pick = offer;
        }
        if (pick < n) linear_elim_swap(order.data(), c, pick);
        else if (status == 0) status = (uint32_t)(1 + c);
        if (status == 0)
            for (int lane = 0; lane < lanes; lane++) linear_elim_reduce(n, M.data(), order.data(), c, lane, lanes);
    }
    if (status == 0) {
        for (int lane = 0; lane < lanes; lane++) linear_elim_invert(n, M.data(), order.data(), inv.data(), lane, lanes);
        for (size_t c = n; c-- > 0;) {
            // every lane reads the right-hand side of row order[c] before any lane's update — which touches the rows r < c only
            for (int lane = 0; lane < lanes; lane++) {
                const Fr xc = linear_elim_back(n, M.data(), order.data(), inv.data(), c, lane, lanes);
                if (lane == 0) x[c] = xc;
                else differ += xc != x[c];
            }
        }
    }
    memcpy(x_out, x.data(), n * sizeof(Fr));
    if (disagree) *disagree = differ;
    return status;
}

}  // extern "C"
