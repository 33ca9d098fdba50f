"""Host-side circuit synthesis through the C ABI (csrc/circuits.hip): the reference's MatrixCircuit (+ Poseidon),
FibonacciCircuit, PrimeCircuit and LinearEquationCircuit as R1CS (CSR) + full assignment, ready for Device.r1cs_load /
Device.witness_load.  No GPU needed."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Zkg16Error


class SynthesizedCircuit:
    """num_instance (incl. the constant 1), num_witness, num_constraints, r1cs (dict of CSR triples), z (Montgomery)."""

    def __init__(self, handle, check_satisfied=None):
        lib = _lib.load()
        ni, nw, nc = C.c_size_t(), C.c_size_t(), C.c_size_t()
        nnz = (C.c_size_t * 3)()
        lib.zkg16_circuit_dims(handle, C.byref(ni), C.byref(nw), C.byref(nc), C.byref(nnz))
        self.num_instance, self.num_witness, self.num_constraints = ni.value, nw.value, nc.value
        self.num_vars = ni.value + nw.value
        self.satisfied = bool(lib.zkg16_circuit_is_satisfied(handle)) if ((nc.value <= 200000 and check_satisfied is not False) or check_satisfied) else None
        rp = [np.zeros(nc.value + 1, dtype=np.uint64) for _ in range(3)]
        col = [np.zeros(max(nnz[m], 1), dtype=np.uint32) for m in range(3)]
        cf = [np.zeros((max(nnz[m], 1), 4), dtype=np.uint64) for m in range(3)]
        z = np.zeros((self.num_vars, 4), dtype=np.uint64)
        arr = lambda xs: (C.c_void_p * 3)(*[x.ctypes.data for x in xs])
        rc = lib.zkg16_circuit_export(handle, C.byref(arr(rp)), C.byref(arr(col)), C.byref(arr(cf)), z)
        if rc:
            raise Zkg16Error(rc, "circuit export")
        self.r1cs = dict(a=(rp[0], col[0][:nnz[0]], cf[0][:nnz[0]]), b=(rp[1], col[1][:nnz[1]], cf[1][:nnz[1]]),
                         c=(rp[2], col[2][:nnz[2]], cf[2][:nnz[2]]), num_inputs=self.num_instance, num_constraints=self.num_constraints)
        self.z = z
        self.public_inputs = z[1:self.num_instance].copy()
        self.domain = 1 << max(self.num_constraints + self.num_instance - 1, 0).bit_length()
        lib.zkg16_circuit_free(handle)


class CircuitHandle:
    """A synthesized circuit that stays inside the library: its dimensions and public inputs only.  Device.circuit_load(self) puts
    its matrices and assignment on the device without exporting them (the request path of circuits that are re-synthesized per
    request); close() (or garbage collection) frees it."""

    def __init__(self, handle):
        lib = _lib.load()
        self.handle = handle
        ni, nw, nc = C.c_size_t(), C.c_size_t(), C.c_size_t()
        nnz = (C.c_size_t * 3)()
        lib.zkg16_circuit_dims(handle, C.byref(ni), C.byref(nw), C.byref(nc), C.byref(nnz))
        self.num_instance, self.num_witness, self.num_constraints = ni.value, nw.value, nc.value
        self.num_vars = ni.value + nw.value
        pub = np.zeros((max(ni.value - 1, 0), 4), dtype=np.uint64)
        if ni.value > 1:
            rc = lib.zkg16_circuit_public_inputs(handle, pub.reshape(-1), ni.value - 1)
            if rc:
                raise Zkg16Error(rc, "zkg16_circuit_public_inputs")
        self.public_inputs = pub
        self.domain = 1 << max(self.num_constraints + self.num_instance - 1, 0).bit_length()
        self.satisfied = None
        self.z = self.r1cs = None

    def close(self):
        if self.handle is not None:
            _lib.load().zkg16_circuit_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 - interpreter shutdown
            pass


def prime_public_inputs(x, j):
    """The PrimeCircuit's public inputs for candidate j (x and the 256 digest bits), computed natively (zkg16_prime_public_inputs)."""
    out = np.zeros((257, 4), dtype=np.uint64)
    rc = _lib.load().zkg16_prime_public_inputs(x, j, out.reshape(-1))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_public_inputs")
    return out


def prime_circuit_handle(x, j):
    """PrimeCircuit of candidate j as a CircuitHandle (nothing exported to Python)."""
    h = C.c_void_p()
    rc = _lib.load().zkg16_circuit_prime(x, j, C.byref(h))
    if rc:
        raise Zkg16Error(rc, "zkg16_circuit_prime")
    c = CircuitHandle(h)
    c.j = j
    return c


def prime_dims(j):
    """The PrimeCircuit's dimensions for candidate index j (zkg16_prime_r1cs_dims; the same for every x) ->
    dict(num_instance, num_witness, num_constraints, nnz)."""
    ni, nw, nc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    nnz = (C.c_size_t * 3)()
    rc = _lib.load().zkg16_prime_r1cs_dims(j, C.byref(ni), C.byref(nw), C.byref(nc), C.byref(nnz))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_r1cs_dims")
    return dict(num_instance=ni.value, num_witness=nw.value, num_constraints=nc.value, nnz=tuple(nnz))


def prime_witness_host(x, j):
    """The PrimeCircuit's assignment for candidate (x, j) from the recorded witness program, evaluated on the host
    (zkg16_prime_witness_host): what Device.witness_prime is tested against -> z [num_vars, 4] (Montgomery)."""
    d = prime_dims(j)
    z = np.zeros((d["num_instance"] + d["num_witness"], 4), dtype=np.uint64)
    rc = _lib.load().zkg16_prime_witness_host(x, j, z.reshape(-1), z.shape[0])
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_witness_host")
    return z


def prime_r1cs_host(x, j):
    """The PrimeCircuit's R1CS for candidate (x, j) from the recorded template (zkg16_prime_r1cs_dims / _host) -> (r1cs dict as
    SynthesizedCircuit.r1cs, num_witness).  What Device.r1cs_prime is tested against."""
    lib = _lib.load()
    ni, nw, nc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    nnz = (C.c_size_t * 3)()
    rc = lib.zkg16_prime_r1cs_dims(j, C.byref(ni), C.byref(nw), C.byref(nc), C.byref(nnz))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_r1cs_dims")
    rp = [np.zeros(nc.value + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(max(nnz[m], 1), dtype=np.uint32) for m in range(3)]
    cf = [np.zeros((max(nnz[m], 1), 4), dtype=np.uint64) for m in range(3)]
    arr = lambda xs: (C.c_void_p * 3)(*[x.ctypes.data for x in xs])
    rc = lib.zkg16_prime_r1cs_host(x, j, C.byref(arr(rp)), C.byref(arr(col)), C.byref(arr(cf)))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_r1cs_host")
    return dict(a=(rp[0], col[0][:nnz[0]], cf[0][:nnz[0]]), b=(rp[1], col[1][:nnz[1]], cf[1][:nnz[1]]),
                c=(rp[2], col[2][:nnz[2]], cf[2][:nnz[2]]), num_inputs=ni.value, num_constraints=nc.value), nw.value


def prime_r1cs_template_host():
    """The template every candidate's R1CS is a patch of (zkg16_prime_r1cs_template_host): the j >= 1 form with the four
    candidate-dependent column-0 coefficients zero -> (r1cs dict as SynthesizedCircuit.r1cs, num_witness, patch_rows [4]: the
    constraint rows of the three A coefficients (n) and of the C coefficient (-j))."""
    lib = _lib.load()
    d = prime_dims(1)
    nnz, nc = d["nnz"], d["num_constraints"]
    rp = [np.zeros(nc + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(max(nnz[m], 1), dtype=np.uint32) for m in range(3)]
    cf = [np.zeros((max(nnz[m], 1), 4), dtype=np.uint64) for m in range(3)]
    rows = np.zeros(4, dtype=np.uint64)
    arr = lambda xs: (C.c_void_p * 3)(*[x.ctypes.data for x in xs])
    rc = lib.zkg16_prime_r1cs_template_host(C.byref(arr(rp)), C.byref(arr(col)), C.byref(arr(cf)), rows.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_r1cs_template_host")
    return dict(a=(rp[0], col[0][:nnz[0]], cf[0][:nnz[0]]), b=(rp[1], col[1][:nnz[1]], cf[1][:nnz[1]]),
                c=(rp[2], col[2][:nnz[2]], cf[2][:nnz[2]]), num_inputs=d["num_instance"], num_constraints=nc), d["num_witness"], rows


def prime_key_corrections(trapdoor_mont, g1_gen):
    """What a candidate's key has over the template's for one trapdoor [5, 4] and generator g1 [12] (zkg16_prime_key_corrections,
    host only) -> (corr [3, 12] = U | V_n | V_j affine Montgomery limbs, inf [3]): a_query[0] = template's + n U,
    gamma_abc_g1[0] = template's + n V_n - j V_j."""
    trap = np.ascontiguousarray(trapdoor_mont, dtype=np.uint64).reshape(-1)
    g1 = np.ascontiguousarray(g1_gen, dtype=np.uint64).reshape(-1)
    if trap.size != 20 or g1.size != 12:
        raise ValueError("prime_key_corrections: trapdoor 5 x 4 limbs, g1 12 limbs")
    corr = np.zeros((3, 12), dtype=np.uint64)
    inf = np.zeros(3, dtype=np.uint8)
    rc = _lib.load().zkg16_prime_key_corrections(trap.ctypes.data, g1.ctypes.data, corr.ctypes.data, inf.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_key_corrections")
    return corr, inf


def prime_vk_extend(gamma_abc_g1, corr):
    """The extended key's points (zkg16_prime_vk_extend, host only): the template's gamma_abc_g1 [258, 12] followed by V_n and -V_j
    of corr (prime_key_corrections) -> [260, 12].  Under it every request of the trapdoor has the inputs prime_ext_inputs(x, j)."""
    gabc = np.ascontiguousarray(gamma_abc_g1, dtype=np.uint64).reshape(-1, 12)
    corr = np.ascontiguousarray(corr, dtype=np.uint64).reshape(-1)
    if gabc.shape[0] != 258 or corr.size != 36:
        raise ValueError("prime_vk_extend: gamma_abc_g1 258 x 12 limbs, corr 3 x 12 limbs")
    out = np.zeros((260, 12), dtype=np.uint64)
    rc = _lib.load().zkg16_prime_vk_extend(gabc.ctypes.data, corr.ctypes.data, out.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_vk_extend")
    return out


def prime_ext_inputs(x, j):
    """A request's 259 public inputs under the extended key (zkg16_prime_ext_inputs): prime_public_inputs(x, j), then n = the digest
    mod 2^20, then j -> [259, 4] Montgomery."""
    out = np.zeros((259, 4), dtype=np.uint64)
    rc = _lib.load().zkg16_prime_ext_inputs(x, j, out.reshape(-1))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_ext_inputs")
    return out


def r1cs_check_host(r1cs, z, num_variables):
    """Does the assignment z [num_variables, 4] (Montgomery) satisfy the system r1cs (a dict as SynthesizedCircuit.r1cs)?  Host only
    (zkg16_r1cs_check_host): the reference of Device.r1cs_check -> (n_bad, first_bad): failing constraint rows and the smallest of
    them, 2^64 - 1 when there is none."""
    keep, tabs = [], []
    for k, dt in ((0, np.uint64), (1, np.uint32), (2, np.uint64)):
        arrs = [np.ascontiguousarray(r1cs[m][k], dtype=dt) for m in "abc"]
        keep += arrs
        tabs.append((C.c_void_p * 3)(*[x.ctypes.data if x.size else None for x in arrs]))
    z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
    if z.shape[0] != num_variables or any(x.shape[0] != r1cs["num_constraints"] + 1 for x in keep[:3]):
        raise ValueError("r1cs_check_host: z has num_variables rows, every row pointer num_constraints + 1 entries")
    nb, fb = C.c_uint64(0), C.c_uint64(0)
    rc = _lib.load().zkg16_r1cs_check_host(C.byref(tabs[0]), C.byref(tabs[1]), C.byref(tabs[2]), r1cs["num_constraints"], num_variables,
                                           z.ctypes.data, C.byref(nb), C.byref(fb))
    if rc:
        raise Zkg16Error(rc, "zkg16_r1cs_check_host")
    return int(nb.value), int(fb.value)


def matrix_circuit(a, b):
    """MatrixCircuit for u64 matrices a, b (n x n lists/arrays); public inputs = Poseidon hashes of A, B, C = A*B."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    n = a.shape[0]
    assert a.shape == (n, n) and b.shape == (n, n)
    h = C.c_void_p()
    rc = _lib.load().zkg16_circuit_matrix(n, a.reshape(-1), b.reshape(-1), C.byref(h))
    if rc:
        raise Zkg16Error(rc, "zkg16_circuit_matrix")
    return SynthesizedCircuit(h)


def matrix_witness(a, b, num_vars):
    """Only the full assignment of matrix_circuit(a, b) (zkg16_circuit_matrix_witness): for callers that kept the matrices of
    this size.  num_vars = that circuit's num_instance + num_witness."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    n = a.shape[0]
    z = np.zeros((num_vars, 4), dtype=np.uint64)
    rc = _lib.load().zkg16_circuit_matrix_witness(n, a.reshape(-1), b.reshape(-1), z.reshape(-1), num_vars)
    if rc:
        raise Zkg16Error(rc, "zkg16_circuit_matrix_witness")
    return z


def matrix_sponge_states(a, b):
    """The host half of the device witness generator (zkg16_matrix_sponge_states; no GPU): the three native sponges of the
    matrix handler with the state in front of every permutation -> (states [3, ceil(n^2/2), 3, 4], hashes [3, 4])."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    n = a.shape[0]
    perms = (n * n + 1) // 2
    states = np.zeros((3, perms, 3, 4), dtype=np.uint64)
    hashes = np.zeros((3, 4), dtype=np.uint64)
    rc = _lib.load().zkg16_matrix_sponge_states(n, a.reshape(-1), b.reshape(-1), states.ctypes.data, hashes.reshape(-1))
    if rc:
        raise Zkg16Error(rc, "zkg16_matrix_sponge_states")
    return states, hashes


def matrix_sponge_states_batch(a, b, threads=0, want_states=True):
    """matrix_sponge_states for k requests of one size on a pool of host threads (zkg16_matrix_sponge_states_batch; no GPU):
    a, b [k, n, n] -> (states [k, 3, ceil(n^2/2), 3, 4] or None, hashes [k, 3, 4]); threads: 0 = 8."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if a.ndim != 3 or a.shape[1] != a.shape[2] or b.shape != a.shape:
        raise ValueError("matrix_sponge_states_batch: a and b must be k x n x n")
    k, n = a.shape[0], a.shape[1]
    perms = (n * n + 1) // 2
    states = np.zeros((k, 3, perms, 3, 4), dtype=np.uint64) if want_states else None
    hashes = np.zeros((k, 3, 4), dtype=np.uint64)
    rc = _lib.load().zkg16_matrix_sponge_states_batch(n, a.ctypes.data, b.ctypes.data, k, threads,
                                                      states.ctypes.data if want_states else None, hashes.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_matrix_sponge_states_batch")
    return states, hashes


def matrix_r1cs_from_plan(n):
    """The MatrixCircuit's R1CS of size n from its plan (zkg16_matrix_r1cs_dims / _host: templates + closed forms, host loops) ->
    (r1cs dict as SynthesizedCircuit.r1cs, num_witness).  What the device kernel of zkg16_r1cs_matrix is tested against."""
    lib = _lib.load()
    nc, nw = C.c_size_t(), C.c_size_t()
    nnz = (C.c_size_t * 3)()
    rc = lib.zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), C.byref(nnz))
    if rc:
        raise Zkg16Error(rc, "zkg16_matrix_r1cs_dims")
    rp = [np.zeros(nc.value + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(max(nnz[m], 1), dtype=np.uint32) for m in range(3)]
    cf = [np.zeros((max(nnz[m], 1), 4), dtype=np.uint64) for m in range(3)]
    arr = lambda xs: (C.c_void_p * 3)(*[x.ctypes.data for x in xs])
    rc = lib.zkg16_matrix_r1cs_host(n, C.byref(arr(rp)), C.byref(arr(col)), C.byref(arr(cf)))
    if rc:
        raise Zkg16Error(rc, "zkg16_matrix_r1cs_host")
    return dict(a=(rp[0], col[0][:nnz[0]], cf[0][:nnz[0]]), b=(rp[1], col[1][:nnz[1]], cf[1][:nnz[1]]),
                c=(rp[2], col[2][:nnz[2]], cf[2][:nnz[2]]), num_inputs=4, num_constraints=nc.value), nw.value


def fibonacci_circuit(a, b, steps):
    h = C.c_void_p()
    rc = _lib.load().zkg16_circuit_fibonacci(a, b, steps, C.byref(h))
    if rc:
        raise Zkg16Error(rc, "zkg16_circuit_fibonacci")
    return SynthesizedCircuit(h)


def fibonacci_circuit_handle(a, b, steps):
    """FibonacciCircuit as a CircuitHandle (nothing exported to Python)."""
    h = C.c_void_p()
    rc = _lib.load().zkg16_circuit_fibonacci(a, b, steps, C.byref(h))
    if rc:
        raise Zkg16Error(rc, "zkg16_circuit_fibonacci")
    return CircuitHandle(h)


def fibonacci_results_host(steps, a, b):
    """The `result` public input of fibonacci_circuit(a[i], b[i], steps) for k requests of one round count, by the mirror's additive
    chain in Fr (zkg16_fibonacci_results_host; no GPU): a, b [k] u64 -> [k, 4] Montgomery.  What the batched assignment kernel of
    Device.witness_fibonacci_batch is tested against."""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError("fibonacci_results_host: one b per a")
    out = np.zeros((a.shape[0], 4), dtype=np.uint64)
    rc = _lib.load().zkg16_fibonacci_results_host(steps, a.ctypes.data, b.ctypes.data, a.shape[0], out.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_fibonacci_results_host")
    return out


def _linear_system(what, a, b):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1)
    n = b.shape[0]
    if a.shape != (n, n):
        raise ValueError(what + ": a must be n x n for the n entries of b")
    return a, b, n


LINEAR_SOLVERS = {"forward": 0, "elimination": 1}       # option "linear_solver"


def linear_solver_id(solver):
    """"forward" | "elimination" -> the value of option "linear_solver"."""
    if solver not in LINEAR_SOLVERS:
        raise ValueError("solver must be 'forward' or 'elimination', not %r" % (solver,))
    return LINEAR_SOLVERS[solver]


def _linear_raw(a, b, solver="forward"):
    a, b, n = _linear_system("linear_circuit", a, b)
    name = "zkg16_circuit_linear_general" if linear_solver_id(solver) else "zkg16_circuit_linear"
    h = C.c_void_p()
    rc = getattr(_lib.load(), name)(n, a.ctypes.data, b.ctypes.data, C.byref(h))
    if rc:
        raise Zkg16Error(rc, name)
    return h


def linear_circuit(a, b, solver="forward"):
    """LinearEquationCircuit for the square system a [n, n], b [n] (u64) with the handler's own solution as the witness
    (zkg16_circuit_linear): x solves the LOWER triangle of a, so the circuit is satisfied exactly when the strict upper triangle
    times x is zero — `satisfied` says which.  Public inputs: a[0][*], b[0], a[1][*], b[1], ...  A zero diagonal entry: Zkg16Error
    (ZKG16_ERR_UNSUPPORTED; the reference panics).
    solver="elimination" (zkg16_circuit_linear_general): the same matrices with x from Gaussian elimination over Fr, satisfied for
    every a that is non-singular mod r; a singular a: Zkg16Error (ZKG16_ERR_UNSUPPORTED)."""
    return SynthesizedCircuit(_linear_raw(a, b, solver))


def linear_circuit_handle(a, b, solver="forward"):
    """linear_circuit as a CircuitHandle (nothing exported to Python)."""
    return CircuitHandle(_linear_raw(a, b, solver))


def linear_solve_host(a, b):
    """The linear handler's solver (linear_equations.rs:20-41) for k systems of one size on the host (zkg16_linear_solve_host; no GPU):
    a [k, n, n], b [k, n] u64 -> x [k, n, 4] Montgomery.  What the kernels of Device.witness_linear_batch are tested against."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if a.ndim != 3 or a.shape[1] != a.shape[2] or b.shape != a.shape[:2]:
        raise ValueError("linear_solve_host: a must be k x n x n and b k x n")
    k, n = b.shape
    x = np.zeros((k, n, 4), dtype=np.uint64)
    rc = _lib.load().zkg16_linear_solve_host(n, a.ctypes.data, b.ctypes.data, k, x.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_linear_solve_host")
    return x


def linear_solve_general_host(a, b):
    """Gaussian elimination over Fr with row pivoting for k systems of one size on the host (zkg16_linear_solve_general_host; no GPU;
    the phase functions of wit_linear_elim_kernel on one lane): a [k, n, n], b [k, n] u64 -> (x [k, n, 4] Montgomery or None, status
    [k] u32).  status[i] is 0, or 1 + c with c the smallest column index for which columns 0..c of a[i] are linearly dependent mod r;
    x is None when any request is singular."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if a.ndim != 3 or a.shape[1] != a.shape[2] or b.shape != a.shape[:2]:
        raise ValueError("linear_solve_general_host: a must be k x n x n and b k x n")
    k, n = b.shape
    x = np.zeros((k, n, 4), dtype=np.uint64)
    status = np.zeros(k, dtype=np.uint32)
    rc = _lib.load().zkg16_linear_solve_general_host(n, a.ctypes.data, b.ctypes.data, k, x.ctypes.data, status.ctypes.data)
    if rc == 7 and status.any():           # ZKG16_ERR_UNSUPPORTED: some request is singular
        return None, status
    if rc:
        raise Zkg16Error(rc, "zkg16_linear_solve_general_host")
    return x, status


def linear_r1cs_dims(n):
    """The linear-equations circuit's dimensions for size n (zkg16_linear_r1cs_dims; the same for every request) ->
    dict(num_instance, num_witness, num_constraints, nnz)."""
    ni, nw, nc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    nnz = (C.c_size_t * 3)()
    rc = _lib.load().zkg16_linear_r1cs_dims(n, C.byref(ni), C.byref(nw), C.byref(nc), C.byref(nnz))
    if rc:
        raise Zkg16Error(rc, "zkg16_linear_r1cs_dims")
    return dict(num_instance=ni.value, num_witness=nw.value, num_constraints=nc.value, nnz=tuple(nnz))


def prime_search(x, i_max):
    """The prime handler's native search (backend/prime_snark.rs:57-70): first j <= i_max whose hash(x + j) mod 2^20 passes the
    Fermat test -> dict(found, j, prime, digest) (zkg16_prime_search)."""
    j, p, found = C.c_uint64(0), C.c_uint32(0), C.c_int(0)
    digest = np.zeros(32, dtype=np.uint8)
    rc = _lib.load().zkg16_prime_search(x, i_max, C.byref(j), C.byref(p), digest, C.byref(found))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_search")
    return dict(found=bool(found.value), j=j.value, prime=p.value, digest=bytes(digest))


def prime_candidate(x, j):
    """check_if_next_is_prime(x, j) natively -> dict(digest, n, bases, r_bytes, is_prime)."""
    n, isp = C.c_uint32(0), C.c_int(0)
    digest, rb = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    bases = np.zeros(3, dtype=np.uint32)
    rc = _lib.load().zkg16_prime_candidate(x, j, digest, C.byref(n), bases, rb, C.byref(isp))
    if rc:
        raise Zkg16Error(rc, "zkg16_prime_candidate")
    return dict(digest=bytes(digest), n=n.value, bases=[int(b) for b in bases], r_bytes=bytes(rb), is_prime=bool(isp.value))


def prime_circuit(x, i_max_or_j, search=True, check_satisfied=True):
    """The reference's PrimeCircuit (C++ mirror).  search=True: as prove_prime — find the first prime candidate j <= i_max and
    build its circuit (raises if none); search=False: the circuit of candidate j itself, as verify_prime rebuilds it.
    check_satisfied: evaluate all 338 k constraints on the assignment on the host.  The reference's prime handler does assert
    cs.is_satisfied() on every request (prime_snark.rs:123-128), and ark-groth16's prover debug_asserts it; the matrix and Fibonacci
    handlers do not.  Here it costs about as much as the synthesis itself, so timed paths pass False — the device check
    (Device.r1cs_check, handlers' check_on_device=True) answers the same question on assignments that were never synthesized."""
    j = i_max_or_j
    if search:
        res = prime_search(x, i_max_or_j)
        if not res["found"]:
            raise ValueError("no prime candidate for x=%d within i=%d" % (x, i_max_or_j))
        j = res["j"]
    h = C.c_void_p()
    rc = _lib.load().zkg16_circuit_prime(x, j, C.byref(h))
    if rc:
        raise Zkg16Error(rc, "zkg16_circuit_prime")
    c = SynthesizedCircuit(h, check_satisfied=check_satisfied)
    c.j = j
    return c


def matrix_hash_batch_host(m, threads=0):
    """The matrix handler's hash of k matrices of one size on host threads (zkg16_matrix_hash_batch_host; no GPU): m [k, n, n] u64 ->
    [k, 4] Montgomery Fr, row i = hash_a of matrix_sponge_states(m[i], .)."""
    m = np.ascontiguousarray(m, dtype=np.uint64)
    if m.ndim != 3 or m.shape[1] != m.shape[2]:
        raise ValueError("matrix_hash_batch_host: m must be k x n x n")
    out = np.zeros((m.shape[0], 4), dtype=np.uint64)
    rc = _lib.load().zkg16_matrix_hash_batch_host(m.shape[1], m.ctypes.data, m.shape[0], threads, out.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_matrix_hash_batch_host")
    return out


def poseidon_hash_batch_host(elems, threads=0):
    """k Poseidon hashes on host threads (zkg16_poseidon_hash_batch_host; no GPU): elems [k, n, 4] Montgomery Fr -> [k, 4]."""
    elems = np.ascontiguousarray(elems, dtype=np.uint64)
    if elems.ndim != 3 or elems.shape[2] != 4:
        raise ValueError("poseidon_hash_batch_host: elems must be k x n x 4")
    out = np.zeros((elems.shape[0], 4), dtype=np.uint64)
    rc = _lib.load().zkg16_poseidon_hash_batch_host(elems.ctypes.data, elems.shape[1], elems.shape[0], threads, out.ctypes.data)
    if rc:
        raise Zkg16Error(rc, "zkg16_poseidon_hash_batch_host")
    return out


def poseidon_hash(elems_mont):
    e = np.ascontiguousarray(elems_mont, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(4, dtype=np.uint64)
    rc = _lib.load().zkg16_poseidon_hash(e, e.shape[0], out)
    if rc:
        raise Zkg16Error(rc, "zkg16_poseidon_hash")
    return out
