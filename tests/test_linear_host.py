"""The host side of the linear-equations route (no GPU), against the big-integer model of tests/linear_cases.py: the host solver, the
mirror's dimensions, matrices and assignment, the fact the shared key rests on — the matrices depend on n alone —, the verdicts
(satisfied for a lower-triangular a, the model's failing rows for a dense one), the argument rules, the kernels' lane functions
(csrc/linear_dev.cuh compiled for the host and driven over 64 simulated lanes), and the order of the handlers' draws on a fake
Device."""
import ctypes as C
import random

import numpy as np
import pytest

import linear_cases as LC
from linear_cases import BAD_ARG, OK, SENTINEL, U64_MAX, UNSUPPORTED


def _vp(x):
    return C.c_void_p(x.ctypes.data)


# ------------------------------------------------------------------------------------------------ the solver
@pytest.mark.parametrize("n", [1, 2, 3, 8, 65])
def test_solve_host_equals_the_model(n):
    from zksnark_finalproject_amd.circuits import linear_solve_host
    a, b, kinds = LC.requests(n, 5, seed=11)
    x = linear_solve_host(a, b)
    assert x.shape == (5, n, 4) and x.dtype == np.uint64
    for q in range(5):
        assert np.array_equal(x[q], LC.mont_limbs(LC.solve(a[q], b[q]))), (n, q, kinds[q])
    assert not x[2].any()                # b = 0: x = 0


def test_the_model_agrees_with_itself():
    """The closed form of the failing rows (U x != 0) is what evaluating every row of the model's matrices on the model's assignment
    gives; a lower-triangular a and b = 0 leave none, the dense requests used below leave some."""
    for n in (1, 2, 3, 8):
        a, b, kinds = LC.requests(n, 5, seed=3)
        for q in range(5):
            assert LC.failing_rows(a[q], b[q]) == LC.rows_unsatisfied(a[q], b[q]), (n, q)
            if kinds[q] != "dense":
                assert LC.failing_rows(a[q], b[q]) == [], (n, q)
    for n in (2, 3, 8):
        a, b = LC.dense_unsatisfied(n)
        assert LC.failing_rows(a, b) and all(r % (n + 1) == n for r in LC.failing_rows(a, b))


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_mirror_equals_the_model(n):
    from zksnark_finalproject_amd.circuits import linear_circuit, linear_r1cs_dims
    d = LC.dims(n)
    assert linear_r1cs_dims(n) == d
    A, B, Cm = LC.matrices(n)
    want = dict(a=LC.csr(A), b=LC.csr(B), c=LC.csr(Cm))
    a, b, kinds = LC.requests(n, 5, seed=21)
    for q in range(5):
        c = linear_circuit(a[q], b[q])
        assert (c.num_instance, c.num_witness, c.num_constraints) == (d["num_instance"], d["num_witness"], d["num_constraints"])
        for m, nnz in zip("abc", d["nnz"]):
            assert c.r1cs[m][1].shape[0] == nnz
            for got, exp in zip(c.r1cs[m], want[m]):
                assert got.dtype == exp.dtype and np.array_equal(got, exp), (n, q, m)
        assert np.array_equal(c.z, LC.mont_limbs(LC.assignment(a[q], b[q]))), (n, q, kinds[q])
        # the handler's public input list: a[i][*], b[i] row by row
        flat = [int(v) for i in range(n) for v in list(a[q][i]) + [b[q][i]]]
        assert np.array_equal(c.public_inputs, LC.mont_limbs(flat))


def test_matrices_do_not_depend_on_the_request():
    from zksnark_finalproject_amd.circuits import linear_circuit, linear_r1cs_dims
    for n in (2, 8):
        lo, de = linear_circuit(*LC.system(n, "lower", 1)), linear_circuit(*LC.dense_unsatisfied(n))
        d = linear_r1cs_dims(n)
        for c in (lo, de):
            assert (c.num_instance, c.num_witness, c.num_constraints) == (d["num_instance"], d["num_witness"], d["num_constraints"])
            assert tuple(c.r1cs[m][1].shape[0] for m in "abc") == d["nnz"]
        for m in "abc":
            for x, y in zip(lo.r1cs[m], de.r1cs[m]):
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (n, m)
        assert not np.array_equal(lo.z, de.z)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_verdicts_are_the_models(n):
    """zkg16_circuit_is_satisfied: true for a lower-triangular a (and for b = 0), false for a dense one; zkg16_r1cs_check_host names
    the model's failing rows."""
    from zksnark_finalproject_amd.circuits import linear_circuit, r1cs_check_host
    for kind in ("lower", "zero_b"):
        c = linear_circuit(*LC.system(n, kind, 5))
        assert c.satisfied is True
        assert r1cs_check_host(c.r1cs, c.z, c.num_vars) == (0, U64_MAX)
    a, b = LC.dense_unsatisfied(n)
    bad = LC.failing_rows(a, b)
    assert bad
    c = linear_circuit(a, b)
    assert c.satisfied is False
    assert r1cs_check_host(c.r1cs, c.z, c.num_vars) == (len(bad), bad[0])


def test_n1_is_always_satisfied():
    from zksnark_finalproject_amd.circuits import linear_circuit
    for kind in ("lower", "dense", "zero_b"):
        assert linear_circuit(*LC.system(1, kind, 2)).satisfied is True


# ------------------------------------------------------------------------------------------------ argument rules
def test_bad_arguments_write_nothing():
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    n = 3
    a, b = LC.lower_requests(n, 2, seed=9)
    x = np.full((2, n, 4), SENTINEL, dtype=np.uint64)
    solve = lib.zkg16_linear_solve_host
    assert solve(n, _vp(a), _vp(b), 0, _vp(x)) == BAD_ARG
    assert solve(0, _vp(a), _vp(b), 2, _vp(x)) == BAD_ARG
    assert solve(LC.N_MAX + 1, _vp(a), _vp(b), 2, _vp(x)) == BAD_ARG
    assert solve(n, None, _vp(b), 2, _vp(x)) == BAD_ARG
    assert solve(n, _vp(a), None, 2, _vp(x)) == BAD_ARG
    assert solve(n, _vp(a), _vp(b), 2, None) == BAD_ARG
    z = a.copy()
    z[1, 2, 2] = 0                      # a zero diagonal entry in the second request
    assert solve(n, _vp(z), _vp(b), 2, _vp(x)) == UNSUPPORTED
    assert (x == SENTINEL).all()
    assert solve(n, _vp(a), _vp(b), 2, _vp(x)) == OK and not (x == SENTINEL).all()

    h = C.c_void_p(SENTINEL)
    circ = lib.zkg16_circuit_linear
    assert circ(0, _vp(a), _vp(b), C.byref(h)) == BAD_ARG
    assert circ(LC.N_MAX + 1, _vp(a), _vp(b), C.byref(h)) == BAD_ARG
    assert circ(n, None, _vp(b), C.byref(h)) == BAD_ARG
    assert circ(n, _vp(a), None, C.byref(h)) == BAD_ARG
    assert circ(n, _vp(a), _vp(b), None) == BAD_ARG
    assert circ(n, _vp(z[1]), _vp(b), C.byref(h)) == UNSUPPORTED
    assert h.value == SENTINEL

    sz = lambda: C.c_size_t(12345)
    ni, nw, nc, nnz = sz(), sz(), sz(), (C.c_size_t * 3)(7, 7, 7)
    for bad in (0, LC.N_MAX + 1):
        assert lib.zkg16_linear_r1cs_dims(bad, C.byref(ni), C.byref(nw), C.byref(nc), C.byref(nnz)) == BAD_ARG
    assert (ni.value, nw.value, nc.value, tuple(nnz)) == (12345, 12345, 12345, (7, 7, 7))
    assert lib.zkg16_linear_r1cs_dims(LC.N_MAX, C.byref(ni), None, None, None) == OK and ni.value == 1 + LC.N_MAX * (LC.N_MAX + 1)

    # the device entries refuse the same before they look at the ctx
    hs = np.full(2, SENTINEL, dtype=np.uint64)
    assert lib.zkg16_witness_linear_batch(None, n, _vp(a), _vp(b), 2, _vp(hs), _vp(x), None) == BAD_ARG
    rh = C.c_uint64(SENTINEL)
    assert lib.zkg16_r1cs_linear(None, n, C.byref(rh)) == BAD_ARG
    proofs, inf = np.full((2, 48), SENTINEL, dtype=np.uint64), np.full((2, 3), 0xA5, dtype=np.uint8)
    r = np.zeros((2, 4), dtype=np.uint64)
    assert lib.zkg16_prove_linear_batch(None, 1, 2, n, _vp(a), _vp(b), 2, _vp(r), _vp(r), _vp(proofs), _vp(inf), None, None) == BAD_ARG
    assert (hs == SENTINEL).all() and rh.value == SENTINEL and (proofs == SENTINEL).all() and (inf == 0xA5).all()


def test_python_wrappers_refuse_shapes():
    from zksnark_finalproject_amd._lib import Zkg16Error
    from zksnark_finalproject_amd.circuits import linear_circuit, linear_solve_host
    with pytest.raises(ValueError):
        linear_circuit(np.ones((2, 3), dtype=np.uint64), np.ones(2, dtype=np.uint64))
    with pytest.raises(ValueError):
        linear_solve_host(np.ones((1, 2, 2), dtype=np.uint64), np.ones((1, 3), dtype=np.uint64))
    with pytest.raises(Zkg16Error) as e:
        linear_circuit(np.array([[1, 2], [3, 0]], dtype=np.uint64), np.ones(2, dtype=np.uint64))
    assert e.value.status == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the kernels' lane functions
@pytest.fixture(scope="module")
def shim():
    return LC.load_shim()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_lane_functions_reproduce_the_model(shim, n):
    """The solve kernel's schedule on 64 simulated lanes (inverses by lane, partial sums, butterfly, lane 0's finish) gives the model's
    x with every lane holding the folded sum, and the fill kernel's element function gives the model's assignment element by element.
    n = 63 | 64 | 65: a last row whose terms fill one stride less one, one stride exactly, and spill into a second; 129: a third."""
    for kind, seed in (("lower", 1), ("dense", 2)):
        a, b = LC.system(n, kind, seed)
        x = np.full((n, 4), SENTINEL, dtype=np.uint64)
        assert shim.lin_solve_lanes(n, _vp(a), _vp(b), _vp(x)) == 0
        assert np.array_equal(x, LC.mont_limbs(LC.solve(a, b))), (n, kind)
        z = np.full((3 * n * n + 2 * n + 1, 4), SENTINEL, dtype=np.uint64)
        shim.lin_fill(n, _vp(a), _vp(b), _vp(x), _vp(z))
        assert np.array_equal(z, LC.mont_limbs(LC.assignment(a, b))), (n, kind)


def test_lane_functions_equal_the_host_solver(shim):
    from zksnark_finalproject_amd.circuits import linear_solve_host
    n = 65
    a, b, _ = LC.requests(n, 3, seed=31)
    want = linear_solve_host(a, b)
    for q in range(3):
        x = np.zeros((n, 4), dtype=np.uint64)
        assert shim.lin_solve_lanes(n, _vp(a[q]), _vp(b[q]), _vp(x)) == 0
        assert np.array_equal(x, want[q])


# ------------------------------------------------------------------------------------------------ the draws of the handlers
class _FakeDevice:
    """The Device methods the linear handlers call: records the key inputs and the blinding pairs it is given."""

    def __init__(self, n):
        self.n, self.keys, self.rs, self.live, self.calls = n, [], [], set(), []
        self._next = 10

    def _new(self):
        self._next += 1
        self.live.add(self._next)
        return self._next

    def _vk(self):
        from zksnark_finalproject_amd import device
        from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
        mul = lambda g, base, k: device.scalar_mul(g, base, np.array([k, 0, 0, 0], dtype=np.uint64))[0]
        g1, g2 = g1_generator(), g2_generator()
        return dict(alpha_g1=mul("g1", g1, 2), beta_g2=mul("g2", g2, 3), gamma_g2=mul("g2", g2, 5), delta_g2=mul("g2", g2, 7),
                    gamma_abc_g1=np.stack([mul("g1", g1, 11 + i) for i in range(1 + self.n * (self.n + 1))]))

    def _proof(self):
        from zksnark_finalproject_amd.workloads import g1_generator, g2_generator
        return np.concatenate([g1_generator(), g2_generator(), g1_generator()]).astype(np.uint64)

    def circuit_load(self, circuit):
        self.calls.append("circuit_load")
        return self._new(), self._new()

    def r1cs_linear(self, n):
        assert n == self.n
        self.calls.append("r1cs_linear")
        return self._new()

    def setup_resident(self, r1cs_h, num_instance, trap, g1, g2):
        assert r1cs_h in self.live and num_instance == 1 + self.n * (self.n + 1)
        self.calls.append("setup_resident")
        self.keys.append((trap.copy(), g1.copy(), g2.copy()))
        return self._new(), self._vk()

    def prove_resident(self, pk_h, r1cs_h, wit_h, r, s):
        assert {pk_h, r1cs_h, wit_h} <= self.live
        self.calls.append("prove_resident")
        self.rs.append((np.array(r), np.array(s)))
        return self._proof(), np.zeros(3, dtype=np.uint8)

    def prove_linear_batch(self, pk_h, r1cs_h, a, b, rs, ss):
        from zksnark_finalproject_amd.circuits import linear_solve_host
        assert {pk_h, r1cs_h} <= self.live
        self.calls.append("prove_linear_batch")
        k = len(a)
        self.rs += [(np.array(rs[i]), np.array(ss[i])) for i in range(k)]
        return np.tile(self._proof(), (k, 1)), np.zeros((k, 3), dtype=np.uint8), linear_solve_host(a, b), {}

    def _free(self, h):
        self.live.remove(h)
    r1cs_free = witness_free = pk_free = _free


def test_batch_handler_draws_in_the_single_handlers_order():
    """The key inputs and (r, s) of request 0 are prove_linear_equations' for the same seed; later requests draw their pairs after it,
    in request order; every handle is released; the record has the reference's OutputData fields plus valid, pvk and vk."""
    from zksnark_finalproject_amd import handlers, wire
    n = 2
    systems = [LC.system(n, kind, 40 + i) for i, kind in enumerate(("lower", "dense", "zero_b"))]
    one, many = _FakeDevice(n), _FakeDevice(n)
    single = handlers.prove_linear_equations(one, *systems[0], seed=0)
    recs = handlers.prove_linear_equations_batch(many, systems, seed=0)
    assert one.calls == ["circuit_load", "setup_resident", "prove_resident"]
    assert many.calls == ["r1cs_linear", "setup_resident", "prove_linear_batch"]
    assert not one.live and not many.live
    assert len(one.keys) == len(many.keys) == 1
    for x, y in zip(one.keys[0], many.keys[0]):
        assert np.array_equal(x, y)
    rng = random.Random(0)
    handlers._draw_key(rng)
    for i in range(3):
        r, s = handlers._draw_rs(rng)
        assert np.array_equal(many.rs[i][0], r) and np.array_equal(many.rs[i][1], s), i
    assert np.array_equal(one.rs[0][0], many.rs[0][0]) and np.array_equal(one.rs[0][1], many.rs[0][1])
    public = lambda rec: {k for k in rec if not k.startswith("_")}
    assert public(single) == {"proof", "public_input", "num_constraints", "num_variables", "proving_time", "verifying_time", "valid", "pvk", "vk"}
    for i, rec in enumerate(recs):
        assert public(rec) == public(single), i
        assert rec["pvk"] == single["pvk"] and rec["vk"] == single["vk"]
        assert rec["num_constraints"] == single["num_constraints"] == n * (n + 1)
        assert rec["num_variables"] == single["num_variables"] == 1 + n * (n + 1)
        assert rec["valid"] is False               # the fake proof verifies under nothing
        a, b = systems[i]
        flat = [int(v) for r_ in range(n) for v in list(a[r_]) + [b[r_]]]
        assert np.array_equal(np.array([wire.decode_hash(s) for s in rec["public_input"]], dtype=np.uint64).reshape(-1, 4), LC.mont_limbs(flat))
    assert recs[0]["public_input"] == single["public_input"]
    # a key that is passed in stays the caller's, and no draw is spent on one
    kept = _FakeDevice(n)
    key = handlers.linear_key(kept, n, random.Random(5))
    assert set(key) == {"ph", "rh", "vk", "setup_time"} and {key["ph"], key["rh"]} == kept.live
    handlers.prove_linear_equations_batch(kept, systems[:1], seed=0, key=key)
    assert {key["ph"], key["rh"]} == kept.live
    r0, s0 = handlers._draw_rs(random.Random(0))
    assert np.array_equal(kept.rs[0][0], r0) and np.array_equal(kept.rs[0][1], s0)
    with pytest.raises(ValueError):
        handlers.prove_linear_equations_batch(kept, [])
    with pytest.raises(ValueError):
        handlers.prove_linear_equations_batch(kept, [systems[0], LC.system(3, "lower", 1)])
    with pytest.raises(ValueError):
        handlers.prove_linear_equations(kept, np.ones((2, 3), dtype=np.uint64), np.ones(2, dtype=np.uint64))


def test_verify_handler_builds_the_inputs():
    """A system becomes its n^2 + n inputs a[i][*], b[i]; a system that is none is invalid for its entry only (host route, no device:
    the fake proofs verify under nothing, so only the shape handling shows)."""
    from zksnark_finalproject_amd import handlers
    n = 2
    dev = _FakeDevice(n)
    systems = [LC.system(n, "lower", 50), LC.system(n, "dense", 51)]
    recs = handlers.prove_linear_equations_batch(dev, systems, seed=1)
    seen = {}
    real = handlers.verify_proofs

    def spy(vk, pubs, proofs, dev=None):
        seen["pubs"] = pubs
        return real(vk, pubs, proofs, dev=dev)
    handlers.verify_proofs = spy
    try:
        out = handlers.verify_linear_equations(recs[0]["pvk"], [systems[0], ([[1, 2], [3, 1 << 64]], [1, 2])], [recs[0]["proof"], recs[1]["proof"]])
    finally:
        handlers.verify_proofs = real
    assert len(out["valid"]) == 2 and out["valid"][1] is False
    a, b = systems[0]
    flat = [int(v) for i in range(n) for v in list(a[i]) + [b[i]]]
    assert np.array_equal(seen["pubs"][0], LC.mont_limbs(flat))
    assert seen["pubs"][1].shape == (0, 4)
    with pytest.raises(ValueError):
        handlers.verify_linear_equations(recs[0]["pvk"], [systems[0]], [])
