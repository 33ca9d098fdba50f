"""The linear route under option "linear_solver" = 1 on the device: wit_linear_elim_kernel (Gaussian elimination over Fr, one workgroup
per request, working matrix in LDS or in the global workspace) behind zkg16_witness_linear_batch / zkg16_prove_linear_batch and the
handlers.  Assignment i must be the bytes the host mirror zkg16_circuit_linear_general exports for request i, x the big-integer
model's (tests/linear_general_cases.py), proof i zkg16_prove_resident's on the mirror's own handles, every proof must verify, and a
singular request must fail the whole call with its status by the column rule and nothing written."""
import ctypes as C
import random

import numpy as np
import pytest

import linear_cases as LC
import linear_general_cases as LG
import pyref as P
from helpers import fr_mont
from linear_cases import SENTINEL, U64_MAX, UNSUPPORTED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def _vars(n):
    return 3 * n * n + 2 * n + 1


def _vp(arr):
    return C.c_void_p(arr.ctypes.data)


@pytest.fixture(scope="module")
def expected():
    """n -> five requests cycling through LG.solvable(n) (a [5, n, n], b [5, n], names, the model's x [5, n, 4]) and the host
    mirror's exported assignments [5, vars, 4]: computed once per size, shared, never written to."""
    cache = {}

    def get(n):
        if n not in cache:
            from zksnark_finalproject_amd.circuits import linear_circuit
            cases = LG.solvable(n)
            picked = [cases[i % len(cases)] for i in range(5)]
            a, b, x = (np.stack([c[j] for c in picked]) for j in (1, 2, 3))
            distinct = min(5, len(cases))
            zs = np.stack([linear_circuit(a[i], b[i], solver="elimination").z for i in range(distinct)])[[i % distinct for i in range(5)]]
            assert zs.shape == (5, _vars(n), 4)
            for arr in (a, b, x, zs):
                arr.setflags(write=False)
            cache[n] = (a, b, [c[0] for c in picked], x, zs)
        return cache[n]
    return get


def _check_witness(dev, exp, n, k):
    a, b, names, x_want, zs = exp(n)
    handles, x, ms = dev.witness_linear_batch(a[:k], b[:k], solver="elimination")
    try:
        assert handles.shape == (k,) and x.shape == (k, n, 4) and len(set(int(h) for h in handles)) == k and ms["call_ms"] > 0
        for i in range(k):
            assert np.array_equal(x[i], x_want[i]), (n, i, names[i])
            assert dev.witness_read(int(handles[i]), _vars(n)).tobytes() == zs[i].tobytes(), (n, i, names[i])
    finally:
        for h in handles:
            dev.witness_free(int(h))


# ---------------------------------------------------------------------------------------------- witness_linear_batch
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("n", LG.SIZES)
def test_witness_elimination_equals_host_export(dev, expected, n, k):
    """n = 63 | 64: the working matrix in LDS, 64 with all 133 KB of it; 65: the global workspace.  Dense, row-exchange, permutation
    and lower-triangular requests in one batch."""
    _check_witness(dev, expected, n, k)


@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("n", [3, 8])
def test_both_placements_and_the_request_loop(dev, expected, n, lds, grid):
    """Option linear_elim_lds_max puts n = 3 and n = 8 on either side of the LDS / global switch, and the grid cap makes one, two and
    three workgroups walk the five requests (the global workspace then has as many slices): the same bytes every time."""
    dev.set_option("linear_elim_lds_max", n if lds else n - 1)
    dev.set_option("matrix_batch_grid", grid)
    try:
        _check_witness(dev, expected, n, 5)
    finally:
        dev.set_option("matrix_batch_grid", 0)
        dev.set_option("linear_elim_lds_max", 0)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_dense_requests_are_satisfied_where_the_forward_solver_fails_rows(dev, n):
    a_de, b_de = LC.dense_unsatisfied(n)                # dense with a non-zero diagonal: both solvers take it
    bad = LC.failing_rows(a_de, b_de)
    assert bad and LG.solve(a_de, b_de) is not None     # the model: unsatisfied by forward substitution, and non-singular
    a_lo, b_lo = LC.lower_requests(n, 2, seed=17)
    a, b = np.stack([a_lo[0], a_de, a_lo[1]]), np.stack([b_lo[0], b_de, b_lo[1]])
    rh = dev.r1cs_linear(n)
    try:
        for solver, want in (("elimination", [(0, U64_MAX)] * 3), ("forward", [(0, U64_MAX), (len(bad), bad[0]), (0, U64_MAX)])):
            handles, x, _ = dev.witness_linear_batch(a, b, solver=solver)
            try:
                assert dev.r1cs_check_batch(rh, handles) == want, (n, solver)
                if solver == "elimination":
                    assert np.array_equal(x[1], LC.mont_limbs(LG.solve(a_de, b_de)))
                    assert np.array_equal(x[0], LC.mont_limbs(LC.solve(a_lo[0], b_lo[0])))      # lower-triangular: the forward solver's x
            finally:
                for h in handles:
                    dev.witness_free(int(h))
    finally:
        dev.r1cs_free(rh)


# ---------------------------------------------------------------------------------------------- prove_linear_batch
def _rs(seed, k):
    rng = random.Random(seed)
    rs = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    ss = np.stack([fr_mont(rng.randrange(P.R_MOD)) for _ in range(k)]).reshape(k, 4)
    return rs, ss


@pytest.fixture(scope="module")
def keys(dev, expected):
    """n -> the shared key on r1cs_linear(n) and the reference for the five requests of expected(n): prove_resident on the general
    mirror's own circuit_load handles with (rs[i], ss[i]).  Made once per size, shared, never written to."""
    import bench
    from zksnark_finalproject_amd.circuits import linear_circuit_handle
    cache = {}

    def get(n):
        if n not in cache:
            a, b, names, x, _ = expected(n)
            rs, ss = _rs(5 + n, 5)
            rh = dev.r1cs_linear(n)
            trap, g1, g2 = bench.draw_key_inputs(11)
            ph, vk = dev.setup_resident(rh, 1 + n * (n + 1), trap, g1, g2)
            proofs, infs = [], []
            for i in range(5):
                rh_i, wh_i = dev.circuit_load(linear_circuit_handle(a[i], b[i], solver="elimination"))
                p, f = dev.prove_resident(ph, rh_i, wh_i, rs[i], ss[i])
                dev.witness_free(wh_i)
                dev.r1cs_free(rh_i)
                proofs.append(p)
                infs.append(f)
            ref = (np.stack(proofs), np.stack(infs))
            for arr in ref:
                arr.setflags(write=False)
            cache[n] = dict(n=n, a=a, b=b, names=names, x=x, rs=rs, ss=ss, rh=rh, ph=ph, vk=vk, ref=ref)
        return cache[n]
    yield get
    for st in cache.values():
        dev.pk_free(st["ph"])
        dev.r1cs_free(st["rh"])


def _pubs(a, b):
    return LC.mont_limbs([int(v) for i in range(len(b)) for v in list(a[i]) + [b[i]]])


def _check_prove(dev, st, k):
    from zksnark_finalproject_amd.device import pvk_prepare, verify_prepared
    proofs, inf, x, ms = dev.prove_linear_batch(st["ph"], st["rh"], st["a"][:k], st["b"][:k], st["rs"][:k], st["ss"][:k], solver="elimination")
    assert proofs.shape == (k, 48) and inf.shape == (k, 3) and x.shape == (k, st["n"], 4) and ms["prove_ms"] > 0
    pvk = pvk_prepare(st["vk"])
    for i in range(k):
        assert np.array_equal(proofs[i], st["ref"][0][i]) and np.array_equal(inf[i], st["ref"][1][i]), (i, st["names"][i])
        assert np.array_equal(x[i], st["x"][i]), (i, st["names"][i])
        assert bool(verify_prepared(pvk, _pubs(st["a"][i], st["b"][i]), proofs[i], inf[i])), (i, st["names"][i])


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("n", [3, 8])
def test_prove_elimination_equals_single_requests_and_verifies(dev, keys, n, k):
    _check_prove(dev, keys(n), k)


def test_prove_elimination_in_sub_batches_and_on_either_placement(dev, keys):
    """batch_max = 2 at K = 5: passes of 2, 2 and 1; then the same with the working matrices in the global workspace."""
    st = keys(3)
    dev.set_option("batch_max", 2)
    try:
        _check_prove(dev, st, 5)
        dev.set_option("linear_elim_lds_max", 2)
        _check_prove(dev, st, 5)
    finally:
        dev.set_option("linear_elim_lds_max", 0)
        dev.set_option("batch_max", 0)


# ---------------------------------------------------------------------------------------------- singular requests
@pytest.mark.parametrize("lds", [True, False])
def test_a_singular_request_fails_the_whole_call(dev, keys, lds):
    """Request 1 of 3 singular, for every singular family at n = 3: ZKG16_ERR_UNSUPPORTED from both entries, the outputs still hold
    the sentinel, zkg16_last_error names request 1 and the model's column, and no handle was registered: the next good call's
    handles follow the last good call's."""
    n = 3
    st = keys(n)
    dev.set_option("linear_solver", 1)
    dev.set_option("linear_elim_lds_max", n if lds else n - 1)
    try:
        before, _, _ = dev.witness_linear_batch(st["a"][:1], st["b"][:1])
        dev.witness_free(int(before[0]))
        for name, sa, sb, c in LG.singular(n):
            a = np.ascontiguousarray(np.stack([st["a"][0], sa, st["a"][1]]))
            b = np.ascontiguousarray(np.stack([st["b"][0], sb, st["b"][1]]))
            handles = np.full(3, SENTINEL, dtype=np.uint64)
            x = np.full((3, n, 4), SENTINEL, dtype=np.uint64)
            ms = (C.c_float * 3)(-1.0, -1.0, -1.0)
            rc = dev.lib.zkg16_witness_linear_batch(dev.ctx, n, _vp(a), _vp(b), 3, _vp(handles), _vp(x), C.addressof(ms))
            assert rc == UNSUPPORTED and (handles == SENTINEL).all() and (x == SENTINEL).all() and list(ms) == [-1.0] * 3, name
            text = dev.lib.zkg16_last_error(dev.ctx)
            assert b"request 1 " in text and b"singular" in text and b"column %d)" % c in text, (name, text)
            proofs, inf = np.full((3, 48), SENTINEL, dtype=np.uint64), np.full((3, 3), 0x5A, dtype=np.uint8)
            rs, ss = np.ascontiguousarray(st["rs"][:3]), np.ascontiguousarray(st["ss"][:3])
            rc = dev.lib.zkg16_prove_linear_batch(dev.ctx, st["ph"], st["rh"], n, _vp(a), _vp(b), 3, _vp(rs), _vp(ss), _vp(proofs), _vp(inf), _vp(x), None)
            assert rc == UNSUPPORTED and (proofs == SENTINEL).all() and (inf == 0x5A).all() and (x == SENTINEL).all(), name
            text = dev.lib.zkg16_last_error(dev.ctx)
            assert b"zkg16_prove_linear_batch: request 1 " in text and b"column %d)" % c in text, (name, text)
        after, _, _ = dev.witness_linear_batch(st["a"][:1], st["b"][:1])
        dev.witness_free(int(after[0]))
        assert int(after[0]) == int(before[0]) + 1
    finally:
        dev.set_option("linear_elim_lds_max", 0)
        dev.set_option("linear_solver", 0)
    _check_prove(dev, st, 2)                            # and the ctx still proves


def test_a_singular_request_in_a_later_sub_batch(dev, keys):
    """batch_max = 2, request 4 of 5 singular: the first two passes have proved when the third finds it — still nothing is written,
    and the request is named by its index in the call."""
    from zksnark_finalproject_amd import Zkg16Error
    st = keys(3)
    _, sa, sb, c = LG.singular(3)[-1]
    a, b = np.array(st["a"]), np.array(st["b"])
    a[4], b[4] = sa, sb
    dev.set_option("batch_max", 2)
    try:
        with pytest.raises(Zkg16Error) as e:
            dev.prove_linear_batch(st["ph"], st["rh"], a, b, st["rs"], st["ss"], solver="elimination")
        assert e.value.status == UNSUPPORTED and "request 4 " in str(e.value) and "column %d)" % c in str(e.value)
    finally:
        dev.set_option("batch_max", 0)


def test_a_singular_request_in_the_second_sub_batch_writes_nothing(dev, keys):
    """batch_max = 2, request 2 of 3 singular: the second pass holds that request alone, so its index in the pass (0) is not its index
    in the call.  Status 7 at the C entry, zkg16_last_error names request 2, and proofs, flags and solutions still hold the sentinel
    although the first pass has proved."""
    n = 3
    st = keys(n)
    _, sa, sb, c = LG.singular(n)[-1]
    a = np.ascontiguousarray(np.stack([st["a"][0], st["a"][1], sa]))
    b = np.ascontiguousarray(np.stack([st["b"][0], st["b"][1], sb]))
    proofs, inf = np.full((3, 48), SENTINEL, dtype=np.uint64), np.full((3, 3), 0x5A, dtype=np.uint8)
    x = np.full((3, n, 4), SENTINEL, dtype=np.uint64)
    rs, ss = np.ascontiguousarray(st["rs"][:3]), np.ascontiguousarray(st["ss"][:3])
    dev.set_option("linear_solver", 1)
    dev.set_option("batch_max", 2)
    try:
        rc = dev.lib.zkg16_prove_linear_batch(dev.ctx, st["ph"], st["rh"], n, _vp(a), _vp(b), 3, _vp(rs), _vp(ss), _vp(proofs), _vp(inf), _vp(x), None)
        text = dev.lib.zkg16_last_error(dev.ctx)
    finally:
        dev.set_option("batch_max", 0)
        dev.set_option("linear_solver", 0)
    assert rc == UNSUPPORTED == 7 and (proofs == SENTINEL).all() and (inf == 0x5A).all() and (x == SENTINEL).all()
    assert b"zkg16_prove_linear_batch: request 2 " in text and b"column %d)" % c in text, text


# ---------------------------------------------------------------------------------------------- the option
def test_the_solver_is_set_for_one_call_only(dev, expected):
    """solver= sets option "linear_solver" for the call and restores it: a following call with the default solver still refuses a zero
    diagonal entry — which the elimination has just solved."""
    from zksnark_finalproject_amd import Zkg16Error
    a, b, names, x_want, _ = expected(3)
    i = names.index("zero_corner")
    handles, x, _ = dev.witness_linear_batch(a[i:i + 1], b[i:i + 1], solver="elimination")
    dev.witness_free(int(handles[0]))
    assert np.array_equal(x[0], x_want[i])
    for kw in ({}, {"solver": "forward"}):
        with pytest.raises(Zkg16Error) as e:
            dev.witness_linear_batch(a[i:i + 1], b[i:i + 1], **kw)
        assert e.value.status == UNSUPPORTED and "zero diagonal" in str(e.value)
    # an option the caller has set survives a call that names the other solver
    dev.set_option("linear_solver", 1)
    try:
        with pytest.raises(Zkg16Error):
            dev.witness_linear_batch(a[i:i + 1], b[i:i + 1], solver="forward")
        handles, _, _ = dev.witness_linear_batch(a[i:i + 1], b[i:i + 1])
        dev.witness_free(int(handles[0]))
    finally:
        dev.set_option("linear_solver", 0)
    with pytest.raises(ValueError):
        dev.witness_linear_batch(a[:1], b[:1], solver="gauss")
    assert dev.lib.zkg16_set_option(dev.ctx, b"linear_solver", 2) != 0 and dev.lib.zkg16_set_option(dev.ctx, b"linear_elim_lds_max", 65) != 0


# ---------------------------------------------------------------------------------------------- handlers
def test_handlers_prove_dense_systems_that_verify(dev):
    from zksnark_finalproject_amd import Zkg16Error, handlers
    n = 3
    systems = [c[1:3] for c in LG.solvable(n) if c[0] in ("dense", "zero_corner", "late_zero_pivot", "permutation")]
    assert len(systems) == 4
    recs = handlers.prove_linear_equations_batch(dev, systems, seed=0, solver="elimination")
    assert [r["valid"] for r in recs] == [True] * 4 and all("satisfied" not in r for r in recs)
    proofs = [r["proof"] for r in recs]
    for use_dev in (dev, None):
        assert handlers.verify_linear_equations(recs[0]["vk"], systems, proofs, dev=use_dev)["valid"] == [True] * 4
    swapped = [systems[1], systems[0]] + systems[2:]
    assert handlers.verify_linear_equations(recs[0]["pvk"], swapped, proofs)["valid"] == [False, False, True, True]
    checked = handlers.prove_linear_equations_batch(dev, systems, seed=0, check_on_device=True, solver="elimination")
    assert [r["satisfied"] for r in checked] == [True] * 4 and [r["valid"] for r in checked] == [True] * 4
    assert [r["proof"] for r in checked] == proofs
    single = handlers.prove_linear_equations(dev, *systems[0], seed=0, solver="elimination")
    assert single["valid"] is True and single["proof"] == recs[0]["proof"] and single["vk"] == recs[0]["vk"]       # the same draws
    assert handlers.prove_linear_equations(dev, *systems[1], seed=2, check_on_device=True, solver="elimination")["satisfied"] is True
    # with the default solver the same dense request is proved and does not verify, as before
    dense_diag = LC.dense_unsatisfied(n)
    assert handlers.prove_linear_equations_batch(dev, [dense_diag], seed=0)[0]["valid"] is False
    assert handlers.prove_linear_equations_batch(dev, [dense_diag], seed=0, solver="elimination")[0]["valid"] is True
    _, sa, sb, _ = LG.singular(n)[2]
    with pytest.raises(Zkg16Error) as e:
        handlers.prove_linear_equations_batch(dev, [systems[0], (sa, sb)], seed=0, solver="elimination")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(Zkg16Error) as e:
        handlers.prove_linear_equations(dev, sa, sb, solver="elimination")
    assert e.value.status == UNSUPPORTED
