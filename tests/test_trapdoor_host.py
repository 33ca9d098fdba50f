"""The trapdoor route without a device: zkg16_prove_trapdoor_host against the CPU oracle's real prover on a key the oracle made from
the same trapdoor (every byte of proof, flags and verifying key), against the big-integer model alone, at the degenerate (r, s)
choices, and its refusals; and the dot kernel's lane body on simulated lanes against Python sums."""
import ctypes as C
import random

import numpy as np
import pytest

import pyref as P
import trapdoor_cases as T
from helpers import fr_canon, fr_from_mont_vec, fr_mont, fr_mont_vec


def _host(*a, **kw):
    from zksnark_finalproject_amd.device import prove_trapdoor_host
    return prove_trapdoor_host(*a, **kw)


def _status(call):
    from zksnark_finalproject_amd._lib import Zkg16Error
    with pytest.raises(Zkg16Error) as e:
        call()
    return e.value.status


def _against_oracle(oracle, r1cs, zm, nv, seed):
    pk, meta, trap, vk = T.oracle_key(oracle, r1cs, nv, seed)
    rs, ss = T.rs_pairs(seed + 1, 1)
    want, want_inf = oracle.prove(pk, rs[0], ss[0], r1cs, zm)
    proofs, inf, got_vk = _host(r1cs, zm, trap, meta["g1"], meta["g2"], rs, ss)
    assert np.array_equal(proofs[0], want) and np.array_equal(inf[0], want_inf)
    assert T.same_vk(got_vk, vk)


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_host_form_equals_the_oracle_prover(oracle, shape):
    r1cs, _, zm, nv = T.random_system(shape)
    _against_oracle(oracle, r1cs, zm, nv, 100 + shape[0])


@pytest.mark.parametrize("kind", ["fibonacci", "linear", "matrix"])
def test_host_form_on_the_reference_circuits(oracle, kind):
    r1cs, _, zm, nv = T.circuit_system(kind)
    _against_oracle(oracle, r1cs, zm, nv, 200)


def test_host_form_equals_the_big_integer_model(oracle):
    """no prover at all: the model's logs (a, b, c) times the generators"""
    shape = (17, 3, 65)
    r1cs, z, zm, nv = T.random_system(shape)
    pk, meta, trap, _ = T.oracle_key(oracle, r1cs, nv, 300)
    rng = random.Random(301)
    r, s = P.rand_fr(rng), P.rand_fr(rng)
    a, b, c, ok = T.model_logs(oracle, meta, r1cs, z, zm, shape[1], r, s)
    assert ok
    proofs, inf, _ = _host(r1cs, zm, trap, meta["g1"], meta["g2"], fr_mont_vec([r]), fr_mont_vec([s]))
    assert not inf.any()
    assert np.array_equal(proofs[0][:12], oracle.point_mul("g1", meta["g1"], fr_canon(a))[0])
    assert np.array_equal(proofs[0][12:36], oracle.point_mul("g2", meta["g2"], fr_canon(b))[0])
    assert np.array_equal(proofs[0][36:], oracle.point_mul("g1", meta["g1"], fr_canon(c))[0])


def test_batch_of_the_host_form_equals_single_calls_and_threads_do_not_matter(oracle):
    shape = (16, 2, 64)
    r1cs, z, zm, nv = T.random_system(shape)
    d = T.draws(oracle, 310)
    zs = np.stack([zm, zm, zm])          # one satisfying assignment, three blinding pairs
    rs, ss = T.rs_pairs(311, 3)
    proofs, inf, vk = _host(r1cs, zs, d["trap"], d["g1"], d["g2"], rs, ss, threads=3)
    for i in range(3):
        p1, i1, vk1 = _host(r1cs, zm, d["trap"], d["g1"], d["g2"], rs[i:i + 1], ss[i:i + 1], threads=1)
        assert np.array_equal(p1[0], proofs[i]) and np.array_equal(i1[0], inf[i]) and T.same_vk(vk1, vk)


# ------------------------------------------------------------------------------------------------ the dot kernel's body
@pytest.fixture(scope="module")
def shim():
    return T.load_shim()


def test_shim_block_shape(shim):
    assert shim.td_block() == 256 and shim.td_chunk() % shim.td_block() == 0


@pytest.mark.parametrize("nv", [1, 255, 256, 257, "two_chunks_plus_one"])
@pytest.mark.parametrize("ni_kind", ["one", "all_but_one"])
def test_dot_body_on_simulated_lanes_equals_python_sums(shim, nv, ni_kind):
    if nv == "two_chunks_plus_one":
        nv = 2 * shim.td_chunk() + 1
    ni = 1 if ni_kind == "one" or nv == 1 else nv - 1
    rng = random.Random(400 + nv)
    # full-width values, with the extremes 0, 1 and r - 1 among them
    col = lambda: [(0, 1, P.R_MOD - 1, P.rand_fr(rng))[rng.randrange(4)] if rng.random() < .2 else P.rand_fr(rng) for _ in range(nv)]
    z, u, v, w, lg = col(), col(), col(), col(), col()
    want = [sum(a * b for a, b in zip(z, x)) % P.R_MOD for x in (u, v, w)] + [sum(a * b for a, b in zip(z[ni:], lg[ni:])) % P.R_MOD]
    arrs = [fr_mont_vec(x) for x in (z, u, v, w, lg)]
    chunks = (nv + shim.td_chunk() - 1) // shim.td_chunk()
    partial = np.full((chunks, 4, 4), T.SENTINEL, dtype=np.uint64)
    sums = np.zeros((4, 4), dtype=np.uint64)
    assert shim.td_dot_lanes(nv, ni, *[a.ctypes.data for a in arrs], partial.ctypes.data, sums.ctypes.data) == chunks
    assert fr_from_mont_vec(sums) == want
    # the partials are fully reduced and add up to the sums whatever the chunking
    per_chunk = [fr_from_mont_vec(partial[c]) for c in range(chunks)]
    assert all(np.array_equal(partial[c], fr_mont_vec(per_chunk[c])) for c in range(chunks))
    assert [sum(pc[j] for pc in per_chunk) % P.R_MOD for j in range(4)] == want


# ------------------------------------------------------------------------------------------------ degenerate outputs
@pytest.fixture(scope="module")
def degenerate(oracle):
    shape = (15, 2, 63)
    r1cs, z, zm, nv = T.random_system(shape)
    pk, meta, trap, vk = T.oracle_key(oracle, r1cs, nv, 500)
    return r1cs, zm, pk, meta, trap, T.degenerate_rs(oracle, meta, r1cs, z, zm, shape[1])


@pytest.mark.parametrize("slot", [0, 1, 2], ids=["a_is_zero", "b_is_zero", "c_is_zero"])
def test_a_log_of_zero_is_the_point_at_infinity_in_that_slot_alone(oracle, degenerate, slot):
    r1cs, zm, pk, meta, trap, choices = degenerate
    r, s = choices[slot]
    rs, ss = fr_mont_vec([r]), fr_mont_vec([s])
    proofs, inf, _ = _host(r1cs, zm, trap, meta["g1"], meta["g2"], rs, ss)
    assert list(inf[0]) == [int(i == slot) for i in range(3)]
    lo, hi = ((0, 12), (12, 36), (36, 48))[slot]
    assert not proofs[0][lo:hi].any()
    want, want_inf = oracle.prove(pk, rs[0], ss[0], r1cs, zm)
    assert np.array_equal(proofs[0], want) and np.array_equal(inf[0], want_inf)


# ------------------------------------------------------------------------------------------------ refusals
def _raw_call(r1cs, zs, nv, k, trap, g1, g2, rs, ss, null=None):
    """zkg16_prove_trapdoor_host with sentinel-filled outputs -> (status, outputs untouched?)"""
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    keep, tabs = [], []
    for i, dt in ((0, np.uint64), (1, np.uint32), (2, np.uint64)):
        arrs = [np.ascontiguousarray(r1cs[m][i], dtype=dt) for m in "abc"]
        keep += arrs
        tabs.append((C.c_void_p * 3)(*[x.ctypes.data if x.size else None for x in arrs]))
    ni = r1cs["num_inputs"]
    outs = [np.full(n, T.SENTINEL, dtype=np.uint64) for n in (48 * max(k, 1), 12, 24, 24, 24, 12 * ni)]
    inf = np.full(3 * max(k, 1), 0xA5, dtype=np.uint8)
    ins = dict(z=np.ascontiguousarray(zs, dtype=np.uint64), trap=np.ascontiguousarray(trap, dtype=np.uint64), g1=np.ascontiguousarray(g1),
               g2=np.ascontiguousarray(g2), r=np.ascontiguousarray(rs), s=np.ascontiguousarray(ss))
    ptr = {n: (None if n == null else a.ctypes.data) for n, a in ins.items()}
    out_ptr = [None if null == "out%d" % i else o.ctypes.data for i, o in enumerate(outs)]
    rc = lib.zkg16_prove_trapdoor_host(C.byref(tabs[0]), C.byref(tabs[1]), C.byref(tabs[2]), ni, r1cs["num_constraints"], nv, ptr["z"], k,
                                       ptr["trap"], ptr["g1"], ptr["g2"], ptr["r"], ptr["s"], 2, out_ptr[0],
                                       None if null == "inf" else inf.ctypes.data, *out_ptr[1:])
    untouched = all((o == np.uint64(T.SENTINEL)).all() for o in outs) and (inf == 0xA5).all()
    return rc, untouched


@pytest.fixture(scope="module")
def small(oracle):
    r1cs, z, zm, nv = T.random_system((15, 2, 63))
    d = T.draws(oracle, 600)
    rs, ss = T.rs_pairs(601, 3)
    return r1cs, zm, nv, d, rs, ss


def test_an_unsatisfied_assignment_is_refused_and_nothing_is_written(small):
    r1cs, zm, nv, d, rs, ss = small
    bad = T.bump(zm, nv - 1)
    assert _raw_call(r1cs, zm, nv, 1, d["trap"], d["g1"], d["g2"], rs[:1], ss[:1]) == (T.OK, False)
    assert _raw_call(r1cs, bad, nv, 1, d["trap"], d["g1"], d["g2"], rs[:1], ss[:1]) == (T.UNSATISFIED, True)
    assert _raw_call(r1cs, np.stack([zm, bad, zm]), nv, 3, d["trap"], d["g1"], d["g2"], rs, ss) == (T.UNSATISFIED, True)
    assert _raw_call(r1cs, np.stack([zm, zm, zm]), nv, 3, d["trap"], d["g1"], d["g2"], rs, ss) == (T.OK, False)


@pytest.mark.parametrize("null", ["z", "trap", "g1", "g2", "r", "s", "inf"] + ["out%d" % i for i in range(6)])
def test_null_pointers_are_bad_arguments(small, null):
    r1cs, zm, nv, d, rs, ss = small
    assert _raw_call(r1cs, zm, nv, 1, d["trap"], d["g1"], d["g2"], rs[:1], ss[:1], null=null) == (T.BAD_ARG, True)


def test_no_requests_is_a_bad_argument(small):
    r1cs, zm, nv, d, rs, ss = small
    assert _raw_call(r1cs, zm, nv, 0, d["trap"], d["g1"], d["g2"], rs[:1], ss[:1]) == (T.BAD_ARG, True)


@pytest.mark.parametrize("entry, word", [(4, "delta"), (3, "gamma")])
def test_a_zero_delta_or_gamma_is_refused_by_name(small, entry, word):
    from zksnark_finalproject_amd import _lib
    r1cs, zm, nv, d, rs, ss = small
    trap = d["trap"].copy()
    trap[entry] = 0
    assert _raw_call(r1cs, zm, nv, 1, trap, d["g1"], d["g2"], rs[:1], ss[:1]) == (T.BAD_ARG, True)
    assert word in _lib.load().zkg16_last_error(None).decode()


def test_a_tau_in_the_evaluation_domain_is_refused(small):
    """tau = omega^5 of the 32-point domain of the (15, 2, 63) system (15 + 2 rows -> 32), and tau = 1"""
    from zksnark_finalproject_amd import _lib
    r1cs, zm, nv, d, rs, ss = small
    omega = pow(7, (P.R_MOD - 1) // 32, P.R_MOD)
    assert pow(omega, 32, P.R_MOD) == 1 and pow(omega, 16, P.R_MOD) != 1
    for tau in (pow(omega, 5, P.R_MOD), 1):
        trap = d["trap"].copy()
        trap[0] = fr_mont(tau)
        assert _raw_call(r1cs, zm, nv, 1, trap, d["g1"], d["g2"], rs[:1], ss[:1]) == (T.BAD_ARG, True)
        assert "tau" in _lib.load().zkg16_last_error(None).decode()
    trap = d["trap"].copy()
    trap[0] = fr_mont(pow(7, (P.R_MOD - 1) // 64, P.R_MOD))      # order 64: not in this domain
    assert _raw_call(r1cs, zm, nv, 1, trap, d["g1"], d["g2"], rs[:1], ss[:1]) == (T.OK, False)


def test_every_entry_is_exported_and_bound():
    from zksnark_finalproject_amd import _lib
    lib = _lib.load()
    for name in ("zkg16_prove_trapdoor", "zkg16_prove_trapdoor_batch", "zkg16_prove_trapdoor_host"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
