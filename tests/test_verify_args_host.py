"""The argument handling of the three host forms of batched verification (zkg16_verify_batch_host, zkg16_verify_prime_batch_host,
zkg16_verify_batch_u64_host) without a GPU: the texts the Python bindings refuse bad shapes with, before the library is asked
anything; what the C entry points refuse, with nothing written; and one set of u64 statements (tests/u64_verify_cases.py, verdicts
known by construction) given as Montgomery limbs and as plain values.  K = 3 under a key of three instance variables; the prime
form's refusals need no valid key, so small arrays of the right sizes stand under its calls."""
import ctypes as C
import random

import numpy as np
import pytest

import u64_verify_cases as U
import verify_batch_cases as VB
from helpers import *

K = 3


@pytest.fixture(scope="module")
def sim(oracle):
    return U.U64Sim(oracle, 2, K, (1,), 7301)


@pytest.fixture(scope="module")
def rho():
    return VB.draw_rho(random.Random(5), K)


# ------------------------------------------------------------------------------------------------ the bindings
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was asked for %s" % name)


@pytest.fixture
def no_library(monkeypatch):
    from zksnark_finalproject_amd import device
    monkeypatch.setattr(device._lib, "load", lambda: _NoLibrary())


def _refused(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text


def test_verify_batch_host_refuses_bad_shapes(sim, rho, no_library):
    from zksnark_finalproject_amd.device import verify_batch_host
    b = sim.batch
    _refused("verify_batch: one multiplier per proof", verify_batch_host, b.pvk, b.pubs, b.proofs, b.infs, rho=rho[:2])
    _refused("verify_batch: one flag triple per proof", verify_batch_host, b.pvk, b.pubs, b.proofs, b.infs[:2], rho=rho)
    wide = np.concatenate([b.pubs, b.pubs[:, :1]], axis=1)
    _refused("verify_batch: 3 public inputs per proof for a key with 3 instance variables", verify_batch_host, b.pvk, wide, b.proofs, b.infs, rho=rho)
    _refused("verify_batch: 1 public inputs per proof for a key with 3 instance variables", verify_batch_host, b.pvk, b.pubs[:, :1], b.proofs, b.infs, rho=rho)


def test_verify_prime_batch_host_refuses_bad_shapes(sim, rho, no_library):
    from zksnark_finalproject_amd.device import verify_prime_batch_host
    b = sim.batch
    xs, js = np.arange(K, dtype=np.uint64), np.ones(K, dtype=np.uint64)
    _refused("verify_prime_batch: one multiplier per proof", verify_prime_batch_host, b.pvk, xs, js, b.proofs, b.infs, rho=rho[:2])
    _refused("verify_prime_batch: one flag triple per proof", verify_prime_batch_host, b.pvk, xs, js, b.proofs, b.infs[:2], rho=rho)
    _refused("verify_prime_batch: one x and one j per proof", verify_prime_batch_host, b.pvk, xs[:2], js, b.proofs, b.infs, rho=rho)
    _refused("verify_prime_batch: one x and one j per proof", verify_prime_batch_host, b.pvk, xs, np.ones(K + 1, dtype=np.uint64), b.proofs, b.infs, rho=rho)


def test_verify_batch_u64_host_refuses_bad_shapes(sim, rho, no_library):
    from zksnark_finalproject_amd.device import verify_batch_u64_host
    b = sim.batch
    text = "verify_batch_u64: values is [k, num_instance - 1] for a key with at least two instance variables"
    _refused("verify_batch_u64: one multiplier per proof", verify_batch_u64_host, b.pvk, sim.values, b.proofs, b.infs, rho=rho[:2])
    _refused("verify_batch_u64: one flag triple per proof", verify_batch_u64_host, b.pvk, sim.values, b.proofs, b.infs[:2], rho=rho)
    for bad in (sim.values[:2], sim.values[:, :1], sim.values.reshape(-1), np.concatenate([sim.values, sim.values[:, :1]], axis=1)):
        _refused(text, verify_batch_u64_host, b.pvk, bad, b.proofs, b.infs, rho=rho)
    one = dict(b.pvk, gamma_abc_g1=np.asarray(b.pvk["gamma_abc_g1"], dtype=np.uint64).reshape(-1, 12)[:1])
    _refused(text, verify_batch_u64_host, one, np.zeros((K, 0), dtype=np.uint64), b.proofs, b.infs, rho=rho)


# ------------------------------------------------------------------------------------------------ the C entry points
def _key_arrays(pvk):
    u = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    return u(pvk["gamma_abc_g1"]).reshape(-1, 12), u(pvk["alpha_beta"]), u(pvk["gamma_neg_pc"]).reshape(-1, 36), u(pvk["delta_neg_pc"]).reshape(-1, 36)


def _refusals(entry, base, inputs, rho, extra):
    """every call of `extra` and the ones the three forms share return 1 with ok and ok_each as they were; base: the argument dict
    of a call that is not refused for its arguments, inputs: the names of the form's input pointers"""
    from zksnark_finalproject_amd import _lib
    fn = getattr(_lib.load(), entry)
    zero = rho.copy()
    zero[1] = 0
    shared = [dict(gabc=None), dict(ab=None), dict(g=None), dict(d=None), dict(proofs=None), dict(inf=None), dict(rho=None), dict(ok_null=True),
              dict(k=0), dict(nc=67), dict(rho=zero.ctypes.data), dict(threads=-1)] + [{name: None} for name in inputs]
    for kw in shared + extra:
        a = dict(base, threads=0)
        a.update(kw)
        ok = C.c_int(-7)
        each = np.full(K, 9, dtype=np.uint8)
        rc = fn(a["gabc"], a["ni"], a["ab"], a["g"], a["d"], a["nc"], *[a[name] for name in inputs], a["proofs"], a["inf"], a["rho"], a["k"], a["threads"],
                None if kw.get("ok_null") else C.byref(ok), each.ctypes.data)
        assert rc == 1 and ok.value == -7 and (each == 9).all(), (entry, kw)


def _base(sim, rho, gabc=None):
    b = sim.batch
    own, ab, g, d = _key_arrays(b.pvk)
    gabc = own if gabc is None else gabc
    keep = (gabc, ab, g, d)
    return dict(gabc=gabc.ctypes.data, ni=gabc.shape[0], ab=ab.ctypes.data, g=g.ctypes.data, d=d.ctypes.data, nc=g.shape[0], proofs=b.proofs.ctypes.data,
                inf=b.infs.ctypes.data, rho=rho.ctypes.data, k=K), keep


def test_verify_batch_host_bad_arguments(sim, rho):
    base, keep = _base(sim, rho)
    assert base["nc"] == 68
    _refusals("zkg16_verify_batch_host", dict(base, pub=sim.batch.pubs.ctypes.data), ("pub",), rho, [dict(ni=0)])


def test_verify_prime_batch_host_bad_arguments(sim, rho):
    # nothing below reaches the arithmetic: 260 points of any limbs do for the extended key
    base, keep = _base(sim, rho, gabc=np.ones((260, 12), dtype=np.uint64))
    xs, js = np.arange(K, dtype=np.uint64), np.ones(K, dtype=np.uint64)
    _refusals("zkg16_verify_prime_batch_host", dict(base, xs=xs.ctypes.data, js=js.ctypes.data), ("xs", "js"), rho,
              [dict(ni=258), dict(ni=259), dict(ni=261), dict(ni=3), dict(k=1 << 32)])


def test_verify_batch_u64_host_bad_arguments(sim, rho):
    base, keep = _base(sim, rho)
    _refusals("zkg16_verify_batch_u64_host", dict(base, values=sim.values.ctypes.data), ("values",), rho, [dict(ni=1), dict(ni=0), dict(k=1 << 32)])


# ------------------------------------------------------------------------------------------------ one statement set, two forms
def test_forms_agree_on_u64_statements(sim, rho):
    """the generic form on the expanded limbs and the u64 form on the values (the prime form takes keys of 260 points only)"""
    from zksnark_finalproject_amd.device import verify_batch_host, verify_batch_u64_host
    b = sim.batch
    assert list(sim.want) == [True, False, True] and np.array_equal(U.expand(sim.values), b.pubs)
    for threads in (0, 1):
        ok, each = verify_batch_host(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True, threads=threads)
        ok_u, each_u = verify_batch_u64_host(b.pvk, sim.values, b.proofs, b.infs, rho=rho, each=True, threads=threads)
        assert ok is False and ok_u is False and np.array_equal(each, sim.want) and np.array_equal(each_u, sim.want)
    good = np.flatnonzero(sim.want)
    assert verify_batch_host(b.pvk, b.pubs[good], b.proofs[good], b.infs[good], rho=rho[good]) is True
    assert verify_batch_u64_host(b.pvk, sim.values[good], b.proofs[good], b.infs[good], rho=rho[good]) is True
