"""The request path of handlers.py on a fake Device (no GPU, only the library's host entry points): every device handle a
request obtains is released on every way out, the assignment thread never outlives its request, the draws from the PRNG keep their
order, the assignment of a cached shape still starts beside the setup, two first requests of one size make one R1CS, and the
verify handlers answer invalid for what cannot be decoded but raise for what is the service's trouble.  The batch handlers are pinned
on every path they have: their own key, a caller's key, check_on_device, the trapdoor route, and a refused trapdoor batch redone on
the key route."""
import base64
import random
import threading
import time

import numpy as np
import pytest

from helpers import fr_mont
from zksnark_finalproject_amd import Zkg16Error, device, handlers, wire
from zksnark_finalproject_amd._lib import ZKG16_ERR_UNSATISFIED
from zksnark_finalproject_amd.workloads import R_MOD, g1_generator, g2_generator

_G1, _G2 = g1_generator(), g2_generator()
_PROOF = np.concatenate([_G1, _G2, _G1]).astype(np.uint64)
_VKS = {}


def _mul(group, k):
    return device.scalar_mul(group, _G1 if group == "g1" else _G2, np.array([k, 0, 0, 0], dtype=np.uint64))[0]


def fake_vk(num_instance):
    """A verifying key of generator multiples: wire.encode_vk / encode_pvk take it."""
    if num_instance not in _VKS:
        _VKS[num_instance] = dict(alpha_g1=_mul("g1", 2), beta_g2=_mul("g2", 3), gamma_g2=_mul("g2", 5), delta_g2=_mul("g2", 7),
                                  gamma_abc_g1=np.stack([_mul("g1", 11 + i) for i in range(num_instance)]))
    return {k: v.copy() for k, v in _VKS[num_instance].items()}


class FakeDevice:
    """The Device methods the handlers call.  Hands out fresh handle numbers and keeps the set of live ones; records every call
    with its arguments; raises `exc` at the fail_at-th call since arm().  The *_free calls are recorded but neither counted nor
    failed: on the real Device they return nothing.  A free of a handle that is not live, or a proof on one, is an AssertionError.
    refuse_trapdoor: prove_trapdoor_batch answers as the library does for an unsatisfied assignment (Zkg16Error, status 8)."""

    def __init__(self, wait_for_assignment=False, r1cs_matrix_sleep=0.0, refuse_trapdoor=False):
        self.refuse_trapdoor = refuse_trapdoor
        self._matrix_shapes = {}
        self._matrix_shapes_lock = threading.Lock()
        self._mu = threading.Lock()
        self._next = 100
        self.live = {}                      # handle -> kind
        self.calls = []
        self.count, self.fail_at, self.exc = 0, None, None
        self.assigning = threading.Event() if wait_for_assignment else None
        self.r1cs_matrix_sleep = r1cs_matrix_sleep

    def arm(self, fail_at=None, exc=None):
        self.calls, self.count, self.fail_at, self.exc = [], 0, fail_at, exc
        if self.assigning is not None:
            self.assigning.clear()

    def names(self):
        return [name for name, _ in self.calls if not name.endswith("_free")]

    def _call(self, name, *args):
        with self._mu:
            i = self.count
            self.count += 1
            self.calls.append((name, args))
        if i == self.fail_at:
            raise self.exc

    def _new(self, kind):
        with self._mu:
            self._next += 1
            self.live[self._next] = kind
            return self._next

    def _free(self, name, kind, h):
        with self._mu:
            self.calls.append((name, (h,)))
            assert self.live.pop(h, None) == kind, "%s(%r): not a live %s handle" % (name, h, kind)

    def _is(self, kind, h):
        assert self.live.get(h) == kind, "%r is not a live %s handle" % (h, kind)

    # R1CS
    def r1cs_load(self, r1cs, num_variables):
        self._call("r1cs_load", r1cs, num_variables)
        return self._new("r1cs")

    def r1cs_matrix(self, n):
        self._call("r1cs_matrix", n)
        time.sleep(self.r1cs_matrix_sleep)
        return self._new("r1cs")

    def r1cs_fibonacci(self, steps):
        self._call("r1cs_fibonacci", steps)
        return self._new("r1cs")

    def r1cs_linear(self, n):
        self._call("r1cs_linear", n)
        return self._new("r1cs")

    def r1cs_prime(self, x, j):
        self._call("r1cs_prime", x, j)
        return self._new("r1cs")

    def r1cs_prime_template(self):
        self._call("r1cs_prime_template")
        return self._new("r1cs")

    def r1cs_free(self, h):
        self._free("r1cs_free", "r1cs", h)

    # assignments
    def witness_load(self, z):
        self._call("witness_load", z)
        return self._new("witness")

    def witness_matrix(self, a, b):
        if self.assigning is not None:
            self.assigning.set()
        self._call("witness_matrix", a, b)
        return self._new("witness"), np.zeros((3, 4), dtype=np.uint64), {}

    def witness_prime(self, x, j):
        self._call("witness_prime", x, j)
        return self._new("witness")

    def _witness_batch(self, name, args, side):
        """A failed call registers nothing, as the library's all-or-nothing entries."""
        self._call(name, *args)
        return np.array([self._new("witness") for _ in range(side.shape[0])], dtype=np.uint64), side, {}

    def witness_matrix_batch(self, a, b):
        return self._witness_batch("witness_matrix_batch", (a, b), np.zeros((a.shape[0], 3, 4), dtype=np.uint64))

    def witness_fibonacci_batch(self, steps, a, b):
        return self._witness_batch("witness_fibonacci_batch", (steps, a, b), np.zeros((a.shape[0], 3, 4), dtype=np.uint64))

    def witness_linear_batch(self, a, b, solver=None):
        return self._witness_batch("witness_linear_batch", (a, b), np.zeros(b.shape + (4,), dtype=np.uint64))

    def witness_free(self, h):
        self._free("witness_free", "witness", h)

    # satisfaction: every assignment satisfied
    def r1cs_check_batch(self, r1cs_h, witness_handles):
        self._call("r1cs_check_batch", r1cs_h, witness_handles)
        self._is("r1cs", r1cs_h)
        for wh in witness_handles:
            self._is("witness", int(wh))
        return [(0, 2 ** 64 - 1)] * len(witness_handles)

    def prime_check_batch(self, r1cs_h, xs, js):
        self._call("prime_check_batch", r1cs_h, xs, js)
        self._is("r1cs", r1cs_h)
        return [(0, 2 ** 64 - 1)] * len(xs)

    def circuit_load(self, circuit):
        self._call("circuit_load", circuit)
        return self._new("r1cs"), self._new("witness")

    # keys
    def setup(self, r1cs_h, num_instance, num_vars, domain, trap, g1, g2):
        self._call("setup", r1cs_h, num_instance, num_vars, domain, trap, g1, g2)
        self._is("r1cs", r1cs_h)
        return dict(host_key=True), fake_vk(num_instance)

    def setup_resident(self, r1cs_h, num_instance, trap, g1, g2):
        if self.assigning is not None:      # the assignment of a cached shape has started before the setup returns
            assert self.assigning.wait(5.0), "setup_resident: no witness_matrix beside it"
        self._call("setup_resident", r1cs_h, num_instance, trap, g1, g2)
        self._is("r1cs", r1cs_h)
        return self._new("pk"), fake_vk(num_instance)

    def pk_load(self, pk, num_instance):
        self._call("pk_load", pk, num_instance)
        return self._new("pk")

    def pk_free(self, h):
        self._free("pk_free", "pk", h)

    # proofs: (G1 generator, G2 generator, G1 generator)
    def prove_resident(self, pk_h, r1cs_h, wit_h, r, s):
        self._call("prove_resident", pk_h, r1cs_h, wit_h, r, s)
        self._is("pk", pk_h), self._is("r1cs", r1cs_h), self._is("witness", wit_h)
        return _PROOF.copy(), np.zeros(3, dtype=np.uint8)

    def prove_matrix_batch(self, pk_h, r1cs_h, a, b, rs, ss):
        self._call("prove_matrix_batch", pk_h, r1cs_h, a, b, rs, ss)
        self._is("pk", pk_h), self._is("r1cs", r1cs_h)
        k = a.shape[0]
        return np.tile(_PROOF, (k, 1)), np.zeros((k, 3), dtype=np.uint8), np.zeros((k, 3, 4), dtype=np.uint64), {}

    @staticmethod
    def _proofs(k):
        return np.tile(_PROOF, (k, 1)), np.zeros((k, 3), dtype=np.uint8)

    def prove_batch(self, pk_h, r1cs_h, witness_handles, rs, ss):
        self._call("prove_batch", pk_h, r1cs_h, witness_handles, rs, ss)
        self._is("pk", pk_h), self._is("r1cs", r1cs_h)
        for wh in witness_handles:
            self._is("witness", int(wh))
        return self._proofs(len(witness_handles))

    def prove_fibonacci_batch(self, pk_h, r1cs_h, steps, a, b, rs, ss):
        self._call("prove_fibonacci_batch", pk_h, r1cs_h, steps, a, b, rs, ss)
        self._is("pk", pk_h), self._is("r1cs", r1cs_h)
        return self._proofs(len(a)) + (np.zeros((len(a), 3, 4), dtype=np.uint64), {})

    def prove_linear_batch(self, pk_h, r1cs_h, a, b, rs, ss, solver=None):
        self._call("prove_linear_batch", pk_h, r1cs_h, a, b, rs, ss)
        self._is("pk", pk_h), self._is("r1cs", r1cs_h)
        return self._proofs(len(a)) + (np.zeros(b.shape + (4,), dtype=np.uint64), {})

    def prove_trapdoor_batch(self, r1cs_h, witness_handles, num_instance, trap, g1, g2, rs, ss):
        self._call("prove_trapdoor_batch", r1cs_h, witness_handles, num_instance, trap, g1, g2, rs, ss)
        self._is("r1cs", r1cs_h)
        for wh in witness_handles:
            self._is("witness", int(wh))
        if self.refuse_trapdoor:
            raise Zkg16Error(ZKG16_ERR_UNSATISFIED, "prove_trapdoor_batch: refused")
        return self._proofs(len(witness_handles)) + (fake_vk(num_instance),)

    def prove_prime_batch(self, pk_h, r1cs_h, corr, gamma_abc0, xs, js, rs, ss):
        self._call("prove_prime_batch", pk_h, r1cs_h, corr, gamma_abc0, xs, js, rs, ss)
        self._is("pk", pk_h), self._is("r1cs", r1cs_h)
        k = len(xs)
        return (np.tile(_PROOF, (k, 1)), np.zeros((k, 3), dtype=np.uint8), np.tile(_G1, (k, 1)), np.zeros((k, 257, 4), dtype=np.uint64), {})


class Boom(Exception):
    pass


_A2 = np.array([[1, 2], [3, 4]], dtype=np.uint64)
_B2 = np.array([[5, 6], [7, 8]], dtype=np.uint64)
_PAIRS = [(_A2, _B2), (_B2, _A2)]
_PRIMES = [(12345, 32), (12346, 32)]
_FIBS = [(0, 1), (2, 3)]
_SYSTEMS = [(np.array([[1, 0], [2, 3]], dtype=np.uint64), np.array([4, 5], dtype=np.uint64)),
            (np.array([[2, 0], [1, 1]], dtype=np.uint64), np.array([6, 7], dtype=np.uint64))]


def _matrices_key(dev):
    handlers.prove_matrices(dev, 2, _PAIRS)          # makes the cached shape
    return dev.setup_resident(dev._matrix_shapes[2].rh, 4, None, None, None)


def _warm(dev):
    handlers.prove_matrix(dev, 2, _B2, _A2)          # the first request of the size: later ones borrow its R1CS


def _primes_key(dev):
    return handlers.prime_template_key(dev, random.Random(1))


def _fibonaccis_key(dev):
    return handlers.fibonacci_key(dev, 3, random.Random(1))


def _linears_key(dev):
    return handlers.linear_key(dev, 2, random.Random(1))


# The batch handlers: name -> (the request with the path's keywords, what makes a caller's key, the R1CS call of a first request, the
# witness-batch call, the fused proving call).  Each is pinned on six paths (_BATCH_PATHS); "refused" in a name arms the fake's
# prove_trapdoor_batch to refuse.
_BATCH_HANDLERS = {
    "matrices": (lambda dev, **kw: handlers.prove_matrices(dev, 2, _PAIRS, seed=3, **kw), _matrices_key,
                 "r1cs_matrix", "witness_matrix_batch", "prove_matrix_batch"),
    "fibonaccis": (lambda dev, **kw: handlers.prove_fibonaccis(dev, _FIBS, 3, seed=3, **kw), _fibonaccis_key,
                   "r1cs_fibonacci", "witness_fibonacci_batch", "prove_fibonacci_batch"),
    "linears": (lambda dev, **kw: handlers.prove_linear_equations_batch(dev, _SYSTEMS, seed=3, **kw), _linears_key,
                "r1cs_linear", "witness_linear_batch", "prove_linear_batch"),
}
# path -> (the handler's keywords, the calls after the R1CS call as (r1cs, witness, fused) -> names)
_BATCH_PATHS = {
    "": (dict(), lambda r, w, f: [r, "setup_resident", f]),
    "_key": (dict(), lambda r, w, f: [f]),
    "_check": (dict(check_on_device=True), lambda r, w, f: [r, "setup_resident", w, "r1cs_check_batch", "prove_batch"]),
    "_trapdoor": (dict(route="trapdoor"), lambda r, w, f: [r, w, "prove_trapdoor_batch"]),
    "_trapdoor_refused": (dict(route="trapdoor"), lambda r, w, f: [r, w, "prove_trapdoor_batch", "setup_resident", f]),
    "_trapdoor_refused_check": (dict(route="trapdoor", check_on_device=True),
                                lambda r, w, f: [r, w, "prove_trapdoor_batch", "setup_resident", w, "r1cs_check_batch", "prove_batch"]),
}


def _batch_request(call, kw, with_key):
    return (lambda dev, key: call(dev, key=key, **kw)) if with_key else (lambda dev, key: call(dev, **kw))


# name -> (request(dev, key), what runs on dev before the request: it may return a key, which stays the caller's)
REQUESTS = {
    "matrix_first": (lambda dev, key: handlers.prove_matrix(dev, 2, _A2, _B2, seed=3), None),
    "matrix_cached": (lambda dev, key: handlers.prove_matrix(dev, 2, _A2, _B2, seed=3), _warm),
    "matrix_n1": (lambda dev, key: handlers.prove_matrix(dev, 1, [[3]], [[4]], seed=3), None),
    "matrix_keep_key": (lambda dev, key: handlers.prove_matrix(dev, 2, _A2, _B2, seed=3, keep_key=True), None),
    "fibonacci": (lambda dev, key: handlers.prove_fibonacci(dev, 0, 1, 3, seed=3), None),
    "fibonacci_keep_key": (lambda dev, key: handlers.prove_fibonacci(dev, 0, 1, 3, seed=3, keep_key=True), None),
    "prime": (lambda dev, key: handlers.prove_prime(dev, 12345, 32, seed=3), None),
    "primes": (lambda dev, key: handlers.prove_primes(dev, _PRIMES, seed=3), None),
    "primes_key": (lambda dev, key: handlers.prove_primes(dev, _PRIMES, seed=3, key=key), _primes_key),
    "primes_check": (lambda dev, key: handlers.prove_primes(dev, _PRIMES, seed=3, check_on_device=True), None),
}
EXPECTED_CALLS = {
    "matrix_first": ["r1cs_matrix", "witness_matrix", "setup_resident", "prove_resident"],
    "matrix_cached": ["witness_matrix", "setup_resident", "prove_resident"],
    "matrix_n1": ["r1cs_load", "witness_load", "setup_resident", "prove_resident"],
    "matrix_keep_key": ["r1cs_load", "witness_load", "setup", "pk_load", "prove_resident"],
    "fibonacci": ["circuit_load", "setup_resident", "prove_resident"],
    "fibonacci_keep_key": ["r1cs_load", "witness_load", "setup", "pk_load", "prove_resident"],
    "prime": ["r1cs_prime", "witness_prime", "setup_resident", "prove_resident"],
    "primes": ["r1cs_prime_template", "setup_resident", "prove_prime_batch"],
    "primes_key": ["prove_prime_batch"],
    "primes_check": ["r1cs_prime_template", "setup_resident", "prime_check_batch", "prove_prime_batch"],
}
for _h, (_call, _key, _r, _w, _f) in _BATCH_HANDLERS.items():
    for _p, (_kw, _calls) in _BATCH_PATHS.items():
        REQUESTS[_h + _p] = (_batch_request(_call, _kw, _p == "_key"), _key if _p == "_key" else None)
        EXPECTED_CALLS[_h + _p] = _calls(_r, _w, _f)
_PROVING_BATCH_CALLS = ("prove_matrix_batch", "prove_fibonacci_batch", "prove_linear_batch", "prove_prime_batch", "prove_batch", "prove_trapdoor_batch")


def _run(name, fail_at=None):
    """The request on a fresh fake -> (dev, handles that may stay live, what came out: the result or the exception)."""
    request, before = REQUESTS[name]
    dev = FakeDevice(wait_for_assignment=name in ("matrix_first", "matrix_cached"), refuse_trapdoor="refused" in name)
    key = before(dev) if before else None
    borrowed = set() if key is None else {key[0]} if isinstance(key, tuple) else {key["ph"], key["rh"]}
    exc = Boom(name)
    dev.arm(fail_at, exc)
    threads = threading.active_count()
    try:
        out = request(dev, key)
    except Boom as e:
        out = e
        assert e is exc
    assert threading.active_count() == threads
    assert set(dev.live) == borrowed | {s.rh for s in dev._matrix_shapes.values()}
    return dev, out


@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_handles_released_on_every_path(name):
    """A clean run, then the same request with a failure injected at each of its device calls in turn: the injected exception
    comes out, only the cached shape's rh and the caller's key stay live, and no thread is left."""
    dev, out = _run(name)
    assert isinstance(out, (dict, list))
    assert dev.names() == EXPECTED_CALLS[name]
    for i in range(len(EXPECTED_CALLS[name])):
        dev, out = _run(name, fail_at=i)
        assert isinstance(out, Boom), (name, i)
        # the setup still runs beside an assignment that failed on its thread; every other failure ends the request there
        ran = i + 1 if EXPECTED_CALLS[name][i] != "witness_matrix" else i + 2
        assert dev.names() == EXPECTED_CALLS[name][:ran], (name, i)


def test_thread_result_released_when_the_setup_fails():
    """The assignment a cached shape's request obtained on its thread is released when the setup beside it raised."""
    dev, out = _run("matrix_cached", fail_at=1)
    assert isinstance(out, Boom) and dev.names() == ["witness_matrix", "setup_resident"]
    freed = [args[0] for name, args in dev.calls if name == "witness_free"]
    assert len(freed) == 1 and "witness" not in dev.live.values()


def _expected_draws(seed, proofs):
    """The order of draws restated: 5 x randrange(1, R_MOD) for the trapdoor, 4 x getrandbits(62) for the generator scalar, then
    per proof randrange(R_MOD) for r and for s."""
    rng = random.Random(seed)
    trap = np.stack([fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    rs = [(fr_mont(rng.randrange(R_MOD)), fr_mont(rng.randrange(R_MOD))) for _ in range(proofs)]
    return trap, device.scalar_mul("g1", _G1, k)[0], device.scalar_mul("g2", _G2, k)[0], rs


@pytest.mark.parametrize("name", sorted(n for n in REQUESTS if not n.endswith("_key") or n.endswith("keep_key")))
def test_draw_order(name):
    dev, out = _run(name)
    calls = dict(dev.calls)
    batches = [args for call, args in dev.calls if call in _PROVING_BATCH_CALLS]
    proofs = len(batches[0][-1]) if batches else 1
    trap, g1, g2, rs = _expected_draws(3, proofs)
    # the key's draws reach the setup, or the trapdoor call in front of r and s; a refused trapdoor batch shows them to both
    keyed = [args[-3:] for call, args in dev.calls if call in ("setup", "setup_resident")]
    keyed += [args[-5:-2] for call, args in dev.calls if call == "prove_trapdoor_batch"]
    assert len(keyed) == (2 if "refused" in name else 1)
    for got in keyed:
        assert np.array_equal(got[0], trap) and np.array_equal(got[1], g1) and np.array_equal(got[2], g2)
    if batches:
        assert len(batches) == (2 if "refused" in name else 1)
        assert proofs == (sum(1 for q in out if q["found_prime"]) if name.startswith("primes") else 2)
        for batch in batches:
            assert np.array_equal(batch[-2], np.stack([r for r, _ in rs])) and np.array_equal(batch[-1], np.stack([s for _, s in rs]))
    else:
        assert np.array_equal(calls["prove_resident"][-2], rs[0][0]) and np.array_equal(calls["prove_resident"][-1], rs[0][1])
        assert np.array_equal(out["_detail"]["r"], rs[0][0]) and np.array_equal(out["_detail"]["s"], rs[0][1])


@pytest.mark.parametrize("name", ["matrices_key", "fibonaccis_key", "linears_key", "primes_key"])
def test_draw_order_with_a_callers_key(name):
    """key=: no trapdoor is drawn, the first draws are r and s of the first proof."""
    dev, out = _run(name)
    (batch,) = [args for call, args in dev.calls if call in _PROVING_BATCH_CALLS]
    rng = random.Random(3)
    rs = [(fr_mont(rng.randrange(R_MOD)), fr_mont(rng.randrange(R_MOD))) for _ in range(len(batch[-1]))]
    assert np.array_equal(batch[-2], np.stack([r for r, _ in rs])) and np.array_equal(batch[-1], np.stack([s for _, s in rs]))


def test_circuit_record_and_response_fields():
    """What a request returns under "_circuit" keeps its attributes on every path; host-synthesized ones also carry r1cs and z."""
    for name in ("matrix_first", "matrix_cached", "matrix_n1", "matrix_keep_key", "fibonacci", "fibonacci_keep_key", "prime"):
        _, out = _run(name)
        circ = out["_circuit"]
        for attr in ("public_inputs", "num_constraints", "num_instance", "num_witness", "num_vars", "domain", "satisfied"):
            assert hasattr(circ, attr), (name, attr)
        assert circ.num_vars == circ.num_instance + circ.num_witness
        assert circ.domain == 1 << (circ.num_constraints + circ.num_instance - 1).bit_length()
        assert len(circ.public_inputs) == circ.num_instance - 1
        if name in ("matrix_n1", "matrix_keep_key", "fibonacci_keep_key"):
            assert circ.r1cs is not None and circ.z is not None
        assert (out["_detail"]["pk"] is not None) == name.endswith("keep_key")
    _, out = _run("matrix_cached")
    assert out["num_constraints"] == out["num_constraints_circuit"] + 2 * 2 ** 3 and out["num_variables"] == 4


_BATCH_RECORD_FIELDS = {       # handler -> (a request's record, its "_detail"); prove_matrices: (the response, a request, "_detail")
    "matrices": ({"vk", "pvk", "setup_time", "proving_time", "num_constraints_circuit", "num_variables", "requests", "_detail"},
                 {"hash_a", "hash_b", "hash_c", "proof"}, {"proofs", "inf", "public_inputs", "vk", "rs", "ss", "ms", "route"}),
    "fibonaccis": ({"proof", "proving_time", "setup_time", "num_constraints", "num_variables", "fib_number", "pvk", "vk", "_circuit", "_detail"},
                   {"proof", "inf", "vk", "r", "s", "public_inputs", "ms", "route"}),
    "linears": ({"proof", "public_input", "num_constraints", "num_variables", "proving_time", "verifying_time", "valid", "pvk", "vk", "_circuit",
                 "_detail"}, {"proof", "inf", "vk", "r", "s", "public_inputs", "x", "ms", "setup_time", "route"}),
    "primes": ({"proof", "j", "num_constraints", "num_variables", "setup_time", "proving_time", "found_prime", "prime_num", "pvk", "vk",
                "satisfied", "_detail"}, {"proof", "inf", "vk", "r", "s", "public_inputs", "ms"}),
}


@pytest.mark.parametrize("name", sorted(n for n in REQUESTS if n.split("_")[0] in _BATCH_RECORD_FIELDS))
def test_batch_record_fields(name):
    """The fields of a batch handler's records, keys only, on every path: "satisfied" joins a record only with check_on_device (a
    prime record always has it); "route" names the route that answered; setup_time is 0.0 with a caller's key and when the trapdoor
    route answered."""
    handler = name.split("_")[0]
    _, out = _run(name)
    checked = {"satisfied"} if name.endswith("_check") else set()
    if handler == "matrices":
        top, request, detail = _BATCH_RECORD_FIELDS[handler]
        assert set(out) == top and set(out["_detail"]) == detail and len(out["requests"]) == 2
        assert all(set(q) == request | checked for q in out["requests"])
        details, setup_times = [out["_detail"]], [out["setup_time"]]
    else:
        record, detail = _BATCH_RECORD_FIELDS[handler]
        assert len(out) == 2 and all(set(q) == record | checked and set(q["_detail"]) == detail for q in out)
        details = [q["_detail"] for q in out]
        setup_times = [q["_detail"]["setup_time"] if handler == "linears" else q["setup_time"] for q in out]
    answered = "trapdoor" if name.endswith("_trapdoor") else "key"
    assert handler == "primes" or all(d["route"] == answered for d in details)
    if name.endswith("_key") or answered == "trapdoor":
        assert setup_times == [0.0] * len(setup_times)
    else:
        assert all(t > 0.0 for t in setup_times)


@pytest.mark.parametrize("name", sorted(_BATCH_HANDLERS))
def test_trapdoor_route_takes_no_key(name):
    """route="trapdoor" draws its own key: with key= the handler raises before any device call."""
    call, make_key = _BATCH_HANDLERS[name][:2]
    dev = FakeDevice()
    key = make_key(dev)
    dev.arm()
    with pytest.raises(ValueError):
        call(dev, key=key, route="trapdoor")
    assert dev.calls == []


def test_two_first_requests_make_one_r1cs():
    dev = FakeDevice(r1cs_matrix_sleep=0.05)
    errors = []

    def request(seed):
        try:
            handlers.prove_matrix(dev, 2, _A2, _B2, seed=seed)
        except Exception as e:      # noqa: BLE001 - reported below
            errors.append(e)
    threads = [threading.Thread(target=request, args=(seed,)) for seed in (1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert dev.names().count("r1cs_matrix") == 1
    assert dev.live == {dev._matrix_shapes[2].rh: "r1cs"}


# ---- the verify handlers' error mapping
def _raiser(status):
    def fn(*args, **kwargs):
        raise Zkg16Error(status, "injected")
    return fn


@pytest.fixture(scope="module")
def signed():
    vk = fake_vk(2)
    return dict(vk=vk, pvk=device.pvk_prepare(vk), pub=np.stack([fr_mont(9)]), proof=wire.encode_proof(_PROOF, np.zeros(3, dtype=np.uint8)))


@pytest.mark.parametrize("key,entry", [("vk", "verify"), ("pvk", "verify_prepared")])
def test_verify_proof_error_mapping(monkeypatch, signed, key, entry):
    assert handlers.verify_proof(signed[key], signed["pub"], signed["proof"])["valid"] is False      # decodes; not a proof of anything
    monkeypatch.setattr(device, entry, _raiser(1))          # ZKG16_ERR_BAD_ARG: a malformed key or input list
    assert handlers.verify_proof(signed[key], signed["pub"], signed["proof"])["valid"] is False
    monkeypatch.setattr(device, entry, _raiser(4))          # ZKG16_ERR_OOM: not the proof's fault
    with pytest.raises(Zkg16Error) as e:
        handlers.verify_proof(signed[key], signed["pub"], signed["proof"])
    assert e.value.status == 4
    # what does not decode is answered before the verifier is reached
    assert handlers.verify_proof(signed[key], signed["pub"], signed["proof"][:-6])["valid"] is False
    assert handlers.verify_proof(signed[key], signed["pub"], "not base64!")["valid"] is False


def test_verify_proofs_error_mapping(monkeypatch, signed):
    pubs, proofs = [signed["pub"]] * 3, [signed["proof"], signed["proof"][:-6], signed["proof"]]
    assert handlers.verify_proofs(signed["vk"], pubs, proofs)["valid"] == [False, False, False]
    monkeypatch.setattr(device, "pvk_prepare", _raiser(1))
    assert handlers.verify_proofs(signed["vk"], pubs, proofs)["valid"] == [False, False, False]
    monkeypatch.setattr(device, "pvk_prepare", _raiser(4))
    with pytest.raises(Zkg16Error) as e:
        handlers.verify_proofs(signed["vk"], pubs, proofs)
    assert e.value.status == 4
    # an already prepared key needs no pvk_prepare; a truncated proof is invalid for its entry, a truncated key for all
    assert handlers.verify_proofs(signed["pvk"], pubs, proofs)["valid"] == [False, False, False]
    short_key = base64.standard_b64encode(wire.vk_serialize_compressed(signed["vk"])[:-5]).decode()
    assert handlers.verify_proofs(short_key, pubs, proofs)["valid"] == [False, False, False]


def test_deleting_the_shape_cache_starts_an_empty_one():
    """Callers reset the cache of a Device by deleting the attribute (dev.__dict__.pop("_matrix_shapes")): the next look finds
    an empty dict that stays, not an AttributeError.  No ctx is needed for that."""
    dev = device.Device.__new__(device.Device)
    dev._matrix_shapes = {2: "shape"}
    dev.__dict__.pop("_matrix_shapes", None)
    assert dev._matrix_shapes == {} and dev._matrix_shapes is dev.__dict__["_matrix_shapes"]
    with pytest.raises(AttributeError):
        dev.no_such_attribute
