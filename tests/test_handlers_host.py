"""The request path of handlers.py on a fake Device (no GPU, only the library's host entry points): every device handle a
request obtains is released on every way out, the assignment thread never outlives its request, the draws from the PRNG keep their
order, the assignment of a cached shape still starts beside the setup, two first requests of one size make one R1CS, and the
verify handlers answer invalid for what cannot be decoded but raise for what is the service's trouble."""
import base64
import random
import threading
import time

import numpy as np
import pytest

from helpers import fr_mont
from zksnark_finalproject_amd import Zkg16Error, device, handlers, wire
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
    failed: on the real Device they return nothing.  A free of a handle that is not live, or a proof on one, is an AssertionError."""

    def __init__(self, wait_for_assignment=False, r1cs_matrix_sleep=0.0):
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

    def witness_free(self, h):
        self._free("witness_free", "witness", h)

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


def _matrices_key(dev):
    handlers.prove_matrices(dev, 2, _PAIRS)          # makes the cached shape
    return dev.setup_resident(dev._matrix_shapes[2].rh, 4, None, None, None)


def _warm(dev):
    handlers.prove_matrix(dev, 2, _B2, _A2)          # the first request of the size: later ones borrow its R1CS


def _primes_key(dev):
    return handlers.prime_template_key(dev, random.Random(1))


# name -> (request(dev, key), what runs on dev before the request: it may return a key, which stays the caller's)
REQUESTS = {
    "matrix_first": (lambda dev, key: handlers.prove_matrix(dev, 2, _A2, _B2, seed=3), None),
    "matrix_cached": (lambda dev, key: handlers.prove_matrix(dev, 2, _A2, _B2, seed=3), _warm),
    "matrix_n1": (lambda dev, key: handlers.prove_matrix(dev, 1, [[3]], [[4]], seed=3), None),
    "matrix_keep_key": (lambda dev, key: handlers.prove_matrix(dev, 2, _A2, _B2, seed=3, keep_key=True), None),
    "fibonacci": (lambda dev, key: handlers.prove_fibonacci(dev, 0, 1, 3, seed=3), None),
    "fibonacci_keep_key": (lambda dev, key: handlers.prove_fibonacci(dev, 0, 1, 3, seed=3, keep_key=True), None),
    "prime": (lambda dev, key: handlers.prove_prime(dev, 12345, 32, seed=3), None),
    "matrices": (lambda dev, key: handlers.prove_matrices(dev, 2, _PAIRS, seed=3), None),
    "matrices_key": (lambda dev, key: handlers.prove_matrices(dev, 2, _PAIRS, seed=3, key=key), _matrices_key),
    "primes": (lambda dev, key: handlers.prove_primes(dev, _PRIMES, seed=3), None),
    "primes_key": (lambda dev, key: handlers.prove_primes(dev, _PRIMES, seed=3, key=key), _primes_key),
}
EXPECTED_CALLS = {
    "matrix_first": ["r1cs_matrix", "witness_matrix", "setup_resident", "prove_resident"],
    "matrix_cached": ["witness_matrix", "setup_resident", "prove_resident"],
    "matrix_n1": ["r1cs_load", "witness_load", "setup_resident", "prove_resident"],
    "matrix_keep_key": ["r1cs_load", "witness_load", "setup", "pk_load", "prove_resident"],
    "fibonacci": ["circuit_load", "setup_resident", "prove_resident"],
    "fibonacci_keep_key": ["r1cs_load", "witness_load", "setup", "pk_load", "prove_resident"],
    "prime": ["r1cs_prime", "witness_prime", "setup_resident", "prove_resident"],
    "matrices": ["r1cs_matrix", "setup_resident", "prove_matrix_batch"],
    "matrices_key": ["prove_matrix_batch"],
    "primes": ["r1cs_prime_template", "setup_resident", "prove_prime_batch"],
    "primes_key": ["prove_prime_batch"],
}


def _run(name, fail_at=None):
    """The request on a fresh fake -> (dev, handles that may stay live, what came out: the result or the exception)."""
    request, before = REQUESTS[name]
    dev = FakeDevice(wait_for_assignment=name in ("matrix_first", "matrix_cached"))
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
    batch = calls.get("prove_matrix_batch") or calls.get("prove_prime_batch")
    proofs = len(batch[-1]) if batch else 1
    trap, g1, g2, rs = _expected_draws(3, proofs)
    setup = calls.get("setup") or calls.get("setup_resident")
    assert np.array_equal(setup[-3], trap) and np.array_equal(setup[-2], g1) and np.array_equal(setup[-1], g2)
    if batch:
        assert proofs == (2 if name == "matrices" else sum(1 for q in out if q["found_prime"]))
        assert np.array_equal(batch[-2], np.stack([r for r, _ in rs])) and np.array_equal(batch[-1], np.stack([s for _, s in rs]))
    else:
        assert np.array_equal(calls["prove_resident"][-2], rs[0][0]) and np.array_equal(calls["prove_resident"][-1], rs[0][1])
        assert np.array_equal(out["_detail"]["r"], rs[0][0]) and np.array_equal(out["_detail"]["s"], rs[0][1])


@pytest.mark.parametrize("name", ["matrices_key", "primes_key"])
def test_draw_order_with_a_callers_key(name):
    """key=: no trapdoor is drawn, the first draws are r and s of the first proof."""
    dev, out = _run(name)
    batch = dict(dev.calls).get("prove_matrix_batch") or dict(dev.calls).get("prove_prime_batch")
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
