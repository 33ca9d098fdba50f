"""The PrimeCircuit of candidate (x, j) built ON THE DEVICE (zkg16_r1cs_prime / zkg16_witness_prime, csrc/prime_device.hip): the same
bytes as the host synthesis (zkg16_circuit_prime + zkg16_circuit_export), the same key and proof, and prove_prime's request path
(device-built) equal to its host-synthesized path for the same seed."""
import threading

import numpy as np
import pytest

from test_prime_device_host import N_ZERO, candidates, resolve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def _check_handles(dev, x, j, rh, wh, full):
    got, nv = dev.r1cs_read(rh)
    assert nv == full.num_vars and got["num_inputs"] == full.num_instance and got["num_constraints"] == full.num_constraints
    for m in "abc":
        for g, w in zip(got[m], full.r1cs[m]):
            assert g.shape == w.shape and np.array_equal(g, w), (x, j, m)
    assert np.array_equal(dev.witness_read(wh, full.num_vars), full.z), (x, j)


@pytest.mark.parametrize("x,j", candidates())
def test_device_circuit_equals_synthesis(dev, x, j):
    from zksnark_finalproject_amd.circuits import prime_circuit
    x, j = resolve(x, j)
    full = prime_circuit(x, j, search=False, check_satisfied=False)
    rh, wh = dev.r1cs_prime(x, j), dev.witness_prime(x, j)
    try:
        _check_handles(dev, x, j, rh, wh, full)
    finally:
        dev.r1cs_free(rh)
        dev.witness_free(wh)


@pytest.mark.parametrize("x,j", N_ZERO)
def test_device_entries_refuse_what_the_builder_refuses(dev, x, j):
    from zksnark_finalproject_amd import Zkg16Error
    for fn in (dev.r1cs_prime, dev.witness_prime):
        with pytest.raises(Zkg16Error) as e:
            fn(x, j)
        assert e.value.status == 7


def test_resident_key_and_proof_equal_host_flow(dev):
    """setup_resident + prove_resident on the device-built handles == on the handles of the host synthesis (zkg16_circuit_load), same
    trapdoor, generators, r and s: byte-identical verifying key and proof."""
    import random
    from zksnark_finalproject_amd.circuits import prime_circuit_handle, prime_dims, prime_search
    from zksnark_finalproject_amd.device import scalar_mul
    from zksnark_finalproject_amd.handlers import _fr_mont
    from zksnark_finalproject_amd.workloads import R_MOD, g1_generator, g2_generator
    rng = random.Random(11)
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1, g2 = scalar_mul("g1", g1_generator(), k)[0], scalar_mul("g2", g2_generator(), k)[0]
    r, s = _fr_mont(rng.randrange(R_MOD)), _fr_mont(rng.randrange(R_MOD))
    x = 99
    j = prime_search(x, 32)["j"]
    ni = prime_dims(j)["num_instance"]
    out = []
    for source in ("host", "device"):
        if source == "host":
            h = prime_circuit_handle(x, j)
            assert h.num_instance == ni
            rh, wh = dev.circuit_load(h)
            h.close()
        else:
            rh, wh = dev.r1cs_prime(x, j), dev.witness_prime(x, j)
        ph, vk = dev.setup_resident(rh, ni, trap, g1, g2)
        proof, inf = dev.prove_resident(ph, rh, wh, r, s)
        out.append((vk, proof, inf))
        for f, hd in ((dev.pk_free, ph), (dev.witness_free, wh), (dev.r1cs_free, rh)):
            f(hd)
    (vk_h, p_h, i_h), (vk_d, p_d, i_d) = out
    assert np.array_equal(p_h, p_d) and np.array_equal(i_h, i_d)
    assert set(vk_h) == set(vk_d)
    for key in vk_h:
        assert np.array_equal(np.asarray(vk_h[key]), np.asarray(vk_d[key])), key


@pytest.mark.parametrize("x", [12345, 0x123456789ABCDEF])
def test_prove_prime_device_path_equals_host_path(dev, x):
    from zksnark_finalproject_amd import handlers
    res = handlers.prove_prime(dev, x, 32, seed=3)                           # request path: device-built circuit
    host = handlers.prove_prime(dev, x, 32, seed=3, check_satisfied=True)    # host synthesis (+ the satisfaction check)
    assert host["satisfied"] is True and res["satisfied"] is None
    for key in ("proof", "vk", "pvk", "j", "num_constraints", "num_variables", "prime_num", "found_prime"):
        assert res[key] == host[key], key
    assert np.array_equal(res["_circuit"].public_inputs, host["_circuit"].public_inputs)
    assert handlers.verify_prime(res["pvk"], x, res["j"], res["proof"])["valid"] is True
    assert handlers.verify_prime(res["pvk"], x + 1, res["j"], res["proof"])["valid"] is False


def test_two_threads_on_one_ctx():
    """Two threads build different candidates on ONE fresh ctx, starting together (both first calls race for the template upload)."""
    from zksnark_finalproject_amd import Device
    from zksnark_finalproject_amd.circuits import prime_circuit
    cases = [resolve(5, None), (7, 0)]
    want = {c: prime_circuit(*c, search=False, check_satisfied=False) for c in cases}
    d = Device(0)
    errors, go = [], threading.Barrier(len(cases))

    def run(c):
        try:
            go.wait()
            for _ in range(2):
                rh, wh = d.r1cs_prime(*c), d.witness_prime(*c)
                _check_handles(d, c[0], c[1], rh, wh, want[c])
                d.r1cs_free(rh)
                d.witness_free(wh)
        except Exception as e:      # noqa: BLE001 - reported on the main thread
            errors.append((c, e))
    try:
        ts = [threading.Thread(target=run, args=(c,)) for c in cases]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        d.close()
    assert not errors, errors
