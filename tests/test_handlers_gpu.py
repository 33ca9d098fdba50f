"""The prove handlers on the device: a seed gives the bytes recorded in tests/golden/handlers_kat.json (tools/handlers_kat.py,
run before the handlers were folded into one request path), and the real Device does what tests/test_handlers_host.py's fake
models: after the five handlers ran once each, the only handle still live is the cached shape's R1CS."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.close()


def _kat_tool():
    spec = importlib.util.spec_from_file_location("handlers_kat", os.path.join(ROOT, "tools", "handlers_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recording:
    """A Device behind a thin proxy: everything is delegated; which handles a call returned and which were freed is noted."""
    OBTAIN = {"r1cs_load": "r1cs", "r1cs_matrix": "r1cs", "r1cs_prime": "r1cs", "r1cs_prime_template": "r1cs", "witness_load": "witness",
              "witness_matrix": "witness", "witness_prime": "witness", "circuit_load": ("r1cs", "witness"), "pk_load": "pk", "setup_resident": "pk"}
    FREE = {"r1cs_free": "r1cs", "witness_free": "witness", "pk_free": "pk"}

    def __init__(self, dev):
        self._dev = dev
        self.live = set()

    def __getattr__(self, name):
        attr = getattr(self._dev, name)
        if name in self.OBTAIN:
            kinds = self.OBTAIN[name]

            def obtain(*args, **kwargs):
                out = attr(*args, **kwargs)
                if isinstance(kinds, tuple):        # circuit_load: (r1cs handle, witness handle)
                    self.live.update(zip(kinds, out))
                else:                               # the handle, or a tuple that begins with it
                    self.live.add((kinds, out[0] if isinstance(out, tuple) else out))
                return out
            return obtain
        if name in self.FREE:
            def free(h):
                self.live.remove((self.FREE[name], h))
                attr(h)
            return free
        return attr


def test_same_bytes_as_before_the_refactor(dev):
    from zksnark_finalproject_amd import handlers
    with open(os.path.join(ROOT, "tests", "golden", "handlers_kat.json")) as f:
        expected = json.load(f)
    assert _kat_tool().digests(dev, handlers) == expected


def test_only_the_cached_shape_stays_live(dev):
    from zksnark_finalproject_amd import handlers
    for n in list(dev._matrix_shapes):              # shapes the module's earlier requests cached are not this proxy's
        dev.r1cs_free(dev._matrix_shapes.pop(n).rh)
    rec = Recording(dev)
    ones = np.ones((3, 3), dtype=np.uint64)
    assert handlers.prove_matrix(rec, 3, ones, 2 * ones, seed=5)["proof"]
    assert handlers.prove_fibonacci(rec, 0, 1, 20, seed=6)["proof"]
    assert handlers.prove_prime(rec, 12345, 32, seed=7)["found_prime"]
    assert len(handlers.prove_matrices(rec, 3, [(ones, 2 * ones), (2 * ones, ones)], seed=9)["requests"]) == 2
    assert any(q["found_prime"] for q in handlers.prove_primes(rec, [(12345, 32), (12346, 32)], seed=7))
    assert rec.live == {("r1cs", dev._matrix_shapes[3].rh)}
