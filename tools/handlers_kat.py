"""SHA-256 of the proof, vk and pvk strings the prove handlers return for fixed requests and seeds, as one JSON object: the known
answers of tests/golden/handlers_kat.json (tests/test_handlers_gpu.py).  Only the public handler API is used, so the tool runs on
any commit that has the handlers.
   python tools/handlers_kat.py > tests/golden/handlers_kat.json"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _sha(res):
    return {k: hashlib.sha256(res[k].encode()).hexdigest() for k in ("proof", "vk", "pvk") if k in res}


def digests(dev, handlers):
    ones = np.ones((3, 3), dtype=np.uint64)
    pairs = [(ones, 2 * ones), (np.arange(9, dtype=np.uint64).reshape(3, 3), ones)]
    many = handlers.prove_matrices(dev, 3, pairs, seed=9)
    return dict(
        prove_matrix=_sha(handlers.prove_matrix(dev, 3, ones, 2 * ones, seed=5)),
        prove_fibonacci=_sha(handlers.prove_fibonacci(dev, 0, 1, 20, seed=6)),
        prove_prime=_sha(handlers.prove_prime(dev, 12345, 32, seed=7)),
        prove_matrices=dict(_sha(many), requests=[_sha(q) for q in many["requests"]]),
        prove_primes=[_sha(q) for q in handlers.prove_primes(dev, [(12345, 32), (12346, 32)], seed=7)])


if __name__ == "__main__":
    from zksnark_finalproject_amd import Device, handlers
    dev = Device(0)
    print(json.dumps(digests(dev, handlers), indent=1, sort_keys=True))
    dev.close()
