"""In-process mirrors of the reference's request handlers around the hot path (the callers of `Groth16::prove`):
    prove_matrix     src/arkworks/backend/matrix_proof.rs:94-166   (POST /api/matrix_prove/prove)
    prove_matrices   K such requests of one size under one key, in batched device passes (no counterpart upstream)
    prove_fibonacci  src/arkworks/backend/fibbonaci_handler.rs:98-145
    prove_prime / verify_prime  src/arkworks/backend/prime_snark.rs:49-146, 165-206
    prove_primes     K prime requests under one trapdoor on ONE template key, in batched device passes (no counterpart upstream)
Same steps, same response fields: synthesize the circuit (host C++ mirror), per-request Groth16 setup (on the device,
zkg16_setup), prove (zkg16_prove_resident), encode (wire.py).  The reference's HTTP layer (actix-web) is out of scope; the
trapdoor and r, s come from Python's PRNG rather than arkworks' StdRng stream, so proofs are valid Groth16 proofs for the
same statement but not the byte string the Rust server would emit for its seed."""
import random
import time

import numpy as np

from . import wire
from .circuits import (fibonacci_circuit, fibonacci_circuit_handle, matrix_circuit, matrix_hash_batch_host, prime_circuit, prime_dims, prime_key_corrections,
                       prime_public_inputs, prime_search)
from .workloads import R_MOD, g1_generator, g2_generator


def _fr_mont(x):
    v = (x << 256) % R_MOD
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


class _CachedShape:
    """What a request needs of a MatrixCircuit whose matrices are already on the device: the matrices depend on the size
    alone, so they are synthesized, exported and uploaded once per size and ctx; a request then only computes its assignment
    (zkg16_circuit_matrix_witness)."""

    def __init__(self, circ, rh):
        self.rh = rh
        self.num_instance, self.num_witness, self.num_vars = circ.num_instance, circ.num_witness, circ.num_vars
        self.num_constraints, self.domain = circ.num_constraints, circ.domain

    @classmethod
    def on_device(cls, dev, n):
        """The shape with its matrices written ON THE DEVICE (zkg16_r1cs_matrix): nothing of the circuit is synthesized on the host."""
        import ctypes as C
        from . import _lib
        nc, nw = C.c_size_t(), C.c_size_t()
        rc = _lib.load().zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), None)
        if rc:
            raise _lib.Zkg16Error(rc, "zkg16_matrix_r1cs_dims")
        self = cls.__new__(cls)
        self.rh = dev.r1cs_matrix(n)
        self.num_instance, self.num_witness, self.num_vars = 4, nw.value, 4 + nw.value
        self.num_constraints = nc.value
        self.domain = 1 << max(nc.value + 4 - 1, 0).bit_length()
        return self

    def instantiate(self, a, b):
        """The request's circuit without a host assignment: z is built on the device inside the proof (zkg16_prove_matrix)."""
        inst = _CachedShape.__new__(_CachedShape)
        inst.__dict__.update(self.__dict__)
        inst.z = None
        inst.matrices = (a, b)
        inst.public_inputs = None           # hash_a, hash_b, hash_c come back from the proof call
        inst.r1cs = None
        return inst


def _setup_and_prove(dev, circ, rng, keep_key=False):
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    # arkworks draws random generators; any subgroup generator gives a valid key: [k]G for random k
    from .device import scalar_mul
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1 = scalar_mul("g1", g1_generator(), k)[0]
    g2 = scalar_mul("g2", g2_generator(), k)[0]
    cached = getattr(circ, "rh", None) is not None
    direct = getattr(circ, "handle", None) is not None          # a CircuitHandle: matrices and assignment go to the device unexported
    wh_direct = None
    if direct:
        rh, wh_direct = dev.circuit_load(circ)
        circ.close()
    else:
        rh = circ.rh if cached else dev.r1cs_load(circ.r1cs, circ.num_vars)
    # cached shape: the assignment needs neither the key nor (for its host half, the three Poseidon chains) the device, so it is
    # started now and runs beside the setup's kernels (zkg16_witness_matrix takes the ctx only for its ~1 ms of kernels): at 128x128
    # the 61 ms of chains disappear under the 0.2 s setup and the proof is the plain resident one (0.17 s instead of 0.195 s streamed)
    early = None
    if circ.z is None and not keep_key and not direct:
        import threading
        early = {}

        def _assign():
            try:
                early["out"] = dev.witness_matrix(circ.matrices[0], circ.matrices[1])
            except Exception as e:      # noqa: BLE001 - re-raised on the caller's thread
                early["err"] = e
        early["thread"] = threading.Thread(target=_assign)
        early["thread"].start()
    t0 = time.perf_counter()
    try:
        if keep_key:        # tests want the key on the host as well
            pk, vk = dev.setup(rh, circ.num_instance, circ.num_vars, circ.domain, trap, g1, g2)
            ph = dev.pk_load(pk, circ.num_instance)
        else:               # the request path: the key never leaves the device
            pk = None
            ph, vk = dev.setup_resident(rh, circ.num_instance, trap, g1, g2)
    except Exception:
        if early is not None:           # the assignment thread must not outlive the request
            early["thread"].join()
            if "out" in early:
                dev.witness_free(early["out"][0])
        raise
    setup_time = time.perf_counter() - t0
    r, s = _fr_mont(rng.randrange(R_MOD)), _fr_mont(rng.randrange(R_MOD))
    if early is not None:               # cached shape, assignment started before the setup
        t0 = time.perf_counter()
        early["thread"].join()
        if "err" in early:
            dev.pk_free(ph)
            raise early["err"]
        wh, pub, _ = early["out"]
        proof, inf = dev.prove_resident(ph, rh, wh, r, s)
        proving_time = time.perf_counter() - t0
        circ.public_inputs = pub
    elif circ.z is None and not direct:  # cached shape: the assignment is produced on the device while the proof runs
        t0 = time.perf_counter()
        proof, inf, pub, _ = dev.prove_matrix(ph, rh, circ.matrices[0], circ.matrices[1], r, s)
        proving_time = time.perf_counter() - t0
        circ.public_inputs = pub
        wh = None
    else:
        wh = wh_direct if direct else dev.witness_load(circ.z)
        t0 = time.perf_counter()
        proof, inf = dev.prove_resident(ph, rh, wh, r, s)
        proving_time = time.perf_counter() - t0
    for f, h in ((dev.pk_free, ph),) + (((dev.witness_free, wh),) if wh is not None else ()) + (() if cached else ((dev.r1cs_free, rh),)):
        f(h)
    return dict(proof=proof, inf=inf, vk=vk, pk=pk, setup_time=setup_time, proving_time=proving_time, r=r, s=s)


class _PrimeShape:
    """What a prime request needs of a PrimeCircuit whose matrices and assignment are built on the device (zkg16_r1cs_prime /
    zkg16_witness_prime): its dimensions and public inputs, nothing synthesized on the host."""

    def __init__(self, x, j):
        dims = prime_dims(j)
        self.num_instance, self.num_witness, self.num_constraints = dims["num_instance"], dims["num_witness"], dims["num_constraints"]
        self.num_vars = self.num_instance + self.num_witness
        self.domain = 1 << max(self.num_constraints + self.num_instance - 1, 0).bit_length()
        self.public_inputs = prime_public_inputs(x, j)
        self.satisfied = None
        self.z = self.r1cs = None
        self.j = j


def _setup_and_prove_prime_device(dev, x, j, circ, rng):
    """_setup_and_prove for the prime request path: R1CS and assignment written on the device for candidate (x, j), resident key.
    The same draws from rng in the same order, so a seed gives the same key and proof as the host-synthesized path."""
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    from .device import scalar_mul
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1 = scalar_mul("g1", g1_generator(), k)[0]
    g2 = scalar_mul("g2", g2_generator(), k)[0]
    rh = wh = ph = None
    try:
        rh = dev.r1cs_prime(x, j)
        wh = dev.witness_prime(x, j)
        t0 = time.perf_counter()
        ph, vk = dev.setup_resident(rh, circ.num_instance, trap, g1, g2)
        setup_time = time.perf_counter() - t0
        r, s = _fr_mont(rng.randrange(R_MOD)), _fr_mont(rng.randrange(R_MOD))
        t0 = time.perf_counter()
        proof, inf = dev.prove_resident(ph, rh, wh, r, s)
        proving_time = time.perf_counter() - t0
    finally:
        for f, h in ((dev.pk_free, ph), (dev.witness_free, wh), (dev.r1cs_free, rh)):
            if h is not None:
                f(h)
    return dict(proof=proof, inf=inf, vk=vk, pk=None, setup_time=setup_time, proving_time=proving_time, r=r, s=s)


def hash_matrix(size, matrix):
    """The reference's hash_matrix endpoint (matrix_proof.rs:44-71) -> its OutputData: {"hash": the 32 little-endian bytes of the
    canonical value}.  This is where a client obtains the hashes that become a proof's public inputs.  Host only."""
    return hash_matrices(size, [matrix])[0]


def hash_matrices(size, matrices, dev=None):
    """hash_matrix for K requests of one size in one call -> K OutputData dicts.  With dev the batch goes through
    Device.matrix_hash_batch (a kernel from option "sponge_chains_min" matrices on), else through host threads."""
    if len(matrices) == 0:
        raise ValueError("hash_matrices: no requests")
    m = np.stack([np.asarray(x, dtype=np.uint64).reshape(size, size) for x in matrices])
    hashes = dev.matrix_hash_batch(m) if dev is not None else matrix_hash_batch_host(m)
    return [dict(hash=list(wire.hash_bytes(h))) for h in hashes]   # OutputData.hash: a Vec<u8> (matrix_proof.rs:66-70)


def prove_matrix(dev, size, matrix_a, matrix_b, seed=0, keep_key=False):
    """-> the reference's ProveOutput fields (matrix_proof.rs:80-91)."""
    a = np.asarray(matrix_a, dtype=np.uint64).reshape(size, size)
    b = np.asarray(matrix_b, dtype=np.uint64).reshape(size, size)
    shapes = dev.__dict__.setdefault("_matrix_shapes", {})
    if keep_key or size < 2:            # tests want the host copy of everything
        circ = matrix_circuit(a, b)
    elif size in shapes:
        circ = shapes[size].instantiate(a, b)
    else:
        shapes[size] = _CachedShape.on_device(dev, size)           # first request of this size: matrices written by kernels
        circ = shapes[size].instantiate(a, b)
    out = _setup_and_prove(dev, circ, random.Random(seed), keep_key)
    ha, hb, hc = circ.public_inputs
    return dict(hash_a=wire.encode_hash(ha), hash_b=wire.encode_hash(hb), hash_c=wire.encode_hash(hc),
                setup_time=out["setup_time"], proving_time=out["proving_time"],
                # the reference counts matrix_mul twice (outer cs + circuit: matrix_proof.rs:108,150,160)
                num_constraints=circ.num_constraints + 2 * size ** 3, num_constraints_circuit=circ.num_constraints,
                num_variables=circ.num_instance, proof=wire.encode_proof(out["proof"], out["inf"]),
                # the reference returns the prepared key (encode_pvk, io.rs:62-68); the plain key is kept beside it
                pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]), _detail=out, _circuit=circ)


def prove_matrices(dev, size, pairs, seed=0, key=None):
    """K requests of one size under ONE key, assignments and proofs in batched device passes (Device.prove_matrix_batch).  pairs: K
    (matrix_a, matrix_b).  The key is set up once on the device from `seed` (the draws of prove_matrix, then r, s per request, so
    request 0 is prove_matrix's proof for that seed), or passed in as key=(pk handle, vk dict), which stays the caller's.  The
    matrices come from the shape cache.  -> the shared vk / pvk and, per request, prove_matrix's hash_a / hash_b / hash_c / proof."""
    k = len(pairs)
    if k == 0:
        raise ValueError("prove_matrices: no requests")
    a = np.stack([np.asarray(p[0], dtype=np.uint64).reshape(size, size) for p in pairs])
    b = np.stack([np.asarray(p[1], dtype=np.uint64).reshape(size, size) for p in pairs])
    shapes = dev.__dict__.setdefault("_matrix_shapes", {})
    if size not in shapes:
        shapes[size] = _CachedShape.on_device(dev, size)
    shape = shapes[size]
    rng = random.Random(seed)
    made = []
    try:
        setup_time = 0.0
        if key is None:
            from .device import scalar_mul
            trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
            kk = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
            g1 = scalar_mul("g1", g1_generator(), kk)[0]
            g2 = scalar_mul("g2", g2_generator(), kk)[0]
            t0 = time.perf_counter()
            ph, vk = dev.setup_resident(shape.rh, shape.num_instance, trap, g1, g2)
            made.append(ph)
            setup_time = time.perf_counter() - t0
        else:
            ph, vk = key
        rss = [(_fr_mont(rng.randrange(R_MOD)), _fr_mont(rng.randrange(R_MOD))) for _ in range(k)]
        rs, ss = np.stack([r for r, _ in rss]), np.stack([s for _, s in rss])
        t0 = time.perf_counter()
        proofs, inf, pubs, ms = dev.prove_matrix_batch(ph, shape.rh, a, b, rs, ss)
        proving_time = time.perf_counter() - t0
    finally:
        for h in made:
            dev.pk_free(h)
    requests = [dict(hash_a=wire.encode_hash(pubs[i][0]), hash_b=wire.encode_hash(pubs[i][1]), hash_c=wire.encode_hash(pubs[i][2]),
                     proof=wire.encode_proof(proofs[i], inf[i])) for i in range(k)]
    return dict(vk=wire.encode_vk(vk), pvk=wire.encode_pvk(vk), setup_time=setup_time, proving_time=proving_time,
                num_constraints_circuit=shape.num_constraints, num_variables=shape.num_instance, requests=requests,
                _detail=dict(proofs=proofs, inf=inf, public_inputs=pubs, vk=vk, rs=rs, ss=ss, ms=ms))


def prove_fibonacci(dev, a, b, num_of_rounds, seed=42, keep_key=False):
    """-> the reference's OutputDataFib-like fields (fibbonaci_handler.rs:84-90)."""
    circ = fibonacci_circuit(a, b, num_of_rounds) if keep_key else fibonacci_circuit_handle(a, b, num_of_rounds)
    out = _setup_and_prove(dev, circ, random.Random(seed), keep_key)
    return dict(proof=wire.encode_proof(out["proof"], out["inf"]), proving_time=out["proving_time"], setup_time=out["setup_time"],
                num_constraints=circ.num_constraints, num_variables=circ.num_instance,
                fib_number=[wire.encode_hash(x) for x in circ.public_inputs][-1], pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]),
                _detail=out, _circuit=circ)


def prove_prime(dev, x, i, seed=7, keep_key=False, check_satisfied=False):
    """-> the reference's ProveOutput fields of the prime handler (prime_snark.rs:36-47): search j in 0..=i for the first
    hash(x + j) mod 2^20 that passes the Fermat test, build PrimeCircuit for it, circuit-specific setup, prove."""
    found = prime_search(x, i)
    if not found["found"]:
        return dict(_PRIME_NOT_FOUND)
    if keep_key or check_satisfied:     # tests want the arrays (and the satisfaction check) on the host: host synthesis
        circ = prime_circuit(x, found["j"], search=False, check_satisfied=check_satisfied)
        out = _setup_and_prove(dev, circ, random.Random(seed), keep_key)
    else:                               # the request path: R1CS and assignment built on the device, nothing synthesized on the host
        circ = _PrimeShape(x, found["j"])
        out = _setup_and_prove_prime_device(dev, x, found["j"], circ, random.Random(seed))
    return dict(proof=wire.encode_proof(out["proof"], out["inf"]), j=found["j"], num_constraints=circ.num_constraints,
                num_variables=circ.num_vars, setup_time=out["setup_time"], proving_time=out["proving_time"], found_prime=True,
                prime_num=str(found["prime"]), pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]), satisfied=circ.satisfied,
                _detail=out, _circuit=circ)


_PRIME_NOT_FOUND = dict(proof="", j=0, num_constraints=0, num_variables=0, setup_time=0.0, proving_time=0.0, found_prime=False, prime_num="", vk="")


def prime_template_key(dev, rng):
    """The key every prime request of one trapdoor shares: prove_prime's draws from rng in its order (trapdoor, generators), one
    setup on the template (Device.r1cs_prime_template) -> dict(ph, rh, vk, corr, setup_time).  The trapdoor itself is not kept:
    corr (circuits.prime_key_corrections) is all a request needs of it.  The caller frees ph and rh."""
    from .device import scalar_mul
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    g1 = scalar_mul("g1", g1_generator(), k)[0]
    g2 = scalar_mul("g2", g2_generator(), k)[0]
    corr, inf = prime_key_corrections(trap, g1)
    if inf.any():
        raise ValueError("prime_template_key: a key correction is the point at infinity")
    rh = dev.r1cs_prime_template()
    try:
        t0 = time.perf_counter()
        ph, vk = dev.setup_resident(rh, prime_dims(1)["num_instance"], trap, g1, g2)
        setup_time = time.perf_counter() - t0
    except Exception:
        dev.r1cs_free(rh)
        raise
    return dict(ph=ph, rh=rh, vk=vk, corr=corr, setup_time=setup_time)


def prove_primes(dev, requests, seed=7, key=None):
    """K requests of the prime handler, requests = [(x, i), ...], under ONE trapdoor: the search runs per request, the requests
    that found a prime are proved on one template key in batched device passes (Device.prove_prime_batch).  The key is set up
    once from `seed` with prove_prime's draws (then r, s per proved request), so request 0 is prove_prime's proof and key for that
    seed, byte for byte; or it is passed in as key= (prime_template_key's dict), which stays the caller's.  A request's key is the
    template's with gamma_abc_g1[0] replaced, so the prepared key is made once and only that element changes per request.
    -> a list of prove_prime's fields per request (a request without a prime: its not-found record)."""
    if len(requests) == 0:
        raise ValueError("prove_primes: no requests")
    found = [prime_search(x, i) for x, i in requests]
    hits = [q for q, f in enumerate(found) if f["found"]]
    out = [dict(_PRIME_NOT_FOUND) for _ in requests]
    if not hits:
        return out
    rng = random.Random(seed)
    own = key is None
    if own:
        key = prime_template_key(dev, rng)
    try:
        rss = [(_fr_mont(rng.randrange(R_MOD)), _fr_mont(rng.randrange(R_MOD))) for _ in hits]
        rs, ss = np.stack([r for r, _ in rss]), np.stack([s for _, s in rss])
        xs = np.array([requests[q][0] for q in hits], dtype=np.uint64)
        js = np.array([found[q]["j"] for q in hits], dtype=np.uint64)
        t0 = time.perf_counter()
        proofs, inf, g0, pubs, ms = dev.prove_prime_batch(key["ph"], key["rh"], key["corr"], key["vk"]["gamma_abc_g1"][0], xs, js, rs, ss)
        proving_time = time.perf_counter() - t0
    finally:
        if own:
            dev.pk_free(key["ph"])
            dev.r1cs_free(key["rh"])
    vk = key["vk"]
    dims = prime_dims(1)
    # one prepared key and one encoding for the batch: a request's key is the template's with gamma_abc_g1[0] replaced, and both
    # byte strings begin alpha_g1 (48) | beta_g2, gamma_g2, delta_g2 (96 each) | count (8), so that point is bytes 344 .. 392
    from .device import pvk_prepare
    import base64
    vk_bytes, pvk_bytes = wire.vk_serialize_compressed(vk), wire.pvk_serialize_compressed(pvk_prepare(vk))
    for n, q in enumerate(hits):
        point = wire.points_compress("g1", g0[n])
        vk_q = dict(vk, gamma_abc_g1=np.concatenate([g0[n:n + 1], vk["gamma_abc_g1"][1:]]))
        out[q] = dict(proof=wire.encode_proof(proofs[n], inf[n]), j=found[q]["j"], num_constraints=dims["num_constraints"],
                      num_variables=dims["num_instance"] + dims["num_witness"], setup_time=key["setup_time"] if own else 0.0,
                      proving_time=proving_time / len(hits), found_prime=True, prime_num=str(found[q]["prime"]),
                      pvk=base64.standard_b64encode(pvk_bytes[:344] + point + pvk_bytes[392:]).decode(),
                      vk=base64.standard_b64encode(vk_bytes[:344] + point + vk_bytes[392:]).decode(), satisfied=None,
                      _detail=dict(proof=proofs[n], inf=inf[n], vk=vk_q, r=rs[n], s=ss[n], public_inputs=pubs[n], ms=ms))
    return out


def verify_prime(vk, x, j, proof_b64):
    """Mirror of verify_prime (prime_snark.rs:165-206): the reference re-synthesizes PrimeCircuit for (x, j) to recover the
    public inputs (x and the 256 digest bits); here they are computed natively (the same values: test_prime_circuit.py), then
    the proof is checked."""
    return verify_proof(vk, prime_public_inputs(x, j), proof_b64)


def verify_proof(vk, public_inputs_mont, proof_b64):
    """Mirror of the verify handlers (matrix_proof.rs:183-205, fibbonaci_handler.rs:118-145): decode the base64 compressed
    proof (and key, when given as the base64 string the prove mirrors return), check the Groth16 equation with the host
    verifier (zkg16_verify) -> {valid, verifying_time}."""
    from ._lib import Zkg16Error
    from .device import verify, verify_prepared
    t0 = time.perf_counter()
    try:
        if isinstance(vk, str):
            raw = __import__("base64").standard_b64decode(vk)
            n = int.from_bytes(raw[336:344], "little") if len(raw) >= 344 else 0
            vk = wire.pvk_deserialize_compressed(raw) if len(raw) > 344 + 48 * n else wire.vk_deserialize_compressed(raw)
        proof, inf = wire.decode_proof(proof_b64)
        t1 = time.perf_counter()
        ok = verify_prepared(vk, public_inputs_mont, proof, inf) if "alpha_beta" in vk else verify(vk, public_inputs_mont, proof, inf)
        t2 = time.perf_counter()
    except (ValueError, IndexError, Zkg16Error):
        # the reference's decode_proof / decode_pvk return None and the handler answers invalid; a key or input list of the
        # wrong shape is the same answer, never an exception out of the handler
        return dict(valid=False, verifying_time=0.0, decode_time=time.perf_counter() - t0)
    # verifying_time = the verification call alone, as the reference's timer (matrix_proof.rs:199-206, prime_snark.rs:191-200: started
    # after decode_pvk / decode_proof); decode_time = base64 + decompression + subgroup checks of key and proof (Python big ints)
    return dict(valid=bool(ok), verifying_time=t2 - t1, decode_time=t1 - t0)


def verify_proofs(vk, public_inputs_list, proofs_b64, dev=None):
    """verify_proof for K proofs under one key, checked together (Device.verify_batch_wire with `dev`: the compressed proofs are
    decoded on the device; else host decoding and the host form verify_batch_host): one final exponentiation for the batch instead
    of one per proof.  -> {valid: [K bools], verifying_time, decode_time}.  A proof that does not decode, or whose public inputs have the wrong shape, is valid=False for that entry only;
    a key that does not decode makes every entry invalid."""
    from ._lib import Zkg16Error
    from .device import pvk_prepare, verify_batch_host
    t0 = time.perf_counter()
    k = len(proofs_b64)
    valid = [False] * k
    if len(public_inputs_list) != k:
        raise ValueError("verify_proofs: one public input list per proof")
    try:
        if isinstance(vk, str):
            raw = __import__("base64").standard_b64decode(vk)
            n = int.from_bytes(raw[336:344], "little") if len(raw) >= 344 else 0
            vk = wire.pvk_deserialize_compressed(raw) if len(raw) > 344 + 48 * n else wire.vk_deserialize_compressed(raw)
        pvk = vk if "alpha_beta" in vk else pvk_prepare(vk)
        ni = np.asarray(pvk["gamma_abc_g1"]).reshape(-1, 12).shape[0]
    except (ValueError, IndexError, Zkg16Error):
        return dict(valid=valid, verifying_time=0.0, decode_time=time.perf_counter() - t0)
    if dev is not None:
        # the proofs stay bytes: base64 and the shape checks here, the square roots in a kernel (Device.verify_batch_wire)
        idx, raws, pubs = [], [], []
        for i, (pub, pb) in enumerate(zip(public_inputs_list, proofs_b64)):
            try:
                raw = __import__("base64").standard_b64decode(pb)
                pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
                if len(raw) != 192 or pub.shape[0] != ni - 1:
                    continue
            except (ValueError, IndexError, TypeError):
                continue
            idx.append(i)
            raws.append(raw)
            pubs.append(pub)
        t1 = time.perf_counter()
        if idx:
            _, each = dev.verify_batch_wire(pvk, np.array(pubs, dtype=np.uint64).reshape(len(idx), ni - 1, 4), b"".join(raws), each=True)
            for i, ok in zip(idx, each):
                valid[i] = bool(ok)
        return dict(valid=valid, verifying_time=time.perf_counter() - t1, decode_time=t1 - t0)
    idx, proofs, infs, pubs = [], [], [], []
    for i, (pub, pb) in enumerate(zip(public_inputs_list, proofs_b64)):
        try:
            proof, inf = wire.decode_proof(pb)
            pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
            if pub.shape[0] != ni - 1:
                continue
        except (ValueError, IndexError, TypeError):
            continue
        idx.append(i)
        proofs.append(proof)
        infs.append(inf)
        pubs.append(pub)
    t1 = time.perf_counter()
    if idx:
        args = (pvk, np.array(pubs, dtype=np.uint64).reshape(len(idx), ni - 1, 4), np.array(proofs, dtype=np.uint64), np.array(infs, dtype=np.uint8))
        _, each = dev.verify_batch(*args, each=True) if dev is not None else verify_batch_host(*args, each=True)
        for i, ok in zip(idx, each):
            valid[i] = bool(ok)
    return dict(valid=valid, verifying_time=time.perf_counter() - t1, decode_time=t1 - t0)
