"""In-process mirrors of the reference's request handlers around the hot path (the callers of `Groth16::prove`):
    prove_matrix     src/arkworks/backend/matrix_proof.rs:94-166   (POST /api/matrix_prove/prove)
    prove_matrices   K such requests of one size under one key, in batched device passes (no counterpart upstream)
    prove_fibonacci  src/arkworks/backend/fibbonaci_handler.rs:98-145
    prove_fibonaccis / verify_fibonaccis  K Fibonacci requests of one round count under ONE key, in batched device passes (no
                     counterpart upstream)
    prove_linear_equations  src/arkworks/backend/linear_equations.rs:43-106
    prove_linear_equations_batch / verify_linear_equations  K linear requests of one size under ONE key, in batched device passes
                     (no counterpart upstream)
    prove_prime / verify_prime  src/arkworks/backend/prime_snark.rs:49-146, 165-206
    prove_primes     K prime requests under one trapdoor on ONE template key, in batched device passes (no counterpart upstream)
    verify_primes    K such proofs checked together under the ONE extended key of their trapdoor (no counterpart upstream)
    rerandomize_proofs  K proofs of one key re-randomised (ark-groth16 rerandomize_proof; no handler upstream calls it)
Same steps, same response fields: the circuit's R1CS and assignment (built on the device for matrix and prime requests,
synthesized inside the library and loaded unexported for Fibonacci; the host C++ mirror's arrays only where a test wants them),
per-request Groth16 setup (on the device, zkg16_setup_resident), prove (zkg16_prove_resident), encode (wire.py): one sequence for
every handler, _request.  A matrix request on cached matrices builds its assignment (Device.witness_matrix) on a thread beside the
setup and then proves with prove_resident; the overlapped Device.prove_matrix (zkg16_prove_matrix) is not used here: bench.py and
the tests call it directly.  The reference's HTTP layer (actix-web) is out of scope; the trapdoor and r, s come from Python's PRNG
rather than arkworks' StdRng stream, so proofs are valid Groth16 proofs for the same statement but not the byte string the Rust
server would emit for its seed."""
import base64
import collections
import contextlib
import ctypes as C
import random
import threading
import time

import numpy as np

from . import _lib, device, wire
from ._lib import ZKG16_ERR_BAD_ARG, ZKG16_ERR_UNSATISFIED, Zkg16Error
from .circuits import (fibonacci_circuit, fibonacci_circuit_handle, linear_circuit, linear_circuit_handle, linear_r1cs_dims, linear_solver_id, matrix_circuit, matrix_hash_batch_host, prime_circuit, prime_dims, prime_key_corrections,
                       prime_public_inputs, prime_search, prime_vk_extend)
from .workloads import R_MOD, g1_generator, g2_generator


def _fr_mont(x):
    v = (x << 256) % R_MOD
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _draw_key(rng):
    """A request's first draws, in this order: the trapdoor (5 x randrange(1, R_MOD)), then the generator scalar (4 x
    getrandbits(62)) -> (trap [5, 4], g1, g2).  arkworks draws random generators; any subgroup generator gives a valid key: [k]G."""
    trap = np.stack([_fr_mont(rng.randrange(1, R_MOD)) for _ in range(5)])
    k = np.array([rng.getrandbits(62) for _ in range(4)], dtype=np.uint64)
    return trap, device.scalar_mul("g1", g1_generator(), k)[0], device.scalar_mul("g2", g2_generator(), k)[0]


def _draw_rs(rng):
    """A proof's blinding pair, r then s, drawn after the setup."""
    return _fr_mont(rng.randrange(R_MOD)), _fr_mont(rng.randrange(R_MOD))


def _draw_rs_batch(rng, k):
    """k pairs in request order -> (rs [k, 4], ss [k, 4])."""
    rss = [_draw_rs(rng) for _ in range(k)]
    return np.stack([r for r, _ in rss]), np.stack([s for _, s in rss])


# A MatrixCircuit's matrices depend on the size alone, so they are written on the device once per size and Device
# (zkg16_r1cs_matrix: nothing of the circuit is synthesized on the host) and stay there: rh is borrowed by every later request.
_CachedShape = collections.namedtuple("_CachedShape", "rh num_instance num_witness num_constraints")


def _matrix_shape(dev, n):
    """The cached shape of size n, made by the first request that asks: the lock is held across the look-up and the device call, so
    two first requests of one size make one R1CS."""
    with dev._matrix_shapes_lock:
        shape = dev._matrix_shapes.get(n)
        if shape is None:
            nc, nw = C.c_size_t(), C.c_size_t()
            rc = _lib.load().zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), None)
            if rc:
                raise Zkg16Error(rc, "zkg16_matrix_r1cs_dims")
            shape = dev._matrix_shapes[n] = _CachedShape(dev.r1cs_matrix(n), 4, nw.value, nc.value)
        return shape


class _DeviceCircuit:
    """The "_circuit" of a request whose matrices and assignment were written on the device: the dimensions and public inputs a
    SynthesizedCircuit has, nothing synthesized on the host."""
    satisfied = z = r1cs = None

    def __init__(self, num_instance, num_witness, num_constraints, public_inputs=None):
        self.num_instance, self.num_witness, self.num_constraints = num_instance, num_witness, num_constraints
        self.num_vars = num_instance + num_witness
        self.domain = 1 << max(num_constraints + num_instance - 1, 0).bit_length()
        self.public_inputs = public_inputs


ROUTES = ("key", "trapdoor")


def _route(route):
    if route not in ROUTES:
        raise ValueError("route: 'key' or 'trapdoor'")
    return route


def _request(dev, rng, circ, r1cs, assignment, keep_key=False, overlap=False, check_on_device=False, route="key"):
    """One request of any handler: draw the key, obtain the R1CS and the assignment, set the key up, draw r and s, prove, release.
    circ gives the dimensions.  r1cs(own) -> R1CS handle and assignment(own) -> (witness handle, public inputs or None) say how
    this kind of circuit reaches the device; each passes a handle the request owns through own(free, handle) the moment it has it,
    and that handle is released on every way out.  A borrowed handle (a cached shape's rh) is not passed and never freed.  Public
    inputs that come with the assignment are stored on circ.
    keep_key: the key goes through the host (zkg16_setup -> zkg16_pk_load) and is returned as "pk"; else it never leaves the device.
    overlap: the assignment needs neither the key nor (for its host half, the three Poseidon chains) the device, so it is obtained
    on a thread beside the setup's kernels (zkg16_witness_matrix takes the ctx only for its ~1 ms of kernels): at 128x128 the 61 ms
    of chains disappear under the 0.2 s setup.
    check_on_device: before proving, Device.r1cs_check on the two handles the request holds -> "satisfied" (else None) and
    "check_time", which is not part of proving_time; the proof is made either way.
    route: "key" (default) is the above.  "trapdoor" (ignored with keep_key): the request drew the trapdoor itself, so one
    Device.prove_trapdoor call takes the place of setup_resident + prove_resident and no proving key is built — the same draws in the
    same order (trapdoor, generators, then r, s), the same proof and vk bytes for a seed.  setup_time is then reported as 0.0 and
    proving_time is the whole call (the QAP evaluation, the check and the points included); with check_on_device "satisfied" comes
    from the call's own check and check_time is 0.0.  The call refuses an unsatisfied assignment (ZKG16_ERR_UNSATISFIED): the request
    then falls back to the key route and its record is what it is today.  "route" in the result says which route answered."""
    _route(route)
    trap, g1, g2 = _draw_key(rng)
    with contextlib.ExitStack() as stack:
        def own(free, h):
            stack.callback(free, h)
            return h

        rh = r1cs(own)
        if overlap:
            early, held = {}, []

            def assign():
                try:
                    early["out"] = assignment(lambda free, h: held.append((free, h)) or h)
                except Exception as e:      # noqa: BLE001 - re-raised on the caller's thread
                    early["err"] = e

            def finish():                   # the thread never outlives the request, and what it obtained is the request's to release
                thread.join()
                for free, h in held:
                    free(h)
            thread = threading.Thread(target=assign)
            thread.start()
            stack.callback(finish)
        else:
            wh, pub = assignment(own)

        def joined():
            thread.join()
            if "err" in early:
                raise early["err"]
            return early["out"]
        answered, rs_drawn = "key", None
        if route == "trapdoor" and not keep_key:
            rs_drawn = r, s = _draw_rs(rng)
            t0 = time.perf_counter()
            if overlap:
                wh, pub = joined()
            try:
                proof, inf, vk = dev.prove_trapdoor(rh, wh, circ.num_instance, trap, g1, g2, r, s)
                answered = "trapdoor"
            except Zkg16Error as e:
                if e.status != ZKG16_ERR_UNSATISFIED:
                    raise
            proving_time = time.perf_counter() - t0
        if answered == "trapdoor":
            if pub is not None:
                circ.public_inputs = pub
            return dict(proof=proof, inf=inf, vk=vk, pk=None, setup_time=0.0, proving_time=proving_time, r=r, s=s,
                        satisfied=True if check_on_device else None, check_time=0.0, route="trapdoor")
        t0 = time.perf_counter()
        if keep_key:        # tests want the key on the host as well
            pk, vk = dev.setup(rh, circ.num_instance, circ.num_vars, circ.domain, trap, g1, g2)
            ph = own(dev.pk_free, dev.pk_load(pk, circ.num_instance))
        else:               # the request path: the key never leaves the device
            pk = None
            ph, vk = dev.setup_resident(rh, circ.num_instance, trap, g1, g2)
            own(dev.pk_free, ph)
        setup_time = time.perf_counter() - t0
        r, s = rs_drawn or _draw_rs(rng)
        t0 = time.perf_counter()
        if overlap:
            wh, pub = joined()
        satisfied, check_time = None, 0.0
        if check_on_device:
            tc = time.perf_counter()
            satisfied = dev.r1cs_check(rh, wh)[0] == 0
            check_time = time.perf_counter() - tc
        proof, inf = dev.prove_resident(ph, rh, wh, r, s)
        proving_time = time.perf_counter() - t0 - check_time
    if pub is not None:
        circ.public_inputs = pub
    return dict(proof=proof, inf=inf, vk=vk, pk=pk, setup_time=setup_time, proving_time=proving_time, r=r, s=s, satisfied=satisfied,
                check_time=check_time, route="key")


_Batch = collections.namedtuple("_Batch", "proofs inf side ms vk rs ss verdicts setup_time proving_time route")


def _batch_checks(what, k, route, key):
    """What a batch handler refuses before it shapes its input: an unknown route, route="trapdoor" with a caller's key, no requests."""
    if _route(route) == "trapdoor" and key is not None:
        raise ValueError(what + ": route='trapdoor' draws its own key (key must be None)")
    if k == 0:
        raise ValueError(what + ": no requests")


def _batch_request(dev, rng, k, key, route, r1cs, num_instance, witness_batch, prove_fused, check_on_device, check_apart):
    """K requests of one batch handler under one key (after _batch_checks): draw the key, draw r and s per request, prove, release.
    key: None, or the caller's (ph, rh, vk), which stays the caller's.  With None the key is drawn (_request's draws) and set up on
    rh = r1cs(own), which passes a handle the request owns through own(free, handle) and a borrowed one (a cached shape's) not.
    witness_batch() -> (witness handles, side output, ms) and prove_fused(ph, rh, rs, ss) -> (proofs, inf, side output, ms) are the
    handler's two Device calls.  One of three ways to the proofs:
      route "trapdoor" (key must be None): r and s are drawn before any device work, the assignments are made as handles and one
        Device.prove_trapdoor_batch call answers without a key; setup_time stays 0.0.  If it refuses an unsatisfied assignment the
        key is set up after all and the batch is redone below (with check_on_device on a second set of handles);
      check_on_device: handles, Device.r1cs_check_batch, Device.prove_batch; check_apart takes the check out of proving_time;
      else prove_fused.
    -> _Batch; verdicts: None, or with check_on_device [(n_bad, first_bad)] * k ((0, None) when the trapdoor route answered, which
    checks for itself); route: the one that answered."""
    trapdoor = route == "trapdoor"
    with contextlib.ExitStack() as stack:
        def own(free, h):
            stack.callback(free, h)
            return h

        def handles():
            whs, side, ms = witness_batch()
            for wh in whs:
                own(dev.witness_free, int(wh))
            return whs, side, ms
        setup_time, got = 0.0, None
        if key is None:
            trap, g1, g2 = _draw_key(rng)
            rh = r1cs(own)
            if trapdoor:
                rs, ss = _draw_rs_batch(rng, k)
                t0 = time.perf_counter()
                whs, side, ms = handles()
                try:
                    got = dev.prove_trapdoor_batch(rh, whs, num_instance, trap, g1, g2, rs, ss)
                except Zkg16Error as e:
                    if e.status != ZKG16_ERR_UNSATISFIED:
                        raise
            if got is None:
                t0 = time.perf_counter()
                ph, vk = dev.setup_resident(rh, num_instance, trap, g1, g2)
                own(dev.pk_free, ph)
                setup_time = time.perf_counter() - t0
        else:
            ph, rh, vk = key
        if not trapdoor:
            rs, ss = _draw_rs_batch(rng, k)
        if got is None:
            t0 = time.perf_counter()
        verdicts, check_time = None, 0.0
        if got is not None:
            proofs, inf, vk = got
            verdicts = [(0, None)] * k if check_on_device else None
        elif check_on_device:
            whs, side, ms = handles()
            tc = time.perf_counter()
            verdicts = dev.r1cs_check_batch(rh, whs)
            if check_apart:
                check_time = time.perf_counter() - tc
            proofs, inf = dev.prove_batch(ph, rh, whs, rs, ss)
        else:
            proofs, inf, side, ms = prove_fused(ph, rh, rs, ss)
        proving_time = time.perf_counter() - t0 - check_time
    return _Batch(proofs, inf, side, ms, vk, rs, ss, verdicts, setup_time, proving_time, "key" if got is None else "trapdoor")


def _batch_records(out, fields, detail):
    """A batch's per-request records: fields(i) and detail(i) give what only the handler knows; the proof, the key's two encodings
    (made once), "satisfied" (only when the device check ran) and the core of "_detail" are the same for every handler."""
    vk_b64, pvk_b64 = wire.encode_vk(out.vk), wire.encode_pvk(out.vk)
    records = []
    for i in range(len(out.proofs)):
        rec = dict(fields(i), proof=wire.encode_proof(out.proofs[i], out.inf[i]), pvk=pvk_b64, vk=vk_b64,
                   _detail=dict(detail(i), proof=out.proofs[i], inf=out.inf[i], vk=out.vk, r=out.rs[i], s=out.ss[i], ms=out.ms, route=out.route))
        if out.verdicts is not None:
            rec["satisfied"] = out.verdicts[i][0] == 0
        records.append(rec)
    return records


def _from_host(dev, circ):
    """r1cs, assignment of a SynthesizedCircuit: its arrays are uploaded."""
    return (lambda own: own(dev.r1cs_free, dev.r1cs_load(circ.r1cs, circ.num_vars)),
            lambda own: (own(dev.witness_free, dev.witness_load(circ.z)), None))


def _from_handle(dev, circ):
    """r1cs, assignment of a CircuitHandle: one zkg16_circuit_load puts both on the device unexported."""
    loaded = []

    def r1cs(own):
        rh, wh = dev.circuit_load(circ)
        own(dev.r1cs_free, rh)
        loaded.append(own(dev.witness_free, wh))
        circ.close()
        return rh
    return r1cs, lambda own: (loaded[0], None)


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


def _with_verdict(record, out, check_on_device):
    """The record of a handler whose response has no "satisfied" field: it gets one only when the device check was asked for."""
    if check_on_device:
        record["satisfied"] = out["satisfied"]
    return record


def prove_matrix(dev, size, matrix_a, matrix_b, seed=0, keep_key=False, check_on_device=False, route="key"):
    """-> the reference's ProveOutput fields (matrix_proof.rs:80-91).  check_on_device: "satisfied" is added, the verdict of
    Device.r1cs_check on the request's handles (the reference's matrix handler does not check).  route: _request's ("trapdoor": no
    proving key is built; setup_time 0.0, proving_time the whole call)."""
    a = np.asarray(matrix_a, dtype=np.uint64).reshape(size, size)
    b = np.asarray(matrix_b, dtype=np.uint64).reshape(size, size)
    if keep_key or size < 2:            # tests want the host copy of everything
        circ = matrix_circuit(a, b)
        out = _request(dev, random.Random(seed), circ, *_from_host(dev, circ), keep_key=keep_key, check_on_device=check_on_device, route=route)
    else:                               # the request path: resident matrices, the assignment built on the device beside the setup
        shape = _matrix_shape(dev, size)
        circ = _DeviceCircuit(shape.num_instance, shape.num_witness, shape.num_constraints)      # hash_a, hash_b, hash_c come with the assignment

        def assignment(own):
            wh, pub, _ = dev.witness_matrix(a, b)
            return own(dev.witness_free, wh), pub
        out = _request(dev, random.Random(seed), circ, lambda own: shape.rh, assignment, overlap=True, check_on_device=check_on_device, route=route)
    ha, hb, hc = circ.public_inputs
    return _with_verdict(dict(hash_a=wire.encode_hash(ha), hash_b=wire.encode_hash(hb), hash_c=wire.encode_hash(hc),
                setup_time=out["setup_time"], proving_time=out["proving_time"],
                # the reference counts matrix_mul twice (outer cs + circuit: matrix_proof.rs:108,150,160)
                num_constraints=circ.num_constraints + 2 * size ** 3, num_constraints_circuit=circ.num_constraints,
                num_variables=circ.num_instance, proof=wire.encode_proof(out["proof"], out["inf"]),
                # the reference returns the prepared key (encode_pvk, io.rs:62-68); the plain key is kept beside it
                pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]), _detail=out, _circuit=circ), out, check_on_device)


def prove_matrices(dev, size, pairs, seed=0, key=None, check_on_device=False, route="key"):
    """K requests of one size under ONE key, assignments and proofs in batched device passes (Device.prove_matrix_batch).  pairs: K
    (matrix_a, matrix_b).  The key is set up once on the device from `seed` (the draws of prove_matrix, then r, s per request, so
    request 0 is prove_matrix's proof for that seed), or passed in as key=(pk handle, vk dict), which stays the caller's.  The
    matrices come from the shape cache.  -> the shared vk / pvk and, per request, prove_matrix's hash_a / hash_b / hash_c / proof.
    check_on_device: the assignments are built as handles (Device.witness_matrix_batch), checked together (Device.r1cs_check_batch)
    and proved with Device.prove_batch — the same proof bytes — and every request's record gets "satisfied".
    route: "trapdoor" (only with key=None): the key is drawn as above but never built — the assignments are made as handles
    (Device.witness_matrix_batch) and one Device.prove_trapdoor_batch call gives the same proofs and vk; setup_time is 0.0 and
    proving_time the whole pass.  If the call refuses an unsatisfied assignment the whole batch is redone on the key route.
    _detail["route"] says which route answered."""
    k = len(pairs)
    _batch_checks("prove_matrices", k, route, key)
    a = np.stack([np.asarray(p[0], dtype=np.uint64).reshape(size, size) for p in pairs])
    b = np.stack([np.asarray(p[1], dtype=np.uint64).reshape(size, size) for p in pairs])
    shape = _matrix_shape(dev, size)         # its rh is borrowed, with either key
    out = _batch_request(dev, random.Random(seed), k, None if key is None else (key[0], shape.rh, key[1]), route,
                         lambda own: shape.rh, shape.num_instance, lambda: dev.witness_matrix_batch(a, b),
                         lambda ph, rh, rs, ss: dev.prove_matrix_batch(ph, rh, a, b, rs, ss), check_on_device, check_apart=False)
    pubs = out.side
    requests = [dict(hash_a=wire.encode_hash(pubs[i][0]), hash_b=wire.encode_hash(pubs[i][1]), hash_c=wire.encode_hash(pubs[i][2]),
                     proof=wire.encode_proof(out.proofs[i], out.inf[i])) for i in range(k)]
    if out.verdicts is not None:
        for q, (n_bad, _) in zip(requests, out.verdicts):
            q["satisfied"] = n_bad == 0
    return dict(vk=wire.encode_vk(out.vk), pvk=wire.encode_pvk(out.vk), setup_time=out.setup_time, proving_time=out.proving_time,
                num_constraints_circuit=shape.num_constraints, num_variables=shape.num_instance, requests=requests,
                _detail=dict(proofs=out.proofs, inf=out.inf, public_inputs=pubs, vk=out.vk, rs=out.rs, ss=out.ss, ms=out.ms, route=out.route))


def prove_fibonacci(dev, a, b, num_of_rounds, seed=42, keep_key=False, check_on_device=False, route="key"):
    """-> the reference's OutputDataFib-like fields (fibbonaci_handler.rs:84-90).  check_on_device: "satisfied" is added, the verdict
    of Device.r1cs_check on the request's handles.  route: _request's."""
    if keep_key:
        circ = fibonacci_circuit(a, b, num_of_rounds)
        sources = _from_host(dev, circ)
    else:
        circ = fibonacci_circuit_handle(a, b, num_of_rounds)
        sources = _from_handle(dev, circ)
    out = _request(dev, random.Random(seed), circ, *sources, keep_key=keep_key, check_on_device=check_on_device, route=route)
    return _with_verdict(dict(proof=wire.encode_proof(out["proof"], out["inf"]), proving_time=out["proving_time"], setup_time=out["setup_time"],
                num_constraints=circ.num_constraints, num_variables=circ.num_instance,
                fib_number=[wire.encode_hash(x) for x in circ.public_inputs][-1], pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]),
                _detail=out, _circuit=circ), out, check_on_device)


def _key_checked(dev, stack, ph, check_key):
    """-> the fields check_key adds to a kept key's record: key_ok = Device.pk_check's verdict on the resident key.  The key handle
    joins the stack first, so a failing check frees it with the rest."""
    if not check_key:
        return {}
    stack.callback(dev.pk_free, ph)
    return dict(key_ok=dev.pk_check(ph)["ok"])


def key_to_bytes(dev, key):
    """A kept key (fibonacci_key's, linear_key's, prime_template_key's or a matrix key's dict: ph and vk are read) -> its proving key
    as ark-groth16's ProvingKey::serialize_compressed bytes, encoded on the device where it lies (Device.pk_save).  The bytes hold
    the verifying key too.  They do not hold the R1CS handle (a circuit's matrices are rebuilt from its size: Device.r1cs_fibonacci,
    r1cs_linear, r1cs_matrix, r1cs_prime_template), window tables (Device.pk_precompute rebuilds them) or the prime template's
    `corr`: three G1 points outside ark's struct, which stay the caller's to keep, through wire.points_compress."""
    return dev.pk_save(key["ph"], key["vk"])


def key_from_bytes(dev, raw, rh, check_key=False):
    """key_to_bytes' inverse: ProvingKey bytes (bytes or a uint8 array) decoded on the device (Device.pk_load_bytes) -> dict(ph, rh,
    vk), the shape prove_fibonaccis, prove_linear_equations_batch and prove_matrices take as key=; rh is the caller's R1CS handle of
    the key's circuit and is passed through.  The caller frees ph and rh.  Bytes that do not decode raise (Zkg16Error, status 1,
    naming the entry) and leave nothing resident.  check_key: as fibonacci_key — key_ok = Device.pk_check's verdict.  The prime
    template's `corr` is not part of the bytes: a caller that kept it (wire.points_compress) adds it to the dict itself."""
    with contextlib.ExitStack() as stack:
        ph, vk = dev.pk_load_bytes(raw)
        checked = _key_checked(dev, stack, ph, check_key)
        stack.pop_all()
    return dict(ph=ph, rh=rh, vk=vk, setup_time=0.0, **checked)


def fibonacci_key(dev, num_of_rounds, rng, check_key=False):
    """The key every Fibonacci request of one round count shares: the circuit's matrices depend on the round count alone
    (Device.r1cs_fibonacci), so prove_fibonacci's draws from rng in its order (trapdoor, generators) and one setup give the key
    prove_fibonacci makes for any (a, b) -> dict(ph, rh, vk, setup_time).  The caller frees ph and rh.
    check_key: the record also carries key_ok, what Device.pk_check says of the resident key (every element a point of its group)."""
    trap, g1, g2 = _draw_key(rng)
    with contextlib.ExitStack() as stack:
        rh = dev.r1cs_fibonacci(num_of_rounds)
        stack.callback(dev.r1cs_free, rh)
        t0 = time.perf_counter()
        ph, vk = dev.setup_resident(rh, 4, trap, g1, g2)
        setup_time = time.perf_counter() - t0
        checked = _key_checked(dev, stack, ph, check_key)
        stack.pop_all()                 # both handles are the caller's from here
    return dict(ph=ph, rh=rh, vk=vk, setup_time=setup_time, **checked)


def prove_fibonaccis(dev, requests, num_of_rounds, seed=42, key=None, check_on_device=False, route="key"):
    """K requests of the Fibonacci handler of one round count, requests = [(a, b), ...], under ONE key, assignments and proofs in
    batched device passes (Device.prove_fibonacci_batch).  The key is set up once from `seed` with prove_fibonacci's draws (then r,
    s per request), so request 0 is prove_fibonacci's proof and key for that seed, byte for byte; or it is passed in as key=
    (fibonacci_key's dict), which stays the caller's.  The key's two encodings are made once.
    -> a list of prove_fibonacci's fields per request; proving_time is the batch's divided by K.
    check_on_device: the assignments are built as handles (Device.witness_fibonacci_batch), checked together
    (Device.r1cs_check_batch) and proved with Device.prove_batch — the same proof bytes — and every record gets "satisfied".
    route: "trapdoor" (only with key=None): prove_matrices' — Device.witness_fibonacci_batch, then one Device.prove_trapdoor_batch
    call; setup_time 0.0; a refused batch is redone on the key route; _detail["route"] says which route answered."""
    k = len(requests)
    _batch_checks("prove_fibonaccis", k, route, key)
    a = np.array([int(q[0]) for q in requests], dtype=np.uint64)
    b = np.array([int(q[1]) for q in requests], dtype=np.uint64)
    out = _batch_request(dev, random.Random(seed), k, None if key is None else (key["ph"], key["rh"], key["vk"]), route,
                         lambda own: own(dev.r1cs_free, dev.r1cs_fibonacci(num_of_rounds)), 4,
                         lambda: dev.witness_fibonacci_batch(num_of_rounds, a, b),
                         lambda ph, rh, rs, ss: dev.prove_fibonacci_batch(ph, rh, num_of_rounds, a, b, rs, ss), check_on_device, check_apart=True)
    pubs = out.side

    def fields(i):
        circ = _DeviceCircuit(4, 1, num_of_rounds + 1, pubs[i])
        return dict(proving_time=out.proving_time / k, setup_time=out.setup_time, num_constraints=circ.num_constraints,
                    num_variables=circ.num_instance, fib_number=wire.encode_hash(pubs[i][2]), _circuit=circ)
    return _batch_records(out, fields, lambda i: dict(public_inputs=pubs[i]))


def verify_fibonaccis(vk, claims, proofs_b64, dev=None):
    """The Fibonacci verify handler (fibbonaci_handler.rs:118-145) for K proofs under one key, checked together: claims = [(a, b,
    fib_number), ...] with fib_number the base64 string the prove mirrors return.  The three public inputs a, b, fib_number are built
    per proof and the batch is answered by verify_proofs (with dev: Device.verify_batch_wire and its thresholds)
    -> {valid: [K bools], verifying_time, decode_time}.  A claim whose a or b is no u64, or whose fib_number does not decode to 32
    bytes, is valid=False for that entry only."""
    if len(claims) != len(proofs_b64):
        raise ValueError("verify_fibonaccis: one claim per proof")
    pubs = []
    for a, b, fib in claims:
        try:
            a, b = int(a), int(b)
            if not (0 <= a < 1 << 64 and 0 <= b < 1 << 64) or len(base64.standard_b64decode(fib)) != 32:
                raise ValueError("verify_fibonaccis: not a claim")
            pubs.append(np.stack([_fr_mont(a), _fr_mont(b), np.asarray(wire.decode_hash(fib), dtype=np.uint64)]))
        except (ValueError, TypeError):
            pubs.append(np.zeros((0, 4), dtype=np.uint64))       # the wrong shape: verify_proofs answers invalid for this entry
    return verify_proofs(vk, pubs, proofs_b64, dev=dev)


def _linear_request(what, a, b):
    """A square system as arrays: a [n, n], b [n] u64.  The reference indexes x by column and divides by a[i][i], which only works
    for n x n (linear_equations.rs:20-41)."""
    b = np.asarray(b, dtype=np.uint64).reshape(-1)
    a = np.asarray(a, dtype=np.uint64)
    if a.shape != (b.shape[0], b.shape[0]) or b.shape[0] == 0:
        raise ValueError(what + ": a must be n x n for the n >= 1 entries of b")
    return a, b


def _linear_public_inputs(a, b):
    """The handler's public input list a[0][*], b[0], a[1][*], b[1], ... (linear_equations.rs:66-72) -> [n (n + 1), 4] Montgomery."""
    return np.stack([_fr_mont(int(v)) for v in np.concatenate([a, b[:, None]], axis=1).reshape(-1)])


def prove_linear_equations(dev, a, b, seed=0, keep_key=False, check_on_device=False, solver="forward", route="key"):
    """Mirror of prove_linear_equations (backend/linear_equations.rs:43-106): solve the system with the handler's forward
    substitution, build LinearEquationCircuit, circuit-specific setup, prove, verify against a[0][*], b[0], a[1][*], b[1], ...
    The solver is only right for a lower-triangular a: for any other a the circuit is in general unsatisfied, the proof is made all the
    same (as upstream, whose prover does not check in release builds) and "valid" is False.  A zero diagonal entry, a panic upstream,
    raises Zkg16Error (ZKG16_ERR_UNSUPPORTED).
    -> the reference's OutputData fields plus valid, pvk and vk.  Deviations from the reference's record: "proof" and the entries of
    "public_input" are base64 (of the compressed proof / of the 32 little-endian bytes), as in the other mirrors, where upstream
    prints Rust Debug strings; "num_constraints" and "num_variables" (the instance count) are the real system's, where upstream
    reports 0 and 1 from a constraint system it never synthesizes into (:62, :100-101); "proving_time" and "verifying_time" are
    measured, where upstream returns 0.0; "valid" is the verifier's answer, which upstream computes and drops.
    check_on_device: "satisfied" is added, the verdict of Device.r1cs_check on the request's handles.
    solver: "forward" is the above; "elimination" solves a x = b by Gaussian elimination over Fr (circuits.linear_circuit's
    solver=), so "valid" (and "satisfied") is True for every a that is non-singular mod r, and a singular a raises Zkg16Error
    (ZKG16_ERR_UNSUPPORTED) as a zero diagonal does.  Key, matrices and public inputs do not depend on the solver.
    route: _request's; a system the solver leaves unsatisfied (a dense a under "forward") is answered by the key route."""
    a, b = _linear_request("prove_linear_equations", a, b)
    if keep_key:
        circ = linear_circuit(a, b, solver=solver)
        sources = _from_host(dev, circ)
    else:
        circ = linear_circuit_handle(a, b, solver=solver)
        sources = _from_handle(dev, circ)
    out = _request(dev, random.Random(seed), circ, *sources, keep_key=keep_key, check_on_device=check_on_device, route=route)
    t0 = time.perf_counter()
    valid = bool(device.verify(out["vk"], circ.public_inputs, out["proof"], out["inf"]))
    verifying_time = time.perf_counter() - t0
    return _with_verdict(dict(proof=wire.encode_proof(out["proof"], out["inf"]), public_input=[wire.encode_hash(x) for x in circ.public_inputs],
                num_constraints=circ.num_constraints, num_variables=circ.num_instance, proving_time=out["proving_time"],
                verifying_time=verifying_time, valid=valid, pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]),
                _detail=out, _circuit=circ), out, check_on_device)


def linear_key(dev, n, rng, check_key=False):
    """The key every linear request of one size shares: the circuit's matrices depend on n alone (Device.r1cs_linear), so
    prove_linear_equations' draws from rng in its order (trapdoor, generators) and one setup give the key that handler makes for any
    (a, b) -> dict(ph, rh, vk, setup_time).  The caller frees ph and rh.  check_key: as fibonacci_key."""
    trap, g1, g2 = _draw_key(rng)
    with contextlib.ExitStack() as stack:
        rh = dev.r1cs_linear(n)
        stack.callback(dev.r1cs_free, rh)
        t0 = time.perf_counter()
        ph, vk = dev.setup_resident(rh, 1 + n * (n + 1), trap, g1, g2)
        setup_time = time.perf_counter() - t0
        checked = _key_checked(dev, stack, ph, check_key)
        stack.pop_all()                 # both handles are the caller's from here
    return dict(ph=ph, rh=rh, vk=vk, setup_time=setup_time, **checked)


def prove_linear_equations_batch(dev, systems, seed=0, key=None, check_on_device=False, solver="forward", route="key"):
    """K requests of the linear handler of one size, systems = [(a, b), ...], under ONE key, assignments and proofs in batched device
    passes (Device.prove_linear_batch).  The key is set up once from `seed` with prove_linear_equations' draws (then r, s per
    request), so request 0 is that handler's proof and key for that seed, byte for byte; or it is passed in as key= (linear_key's
    dict), which stays the caller's.  The key's two encodings are made once, and the K proofs are verified together on the host.
    -> a list of prove_linear_equations' fields per request; proving_time and verifying_time are the batch's divided by K.
    check_on_device: the assignments are built as handles (Device.witness_linear_batch), checked together
    (Device.r1cs_check_batch) and proved with Device.prove_batch — the same proof bytes — and every record gets "satisfied".
    solver: "forward", or "elimination" (the device passes run under option "linear_solver" = 1): every non-singular request's
    record has valid True, and a singular request raises Zkg16Error (ZKG16_ERR_UNSUPPORTED) for the whole batch.
    route: "trapdoor" (only with key=None): prove_matrices' — Device.witness_linear_batch, then one Device.prove_trapdoor_batch
    call; setup_time 0.0; a batch holding a request its solver leaves unsatisfied is redone on the key route; _detail["route"] says
    which route answered."""
    k = len(systems)
    _batch_checks("prove_linear_equations_batch", k, route, key)
    how = {} if linear_solver_id(solver) == 0 else dict(solver=solver)        # "forward": the Device calls as they always were
    reqs = [_linear_request("prove_linear_equations_batch", a, b) for a, b in systems]
    n = reqs[0][1].shape[0]
    if any(q[1].shape[0] != n for q in reqs):
        raise ValueError("prove_linear_equations_batch: every system of a batch has one size")
    a, b = np.stack([q[0] for q in reqs]), np.stack([q[1] for q in reqs])
    out = _batch_request(dev, random.Random(seed), k, None if key is None else (key["ph"], key["rh"], key["vk"]), route,
                         lambda own: own(dev.r1cs_free, dev.r1cs_linear(n)), 1 + n * (n + 1), lambda: dev.witness_linear_batch(a, b, **how),
                         lambda ph, rh, rs, ss: dev.prove_linear_batch(ph, rh, a, b, rs, ss, **how), check_on_device, check_apart=True)
    pubs = np.stack([_linear_public_inputs(a[i], b[i]) for i in range(k)])
    t0 = time.perf_counter()
    _, each = device.verify_batch_host(device.pvk_prepare(out.vk), pubs, np.asarray(out.proofs, dtype=np.uint64), np.asarray(out.inf, dtype=np.uint8),
                                       each=True)
    verifying_time = time.perf_counter() - t0
    dims = linear_r1cs_dims(n)

    def fields(i):
        circ = _DeviceCircuit(dims["num_instance"], dims["num_witness"], dims["num_constraints"], pubs[i])
        return dict(public_input=[wire.encode_hash(x) for x in pubs[i]], num_constraints=circ.num_constraints,
                    num_variables=circ.num_instance, proving_time=out.proving_time / k, verifying_time=verifying_time / k,
                    valid=bool(each[i]), _circuit=circ)
    return _batch_records(out, fields, lambda i: dict(public_inputs=pubs[i], x=out.side[i], setup_time=out.setup_time))


def verify_linear_equations(vk, systems, proofs_b64, dev=None):
    """The verification the linear handler runs on its own proof (linear_equations.rs:92-94) for K proofs under one key, checked
    together: systems = [(a, b), ...], each n x n with the n entries of b.  The n^2 + n public inputs a[0][*], b[0], a[1][*], b[1], ...
    are built per proof and the batch is answered by verify_proofs; with dev they stay 64-bit values, one uint64 array for the batch,
    and Device.verify_batch_u64_wire answers (its thresholds and its per-proof take-over)
    -> {valid: [K bools], verifying_time, decode_time}.  A system that is not square, or holds a value that is no u64, is valid=False
    for that entry only."""
    if len(systems) != len(proofs_b64):
        raise ValueError("verify_linear_equations: one system per proof")
    if dev is not None:
        return _verify_linear_equations_u64(dev, vk, systems, proofs_b64)
    pubs = []
    for a, b in systems:
        try:
            rows = [[int(v) for v in row] for row in a]
            rhs = [int(v) for v in b]
            if len(rhs) == 0 or len(rows) != len(rhs) or any(len(row) != len(rhs) for row in rows) or \
                    not all(0 <= v < 1 << 64 for row in rows for v in row) or not all(0 <= v < 1 << 64 for v in rhs):
                raise ValueError("verify_linear_equations: not a system")
            pubs.append(_linear_public_inputs(np.array(rows, dtype=np.uint64), np.array(rhs, dtype=np.uint64)))
        except (ValueError, TypeError, OverflowError):
            pubs.append(np.zeros((0, 4), dtype=np.uint64))       # the wrong shape: verify_proofs answers invalid for this entry
    return verify_proofs(vk, pubs, proofs_b64, dev=dev)


def _linear_u64_row(a, b):
    """A request's n (n + 1) public inputs a[0][*], b[0], a[1][*], b[1], ... = the row-major matrix [a | b] as one uint64 vector, or
    None for what verify_linear_equations calls no system.  Integer arrays (and lists numpy reads as such) are checked and laid out
    by numpy, no Python integer per value; anything else (objects, floats, strings) goes value by value through int(), exactly as
    without a device."""
    try:
        am, bv = np.asarray(a), np.asarray(b)
        if am.dtype.kind not in "ui" or bv.dtype.kind not in "ui":
            rows = [[int(v) for v in row] for row in a]
            rhs = [int(v) for v in b]
            if any(len(row) != len(rhs) for row in rows) or not all(0 <= v < 1 << 64 for row in rows for v in row) or \
                    not all(0 <= v < 1 << 64 for v in rhs):
                return None
            am, bv = np.array(rows, dtype=np.uint64).reshape(len(rows), -1), np.array(rhs, dtype=np.uint64)
        n = bv.shape[0] if bv.ndim == 1 else 0
        if n == 0 or am.shape != (n, n) or (am.dtype.kind == "i" and am.min() < 0) or (bv.dtype.kind == "i" and bv.min() < 0):
            return None
        return np.concatenate([am.astype(np.uint64), bv.astype(np.uint64)[:, None]], axis=1).reshape(-1)
    except (ValueError, TypeError, OverflowError):
        return None


def _verify_linear_equations_u64(dev, vk, systems, proofs_b64):
    """verify_linear_equations with a device: every public input of the route is a plain u64, so the K' well-formed requests
    travel as one [K', n (n + 1)] uint64 array and 192 proof bytes each into Device.verify_batch_u64_wire — 8 bytes per input, no
    Montgomery conversion on the host, the multiplier sums and the prepared inputs taken on the device.  Entries that are malformed
    never reach the device; the answers are verify_proofs'."""
    t0 = time.perf_counter()
    k = len(proofs_b64)
    valid = [False] * k
    try:
        vk = _decode_key(vk)
        pvk = vk if "alpha_beta" in vk else device.pvk_prepare(vk)
        ni = np.asarray(pvk["gamma_abc_g1"]).reshape(-1, 12).shape[0]
    except (ValueError, IndexError, Zkg16Error) as e:
        if not _answers_invalid(e):
            raise
        return dict(valid=valid, verifying_time=0.0, decode_time=time.perf_counter() - t0)
    idx, proofs, rows = [], [], []
    for i, ((a, b), pb) in enumerate(zip(systems, proofs_b64)):
        try:
            proof = base64.standard_b64decode(pb)
        except (ValueError, TypeError):
            continue
        row = _linear_u64_row(a, b)
        if row is None or row.shape[0] != ni - 1 or ni < 2 or len(proof) != 192:
            continue
        idx.append(i)
        proofs.append(proof)
        rows.append(row)
    t1 = time.perf_counter()
    if idx:
        _, each = dev.verify_batch_u64_wire(pvk, np.stack(rows), b"".join(proofs), each=True)
        for i, ok in zip(idx, each):
            valid[i] = bool(ok)
    return dict(valid=valid, verifying_time=time.perf_counter() - t1, decode_time=t1 - t0)


def prove_prime(dev, x, i, seed=7, keep_key=False, check_satisfied=False, check_on_device=False, route="key"):
    """-> the reference's ProveOutput fields of the prime handler (prime_snark.rs:36-47): search j in 0..=i for the first
    hash(x + j) mod 2^20 that passes the Fermat test, build PrimeCircuit for it, circuit-specific setup, prove.
    "satisfied": None, or with check_satisfied the host synthesis' verdict (which leaves the device path for the host synthesis),
    or with check_on_device Device.r1cs_check's on the handles of whichever path the request took — what the reference's
    assert!(cs.is_satisfied()) (prime_snark.rs:123-128) looks at.  The proof is returned either way.  route: _request's; a
    candidate whose circuit is not satisfied is answered by the key route."""
    found = prime_search(x, i)
    if not found["found"]:
        return dict(_PRIME_NOT_FOUND)
    if keep_key or check_satisfied:     # tests want the arrays (and the satisfaction check) on the host: host synthesis
        circ = prime_circuit(x, found["j"], search=False, check_satisfied=check_satisfied)
        sources = _from_host(dev, circ)
    else:                               # the request path: R1CS and assignment built on the device, nothing synthesized on the host
        j, dims = found["j"], prime_dims(found["j"])
        circ = _DeviceCircuit(dims["num_instance"], dims["num_witness"], dims["num_constraints"], prime_public_inputs(x, j))
        circ.j = j
        sources = (lambda own: own(dev.r1cs_free, dev.r1cs_prime(x, j)), lambda own: (own(dev.witness_free, dev.witness_prime(x, j)), None))
    out = _request(dev, random.Random(seed), circ, *sources, keep_key=keep_key, check_on_device=check_on_device, route=route)
    return dict(proof=wire.encode_proof(out["proof"], out["inf"]), j=found["j"], num_constraints=circ.num_constraints,
                num_variables=circ.num_vars, setup_time=out["setup_time"], proving_time=out["proving_time"], found_prime=True,
                prime_num=str(found["prime"]), pvk=wire.encode_pvk(out["vk"]), vk=wire.encode_vk(out["vk"]),
                satisfied=out["satisfied"] if check_on_device else circ.satisfied, _detail=out, _circuit=circ)


_PRIME_NOT_FOUND = dict(proof="", j=0, num_constraints=0, num_variables=0, setup_time=0.0, proving_time=0.0, found_prime=False, prime_num="", vk="")


def prime_template_key(dev, rng, check_key=False):
    """The key every prime request of one trapdoor shares: prove_prime's draws from rng in its order (trapdoor, generators), one
    setup on the template (Device.r1cs_prime_template) -> dict(ph, rh, vk, corr, ext_vk, setup_time).  The trapdoor itself is not
    kept: corr (circuits.prime_key_corrections) is all a request needs of it.  ext_vk: the template vk with the 260 gamma_abc_g1
    points of circuits.prime_vk_extend, the ONE key verify_primes checks every request of this trapdoor under (it serialises
    through wire.vk_serialize_compressed like any vk).  The caller frees ph and rh.  check_key: as fibonacci_key."""
    trap, g1, g2 = _draw_key(rng)
    corr, inf = prime_key_corrections(trap, g1)
    if inf.any():
        raise ValueError("prime_template_key: a key correction is the point at infinity")
    with contextlib.ExitStack() as stack:
        rh = dev.r1cs_prime_template()
        stack.callback(dev.r1cs_free, rh)
        t0 = time.perf_counter()
        ph, vk = dev.setup_resident(rh, prime_dims(1)["num_instance"], trap, g1, g2)
        setup_time = time.perf_counter() - t0
        checked = _key_checked(dev, stack, ph, check_key)
        stack.pop_all()                 # both handles are the caller's from here
    ext_vk = dict(vk, gamma_abc_g1=prime_vk_extend(vk["gamma_abc_g1"], corr))
    return dict(ph=ph, rh=rh, vk=vk, corr=corr, ext_vk=ext_vk, setup_time=setup_time, **checked)


def prove_primes(dev, requests, seed=7, key=None, check_on_device=False):
    """K requests of the prime handler, requests = [(x, i), ...], under ONE trapdoor: the search runs per request, the requests
    that found a prime are proved on one template key in batched device passes (Device.prove_prime_batch).  The key is set up
    once from `seed` with prove_prime's draws (then r, s per proved request), so request 0 is prove_prime's proof and key for that
    seed, byte for byte; or it is passed in as key= (prime_template_key's dict), which stays the caller's.  A request's key is the
    template's with gamma_abc_g1[0] replaced, so the prepared key is made once and only that element changes per request.
    -> a list of prove_prime's fields per request (a request without a prime: its not-found record).
    check_on_device: every proved request's "satisfied" is its verdict from Device.prime_check_batch on the template (else None);
    the proofs are returned either way."""
    if len(requests) == 0:
        raise ValueError("prove_primes: no requests")
    found = [prime_search(x, i) for x, i in requests]
    hits = [q for q, f in enumerate(found) if f["found"]]
    out = [dict(_PRIME_NOT_FOUND) for _ in requests]
    if not hits:
        return out
    rng = random.Random(seed)
    own = key is None
    with contextlib.ExitStack() as stack:
        if own:
            key = prime_template_key(dev, rng)
            stack.callback(dev.r1cs_free, key["rh"])
            stack.callback(dev.pk_free, key["ph"])
        rs, ss = _draw_rs_batch(rng, len(hits))
        xs = np.array([requests[q][0] for q in hits], dtype=np.uint64)
        js = np.array([found[q]["j"] for q in hits], dtype=np.uint64)
        verdicts = dev.prime_check_batch(key["rh"], xs, js) if check_on_device else None
        t0 = time.perf_counter()
        proofs, inf, g0, pubs, ms = dev.prove_prime_batch(key["ph"], key["rh"], key["corr"], key["vk"]["gamma_abc_g1"][0], xs, js, rs, ss)
        proving_time = time.perf_counter() - t0
    vk = key["vk"]
    dims = prime_dims(1)
    # one prepared key and one encoding for the batch: a request's key is the template's with gamma_abc_g1[0] replaced, and both
    # byte strings begin alpha_g1 (48) | beta_g2, gamma_g2, delta_g2 (96 each) | count (8), so that point is bytes 344 .. 392
    vk_bytes, pvk_bytes = wire.vk_serialize_compressed(vk), wire.pvk_serialize_compressed(device.pvk_prepare(vk))
    for n, q in enumerate(hits):
        point = wire.points_compress("g1", g0[n])
        vk_q = dict(vk, gamma_abc_g1=np.concatenate([g0[n:n + 1], vk["gamma_abc_g1"][1:]]))
        out[q] = dict(proof=wire.encode_proof(proofs[n], inf[n]), j=found[q]["j"], num_constraints=dims["num_constraints"],
                      num_variables=dims["num_instance"] + dims["num_witness"], setup_time=key["setup_time"] if own else 0.0,
                      proving_time=proving_time / len(hits), found_prime=True, prime_num=str(found[q]["prime"]),
                      pvk=base64.standard_b64encode(pvk_bytes[:344] + point + pvk_bytes[392:]).decode(),
                      vk=base64.standard_b64encode(vk_bytes[:344] + point + vk_bytes[392:]).decode(),
                      satisfied=None if verdicts is None else verdicts[n][0] == 0,
                      _detail=dict(proof=proofs[n], inf=inf[n], vk=vk_q, r=rs[n], s=ss[n], public_inputs=pubs[n], ms=ms))
    return out


def verify_prime(vk, x, j, proof_b64):
    """Mirror of verify_prime (prime_snark.rs:165-206): the reference re-synthesizes PrimeCircuit for (x, j) to recover the
    public inputs (x and the 256 digest bits); here they are computed natively (the same values: test_prime_circuit.py), then
    the proof is checked."""
    return verify_proof(vk, prime_public_inputs(x, j), proof_b64)


def _decode_key(vk):
    """A key as the prove mirrors return it (base64 of the compressed vk or pvk), or already a dict -> the dict.  The two byte
    strings begin alike; a prepared key is longer than its gamma_abc_g1 count accounts for."""
    if not isinstance(vk, str):
        return vk
    raw = base64.standard_b64decode(vk)
    n = int.from_bytes(raw[336:344], "little") if len(raw) >= 344 else 0
    return wire.pvk_deserialize_compressed(raw) if len(raw) > 344 + 48 * n else wire.vk_deserialize_compressed(raw)


def _answers_invalid(e):
    """Whether an exception out of decoding or checking means "invalid": the reference's decode_proof / decode_pvk return None and
    its handler answers invalid, and a key or input list of the wrong shape (ZKG16_ERR_BAD_ARG) is the same answer.  Any other status
    (out of memory, a HIP failure) is the service's trouble, not the proof's, and is raised."""
    return isinstance(e, (ValueError, IndexError)) or (isinstance(e, Zkg16Error) and e.status == ZKG16_ERR_BAD_ARG)


def verify_proof(vk, public_inputs_mont, proof_b64):
    """Mirror of the verify handlers (matrix_proof.rs:183-205, fibbonaci_handler.rs:118-145): decode the base64 compressed
    proof (and key, when given as the base64 string the prove mirrors return), check the Groth16 equation with the host
    verifier (zkg16_verify) -> {valid, verifying_time}."""
    t0 = time.perf_counter()
    try:
        vk = _decode_key(vk)
        proof, inf = wire.decode_proof(proof_b64)
        t1 = time.perf_counter()
        ok = (device.verify_prepared if "alpha_beta" in vk else device.verify)(vk, public_inputs_mont, proof, inf)
        t2 = time.perf_counter()
    except (ValueError, IndexError, Zkg16Error) as e:
        if not _answers_invalid(e):
            raise
        return dict(valid=False, verifying_time=0.0, decode_time=time.perf_counter() - t0)
    # verifying_time = the verification call alone, as the reference's timer (matrix_proof.rs:199-206, prime_snark.rs:191-200: started
    # after decode_pvk / decode_proof); decode_time = base64 + decompression + subgroup checks of key and proof (Python big ints)
    return dict(valid=bool(ok), verifying_time=t2 - t1, decode_time=t1 - t0)


def verify_proofs(vk, public_inputs_list, proofs_b64, dev=None):
    """verify_proof for K proofs under one key, checked together (Device.verify_batch_wire with `dev`: the compressed proofs are
    decoded on the device; else host decoding and the host form verify_batch_host): one final exponentiation for the batch instead
    of one per proof.  -> {valid: [K bools], verifying_time, decode_time}.  A proof that does not decode, or whose public inputs have the wrong shape, is valid=False for that entry only;
    a key that does not decode makes every entry invalid."""
    t0 = time.perf_counter()
    k = len(proofs_b64)
    valid = [False] * k
    if len(public_inputs_list) != k:
        raise ValueError("verify_proofs: one public input list per proof")
    try:
        vk = _decode_key(vk)
        pvk = vk if "alpha_beta" in vk else device.pvk_prepare(vk)
        ni = np.asarray(pvk["gamma_abc_g1"]).reshape(-1, 12).shape[0]
    except (ValueError, IndexError, Zkg16Error) as e:
        if not _answers_invalid(e):
            raise
        return dict(valid=valid, verifying_time=0.0, decode_time=time.perf_counter() - t0)
    # with dev the proofs stay bytes: base64 and the shape checks here, the square roots in a kernel (Device.verify_batch_wire)
    keep_bytes = dev is not None
    idx, proofs, pubs = [], [], []
    for i, (pub, pb) in enumerate(zip(public_inputs_list, proofs_b64)):
        try:
            proof = base64.standard_b64decode(pb) if keep_bytes else wire.decode_proof(pb)
            pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
            if pub.shape[0] != ni - 1 or (keep_bytes and len(proof) != 192):
                continue
        except (ValueError, IndexError, TypeError):
            continue
        idx.append(i)
        proofs.append(proof)
        pubs.append(pub)
    t1 = time.perf_counter()
    if idx:
        pubs = np.array(pubs, dtype=np.uint64).reshape(len(idx), ni - 1, 4)
        if keep_bytes:
            _, each = dev.verify_batch_wire(pvk, pubs, b"".join(proofs), each=True)
        else:
            _, each = device.verify_batch_host(pvk, pubs, np.array([p for p, _ in proofs], dtype=np.uint64),
                                               np.array([f for _, f in proofs], dtype=np.uint8), each=True)
        for i, ok in zip(idx, each):
            valid[i] = bool(ok)
    return dict(valid=valid, verifying_time=time.perf_counter() - t1, decode_time=t1 - t0)


def rerandomize_proofs(vk, proofs_b64, dev=None):
    """K base64 compressed proofs of one key re-randomised (ark-groth16's rerandomize_proof, with r1, r2 of each proof drawn from
    `secrets`): the results verify for exactly the inputs the originals verify for and cannot be linked to them.  vk: a key dict or
    the base64 the prove mirrors return (its delta_g2 is all that is read).  With dev the proofs stay bytes from end to end
    (Device.rerandomize_batch_wire); without, host decoding, device.rerandomize_batch_host and encoding.  -> a list of base64
    proofs, "" for a proof that did not decode (wrong length, bad base64, a point off the curve or outside the subgroup); the other
    entries are unaffected.  Anything else that goes wrong — the key included — is raised."""
    vk = _decode_key(vk)
    k = len(proofs_b64)
    out = [""] * k
    keep_bytes = dev is not None
    idx, proofs = [], []
    for i, pb in enumerate(proofs_b64):
        try:
            proof = base64.standard_b64decode(pb)
            if len(proof) != 192:
                continue
            if not keep_bytes:
                proof = wire.proof_deserialize_compressed(proof)
        except (ValueError, IndexError, TypeError):          # binascii.Error is a ValueError
            continue
        idx.append(i)
        proofs.append(proof)
    if not idx:
        return out
    if keep_bytes:
        new, st = dev.rerandomize_batch_wire(vk, b"".join(proofs))
        for j, i in enumerate(idx):
            if not st[j].any():
                out[i] = base64.standard_b64encode(new[j].tobytes()).decode()
    else:
        new, inf = device.rerandomize_batch_host(vk, np.array([p for p, _ in proofs], dtype=np.uint64), np.array([f for _, f in proofs], dtype=np.uint8))
        for j, i in enumerate(idx):
            out[i] = wire.encode_proof(new[j], inf[j])
    return out


def verify_primes(ext_vk, requests, dev=None):
    """verify_prime for K proofs made under one trapdoor (prove_primes), checked together under its ONE extended key
    (prime_template_key's ext_vk: a dict, or the base64 of its compressed bytes; prepared or not).  requests = [(x, j, proof_b64), ...]
    -> {valid: [K bools], verifying_time, decode_time}.  With dev the proofs stay bytes and the public inputs are never made on
    the host (Device.verify_prime_batch_wire); without, host decoding and device.verify_prime_batch_host.  A proof that does not
    decode, or whose x or j is no u64, is valid=False for that entry only; a key that does not decode, or whose point count is
    not 260, makes every entry invalid — verify_proofs' rules."""
    t0 = time.perf_counter()
    k = len(requests)
    valid = [False] * k
    try:
        vk = _decode_key(ext_vk)
        pvk = vk if "alpha_beta" in vk else device.pvk_prepare(vk)
        if np.asarray(pvk["gamma_abc_g1"]).reshape(-1, 12).shape[0] != 260:
            raise ValueError("verify_primes: an extended key has 260 gamma_abc_g1 points")
    except (ValueError, IndexError, Zkg16Error) as e:
        if not _answers_invalid(e):
            raise
        return dict(valid=valid, verifying_time=0.0, decode_time=time.perf_counter() - t0)
    keep_bytes = dev is not None
    idx, proofs, xs, js = [], [], [], []
    for i, (x, j, pb) in enumerate(requests):
        try:
            proof = base64.standard_b64decode(pb) if keep_bytes else wire.decode_proof(pb)
            x, j = int(x), int(j)
            if not (0 <= x < 1 << 64 and 0 <= j < 1 << 64) or (keep_bytes and len(proof) != 192):
                continue
        except (ValueError, IndexError, TypeError):
            continue
        idx.append(i)
        proofs.append(proof)
        xs.append(x)
        js.append(j)
    t1 = time.perf_counter()
    if idx:
        xs, js = np.array(xs, dtype=np.uint64), np.array(js, dtype=np.uint64)
        if keep_bytes:
            _, each = dev.verify_prime_batch_wire(pvk, xs, js, b"".join(proofs), each=True)
        else:
            _, each = device.verify_prime_batch_host(pvk, xs, js, np.array([p for p, _ in proofs], dtype=np.uint64),
                                                     np.array([f for _, f in proofs], dtype=np.uint8), each=True)
        for i, ok in zip(idx, each):
            valid[i] = bool(ok)
    return dict(valid=valid, verifying_time=time.perf_counter() - t1, decode_time=t1 - t0)
