"""No result may depend on what earlier calls left on a context.  The steps of tests/sequence_cases.py — every kernel family, each
with a reference that shares no device code — played in orders a server's own traffic produces:

a. every ordered pair of a family's steps on one context;
b. a fixed walk of 150 steps across all families on one context, then the same walk reversed;
c. the matching good step right after a refused call;
d. two threads on one context proving circuits of different domains, then swapped;
e. blocks that come back uncleared: a second context in the process of one that ran the large shapes and closed (the first one's
   teardown empties the allocation cache, so these blocks are whatever the runtime hands back), and — on one living context — new
   handles loaded into the blocks of 1 MiB and more that freed handles left in the cache.

Every step of every sequence is compared, byte for byte, and every MSM step asserts through zkg16_last_msm_state the path the
table claims for it.  Workspaces only grow and very little is cleared (DESIGN.md §3 lists every buffer and what makes it valid
again), so a small call after a large one works inside large, dirty buffers: that is what these orders put under each kernel."""
import ctypes as C
import threading

import numpy as np
import pytest

import sequence_cases as Q
from test_msm_limits_gpu import cus, dev      # noqa: F401  (a helper context and the compute units of device 0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(oracle):
    import os
    oracle.set_threads(min(os.cpu_count() or 1, 16))
    yield Q.host_of(oracle)
    oracle.set_threads(1)


@pytest.fixture()
def env(host, cus):
    """a fresh context for one test"""
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield Q.Env(d, host, cus)
    d.close()


# ------------------------------------------------------------------------------------------------ a. ordered pairs inside a family
_FIRST = [(s.family, s.name) for s in Q.STEPS]


@pytest.mark.parametrize("fam,first", _FIRST, ids=["%s:%s" % x for x in _FIRST])
def test_every_step_after_this_one(env, host, fam, first):
    """p, q for every q of p's family (p itself included), on one context: p q1 p q2 ... — every run of either is compared"""
    p = Q.BY_NAME[first]
    order = [s for q in Q.family(fam) for s in (p, q)]
    assert Q.run_sequence(env, order, host.expected) == 2 * len(Q.family(fam))


# ------------------------------------------------------------------------------------------------ b. a walk across families
WALK_PIECES = 5


@pytest.fixture(scope="module")
def walker(host, cus):
    """one context for the whole walk and its reverse, and the step that ran last on it"""
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield {"env": Q.Env(d, host, cus), "before": None, "ran": 0}
    d.close()


@pytest.mark.parametrize("piece", range(2 * WALK_PIECES), ids=["forward-%d" % i for i in range(WALK_PIECES)] + ["reversed-%d" % i for i in range(WALK_PIECES)])
def test_walk_across_families(walker, host, piece):
    """150 steps with a fixed seed — the whole table shuffled, then further draws from it — and the same 150 backwards, on one
    context, in ten pieces of 30: every step asserted, none skipped or tried again.  The pieces share the context and each one
    checks that those before it ran: a single piece cannot be selected alone, the parametrised test runs as a whole."""
    walk = Q.walk()
    steps = (walk + walk[::-1])[30 * piece:30 * (piece + 1)]
    assert len(walk) == 150 == 30 * WALK_PIECES and len(steps) == 30
    assert walker["ran"] == 30 * piece, "an earlier piece of the walk did not run to its end"
    try:
        Q.run_sequence(walker["env"], steps, host.expected, before=walker["before"])
    finally:
        walker["ran"] += 30          # a failed piece does not stop the pieces behind it: they run on what it left, as a server would
        walker["before"] = steps[-1]


# ------------------------------------------------------------------------------------------------ c. after a refusal
def _status(call):
    from zksnark_finalproject_amd import Zkg16Error
    with pytest.raises(Zkg16Error) as e:
        call()
    return e.value.status


def _good(env, host, name):
    Q.run_sequence(env, [Q.BY_NAME[name]], host.expected)


def test_after_an_unsatisfied_assignment_is_refused(env, host):
    from zksnark_finalproject_amd.circuits import r1cs_check_host
    c = host.circuit("X")
    _good(env, host, "prove-resident-X-check-satisfied")
    wb = env.dev.witness_load(c["z_bad"])
    with Q.options(env.dev, {"check_satisfied": 1}):
        assert _status(lambda: env.dev.prove_resident(env.key("X"), env.r1cs("X"), wb, c["rs"][0], c["ss"][0])) == Q.UNSATISFIED
        assert env.dev.last_check() == [r1cs_check_host(c["r1cs"], c["z_bad"], c["nv"])]
    _good(env, host, "prove-resident-X-check-satisfied")


def test_after_a_batch_with_a_bad_handle_is_refused(env, host):
    c = host.circuit("Y")
    _good(env, host, "prove-batch-Y-k3")
    gone = env.dev.witness_load(c["zs"][1])
    env.dev.witness_free(gone)
    whs = np.array([env.wit("Y", 0), gone, env.wit("Y", 2)], dtype=np.uint64)
    assert _status(lambda: env.dev.prove_batch(env.key("Y"), env.r1cs("Y"), whs, c["rs"][:3], c["ss"][:3])) == Q.BAD_HANDLE
    _good(env, host, "prove-batch-Y-k3")


def test_after_a_wire_batch_of_no_whole_proofs_is_refused(env, host):
    """The C entry takes a proof count, not a byte length: this refusal is the binding's (ValueError, before the library is called)
    and the context never sees the refused call.  What is held is that the binding refuses instead of rounding the length down, and
    that the same step gives the same bytes again; no device-side refusal is covered here."""
    b, rho = Q.verify_batch_of(host)
    raw, _ = Q.wire_batch(host)
    _good(env, host, "verify-batch-wire-k65-hostile")
    with Q.options(env.dev, Q.ALWAYS_DEVICE):
        for payload in (raw.tobytes()[:-1], np.zeros(65 * 192 + 1, dtype=np.uint8)):
            with pytest.raises(ValueError):
                env.dev.verify_batch_wire(b.pvk, b.pubs, payload, rho=rho)
    _good(env, host, "verify-batch-wire-k65-hostile")


def test_after_a_trapdoor_in_the_domain_is_refused(env, host):
    """tau a 32nd root of unity on Z's 32-point domain: refused; the same request with the key's own tau equals the host form"""
    import pyref as P
    from helpers import fr_mont, fr_mont_vec, unlimbs
    from zksnark_finalproject_amd.device import prove_trapdoor_host
    c = host.circuit("Z")
    t = c["meta"]["trap"]
    trap = fr_mont_vec([t[k] for k in ("tau", "alpha", "beta", "gamma", "delta")])
    g1, g2 = c["meta"]["g1"], c["meta"]["g2"]
    rs, ss = c["rs"][:1], c["ss"][:1]
    hp, hi, hvk = prove_trapdoor_host(c["r1cs"], c["zs"][0], trap, g1, g2, rs, ss)
    assert Q.proof_blob(hp[0], hi[0]) == Q.proof_blob(*host.proof("Z"))          # the host form is the oracle's proof under the oracle's key

    def good():
        proof, inf, vk = env.dev.prove_trapdoor(env.r1cs("Z"), env.wit("Z"), c["ni"], trap, g1, g2, rs[0], ss[0])
        assert Q.proof_blob(proof, inf) == Q.proof_blob(hp[0], hi[0])
        for k in hvk:
            assert np.array_equal(np.asarray(vk[k]).reshape(-1), np.asarray(hvk[k]).reshape(-1)), k
    good()
    bad = trap.copy()
    bad[0] = fr_mont(pow(7, 5 * (P.R_MOD - 1) // 32, P.R_MOD))
    assert pow(P.fr_from_mont(unlimbs(bad[0])), 32, P.R_MOD) == 1
    assert _status(lambda: env.dev.prove_trapdoor(env.r1cs("Z"), env.wit("Z"), c["ni"], bad, g1, g2, rs[0], ss[0])) == Q.BAD_ARG
    assert "tau" in env.dev.lib.zkg16_last_error(env.dev.ctx).decode()
    good()


def test_after_key_bytes_with_a_point_outside_the_subgroup_are_refused(env, host):
    import pk_bytes_cases as PB
    import pk_check_cases as K
    from zksnark_finalproject_amd import wire
    c = host.circuit("X")
    raw = wire.pk_serialize_compressed(c["pk"], c["vk"])
    sec = PB.sections(c["ni"], c["nv"], c["pk"]["h_query"].shape[0])
    enc = wire.points_compress("g1", K.outside_subgroup("g1").reshape(1, 12))
    tampered = PB.with_point(raw, sec["h_query"], 1500, enc)
    _good(env, host, "pk-save-load-read-X-piece64")
    with Q.options(env.dev, {"pk_bytes_piece": 64}):
        assert _status(lambda: env.dev.pk_load_bytes(tampered, validate=True)) == Q.BAD_ARG
        assert "h_query[1500]" in env.dev.lib.zkg16_last_error(env.dev.ctx).decode()
    _good(env, host, "pk-save-load-read-X-piece64")
    _good(env, host, "pk-check-good-key")


def test_after_a_builder_with_a_null_argument_is_refused(env, host):
    a, b, _ = Q.matrix_requests(host, 8, 6, 806)
    _good(env, host, "witness-matrix-batch-n8-k6-chains-seg4")
    handles, pubs = np.full(6, 0xA5A5, dtype=np.uint64), np.full((6, 3, 4), 0xA5A5, dtype=np.uint64)
    assert env.dev.lib.zkg16_witness_matrix_batch(env.dev.ctx, 8, None, C.c_void_p(b.ctypes.data), 6, handles.ctypes.data, pubs.ctypes.data, None) == Q.BAD_ARG
    assert (handles == 0xA5A5).all() and (pubs == 0xA5A5).all()
    _good(env, host, "witness-matrix-batch-n8-k6")
    _good(env, host, "witness-matrix-batch-n8-k6-chains-seg1")


# ------------------------------------------------------------------------------------------------ d. two lanes, different work
def _prove_rounds(env, host, jobs):
    """jobs: [(circuit, key kind)] — one thread each, three rounds of four proofs, every round started together -> the errors"""
    errors, go = [], threading.Barrier(len(jobs))
    handles = {(circ, kind): (env.key(circ, kind), env.r1cs(circ), [env.wit(circ, i) for i in range(3)]) for circ, kind in jobs}

    def work(circ, kind):
        c = host.circuit(circ)
        ph, rh, whs = handles[(circ, kind)]
        try:
            for _ in range(3):
                go.wait()
                for n in range(4):
                    i = n % 3
                    got = env.dev.prove_resident(ph, rh, whs[i], c["rs"][i], c["ss"][i])
                    if Q.proof_blob(*got) != Q.proof_blob(*host.proof(circ, i)):
                        errors.append((circ, kind, i, "proof differs from the oracle's"))
        except Exception as e:      # noqa: BLE001 - reported on the main thread
            errors.append((circ, kind, e))
            go.abort()
    ts = [threading.Thread(target=work, args=j) for j in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return errors


def test_two_lanes_with_different_domains_then_swapped(env, host):
    """X on its tabled key beside Y on its plain key: two domains, so both lazily built transform table sets are raced for on a
    fresh context; then the circuits change threads and key kinds, and each lane's workspaces meet the other shape"""
    for circ in ("X", "Y"):
        for i in range(3):
            host.proof(circ, i)          # the oracle's proofs, before any thread starts
    assert _prove_rounds(env, host, [("X", "tabled"), ("Y", "plain")]) == []
    lanes = {lane for lane, _, _ in env.dev.lane_log()}
    assert {0, 1} <= lanes, lanes
    assert _prove_rounds(env, host, [("Y", "plain"), ("X", "tabled")]) == []
    assert _prove_rounds(env, host, [("Y", "tabled"), ("X", "plain")]) == []
    # and one thread alone afterwards, on whichever lane it gets
    Q.run_sequence(env, [Q.BY_NAME["prove-resident-Y-plain"], Q.BY_NAME["prove-resident-X-tabled"], Q.BY_NAME["prove-batch-Y-k3"]], host.expected)


# ------------------------------------------------------------------------------------------------ e. blocks that come back uncleared
def test_second_context_after_the_large_shapes(host, cus):
    """The first context runs the 70,000-term G1 and G2 MSMs and a 2^15-domain proof (lists and bucket arrays of several MiB), frees
    its handles and closes; the second runs the same shapes on other data, then the small steps.  zkg16_destroy empties the
    allocation cache, so the second context's blocks come from the runtime, not from the cache: what is held is that nothing
    depends on a fresh context's memory being clear."""
    from zksnark_finalproject_amd import Device
    first = Q.Env(Device(0), host, cus)
    try:
        Q.run_sequence(first, Q.RECYCLED_FIRST, host.expected)
        first.dev.pk_free(first.key("W"))
        first.dev.r1cs_free(first.r1cs("W"))
        first.dev.witness_free(first.wit("W"))
    finally:
        first.dev.close()
    second = Q.Env(Device(0), host, cus)
    try:
        Q.run_sequence(second, Q.RECYCLED_SECOND, host.expected)
    finally:
        second.dev.close()


def test_new_handles_in_blocks_freed_on_a_living_context(env, host):
    """One context: prove W, free its key, system and assignment — the key's queries and the system's arrays are blocks of 1 MiB and
    more, which stay in the allocation cache uncleared — then load handles of the same sizes again, which take those blocks, prove
    another assignment on them, and run small steps in what is left"""
    w0, w1 = Q.RECYCLED_FIRST[2], Q.RECYCLED_SECOND[2]
    c = host.circuit("W")
    assert c["pk"]["a_query"].nbytes > 1 << 20 and c["pk"]["h_query"].nbytes > 1 << 20 and c["r1cs"]["a"][2].nbytes > 1 << 20
    Q.run_sequence(env, [w0], host.expected)
    for _ in range(2):
        env.free("W")
        Q.run_sequence(env, [w1, w0, Q.BY_NAME["prove-resident-X-plain"], Q.BY_NAME["msm-g1-61-c4"], Q.BY_NAME["prove-host-pointers-Z-r0"]], host.expected, before=w0)
