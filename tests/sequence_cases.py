"""Call sequences on one context: a table of steps over every kernel family, and the runner that plays a list of them on a context
and compares EVERY step's bytes with a reference that shares no device code.  Shared by tests/test_call_sequences_host.py (the table
holds what it must, the runner catches a result that depends on its predecessor, the tiny steps agree with the big-integer models)
and tests/test_call_sequences_gpu.py (ordered pairs inside a family, a walk across families, calls after a refusal, two lanes with
different work, contexts whose blocks come back uncleared).

A step is (family, name, the state it dirties or depends on, the path it claims, run(env) -> bytes, expected(host) -> bytes).
`env` is an Env: one context and the handles the steps have loaded on it so far.  `host` is a Host: everything made on the CPU —
circuits, keys, assignments and the expected bytes — computed once per process and never written to.  The expected bytes come from
the CPU oracle (msm through one scalar multiplication of the summed logs, prove, ntt, witness_map), the host forms of the verifiers
and of re-randomisation, and the host builders of the assignments.  Every comparison is byte equality.

The builders are those of msm_limit_cases, msm_tabled_cases, stream_cases, verify_batch_cases, decompress_cases, rerandomize_cases,
u64_verify_cases, prime_verify_cases, sim_proofs, pk_check_cases, linear_cases, linear_general_cases, synth and the system of
test_witness_map_six_gpu; nothing of them is copied here."""
import contextlib
import functools
import random

import numpy as np

import msm_limit_cases as M
import msm_tabled_cases as T
import pyref as P
import stream_cases as S
import synth
from helpers import fr_canon, fr_mont, fr_mont_vec

R = P.R_MOD
NONE = (1 << 64) - 1                          # first_bad of a check that found nothing
UNSATISFIED, BAD_ARG, BAD_HANDLE = 8, 1, 6

# the value that restores each option a step sets
DEFAULTS = {"window_bits": 0, "min_seg": 0, "reduce_mode": 0, "reduce_chunk": 0, "fixup_aux": 0, "g1_waves": 0, "fuse_pointwise": 1,
            "wm_transforms": 6, "matrix_parts": 0, "matrix_slice_min": 0, "check_satisfied": 0, "sponge_chains_min": 0,
            "sponge_chain_segment": 0, "linear_elim_lds_max": 0, "verify_batch_min": 0, "verify_wire_min": 0, "rerandomize_min": 0,
            "pk_bytes_piece": 0, "table_stride": 0}
ALWAYS_DEVICE = {"verify_batch_min": 1, "verify_wire_min": 1, "rerandomize_min": 1}


@contextlib.contextmanager
def options(dev, opts):
    """the options set for the body and put back to their defaults, whatever the body does"""
    try:
        for k, v in opts.items():
            dev.set_option(k, v)
        yield
    finally:
        for k in opts:
            dev.set_option(k, DEFAULTS[k])


def blob(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def point_blob(pt, inf):
    """a point as bytes: the flag, then the limbs — zero limbs for the point at infinity, whatever the buffer held"""
    pt = np.asarray(pt, dtype=np.uint64)
    return bytes([1 if inf else 0]) + (np.zeros_like(pt) if inf else pt).tobytes()


def proof_blob(proof, inf):
    return blob(np.asarray(proof, dtype=np.uint64), np.asarray(inf, dtype=np.uint8))


def verdict_blob(ok, each=None, status=None):
    out = bytes([1 if ok else 0])
    if each is not None:
        out += np.asarray(each, dtype=bool).astype(np.uint8).tobytes()
    if status is not None:
        out += np.asarray(status, dtype=np.uint8).tobytes()
    return out


# ------------------------------------------------------------------------------------------------ steps and the runner
class Step:
    def __init__(self, family, name, state, path, run, expected):
        self.family, self.name, self.state, self.path, self.run, self.expected = family, name, state, path, run, expected

    def __repr__(self):
        return self.name


class SequenceMismatch(AssertionError):
    """a step whose bytes are not the expected ones, with the step before it"""

    def __init__(self, step, before, position, detail):
        self.step, self.before, self.position = step, before, position
        super().__init__("step %d %r after %r: %s" % (position, step, before if before is not None else "a fresh context", detail))


def first_difference(got, want):
    if len(got) != len(want):
        return "%d bytes, expected %d" % (len(got), len(want))
    at = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
    return "%d of %d bytes differ, the first at %d" % (sum(g != w for g, w in zip(got, want)), len(want), at)


def run_sequence(env, steps, expected_of, before=None):
    """Runs the steps in order on env and compares every step's bytes with expected_of(step); no step is skipped or tried again.
    A mismatch, a path a step does not find itself on, or any exception of a step raises SequenceMismatch naming the step and its predecessor (`before`: the
    step that ran last on env before this call, for a sequence played in pieces)."""
    for position, step in enumerate(steps):
        try:
            got = step.run(env)
        except SequenceMismatch:
            raise
        except AssertionError as e:
            raise SequenceMismatch(step, before, position, "path: %s" % (e,)) from e
        except Exception as e:      # noqa: BLE001 - a refusal by the library (Zkg16Error) is how stale state may surface: it names the pair too
            raise SequenceMismatch(step, before, position, "raised %s: %s" % (type(e).__name__, e)) from e
        want = expected_of(step)
        if got != want:
            raise SequenceMismatch(step, before, position, first_difference(got, want))
        before = step
    return len(steps)


class Env:
    """One context and what the steps have loaded on it; `cus` its compute units (the lane counts behind seg_len)."""

    def __init__(self, dev, host, cus):
        self.dev, self.host, self.cus = dev, host, cus
        self._held = {}

    def get(self, key, make):
        if key not in self._held:
            self._held[key] = make()
        return self._held[key]

    def free(self, name):
        """frees every handle of a circuit loaded so far: the next step that needs one loads it again"""
        for key in [k for k in self._held if isinstance(k, tuple) and k[0] in ("r1cs", "wit", "key") and k[1] == name]:
            h = self._held.pop(key)
            {"r1cs": self.dev.r1cs_free, "wit": self.dev.witness_free, "key": self.dev.pk_free}[key[0]](h)

    # handles of the proof circuits
    def r1cs(self, name):
        c = self.host.circuit(name)
        return self.get(("r1cs", name), lambda: self.dev.r1cs_load(c["r1cs"], c["nv"]))

    def wit(self, name, i=0):
        c = self.host.circuit(name)
        return self.get(("wit", name, i), lambda: self.dev.witness_load(c["zs"][i]))

    def key(self, name, kind="plain"):
        c = self.host.circuit(name)

        def make():
            ph = self.dev.pk_load(c["pk"], c["ni"])
            if kind == "tabled":
                self.dev.pk_precompute(ph, 12, 10)
                assert self.dev.pk_table_bits(ph) == (12, 10)
            return ph
        return self.get(("key", name, kind), make)


# ------------------------------------------------------------------------------------------------ what the CPU makes, once
# W is not in the table: the proof of the large-shapes tests, its bucket arrays and term lists above 1 MiB on both sides
CIRCUITS = {"X": (1200, 3, 1000), "Y": (3000, 3, 2500), "Z": (17, 3, 9), "W": (20000, 3, 17000)}
DOMAIN_LOG = {"X": 11, "Y": 12, "Z": 5, "W": 15}
EXTRA_ASSIGNMENTS = {"X": 32, "Y": 2, "Z": 0, "W": 1}          # random ones behind the satisfying one: a proof is a function of (z, r, s)


class Host:
    def __init__(self, oracle):
        self.oracle = oracle
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def expected(self, step):
        return self.once(("expected", step.name), lambda: step.expected(self))

    def vk_of(self, pk, meta):
        o = self.oracle
        gabc, ginf = o.fixed_base("g1", meta["g1"], o.fr_to_canonical(meta["logs"]["gabc"]))
        gabc[ginf != 0] = 0
        gamma_g2 = o.point_mul("g2", meta["g2"], fr_canon(meta["trap"]["gamma"]))[0]
        return dict(alpha_g1=pk["alpha_g1"], beta_g2=pk["beta_g2"], gamma_g2=gamma_g2, delta_g2=pk["delta_g2"], gamma_abc_g1=gabc)

    def keyed(self, r1cs, nv, rng):
        """a known-trapdoor key for the system from the oracle, a point at infinity as zero limbs (what the device writes)"""
        pk, meta = synth.make_pk(self.oracle, r1cs, nv, rng)
        for q in ("a", "b_g1", "b_g2", "h", "l"):
            pk[q + "_query"][pk[q + "_inf"] != 0] = 0
        return pk, meta, self.vk_of(pk, meta)

    def system(self, name):
        """the random satisfiable system of a circuit and its satisfying assignment (no key yet)"""
        def make():
            nc, ni, nv = CIRCUITS[name]
            rng = random.Random("sequence/" + name)
            A, B, C, z = synth.random_r1cs(rng, nc, ni, nv)
            assert (nc + ni - 1).bit_length() == DOMAIN_LOG[name]
            return dict(A=A, B=B, C=C, z=z, r1cs=synth.r1cs_arrays(A, B, C, ni), rng=rng)
        return self.once(("system", name), make)

    def circuit(self, name):
        def make():
            nc, ni, nv = CIRCUITS[name]
            sy = self.system(name)
            A, B, C, z, r1cs, rng = (sy[k] for k in ("A", "B", "C", "z", "r1cs", "rng"))          # the key's draws follow the system's
            pk, meta, vk = self.keyed(r1cs, nv, rng)
            nrng = np.random.default_rng(len(name) + nc)
            zs = [fr_mont_vec(z)]
            for _ in range(EXTRA_ASSIGNMENTS[name]):
                zz = nrng.integers(0, 1 << 62, size=(nv, 4), dtype=np.uint64)
                zz[0] = fr_mont(1)
                zs.append(zz)
            z_bad = zs[0].copy()
            z_bad[int(r1cs["c"][1][0])] = fr_mont(z[int(r1cs["c"][1][0])] + 1)          # a variable of C's first row
            for arr in zs + [z_bad]:
                arr.setflags(write=False)
            rs = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(len(zs))])
            ss = np.stack([fr_mont(P.rand_fr(rng)) for _ in range(len(zs))])
            return dict(name=name, A=A, B=B, C=C, z=z, r1cs=r1cs, ni=ni, nv=nv, pk=pk, meta=meta, vk=vk, zs=zs, z_bad=z_bad, rs=rs, ss=ss)
        return self.once(("circuit", name), make)

    def proof(self, name, i=0, r=None, s=None):
        """the oracle's proof of assignment i of a circuit under (r, s), by default the circuit's own pair i"""
        c = self.circuit(name)
        r = c["rs"][i] if r is None else r
        s = c["ss"][i] if s is None else s
        return self.once(("proof", name, i, blob(r, s)), lambda: self.oracle.prove(c["pk"], r, s, c["r1cs"], c["zs"][i]))


_hosts = {}


def host_of(oracle):
    if id(oracle) not in _hosts:
        _hosts[id(oracle)] = Host(oracle)
    return _hosts[id(oracle)]


# ================================================================================================ MSM, through dev.msm
def _lists(key, n):
    """n scalars below r and n indices into the 64 points of msm_limit_cases, by name: steps that say `the same terms` share a key"""
    rng = random.Random("sequence/msm/" + key)
    return [rng.randrange(R) for _ in range(n)], [rng.randrange(64) for _ in range(n)]


# name -> group, window bits (0: the default for the length, claimed as `c`), terms, the list's key, options, and the claims
MSM_SPECS = {
    "msm-g1-61-c4": dict(group="g1", c=4, n=61, data="61"),
    "msm-g1-5000-c9": dict(group="g1", c=9, n=5000, data="5000"),
    "msm-g1-70000-c13": dict(group="g1", c=13, n=70000, data="70000", default_bits=True, bit_sliced=True),
    "msm-g1-70000-reduce4": dict(group="g1", c=13, n=70000, data="70000", options={"reduce_mode": 4}, mode=4),
    "msm-g1-70000-reduce5": dict(group="g1", c=13, n=70000, data="70000", options={"reduce_mode": 5}, bit_sliced=True),
    "msm-g1-70000-equal": dict(group="g1", c=13, n=70000, data="70000", equal=True, chains=True),
    "msm-g1-70000-equal-fixup-aux": dict(group="g1", c=13, n=70000, data="70000", equal=True, chains=True, options={"fixup_aux": 1}),
    "msm-g1-3000-minseg1": dict(group="g1", c=8, n=3000, data="3000", min_seg=1),
    "msm-g1-3000-zero": dict(group="g1", c=8, n=3000, data="3000", zero=True),
    "msm-g1-empty": dict(group="g1", c=8, n=0, data="0"),
    "msm-g1-70000-waves4": dict(group="g1", c=13, n=70000, data="70000", options={"g1_waves": 4}, waves=4),
    "msm-g1-70000-waves1": dict(group="g1", c=13, n=70000, data="70000", options={"g1_waves": 1}, waves=1),
    "msm-g2-3000": dict(group="g2", c=8, n=3000, data="3000", default_bits=True),
    "msm-g2-70000-c9": dict(group="g2", c=9, n=70000, data="70000"),
}


# the same shapes on other data: what the second context of the large-shapes test runs first (not in the table)
OTHER_DATA_SPECS = {
    "msm-g1-70000-c13-other-data": dict(group="g1", c=13, n=70000, data="70000-other", default_bits=True, bit_sliced=True),
    "msm-g2-70000-c9-other-data": dict(group="g2", c=9, n=70000, data="70000-other"),
}
ALL_MSM_SPECS = dict(MSM_SPECS, **OTHER_DATA_SPECS)


@functools.lru_cache(maxsize=None)
def msm_case(name):
    sp = ALL_MSM_SPECS[name]
    scalars, idx = _lists(sp["data"], sp["n"])
    if sp.get("equal"):
        scalars = [scalars[0]] * len(scalars)
    if sp.get("zero"):
        scalars = [0] * len(scalars)
    case = M.Case(name, sp["group"], sp["c"], scalars, idx, options=sp.get("options"), min_seg=sp.get("min_seg", 0))
    if sp.get("default_bits"):
        del case.options["window_bits"]          # the width the library picks for this length must be the one claimed
    return case


def msm_state(name, cus):
    """what zkg16_last_msm_state must report for the step (None: not asserted)"""
    sp, case = ALL_MSM_SPECS[name], msm_case(name)
    c, nwin = case.c, M.nwin_of(case.c)
    if case.entries == 0:
        return (c, nwin, 0, None, 0, 0, None, None)
    terms = len(case.scalars) * nwin
    lanes_g1 = 4 * cus * sp.get("waves", 2) * 64
    seg = M.seg_lens(case.entries, len(case.counts), lanes_g1, M.lanes("g2", cus, terms), case.min_seg)[0 if case.group == "g1" else 1]
    items, chains = M.fixup_queue(case.counts, seg)
    bs, k2 = M.reduce_state(c, sp["mode"], 0) if "mode" in sp else (None, None)
    return (c, nwin, case.entries, seg, items, chains, bs, k2)


def _msm_path(name):
    sp = ALL_MSM_SPECS[name]
    words = ["%s c%d n%d" % (sp["group"], sp["c"], sp["n"])]
    words += ["%s=%s" % kv for kv in sorted(sp.get("options", {}).items())]
    words += [w for w in ("equal", "zero", "bit_sliced", "chains") if sp.get(w)]
    if sp.get("min_seg"):
        words.append("min_seg=%d" % sp["min_seg"])
    return " ".join(words)


def _msm_step(name):
    sp = ALL_MSM_SPECS[name]

    def run(env):
        case = msm_case(name)
        bases, sc = env.host.once(("msm-arrays", name), lambda: case.arrays(env.host.oracle))
        with options(env.dev, case.options):
            got, ginf = env.dev.msm(case.group, bases, sc)
            state = env.dev.last_msm_state()
            waves = env.dev.last_acc_waves()
        want = msm_state(name, env.cus)
        assert M.state_matches(state, want), (state, want)
        # dev.msm plans on ws_h: the G1 lanes its plan asked for, in waves per SIMD (0: no list was planned)
        assert waves[2] == (sp.get("waves", 2) if sp["n"] else 0), (waves, sp.get("waves", 2))
        if sp.get("bit_sliced"):
            assert state[6] > 0, state
        if sp.get("chains"):
            assert state[4] > 0 and state[5] > 0, state
        return point_blob(got, ginf)

    def expected(host):
        pt, inf = msm_case(name).expected(host.oracle)
        return point_blob(pt, inf)
    state = ("ws_h + slots[0] at %d-byte entries; fix-up queue, seg_meta, buckets" % (224 if sp["group"] == "g1" else 448))
    return Step("msm", name, state, _msm_path(name), run, expected)


TABLED = {"msm-tabled-g1-c20-packed": ("g1", 20, 1), "msm-tabled-g1-c21-padded": ("g1", 21, 2)}


@functools.lru_cache(maxsize=None)
def tabled_case(name):
    return T.digit_case(*TABLED[name])


def _tabled_step(name):
    group, c, stride = TABLED[name]

    def run(env):
        case = tabled_case(name)
        bases, inf, sc = case.arrays(env.host.oracle)
        with options(env.dev, case.options):
            got, ginf = env.dev.diag_msm_tabled(case.group, bases, sc, case.c, case.stride, case.last, inf if inf.any() else None)
            state = env.dev.last_msm_state()
        want = case.state(env.cus)
        assert M.state_matches(state, want), (state, want)
        return b"".join(point_blob(got[v], ginf[v]) for v in range(case.batch))

    def expected(host):
        return b"".join(point_blob(pt, inf) for pt, inf in tabled_case(name).expected(host.oracle))
    path = "%s tabled c%d stride%d %s-pass scatter" % (group, c, stride, "two" if c <= 20 else "three")
    return Step("msm", name, "ws_h + slots[0] as ONE bucket set of 2^%d; a table of its own" % (c - 1), path, run, expected)


# ================================================================================================ transforms and the witness map
NTT_LOGS = (4, 11, 12, 16)
NTT_FORMS = {"inv": (True, False), "coset": (False, True), "coset-inv": (True, True)}          # the three the witness map runs


def ntt_input(log_n):
    rng = np.random.default_rng(9000 + log_n)
    a = rng.integers(0, 1 << 62, size=(1 << log_n, 4), dtype=np.uint64)          # below 2^254 < 2 r: any residue's Montgomery form
    a.setflags(write=False)
    return a


def _ntt_step(log_n, form):
    inverse, coset = NTT_FORMS[form]
    name = "ntt-2^%d-%s" % (log_n, form)

    def run(env):
        data = env.host.once(("ntt-in", log_n), lambda: ntt_input(log_n))
        return blob(env.dev.ntt(data, inverse, coset))

    def expected(host):
        data = host.once(("ntt-in", log_n), lambda: ntt_input(log_n))
        return blob(host.oracle.ntt(data, inverse, coset))
    plan = "single tile" if log_n <= 11 else "two-pass"
    return Step("transform", name, "poly[0]; the lazily built table set of 2^%d" % log_n, "%s %s" % (plan, form), run, expected)


WM_VARIANTS = [(which, t, fuse) for which in ("satisfied", "unsatisfied") for t in (6, 7) for fuse in (1, 0)]


def wm_system(host, log_n):
    """test_witness_map_six_gpu's system of that domain: (r1cs, nv, {name: assignment}, {name: the oracle's h})"""
    def make():
        from test_witness_map_six_gpu import numpy_r1cs
        r1cs, zs, nv = numpy_r1cs(host.oracle, log_n, 600 + log_n)
        names = ("satisfied", "unsatisfied")
        want = {}
        for name, zm in zip(names, zs):
            zm.setflags(write=False)
            want[name] = host.oracle.witness_map(r1cs, zm)
            assert want[name].shape[0] == 1 << log_n and bool(want[name][-1].any()) == (name == "unsatisfied")
        return r1cs, nv, dict(zip(names, zs)), want
    return host.once(("wm", log_n), make)


def _wm_step(log_n, which, transforms, fuse):
    name = "wm-2^%d-%s-t%d-fuse%d" % (log_n, which, transforms, fuse)

    def run(env):
        r1cs, nv, zs, _ = wm_system(env.host, log_n)
        rh = env.get(("wm-r1cs", log_n), lambda: env.dev.r1cs_load(r1cs, nv))
        wh = env.get(("wm-wit", log_n, which), lambda: env.dev.witness_load(zs[which]))
        with options(env.dev, {"wm_transforms": transforms, "fuse_pointwise": fuse}):
            return blob(env.dev.witness_map(rh, wh, 1 << log_n))

    def expected(host):
        return blob(wm_system(host, log_n)[3][which])
    plan = "single tile" if log_n <= 11 else "two-pass"
    return Step("transform", name, "poly[0..3]: the last store reads the subtrahend it overwrites", "%s %s wm%d fuse%d" % (plan, which, transforms, fuse),
                run, expected)


# ================================================================================================ proofs
def _assert_proof_path(env):
    """the last proof built a z list and an h list, and its G1 accumulations ran two (or, from 2^25 terms, four) waves per SIMD"""
    z, b, h = env.dev.last_term_counts()
    assert z > 0 and h > 0, (z, b, h)
    waves = env.dev.last_acc_waves()
    assert waves[0] in (2, 4) and waves[2] in (2, 4), waves


def _resident_step(circ, kind, i=0):
    name = "prove-resident-%s-%s" % (circ, kind) + ("-assignment%d" % i if i else "")

    def run(env):
        c = env.host.circuit(circ)
        ph, rh, wh = env.key(circ, kind), env.r1cs(circ), env.wit(circ, i)
        got = env.dev.prove_resident(ph, rh, wh, c["rs"][i], c["ss"][i])
        _assert_proof_path(env)
        assert env.dev.pk_table_bits(ph) == ((12, 10) if kind == "tabled" else (0, 0))
        return proof_blob(*got)
    return Step("proof", name, "ws_z / ws_zb / ws_h, five slots, poly[0..3] at 2^%d" % DOMAIN_LOG[circ],
                "%s key, domain 2^%d" % (kind, DOMAIN_LOG[circ]), run, lambda host: proof_blob(*host.proof(circ, i)))


def _prove_host_pointers_step():
    zero = fr_mont(0)

    def run(env):
        c = env.host.circuit("Z")
        got = env.dev.prove(env.key("Z"), zero, c["ss"][0], c["r1cs"], c["zs"][0])
        _assert_proof_path(env)
        return proof_blob(*got)
    return Step("proof", "prove-host-pointers-Z-r0", "every workspace at its smallest; the matrices uploaded for the call", "host pointers, domain 2^5, r = 0",
                run, lambda host: proof_blob(*host.proof("Z", 0, r=zero)))


def _batch_step(circ, k):
    name = "prove-batch-%s-k%d" % (circ, k)

    def run(env):
        c = env.host.circuit(circ)
        whs = np.array([env.wit(circ, i) for i in range(k)], dtype=np.uint64)
        proofs, inf = env.dev.prove_batch(env.key(circ), env.r1cs(circ), whs, c["rs"][:k], c["ss"][:k])
        z, _, h = env.dev.last_term_counts()
        assert z > 0 and h > 0
        return proof_blob(proofs, inf)

    def expected(host):
        got = [host.proof(circ, i) for i in range(k)]
        return proof_blob(np.stack([p for p, _ in got]), np.stack([f for _, f in got]))
    sets = k * 32
    return Step("proof", name, "K proofs as windows of one list: %d bucket sets; poly[] at K vectors" % sets,
                "batch k=%d, %s" % (k, "prefix path (more than 32 sets of one proof's windows)" if k > 32 else "window bases in one block"), run, expected)


def _partial_step():
    def run(env):
        c = env.host.circuit("X")
        ph, rh, wh = env.key("X"), env.r1cs("X"), env.wit("X")
        nv, n_h = c["nv"], c["pk"]["h_query"].shape[0]
        parts, pinf = [], []
        for z_lo, z_hi, h_lo, h_hi, blind in ((0, nv // 2, 0, 0, True), (nv // 2, nv, 0, n_h, False)):          # the first shard's h range is empty
            sh = env.dev.pk_slice(ph, z_lo, z_hi, h_lo, h_hi, blind)
            try:
                p, f = env.dev.prove_partial(sh, rh, wh, c["rs"][0], c["ss"][0])
                z, _, h = env.dev.last_term_counts()
            finally:
                env.dev.pk_free(sh)
            assert z > 0 and (h == 0) == (h_hi == h_lo), (z, h, h_lo, h_hi)          # no h list for the shard without an h range
            parts.append(p)
            pinf.append(f)
        return proof_blob(*env.dev.prove_finish(ph, c["rs"][0], c["ss"][0], np.array(parts), np.array(pinf)))
    return Step("proof", "prove-partial-empty-h-then-finish", "a shard without an h list: ws_h and its slot are not touched by the first partial",
                "two shards, h range empty in the first", run, lambda host: proof_blob(*host.proof("X")))


MATRIX_N = 8


def matrix_request(host):
    """one request of the matrix handler at n = 8 with a host-made key: the circuit's own synthesis, the oracle's proof"""
    def make():
        from zksnark_finalproject_amd.circuits import matrix_circuit
        rng = np.random.default_rng(8008)
        a = rng.integers(0, 1 << 63, size=(MATRIX_N, MATRIX_N), dtype=np.uint64)
        b = rng.integers(0, 1 << 63, size=(MATRIX_N, MATRIX_N), dtype=np.uint64)
        c = matrix_circuit(a, b)
        assert c.num_vars == S.Layout(MATRIX_N).total and c.num_instance == 4
        prng = random.Random(8008)
        pk, meta, vk = host.keyed(c.r1cs, c.num_vars, prng)
        r, s = fr_mont(P.rand_fr(prng)), fr_mont(P.rand_fr(prng))
        z = np.ascontiguousarray(c.z, dtype=np.uint64).reshape(-1, 4)
        want = host.oracle.prove(pk, r, s, c.r1cs, z)
        return dict(a=a, b=b, pk=pk, r=r, s=s, pub=z[1:4].copy(), want=want)
    return host.once("matrix-request", make)


def _matrix_step(parts):
    name = "prove-matrix-n8-%s" % ("streamed-parts3" if parts == 3 else "unstreamed")

    def run(env):
        m = matrix_request(env.host)
        rh = env.get("matrix-r1cs", lambda: env.dev.r1cs_matrix(MATRIX_N))
        ph = env.get("matrix-key", lambda: env.dev.pk_load(m["pk"], 4))
        with options(env.dev, {"matrix_parts": parts, "matrix_slice_min": 1}):
            proof, inf, pub, ms = env.dev.prove_matrix(ph, rh, m["a"], m["b"], m["r"], m["s"])
        bounds = S.slice_bounds(S.Layout(MATRIX_N).perms, parts, 1)
        assert ms["parts"] == len(bounds), (ms, bounds)          # parts 1: two rounds, the assignment first
        z, _, h = env.dev.last_term_counts()
        assert z > 0 and h > 0, (z, h)
        assert np.array_equal(pub, m["pub"])
        return proof_blob(proof, inf)
    state = "bucket_sum plus the merge into buckets, round after round" if parts == 3 else "the assignment first, then one round"
    return Step("proof", name, state, "matrix_parts %d" % parts, run, lambda host: proof_blob(*matrix_request(host)["want"]))


def _checked_step():
    def run(env):
        c = env.host.circuit("X")
        with options(env.dev, {"check_satisfied": 1}):
            got = env.dev.prove_resident(env.key("X"), env.r1cs("X"), env.wit("X"), c["rs"][0], c["ss"][0])
            assert env.dev.last_check() == [(0, NONE)]
        return proof_blob(*got)
    return Step("proof", "prove-resident-X-check-satisfied", "check_dev: the verdict words of the call", "check_satisfied 1, satisfied",
                run, lambda host: proof_blob(*host.proof("X")))


# ================================================================================================ builders
def matrix_requests(host, n, k, seed):
    def make():
        from zksnark_finalproject_amd.circuits import matrix_witness
        rng = np.random.default_rng(seed)
        draw = lambda: rng.integers(0, 1 << 63, size=(k, n, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(k, n, n), dtype=np.uint64)
        a, b = draw(), draw()
        a[0] = b[0] = np.uint64(0xFFFFFFFFFFFFFFFF)          # c's entries need the third limb
        zs = [matrix_witness(a[i], b[i], S.Layout(n).total) for i in range(k)]
        return a, b, zs
    return host.once(("matrix-requests", n, k, seed), make)


def _read_and_free(env, handles, nv):
    out = []
    try:
        for h in handles:
            out.append(env.dev.witness_read(int(h), nv))
    finally:
        for h in handles:
            env.dev.witness_free(int(h))
    return out


def _witness_matrix_step(n, k, chains_segment=None):
    seg = "" if chains_segment is None else "-chains-seg%d" % chains_segment
    name = "witness-matrix-batch-n%d-k%d%s" % (n, k, seg)
    opts = {} if chains_segment is None else {"sponge_chains_min": 1, "sponge_chain_segment": chains_segment}

    def run(env):
        a, b, _ = matrix_requests(env.host, n, k, 100 * n + k)
        with options(env.dev, opts):
            handles, pubs, ms = env.dev.witness_matrix_batch(a, b)
        assert (ms["host_sponges_ms"] == 0) == (chains_segment is not None), ms          # who walked the chains
        return blob(*_read_and_free(env, handles, S.Layout(n).total)) + blob(pubs)

    def expected(host):
        _, _, zs = matrix_requests(host, n, k, 100 * n + k)
        return blob(*zs) + blob(np.stack([z[1:4] for z in zs]))
    state = "mbatch_dev staging" + ("" if chains_segment is None else "; the chains' `state` carried between launches of %d permutations" % chains_segment)
    path = "chains on %s" % ("the host" if chains_segment is None else "the device, %d permutations a launch" % chains_segment)
    return Step("builder", name, state, "n%d k%d %s" % (n, k, path), run, expected)


FIB_STEPS = 12


def _witness_fibonacci_step(k):
    def requests():
        rng = random.Random(4040)
        pairs = [((1 << 64) - 1, (1 << 64) - 1), (0, 0), (0, 1)] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(62)]
        return np.array([p[0] for p in pairs[:k]], dtype=np.uint64), np.array([p[1] for p in pairs[:k]], dtype=np.uint64)

    def run(env):
        a, b = requests()
        handles, pubs, _ = env.dev.witness_fibonacci_batch(FIB_STEPS, a, b)
        return blob(*_read_and_free(env, handles, 5)) + blob(pubs)

    def expected(host):
        from zksnark_finalproject_amd.circuits import fibonacci_circuit
        a, b = requests()
        zs = [np.ascontiguousarray(fibonacci_circuit(int(a[i]), int(b[i]), FIB_STEPS).z, dtype=np.uint64).reshape(5, 4) for i in range(k)]
        return blob(*zs) + blob(np.stack([z[1:4] for z in zs]))
    return Step("builder", "witness-fibonacci-batch-k%d" % k, "mbatch_dev staging: one lane per request", "k%d: %s" % (k, "a wave and one lane" if k > 64 else "one lane"),
                run, expected)


LINEAR_N = 8


def _witness_linear_step(solver):
    def requests(host):
        def make():
            import linear_cases as LC
            import linear_general_cases as LG
            from zksnark_finalproject_amd.circuits import linear_circuit
            if solver == "forward":
                a, b = LC.lower_requests(LINEAR_N, 3, seed=88)
                xs = np.stack([LC.mont_limbs(LC.solve(a[i], b[i])) for i in range(3)])
            else:
                cases = LG.solvable(LINEAR_N)[:3]
                a, b, xs = (np.stack([c[j] for c in cases]) for j in (1, 2, 3))
            zs = [np.ascontiguousarray(linear_circuit(a[i], b[i], solver=solver).z, dtype=np.uint64).reshape(-1, 4) for i in range(len(a))]
            return a, b, xs, zs
        return host.once(("linear", solver), make)

    def run(env):
        a, b, _, zs = requests(env.host)
        with options(env.dev, {"linear_elim_lds_max": 3}):
            handles, x, _ = env.dev.witness_linear_batch(a, b, solver=solver)
        return blob(*_read_and_free(env, handles, zs[0].shape[0])) + blob(x)

    def expected(host):
        _, _, xs, zs = requests(host)
        return blob(*zs) + blob(xs)
    where = "the working matrix in the global workspace" if solver == "elimination" else "forward substitution, a wave per request"
    return Step("builder", "witness-linear-batch-n8-%s" % solver, "mbatch_dev staging" + ("; the elimination workspace" if solver == "elimination" else ""),
                "n8 %s: %s" % (solver, where), run, expected)


PRIME_CANDIDATES = {"j0": (0x123456789ABCDEF, 0), "j3": (12345, 3)}          # the patched coefficients: n in A, -j in C (absent at j = 0)


def _witness_prime_step(which):
    x, j = PRIME_CANDIDATES[which]

    def run(env):
        from zksnark_finalproject_amd.circuits import prime_dims
        d = prime_dims(j)
        wh = env.dev.witness_prime(x, j)
        try:
            return blob(env.dev.witness_read(wh, d["num_instance"] + d["num_witness"]))
        finally:
            env.dev.witness_free(wh)

    def expected(host):
        from zksnark_finalproject_amd.circuits import prime_witness_host
        return blob(prime_witness_host(x, j))
    return Step("builder", "witness-prime-%s" % which, "prime_dev: the resident program and its scratch", "witness program, j %s" % ("= 0" if j == 0 else ">= 1"),
                run, expected)


def _r1cs_blob(r1cs, nv):
    return blob(np.array([r1cs["num_inputs"], r1cs["num_constraints"], nv], dtype=np.uint64),
                *[np.asarray(r1cs[m][i]) for m in "abc" for i in range(3)])


def _r1cs_prime_step(which):
    x, j = PRIME_CANDIDATES[which]

    def run(env):
        rh = env.dev.r1cs_prime(x, j)
        try:
            got, nv = env.dev.r1cs_read(rh)
        finally:
            env.dev.r1cs_free(rh)
        return _r1cs_blob(got, nv)

    def expected(host):
        from zksnark_finalproject_amd.circuits import prime_r1cs_host
        r1cs, nw = prime_r1cs_host(x, j)
        return _r1cs_blob(r1cs, r1cs["num_inputs"] + nw)
    return Step("builder", "r1cs-prime-%s" % which, "prime_dev: the resident template, four patched non-zeros", "template patch, j %s" % ("= 0" if j == 0 else ">= 1"),
                run, expected)


def _setup_step(circ):
    def run(env):
        from zksnark_finalproject_amd import wire
        c = env.host.circuit(circ)
        t = c["meta"]["trap"]
        trap = fr_mont_vec([t[k] for k in ("tau", "alpha", "beta", "gamma", "delta")])
        ph, vk = env.dev.setup_resident(env.r1cs(circ), c["ni"], trap, c["meta"]["g1"], c["meta"]["g2"])
        try:
            pk = env.dev.pk_read(ph)
        finally:
            env.dev.pk_free(ph)
        return wire.pk_serialize_compressed(pk, vk)

    def expected(host):
        from zksnark_finalproject_amd import wire
        c = host.circuit(circ)
        return wire.pk_serialize_compressed(c["pk"], c["vk"])
    return Step("builder", "setup-resident-%s" % circ, "the fixed-base cache, sums, prefix products and canonical scalars of setup",
                "setup at domain 2^%d" % DOMAIN_LOG[circ], run, expected)


# ================================================================================================ the verification side
VERIFY_K = 65


def verify_batch_of(host, k=VERIFY_K):
    """k valid proofs of one key: eight proved by the oracle, the others re-randomised from them; multipliers from a seed"""
    def make():
        import verify_batch_cases as VB
        b = VB.rerandomised(host.oracle, VB.make_batch(host.oracle, 8), k, random.Random(650))
        return b, VB.draw_rho(random.Random(651), k)
    return host.once(("verify-batch", k), make)


def _verify_valid_step(k):
    def run(env):
        b, rho = verify_batch_of(env.host)
        with options(env.dev, ALWAYS_DEVICE):
            ok = env.dev.verify_batch(b.pvk, b.pubs[:k], b.proofs[:k], b.infs[:k], rho=rho[:k])
            assert env.dev.verify_batch_timings()["host_form"] == 0
        return verdict_blob(ok)

    def expected(host):
        b, _ = verify_batch_of(host)
        return verdict_blob(bool(b.head(k).loop().all()))
    return Step("verify", "verify-batch-k%d-valid" % k, "the verify scratch: Miller values, the product tree, the MSM", "k%d all valid: one range test" % k, run, expected)


def _verify_tampered_step():
    at = 40

    def batch(host):
        import verify_batch_cases as VB
        b, rho = verify_batch_of(host)
        return host.once("verify-tampered", lambda: VB.tamper(host.oracle, b, "c_plus_g", (at,))), rho

    def run(env):
        b, rho = batch(env.host)
        with options(env.dev, ALWAYS_DEVICE):
            ok, each = env.dev.verify_batch(b.pvk, b.pubs, b.proofs, b.infs, rho=rho, each=True)
            assert env.dev.verify_batch_timings()["host_form"] == 0
        return verdict_blob(ok, each)

    def expected(host):
        each = batch(host)[0].loop()
        assert list(np.flatnonzero(~each)) == [at]
        return verdict_blob(False, each)
    return Step("verify", "verify-batch-k65-one-tampered-each", "the verify scratch, then bisecting over ranges of it", "k65 one tampered, each: bisecting", run, expected)


def wire_batch(host):
    """the K = 65 batch as bytes with the hostile encodings of decompress_cases planted in A, B and C -> (bytes, who decodes, statuses)"""
    def make():
        import decompress_cases as DC
        import verify_batch_cases as VB
        b, _ = verify_batch_of(host)
        raw = VB.to_wire(b)
        g1 = {n: e for n, (e, _) in DC.hostile("g1", raw[0, 0:48].tobytes()).items()}
        g2 = {n: e for n, (e, _) in DC.hostile("g2", raw[0, 48:144].tobytes()).items()}
        plant = {7: (48, g2["infinity_stray_byte"]), 63: (144, g1["x_is_q"]), 64: (0, g1["no_point"]), 20: (48, g2["no_point"]), 33: (48, g2["c0_is_q"]),
                 41: (144, g1["infinity_with_sign"])}
        for i, (off, enc) in plant.items():
            raw[i, off:off + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
        st = np.stack([DC.host_decode("g1", raw[:, 0:48].tobytes(), True)[2], DC.host_decode("g2", raw[:, 48:144].tobytes(), True)[2],
                       DC.host_decode("g1", raw[:, 144:192].tobytes(), True)[2]], axis=1).astype(np.uint8)
        assert sorted(np.flatnonzero(st.any(axis=1))) == sorted(plant)
        return raw, st
    return host.once("wire-batch", make)


def _verify_wire_step():
    def run(env):
        b, rho = verify_batch_of(env.host)
        raw, _ = wire_batch(env.host)
        with options(env.dev, ALWAYS_DEVICE):
            ok, each, st = env.dev.verify_batch_wire(b.pvk, b.pubs, raw, rho=rho, each=True, status=True)
            assert env.dev.verify_batch_timings()["host_form"] == 0
        return verdict_blob(ok, each, st)

    def expected(host):
        b, _ = verify_batch_of(host)
        _, st = wire_batch(host)
        each = b.loop() & ~st.any(axis=1)          # the proofs are valid: one that decodes verifies, one that does not counts as invalid
        return verdict_blob(False, each, st)
    return Step("verify", "verify-batch-wire-k65-hostile", "the decode scratch in front of the verify scratch", "k65 wire, six undecodable proofs", run, expected)


def u64_sim(host):
    def make():
        import sim_proofs
        import u64_verify_cases as U
        import verify_batch_cases as VB
        from zksnark_finalproject_amd.device import verify_batch_u64_host
        k = 66
        sim = U.U64Sim(host.oracle, 12, k, sim_proofs.spread(k), 6600)
        rho = VB.draw_rho(random.Random(6601), k)
        want = verify_batch_u64_host(sim.batch.pvk, sim.values, sim.batch.proofs, sim.batch.infs, rho=rho, each=True)
        assert np.array_equal(want[1], sim.want)
        return sim, rho, want
    return host.once("u64-sim", make)


def _verify_u64_step():
    def run(env):
        sim, rho, _ = u64_sim(env.host)
        b = sim.batch
        with options(env.dev, ALWAYS_DEVICE):
            ok, each = env.dev.verify_batch_u64(b.pvk, sim.values, b.proofs, b.infs, rho=rho, each=True)
            assert env.dev.verify_batch_timings(u64=True)["host_form"] == 0
        return verdict_blob(ok, each)
    return Step("verify", "verify-batch-u64-k66", "the u64 sums and X scratch beside the verify scratch", "u64 inputs, negatives spread: per-proof pass",
                run, lambda host: verdict_blob(*u64_sim(host)[2]))


def prime_sim(host):
    def make():
        import prime_verify_cases as PV
        import sim_proofs
        import verify_batch_cases as VB
        from zksnark_finalproject_amd.device import verify_prime_batch_host
        k = 66
        sim = PV.PrimeSim(host.oracle, 2601)
        claims = sim.negatives([sim.valid(x, j) for x, j in PV.sim_pairs(k, seed=k)], [5, 64])          # one in each wave: few range tests
        b, xs, js, want = sim.batch(claims)
        rho = VB.draw_rho(random.Random(6602), k)
        host_says = verify_prime_batch_host(b.pvk, xs, js, b.proofs, b.infs, rho=rho, each=True)
        assert np.array_equal(host_says[1], want)
        return b, xs, js, rho, host_says
    return host.once("prime-sim", make)


def _verify_prime_step():
    def run(env):
        b, xs, js, rho, _ = prime_sim(env.host)
        with options(env.dev, ALWAYS_DEVICE):
            ok, each = env.dev.verify_prime_batch(b.pvk, xs, js, b.proofs, b.infs, rho=rho, each=True)
            assert env.dev.verify_batch_timings()["host_form"] == 0
        return verdict_blob(ok, each)
    return Step("verify", "verify-prime-batch-k66", "the prime inputs and sums scratch beside the verify scratch", "prime form, 259 inputs from 16 bytes",
                run, lambda host: verdict_blob(*prime_sim(host)[4]))


def rerandomize_table(host):
    def make():
        import rerandomize_cases as RC
        from zksnark_finalproject_amd.device import rerandomize_batch_host
        t = RC.table(host.oracle, VERIFY_K)
        out, inf = rerandomize_batch_host(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
        assert np.array_equal(out, t.want) and np.array_equal(inf, t.want_inf)
        return t, out, inf
    return host.once("rerandomize", make)


def _rerandomize_step():
    def run(env):
        t, _, _ = rerandomize_table(env.host)
        with options(env.dev, ALWAYS_DEVICE):
            out, inf = env.dev.rerandomize_batch(t.delta, t.batch.proofs, t.batch.infs, t.r1, t.r2)
            assert env.dev.rerandomize_timings()["host_form"] == 0
        return proof_blob(out, inf)
    return Step("verify", "rerandomize-batch-k65", "the rerandomize scratch: a lane per (proof, group)", "k65 limbs", run,
                lambda host: proof_blob(*rerandomize_table(host)[1:]))


def rerandomize_wire(host):
    """the table as bytes with two proofs that do not decode -> (bytes sent, bytes expected back, statuses)"""
    def make():
        import decompress_cases as DC
        import verify_batch_cases as VB
        t, out, inf = rerandomize_table(host)
        sent = VB.to_wire(t.batch)
        clean = VB.to_wire(VB.Batch(None, np.zeros((t.k, 0, 4), np.uint64), out, inf))
        ordinary = next(i for i in range(t.k) if not t.batch.infs[i].any())
        st = np.zeros((t.k, 3), dtype=np.uint8)
        for i, group, lo, col, kind in ((3, "g1", 0, 0, "no_point"), (t.k - 1, "g2", 48, 1, "not_compressed")):
            enc, status = DC.hostile(group, sent[ordinary, lo:lo + DC.SIZE[group]].tobytes())[kind]
            sent[i, lo:lo + len(enc)] = np.frombuffer(enc, dtype=np.uint8)
            st[i, col] = status
            clean[i] = 0
        return sent, clean, st
    return host.once("rerandomize-wire", make)


def _rerandomize_wire_step():
    def run(env):
        t, _, _ = rerandomize_table(env.host)
        sent, _, _ = rerandomize_wire(env.host)
        with options(env.dev, ALWAYS_DEVICE):
            raw, st = env.dev.rerandomize_batch_wire(t.delta, sent, t.r1, t.r2)
            assert env.dev.rerandomize_timings()["host_form"] == 0
        return blob(raw, st)
    return Step("verify", "rerandomize-batch-wire-two-undecodable", "decode, rerandomize and compress scratch without leaving the device", "k65 wire, two undecodable",
                run, lambda host: blob(*rerandomize_wire(host)[1:]))


def bad_key(host):
    """X's key with one element of a_query, in the second wave of its kernel, moved off the curve -> (key, the element's index)"""
    def make():
        import pk_check_cases as K
        c = host.circuit("X")
        pk = {k: np.array(v, copy=True) for k, v in c["pk"].items()}
        at = int(np.flatnonzero(pk["a_inf"] == 0)[70])
        assert at >= 70
        pk["a_query"][at] = K.off_curve("g1", pk["a_query"][at])
        return pk, at
    return host.once("bad-key", make)


def _check_blob(res):
    from zksnark_finalproject_amd.device import PK_QUERIES, PK_SINGLES
    first = [NONE if res["first_bad"][q] is None else res["first_bad"][q] for q in PK_QUERIES]
    return blob(np.array([int(res["ok"])] + [res["n_bad"][q] for q in PK_QUERIES] + first + [int(res["singles"][q]) for q in PK_SINGLES], dtype=np.uint64))


def _pk_check_step(good):
    def run(env):
        if good:
            return _check_blob(env.dev.pk_check(env.key("X")))
        ph = env.get("bad-key", lambda: env.dev.pk_load(bad_key(env.host)[0], env.host.circuit("X")["ni"]))
        return _check_blob(env.dev.pk_check(ph))

    def expected(host):
        from zksnark_finalproject_amd.device import PK_QUERIES, PK_SINGLES
        import pk_check_cases as K
        res = dict(ok=good, n_bad={q: 0 for q in PK_QUERIES}, first_bad={q: None for q in PK_QUERIES}, singles={q: False for q in PK_SINGLES})
        if not good:
            pk, at = bad_key(host)
            verdicts = K.expected("g1", pk["a_query"][at - 2:at + 3], pk["a_inf"][at - 2:at + 3])          # the host check
            assert verdicts.tolist() == [True, True, False, True, True]
            res["n_bad"]["a_query"], res["first_bad"]["a_query"] = 1, at
        return _check_blob(res)
    return Step("verify", "pk-check-%s" % ("good-key" if good else "one-off-curve"), "pk_check scratch: the counters and first indices of five queries",
                "pk_check %s" % ("clean" if good else "one element of a_query off the curve"), run, expected)


def _pk_bytes_step():
    def run(env):
        from zksnark_finalproject_amd import wire
        c = env.host.circuit("X")
        with options(env.dev, {"pk_bytes_piece": 64}):
            raw = env.dev.pk_save(env.key("X"), c["vk"])
            ph, vk = env.dev.pk_load_bytes(raw)
            try:
                pk = env.dev.pk_read(ph)
            finally:
                env.dev.pk_free(ph)
        return raw + wire.pk_serialize_compressed(pk, vk)

    def expected(host):
        from zksnark_finalproject_amd import wire
        c = host.circuit("X")
        return wire.pk_serialize_compressed(c["pk"], c["vk"]) * 2
    return Step("verify", "pk-save-load-read-X-piece64", "pk_bytes scratch and the staging ring, 64 points a piece", "save, load_bytes, read in pieces of 64", run, expected)


def decompress_points(host):
    def make():
        import decompress_cases as DC
        import verify_batch_cases as VB
        b, _ = verify_batch_of(host)
        data = bytearray(VB.to_wire(b)[:, 48:144].tobytes())          # the 65 B points
        bad = DC.hostile("g2", bytes(data[:96]))
        for i, kind in ((0, "no_point"), (64, "outside_subgroup")):
            data[96 * i:96 * (i + 1)] = bad[kind][0]
        return bytes(data), {n: DC.host_decode("g2", bytes(data[:96 * n]), True) for n in (65, 1)}
    return host.once("decompress", make)


def _decompress_step(n):
    def run(env):
        data, _ = decompress_points(env.host)
        return blob(*env.dev.decompress_batch("g2", data[:96 * n], True))

    def expected(host):
        out, inf, st, _ = decompress_points(host)[1][n]
        return blob(out, inf, np.asarray(st, dtype=np.int32))
    return Step("verify", "decompress-batch-g2-n%d" % n, "the decode scratch", "n%d: %s" % (n, "a wave and one lane" if n > 64 else "one lane"), run, expected)


# ================================================================================================ the table
def build_steps():
    steps = [_msm_step(n) for n in MSM_SPECS] + [_tabled_step(n) for n in TABLED]
    steps += [_ntt_step(log_n, form) for log_n in NTT_LOGS for form in NTT_FORMS]
    steps += [_wm_step(log_n, *v) for log_n in (11, 12) for v in WM_VARIANTS]
    steps += [_resident_step(c, kind) for c in ("X", "Y") for kind in ("plain", "tabled")]
    steps += [_prove_host_pointers_step(), _batch_step("Y", 3), _batch_step("X", 33), _partial_step(), _matrix_step(3), _matrix_step(1), _checked_step()]
    steps += [_witness_matrix_step(8, 6), _witness_matrix_step(4, 1), _witness_matrix_step(8, 6, 4), _witness_matrix_step(8, 6, 1), _witness_matrix_step(4, 1, 1),
              _witness_fibonacci_step(65), _witness_fibonacci_step(1), _witness_linear_step("forward"), _witness_linear_step("elimination")]
    steps += [_witness_prime_step(w) for w in PRIME_CANDIDATES] + [_r1cs_prime_step(w) for w in PRIME_CANDIDATES]
    steps += [_setup_step("Y"), _setup_step("Z")]
    steps += [_verify_valid_step(65), _verify_tampered_step(), _verify_valid_step(1), _verify_wire_step(), _verify_u64_step(), _verify_prime_step(),
              _rerandomize_step(), _rerandomize_wire_step(), _pk_check_step(False), _pk_check_step(True), _pk_bytes_step(), _decompress_step(65),
              _decompress_step(1)]
    assert len({s.name for s in steps}) == len(steps)
    return steps


STEPS = build_steps()
BY_NAME = {s.name: s for s in STEPS}
FAMILIES = ("msm", "transform", "proof", "builder", "verify")


# the large-shapes test: what its first context runs before it closes, and what the second one runs
RECYCLED_FIRST = [BY_NAME["msm-g1-70000-c13"], BY_NAME["msm-g2-70000-c9"], _resident_step("W", "plain")]
RECYCLED_SECOND = [_msm_step("msm-g1-70000-c13-other-data"), _msm_step("msm-g2-70000-c9-other-data"), _resident_step("W", "plain", 1)] + \
    [BY_NAME[n] for n in ("msm-g1-61-c4", "msm-g1-3000-minseg1", "msm-g2-3000", "msm-g1-empty", "ntt-2^4-inv", "ntt-2^11-coset", "wm-2^11-unsatisfied-t6-fuse0",
                          "prove-host-pointers-Z-r0", "prove-resident-X-plain", "prove-resident-Y-tabled")]


def family(name):
    return [s for s in STEPS if s.family == name]


def walk(seed=20261021, length=150):
    """the fixed walk across families: the whole table in a shuffled order, then further draws from it up to `length` steps — no
    step of the table is left out"""
    rng = random.Random(seed)
    steps = list(STEPS)
    rng.shuffle(steps)
    assert length >= len(steps)
    return steps + [STEPS[rng.randrange(len(STEPS))] for _ in range(length - len(steps))]
