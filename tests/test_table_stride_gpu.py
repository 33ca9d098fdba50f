"""Option "table_stride": window tables with packed (112 / 224-byte) or padded (128 / 256-byte) entries.  The layout changes which bytes
a gather touches, never a point: a proof on either table is byte-identical to the plain key's proof of the same (key, assignment, r, s).
The shapes hold a few thousand terms, so a wrong stride or level base gathers a wrong point and the proof differs: byte equality is
the whole assertion."""
import random

import numpy as np
import pytest

import pyref as P
from helpers import *

pytestmark = pytest.mark.gpu

STRIDES = (1, 2)
# one table width on each side of the two- / three-pass bucket scatter (<= 20 / > 20 bucket bits), then one side only
WIDTHS = [(12, 12), (22, 22), (12, -1), (-1, 22)]


@pytest.fixture(scope="module")
def dev():
    from zksnark_finalproject_amd import Device
    d = Device(0)
    yield d
    d.set_option("table_stride", 0)
    d.close()


def _circuit(dev, kind):
    """-> r1cs handle, witness handles (two assignments), number of instance variables"""
    if kind == "fib1000":
        from zksnark_finalproject_amd.circuits import fibonacci_circuit
        cs = [fibonacci_circuit(a, b, 1000) for a, b in ((0, 1), (2, 3))]
        return dev.r1cs_load(cs[0].r1cs, cs[0].num_vars), [dev.witness_load(c.z) for c in cs], cs[0].num_instance
    n = int(kind[len("matrix"):])
    rng = np.random.default_rng(n)
    whs = [dev.witness_matrix(rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64), rng.integers(0, 1 << 32, size=(n, n), dtype=np.uint64))[0]
           for _ in range(2)]
    return dev.r1cs_matrix(n), whs, 4


_cache = {}


@pytest.fixture(scope="module")
def keys(dev):
    """kind -> the circuit, its resident plain key and the plain-key proofs (the reference of every case), built once per kind."""
    import bench

    def get(kind):
        if kind not in _cache:
            rh, whs, ni = _circuit(dev, kind)
            trap, g1, g2 = bench.draw_key_inputs(23)
            ph, _ = dev.setup_resident(rh, ni, trap, g1, g2)
            r1cs, nv = dev.r1cs_read(rh)
            n_h = (1 << (r1cs["num_constraints"] + ni - 1).bit_length()) - 1
            rng = random.Random(len(kind))
            rs = [fr_mont(P.rand_fr(rng)) for _ in whs]
            ss = [fr_mont(P.rand_fr(rng)) for _ in whs]
            plain = [dev.prove_resident(ph, rh, w, rs[i], ss[i]) for i, w in enumerate(whs)]
            _cache[kind] = dict(rh=rh, whs=whs, ph=ph, nv=nv, n_h=n_h, rs=rs, ss=ss, plain=plain)
        return _cache[kind]

    yield get
    for st in _cache.values():
        for w in st["whs"]:
            dev.witness_free(w)
        dev.pk_free(st["ph"])
        dev.r1cs_free(st["rh"])
    _cache.clear()


def _tabled_copy(dev, st, stride, cz, ch):
    """A second whole key cut out of the plain one, with tables of the given stride mode -> (handle, bytes added)"""
    h = dev.pk_slice(st["ph"], 0, st["nv"], 0, st["n_h"], True)
    dev.set_option("table_stride", stride)
    added = dev.pk_precompute(h, cz, ch)
    dev.set_option("table_stride", 0)         # read when the tables are built: the proofs below run on the layout the key has
    return h, added


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("cz,ch", WIDTHS)
@pytest.mark.parametrize("kind", ["matrix4", "matrix8", "fib1000"])
def test_packed_and_padded_tables_same_proof(dev, keys, kind, cz, ch):
    from zksnark_finalproject_amd.device import table_layout
    st = keys(kind)
    proofs = {}
    for stride in STRIDES:
        h, added = _tabled_copy(dev, st, stride, cz, ch)
        assert dev.pk_table_bits(h) == (max(cz, 0), max(ch, 0))
        want = 0
        if cz > 0:        # three G1 tables and the G2 one replace the plain queries of nv + 3 points
            nz, d = st["nv"] + 3, 254 // cz + 1
            want += 3 * table_layout("g1", nz, d, stride)[1] + table_layout("g2", nz, d, stride)[1] - nz * (3 * 112 + 224)
        if ch > 0:
            want += table_layout("g1", st["n_h"], 254 // ch + 1, stride)[1] - st["n_h"] * 112
        assert added == want, (stride, added, want)
        proofs[stride] = dev.prove_resident(h, st["rh"], st["whs"][0], st["rs"][0], st["ss"][0])
        dev.pk_free(h)
    assert _same(proofs[1], st["plain"][0]) and _same(proofs[2], st["plain"][0])
    assert _same(proofs[1], proofs[2])


@pytest.mark.parametrize("own_tables", [False, True])
@pytest.mark.parametrize("stride", STRIDES)
def test_shards_at_odd_offsets(dev, keys, stride, own_tables):
    """Three shards of the 8x8 key cut at z and h offsets that are no multiple of 8: cut out of a key that carries tables of the
    given stride (a shard is level 0 of every table, packed again), or cut out of the plain key and given tables of their own."""
    st = keys("matrix8")
    nv, n_h = st["nv"], st["n_h"]
    z1, z2, h1 = (nv // 3) | 1, (2 * nv // 3) | 3, (n_h // 2) | 1
    assert z1 % 8 and z2 % 8 and h1 % 8 and (z2 - z1) % 8
    plan = [(0, z1, 0, h1, True), (z1, z2, h1, n_h, False), (z2, nv, 0, 0, False)]
    src = st["ph"] if own_tables else _tabled_copy(dev, st, stride, 12, 12)[0]
    parts, pinf = [], []
    for i, (z_lo, z_hi, h_lo, h_hi, blind) in enumerate(plan):
        sh = dev.pk_slice(src, z_lo, z_hi, h_lo, h_hi, blind)
        if own_tables:
            dev.set_option("table_stride", stride)
            dev.pk_precompute(sh, 11 + i, 10)
            dev.set_option("table_stride", 0)
        pp, ff = dev.prove_partial(sh, st["rh"], st["whs"][0], st["rs"][0], st["ss"][0])
        parts.append(pp)
        pinf.append(ff)
        dev.pk_free(sh)
    fin = dev.prove_finish(src, st["rs"][0], st["ss"][0], np.array(parts), np.array(pinf))
    if not own_tables:
        dev.pk_free(src)
    assert _same(fin, st["plain"][0])


@pytest.mark.parametrize("stride", STRIDES)
def test_batch_of_two(dev, keys, stride):
    """zkg16_prove_batch builds its own accumulation arguments: K = 2 at 4x4 on a tabled key of either stride."""
    st = keys("matrix4")
    h, _ = _tabled_copy(dev, st, stride, 0, 0)
    proofs, inf = dev.prove_batch(h, st["rh"], np.array(st["whs"], dtype=np.uint64), np.stack(st["rs"]), np.stack(st["ss"]))
    dev.pk_free(h)
    for k in range(2):
        assert np.array_equal(proofs[k], st["plain"][k][0]) and np.array_equal(inf[k], st["plain"][k][1]), k
