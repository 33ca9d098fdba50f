"""Thin object layer over the C ABI: one `Device` == one zkg16_ctx == one MI355X."""
import contextlib
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import Zkg16Error


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _opt_u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


def _check_host(rc):
    """The status of a host-only entry point (no ctx, so no zkg16_last_error)."""
    if rc != 0:
        raise Zkg16Error(rc, _lib.load().zkg16_strerror(rc).decode())


# ---- what the batch proving methods share
def _rs_ss(who, rs, ss, k, each="one r and one s per request"):
    """The blinding pairs of a batch of k -> (rs [k, 4], ss [k, 4]) u64."""
    rs, ss = _u64(rs).reshape(-1, 4), _u64(ss).reshape(-1, 4)
    if rs.shape[0] != k or ss.shape[0] != k:
        raise ValueError(who + ": " + each)
    return rs, ss


def _proof_outputs(k):
    """-> (proofs [k, 48], inf [k, 3]) for an entry point to fill."""
    return np.zeros((k, 48), dtype=np.uint64), np.zeros((k, 3), dtype=np.uint8)


def _ms(times, *names):
    """An entry point's c_float times under their names."""
    return {name: float(t) for name, t in zip(names, times)}


PK_QUERIES = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")          # the order of zkg16_pk_check's arrays
PK_SINGLES = ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2")               # ... and of its single_mask bits


class Device:
    def __init__(self, device_id=0):
        # MatrixCircuit shapes resident on this device, by size (handlers._matrix_shape); entries have .rh
        self._matrix_shapes = {}
        self._matrix_shapes_lock = threading.Lock()
        self._options = {}              # what set_option was last given, by name (the ABI has no getter)
        self.lib = _lib.load()
        self.ctx = C.c_void_p()
        ids = (C.c_int * 1)(device_id)
        _check_host(self.lib.zkg16_init(ids, 1, C.byref(self.ctx)))

    def __getattr__(self, name):
        # reached only when the attribute is missing: callers drop the whole shape cache by deleting it, the next look starts an empty one
        if name == "_matrix_shapes":
            self._matrix_shapes = {}
            return self._matrix_shapes
        raise AttributeError(name)

    def close(self):
        if self.ctx:
            self.lib.zkg16_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            detail = self.lib.zkg16_last_error(self.ctx).decode()
            raise Zkg16Error(rc, self.lib.zkg16_strerror(rc).decode() + (" — " + detail if detail else ""))

    # ---- residency
    def pk_load(self, pk, num_instance, shard_index=0, shard_count=1):
        """pk: dict of numpy arrays (see groth16.ProvingKey.as_arrays)."""
        a, b1, b2 = _u64(pk["a_query"]).reshape(-1, 12), _u64(pk["b_g1_query"]).reshape(-1, 12), _u64(pk["b_g2_query"]).reshape(-1, 24)
        h, l = _u64(pk["h_query"]).reshape(-1, 12), _u64(pk["l_query"]).reshape(-1, 12)
        infs = [_opt_u8(pk.get(k)) for k in ("a_inf", "b_g1_inf", "b_g2_inf", "h_inf", "l_inf")]
        handle = C.c_uint64()
        self._check(self.lib.zkg16_pk_load(
            self.ctx, a, _ptr(infs[0]), a.shape[0], b1, _ptr(infs[1]), b1.shape[0], b2, _ptr(infs[2]), b2.shape[0],
            _ptr(h), _ptr(infs[3]), h.shape[0], _ptr(l), _ptr(infs[4]), l.shape[0],
            _u64(pk["alpha_g1"]), _u64(pk["beta_g1"]), _u64(pk["beta_g2"]), _u64(pk["delta_g1"]), _u64(pk["delta_g2"]),
            num_instance, shard_index, shard_count, C.byref(handle)))
        return handle.value

    def pk_load_range(self, pk, num_instance, z_lo, z_hi, h_lo, h_hi, blinding):
        """A shard given by explicit index ranges (zkg16_pk_load_range); see shard_plan."""
        a, b1, b2 = _u64(pk["a_query"]).reshape(-1, 12), _u64(pk["b_g1_query"]).reshape(-1, 12), _u64(pk["b_g2_query"]).reshape(-1, 24)
        h, l = _u64(pk["h_query"]).reshape(-1, 12), _u64(pk["l_query"]).reshape(-1, 12)
        infs = [_opt_u8(pk.get(k)) for k in ("a_inf", "b_g1_inf", "b_g2_inf", "h_inf", "l_inf")]
        handle = C.c_uint64()
        self._check(self.lib.zkg16_pk_load_range(
            self.ctx, a, _ptr(infs[0]), a.shape[0], b1, _ptr(infs[1]), b1.shape[0], b2, _ptr(infs[2]), b2.shape[0],
            _ptr(h), _ptr(infs[3]), h.shape[0], _ptr(l), _ptr(infs[4]), l.shape[0],
            _u64(pk["alpha_g1"]), _u64(pk["beta_g1"]), _u64(pk["beta_g2"]), _u64(pk["delta_g1"]), _u64(pk["delta_g2"]),
            num_instance, z_lo, z_hi, h_lo, h_hi, int(bool(blinding)), C.byref(handle)))
        return handle.value

    def pk_check(self, pk_h):
        """Is every element of a resident key or shard a point of its group (zkg16_pk_check: curve and prime-order subgroup, on the
        device where the key lies)?  -> dict(ok, n_bad, first_bad, singles): n_bad / first_bad keyed by query name (first_bad in the
        whole key's numbering, None where nothing failed), singles keyed by point name (True = at infinity or not in the group)."""
        n_bad, first_bad = np.zeros(5, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
        mask, ok = C.c_uint32(0), C.c_int(0)
        self._check(self.lib.zkg16_pk_check(self.ctx, pk_h, _ptr(n_bad), _ptr(first_bad), C.byref(mask), C.byref(ok)))
        return dict(ok=bool(ok.value),
                    n_bad={q: int(n_bad[i]) for i, q in enumerate(PK_QUERIES)},
                    first_bad={q: (int(first_bad[i]) if n_bad[i] else None) for i, q in enumerate(PK_QUERIES)},
                    singles={q: bool(mask.value >> i & 1) for i, q in enumerate(PK_SINGLES)})

    def pk_check_timings(self):
        """ms of the last pk_check (or validated load) and the last points_check_bulk (zkg16_pk_check_timings): the kernel of each
        query by name (device events; they run side by side), total_ms (wall), and the stage entry's bulk_kernel_ms / bulk_upload_ms."""
        ms = (C.c_float * 8)()
        n = self.lib.zkg16_pk_check_timings(self.ctx, ms, 8)
        return {name: float(ms[i]) for i, name in enumerate((PK_QUERIES + ("total_ms", "bulk_kernel_ms", "bulk_upload_ms"))[:n])}

    # ---- a resident key as arkworks' ProvingKey bytes (wire.pk_serialize_compressed / pk_deserialize_compressed are the host forms)
    def pk_read(self, pk_h):
        """A whole resident key copied back as the dict pk_load takes, flags included (zkg16_pk_read): level 0 of a window table at
        either stride, without the blinding slots.  A shard: Zkg16Error, status 7."""
        from . import wire
        d = [C.c_size_t() for _ in range(3)]
        self._check(self.lib.zkg16_pk_read(self.ctx, pk_h, *([None] * 15), *[C.byref(x) for x in d]))
        ni, m, n_h = (int(x.value) for x in d)
        pk, _, ptrs = wire._pk_arrays(ni, m, n_h)
        self._check(self.lib.zkg16_pk_read(self.ctx, pk_h, *ptrs, None, None, None))
        pk["num_instance"] = ni
        return pk

    def pk_save(self, pk_h, vk):
        """A whole resident key -> ProvingKey::serialize_compressed bytes, encoded on the device (zkg16_pk_save): byte for byte
        wire.pk_serialize_compressed(self.pk_read(pk_h), vk).  vk: gamma_g2 and gamma_abc_g1 are read (the handle holds neither)."""
        from . import wire
        d = [C.c_size_t() for _ in range(3)]
        self._check(self.lib.zkg16_pk_read(self.ctx, pk_h, *([None] * 15), *[C.byref(x) for x in d]))
        ni, m, n_h = (int(x.value) for x in d)
        gabc = _u64(vk["gamma_abc_g1"]).reshape(-1, 12)
        if gabc.shape[0] != ni:
            raise ValueError("pk_save: %d gamma_abc_g1 points for a key with %d instance variables" % (gabc.shape[0], ni))
        out = np.zeros(wire.pk_bytes_size(ni, m, n_h), dtype=np.uint8)
        written = C.c_size_t()
        self._check(self.lib.zkg16_pk_save(self.ctx, pk_h, _ptr(_u64(vk["gamma_g2"]).reshape(24)), _ptr(gabc), _ptr(out), out.size, C.byref(written)))
        return out[:written.value].tobytes()

    def pk_load_bytes(self, raw, validate=False):
        """ProvingKey bytes (bytes or a uint8 array: np.fromfile, np.memmap) -> (pk handle, vk dict), decoded on the device
        (zkg16_pk_load_bytes): the handle pk_load gives for wire.pk_deserialize_compressed(raw).  validate: pk_check's test before
        the handle exists.  A refusal (Zkg16Error, status 1) names the entry and its decoder status and leaves nothing behind."""
        from . import wire
        b = wire._raw_u8(raw)
        ni = wire.pk_bytes_dims(b)[0]
        vk = dict(alpha_g1=np.zeros(12, np.uint64), beta_g2=np.zeros(24, np.uint64), gamma_g2=np.zeros(24, np.uint64),
                  delta_g2=np.zeros(24, np.uint64), gamma_abc_g1=np.zeros((ni, 12), np.uint64))
        h = C.c_uint64()
        self._check(self.lib.zkg16_pk_load_bytes(self.ctx, _ptr(b), b.size, 1 if validate else 0, C.byref(h), _ptr(vk["alpha_g1"]), _ptr(vk["beta_g2"]),
                                                 _ptr(vk["gamma_g2"]), _ptr(vk["delta_g2"]), _ptr(vk["gamma_abc_g1"]), ni))
        return h.value, vk

    def pk_bytes_timings(self):
        """ms of the last pk_load_bytes / pk_save / pk_read (zkg16_pk_bytes_timings): copy_ms (host time in the staging ring), the
        kernels of each query by name (device events, first piece to last), vk_ms, check_ms, total_ms (wall)."""
        ms = (C.c_float * 9)()
        n = self.lib.zkg16_pk_bytes_timings(self.ctx, ms, 9)
        return {name: float(ms[i]) for i, name in enumerate((("copy_ms",) + PK_QUERIES + ("vk_ms", "check_ms", "total_ms"))[:n])}

    def pk_precompute(self, pk_h, window_bits_z=0, window_bits_h=0):
        """Window tables for a key that stays resident (zkg16_pk_precompute): same proofs, fewer bucket additions.
        0 = width chosen from the query length, < 0 = leave that side without a table.  The entries are laid out as option
        "table_stride" says at this call (table_layout).  -> HBM bytes added."""
        added = C.c_uint64(0)
        self._check(self.lib.zkg16_pk_precompute(self.ctx, pk_h, int(window_bits_z), int(window_bits_h), C.byref(added)))
        return added.value

    def last_term_counts(self):
        """-> (z list, B list (0 = the z list was used), h list): mixed additions per MSM of the last proof (zkg16_last_term_counts)."""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.zkg16_last_term_counts(self.ctx, out))
        return int(out[0]), int(out[1]), int(out[2])

    def lane_log(self, rows=64):
        """-> list of (lane, start_ms, end_ms) of the most recent proofs on this ctx (zkg16_lane_log), oldest first."""
        buf = (C.c_double * (3 * rows))()
        n = self.lib.zkg16_lane_log(self.ctx, buf, rows)
        return [(int(buf[3 * i]), float(buf[3 * i + 1]), float(buf[3 * i + 2])) for i in range(n)]

    def last_acc_waves(self):
        """-> G1 accumulation waves per SIMD of the last proof's (z, B, h) term lists (zkg16_last_acc_waves); 0 = list not built."""
        out = (C.c_int * 3)()
        self._check(self.lib.zkg16_last_acc_waves(self.ctx, out))
        return int(out[0]), int(out[1]), int(out[2])

    def last_msm_state(self):
        """-> (c, nwin, entries, seg_len, fixup_items, fixup_chains, bit_sliced, two_level_k) of the last msm() on this device
        (zkg16_last_msm_state): the path that MSM took, for tests that pin a boundary."""
        out = (C.c_uint32 * 8)()
        self._check(self.lib.zkg16_last_msm_state(self.ctx, out))
        return tuple(int(x) for x in out)

    def diag_bucket_sort(self, codes, c):
        """codes: (nwin, n) uint32 digit codes ((|d| - 1) << 1 | negate, ~0 for digit 0) -> (entries (length, 2) uint32 of (x, y),
        win_totals (nwin,) uint32, length): the bucket scatter alone, in a workspace of its own (zkg16_diag_bucket_sort)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        nwin, n = codes.shape
        entries = np.zeros((nwin * n, 2), dtype=np.uint32)
        totals = np.zeros(nwin, dtype=np.uint32)
        length = C.c_uint64(0)
        self._check(self.lib.zkg16_diag_bucket_sort(self.ctx, _ptr(codes) if n else None, n, nwin, int(c), _ptr(entries) if n else None,
                                                    totals.ctypes.data, C.byref(length)))
        return entries[:length.value], totals, int(length.value)

    def diag_term_list(self, scalars, window_bits, tabled=False, mask=None, mask_mode=0):
        """scalars: (batch, n, 4) or (n, 4) canonical u64 limbs -> (plan (c, windows, digits, total buckets), entries (length, 2) uint32
        of (x, y), offsets (total buckets + 1,) uint32): the sorted term list a proof would build (zkg16_diag_term_list).  mask_mode
        1 = mask in the digit kernel, 2 = the full list filtered."""
        sc = _u64(scalars)
        if sc.ndim == 2:
            sc = sc[None]
        batch, n = sc.shape[0], sc.shape[1]
        if not 2 <= int(window_bits) <= (24 if tabled else 20):
            raise ValueError("diag_term_list: name the window bits (the buffers are sized from them)")
        digits = 254 // int(window_bits) + 1
        tb = (1 << (int(window_bits) - 1)) * batch * (1 if tabled else digits)
        entries = np.zeros((batch * n * digits, 2), dtype=np.uint32)
        offsets = np.zeros(tb + 1, dtype=np.uint32)
        mask = _opt_u8(mask)
        if mask is not None and mask.shape != (n,):
            raise ValueError("diag_term_list: one mask byte per scalar")
        plan = (C.c_uint32 * 4)()
        length = C.c_uint64(0)
        self._check(self.lib.zkg16_diag_term_list(self.ctx, _ptr(sc) if n else None, n, batch, int(window_bits), int(bool(tabled)), _ptr(mask),
                                                  int(mask_mode), plan, _ptr(entries) if n else None, entries.shape[0],
                                                  _ptr(offsets) if n else None, offsets.shape[0], C.byref(length)))
        return tuple(int(x) for x in plan), entries[:length.value], offsets

    def diag_msm_tabled(self, group, bases, scalars, window_bits, stride_mode=1, last_of_proof=False, inf=None, want_table=False):
        """One MSM on window tables, as a proof runs one query of a key that carries them (zkg16_diag_msm_tabled).  group "g1" | "g2";
        bases (n, 12 | 24) with an optional infinity mask; scalars (batch, n, 4) or (n, 4) canonical u64 limbs; stride_mode 1 packed,
        2 padded.  -> (points (batch, 12 | 24), inf (batch,)), and with want_table also (table (levels, n, 12 | 24), table_inf
        (levels, n)).  last_msm_state() reports the call, nwin reading as the batch."""
        w = 12 if group == "g1" else 24
        bases = _u64(bases).reshape(-1, w)
        sc = _u64(scalars)
        if sc.ndim == 2:
            sc = sc[None]
        batch, n = sc.shape[0], sc.shape[1]
        if bases.shape[0] != n or sc.shape[2] != 4:
            raise ValueError("diag_msm_tabled: one base per scalar of a vector")
        inf = _opt_u8(inf)
        if inf is not None and inf.shape != (n,):
            raise ValueError("diag_msm_tabled: one mask byte per base")
        c = int(window_bits)
        levels = 254 // c + 1 if 2 <= c <= 24 else 0      # a width the library refuses: it says so itself
        out = np.zeros((max(batch, 1), w), dtype=np.uint64)
        oinf = np.zeros(max(batch, 1), dtype=np.uint8)
        table = np.zeros((levels, n, w), dtype=np.uint64) if want_table else None
        tinf = np.zeros((levels, n), dtype=np.uint8) if want_table else None
        self._check(self.lib.zkg16_diag_msm_tabled(self.ctx, 1 if group == "g1" else 2, _ptr(bases) if n else None, _ptr(inf), _ptr(sc) if n else None, n,
                                                   batch, c, int(stride_mode), int(bool(last_of_proof)), out.ctypes.data, oinf.ctypes.data,
                                                   table.ctypes.data if want_table else None, tinf.ctypes.data if want_table else None))
        return (out, oinf, table, tinf) if want_table else (out, oinf)

    def diag_msm_rounds(self, group, bases, scalars, part_of, parts, window_bits, inf=None):
        """One plain-key MSM fed in `parts` rounds, as a proof on a streamed assignment runs one z-side query (zkg16_diag_msm_rounds).
        group "g1" | "g2"; bases (n, 12 | 24) with an optional infinity mask; scalars (n, 4) canonical u64 limbs; part_of (n,) the
        round each scalar takes part in.  -> (point (12 | 24,), inf, round_entries (parts,) uint32: the length of every round's term
        list).  last_msm_state() reports the last round."""
        w = 12 if group == "g1" else 24
        bases = _u64(bases).reshape(-1, w)
        sc = _u64(scalars).reshape(-1, 4)
        n = sc.shape[0]
        part_of = np.ascontiguousarray(part_of, dtype=np.uint8)
        if bases.shape[0] != n or part_of.shape != (n,):
            raise ValueError("diag_msm_rounds: one base and one part label per scalar")
        inf = _opt_u8(inf)
        if inf is not None and inf.shape != (n,):
            raise ValueError("diag_msm_rounds: one mask byte per base")
        out = np.zeros(w, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        entries = np.zeros(max(int(parts), 1), dtype=np.uint32)
        self._check(self.lib.zkg16_diag_msm_rounds(self.ctx, 1 if group == "g1" else 2, _ptr(bases) if n else None, _ptr(inf), _ptr(sc) if n else None, n,
                                                   _ptr(part_of) if n else None, int(parts), int(window_bits), out.ctypes.data, oinf.ctypes.data,
                                                   entries.ctypes.data))
        return out, int(oinf[0]), entries

    def diag_matrix_stream(self, a, b):
        """The streamed assignment of prove_matrix(a, b) alone, part by part, under this device's matrix_parts and matrix_slice_min
        (zkg16_diag_matrix_stream) -> (part_of (total + 3,) uint8: the device's part map, first_valid (total,) uint8: the first part
        after which each entry had been written (255 = never), z (total, 4): the finished assignment, parts)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        n = a.shape[0]
        if a.shape != (n, n) or b.shape != (n, n):
            raise ValueError("diag_matrix_stream: a and b must be n x n")
        total = matrix_variables(n)
        part_of = np.zeros(total + 3, dtype=np.uint8)
        first = np.zeros(total, dtype=np.uint8)
        z = np.zeros((total, 4), dtype=np.uint64)
        parts = C.c_int(0)
        self._check(self.lib.zkg16_diag_matrix_stream(self.ctx, n, a.ctypes.data, b.ctypes.data, part_of.ctypes.data, first.ctypes.data,
                                                      z.ctypes.data, total, C.byref(parts)))
        return part_of, first, z, parts.value

    def circuit_load(self, circuit):
        """circuit: a circuits.CircuitHandle (a synthesized circuit still held by the library) -> (r1cs_handle, witness_handle), loaded
        without exporting its arrays to Python (zkg16_circuit_load)."""
        rh, wh = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zkg16_circuit_load(self.ctx, circuit.handle, C.byref(rh), C.byref(wh)))
        return rh.value, wh.value

    def acc_resident_waves(self):
        """-> (G1, G2) waves of the accumulation kernels one SIMD holds at once (zkg16_acc_resident_waves)."""
        out = (C.c_int * 2)()
        self._check(self.lib.zkg16_acc_resident_waves(self.ctx, out))
        return int(out[0]), int(out[1])

    def pk_table_bits(self, pk_h):
        """-> (window bits of the z-side tables, of the h-side table); 0 = none (zkg16_pk_table_bits)."""
        bz, bh = C.c_int(0), C.c_int(0)
        self._check(self.lib.zkg16_pk_table_bits(self.ctx, pk_h, C.byref(bz), C.byref(bh)))
        return bz.value, bh.value

    def pk_slice(self, pk_h, z_lo, z_hi, h_lo, h_hi, blinding):
        """A shard cut out of a whole resident key, device to device (zkg16_pk_slice)."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_pk_slice(self.ctx, pk_h, z_lo, z_hi, h_lo, h_hi, int(bool(blinding)), C.byref(handle)))
        return handle.value

    def pk_free(self, h):
        self.lib.zkg16_pk_free(self.ctx, h)

    @staticmethod
    def _csr(r1cs):
        args, keep = [], []
        for m in ("a", "b", "c"):
            rp, col, cf = r1cs[m]
            rp = _u64(rp)
            col = np.ascontiguousarray(col, dtype=np.uint32)
            cf = _u64(cf).reshape(-1, 4)
            keep += [rp, col, cf]
            args += [rp, _ptr(col) if col.size else None, _ptr(cf) if cf.size else None]
        return args, keep

    def r1cs_load(self, r1cs, num_variables):
        args, keep = self._csr(r1cs)
        handle = C.c_uint64()
        self._check(self.lib.zkg16_r1cs_load(self.ctx, *args, r1cs["num_inputs"], r1cs["num_constraints"], num_variables, C.byref(handle)))
        return handle.value

    def r1cs_matrix(self, n):
        """The MatrixCircuit's R1CS of size n written on the device (zkg16_r1cs_matrix) -> r1cs handle."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_r1cs_matrix(self.ctx, n, C.byref(handle)))
        return handle.value

    def r1cs_fibonacci(self, steps):
        """The FibonacciCircuit's R1CS of `steps` rounds, which no request's (a, b) enters (zkg16_r1cs_fibonacci) -> r1cs handle: what
        the key of prove_fibonacci_batch is set up on."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_r1cs_fibonacci(self.ctx, steps, C.byref(handle)))
        return handle.value

    def r1cs_linear(self, n):
        """The linear-equations circuit's R1CS of size n, which no request's (a, b) enters (zkg16_r1cs_linear) -> r1cs handle: what the
        key of prove_linear_batch is set up on."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_r1cs_linear(self.ctx, n, C.byref(handle)))
        return handle.value

    def r1cs_prime(self, x, j):
        """The PrimeCircuit's R1CS for candidate (x, j) from the template resident on the device (zkg16_r1cs_prime) -> r1cs handle."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_r1cs_prime(self.ctx, x, j, C.byref(handle)))
        return handle.value

    def witness_prime(self, x, j):
        """The PrimeCircuit's assignment for candidate (x, j) built on the device (zkg16_witness_prime) -> witness handle."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_witness_prime(self.ctx, x, j, C.byref(handle)))
        return handle.value

    def r1cs_prime_template(self):
        """The template every candidate's R1CS is a patch of, as an r1cs handle (zkg16_r1cs_prime_template): what the key of
        prove_prime_batch is set up on, and the only r1cs handle it takes."""
        handle = C.c_uint64()
        self._check(self.lib.zkg16_r1cs_prime_template(self.ctx, C.byref(handle)))
        return handle.value

    def witness_prime_batch(self, xs, js):
        """The PrimeCircuit's assignments of k candidates (xs[i], js[i]) built in one device pass (zkg16_witness_prime_batch) ->
        witness handles [k]; handle i holds what witness_prime(xs[i], js[i]) would, each is freed on its own.  A refused candidate
        fails the whole call and registers nothing."""
        xs, js = _u64(xs).reshape(-1), _u64(js).reshape(-1)
        if xs.shape != js.shape:
            raise ValueError("witness_prime_batch: one j per x")
        handles = np.zeros(xs.shape[0], dtype=np.uint64)
        self._check(self.lib.zkg16_witness_prime_batch(self.ctx, _ptr(xs), _ptr(js), xs.shape[0], _ptr(handles)))
        return handles

    def r1cs_read(self, h):
        """-> the r1cs dict (as SynthesizedCircuit.r1cs) + num_variables behind a handle (zkg16_r1cs_read)."""
        ni, nc, nv = C.c_size_t(), C.c_size_t(), C.c_size_t()
        nnz = (C.c_size_t * 3)()
        self._check(self.lib.zkg16_r1cs_read(self.ctx, h, None, None, None, C.byref(ni), C.byref(nc), C.byref(nv), C.byref(nnz)))
        rp = [np.zeros(nc.value + 1, dtype=np.uint64) for _ in range(3)]
        col = [np.zeros(max(nnz[m], 1), dtype=np.uint32) for m in range(3)]
        cf = [np.zeros((max(nnz[m], 1), 4), dtype=np.uint64) for m in range(3)]
        arr = lambda xs: (C.c_void_p * 3)(*[x.ctypes.data for x in xs])
        a, b, c = arr(rp), arr(col), arr(cf)
        self._check(self.lib.zkg16_r1cs_read(self.ctx, h, C.addressof(a), C.addressof(b), C.addressof(c), None, None, None, None))
        return dict(a=(rp[0], col[0][:nnz[0]], cf[0][:nnz[0]]), b=(rp[1], col[1][:nnz[1]], cf[1][:nnz[1]]),
                    c=(rp[2], col[2][:nnz[2]], cf[2][:nnz[2]]), num_inputs=ni.value, num_constraints=nc.value), nv.value

    def r1cs_spmv_state(self, h):
        """-> (dict_state, ndict, perm_ok, spmv_uses) of an r1cs handle (zkg16_r1cs_spmv_state): dict_state 0 = not tried yet,
        1 = coefficient dictionary in use with ndict values, 2 = plain kernel for good; perm_ok 1 = rows in length-class order."""
        out = (C.c_uint32 * 4)()
        self._check(self.lib.zkg16_r1cs_spmv_state(self.ctx, h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def r1cs_free(self, h):
        self.lib.zkg16_r1cs_free(self.ctx, h)

    # ---- satisfaction: (A z)_i (B z)_i == (C z)_i on the device
    def r1cs_check(self, r1cs_h, wit_h):
        """Does the assignment satisfy the system (zkg16_r1cs_check)? -> (n_bad, first_bad): failing constraint rows and the smallest
        of them, 2^64 - 1 when there is none.  One sparse product and one kernel; counts as a use of the r1cs handle."""
        nb, fb = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zkg16_r1cs_check(self.ctx, r1cs_h, wit_h, C.byref(nb), C.byref(fb)))
        return int(nb.value), int(fb.value)

    @staticmethod
    def _verdicts(nb, fb):
        return [(int(n), int(f)) for n, f in zip(nb, fb)]

    def r1cs_check_batch(self, r1cs_h, witness_handles):
        """k assignments of one system in batched device passes (zkg16_r1cs_check_batch) -> [(n_bad, first_bad)] * k, entry i what
        r1cs_check(r1cs_h, witness_handles[i]) gives."""
        hs = np.ascontiguousarray(witness_handles, dtype=np.uint64).reshape(-1)
        nb, fb = np.zeros(hs.shape[0], dtype=np.uint64), np.zeros(hs.shape[0], dtype=np.uint64)
        self._check(self.lib.zkg16_r1cs_check_batch(self.ctx, r1cs_h, _ptr(hs), hs.shape[0], _ptr(nb), _ptr(fb)))
        return self._verdicts(nb, fb)

    def prime_check_batch(self, r1cs_h, xs, js):
        """k prime requests on the template handle (zkg16_prime_check_batch): the assignments built, multiplied and checked on the
        device -> [(n_bad, first_bad)] * k, entry i what r1cs_check gives on r1cs_prime / witness_prime(xs[i], js[i]).  A candidate
        the circuit refuses fails the whole call (status 7) before any device work."""
        xs, js = _u64(xs).reshape(-1), _u64(js).reshape(-1)
        if xs.shape != js.shape:
            raise ValueError("prime_check_batch: one j per x")
        nb, fb = np.zeros(xs.shape[0], dtype=np.uint64), np.zeros(xs.shape[0], dtype=np.uint64)
        self._check(self.lib.zkg16_prime_check_batch(self.ctx, r1cs_h, _ptr(xs), _ptr(js), xs.shape[0], _ptr(nb), _ptr(fb)))
        return self._verdicts(nb, fb)

    def last_check(self):
        """-> [(n_bad, first_bad)] per proof of the last proving call, when it ran with option "check_satisfied" = 1 (zkg16_last_check);
        [] when it did not check."""
        k = C.c_size_t(0)
        self.lib.zkg16_last_check(self.ctx, None, None, 0, C.byref(k))
        nb, fb = np.zeros(max(k.value, 1), dtype=np.uint64), np.zeros(max(k.value, 1), dtype=np.uint64)
        n = self.lib.zkg16_last_check(self.ctx, _ptr(nb), _ptr(fb), k.value, None)
        return self._verdicts(nb[:n], fb[:n])

    def witness_load(self, z):
        z = _u64(z).reshape(-1, 4)
        handle = C.c_uint64()
        self._check(self.lib.zkg16_witness_load(self.ctx, z, z.shape[0], C.byref(handle)))
        return handle.value

    def witness_matrix(self, a, b):
        """The MatrixCircuit's assignment for (a, b) built on the device (zkg16_witness_matrix) ->
        (witness handle, public inputs [3, 4] = hash_a, hash_b, hash_c, dict of ms: host sponges / device / whole call)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        n = a.shape[0]
        if a.shape != (n, n) or b.shape != (n, n):
            raise ValueError("witness_matrix: a and b must be n x n")
        handle = C.c_uint64()
        pub = np.zeros((3, 4), dtype=np.uint64)
        ms = (C.c_float * 3)()
        self._check(self.lib.zkg16_witness_matrix(self.ctx, n, a.reshape(-1), b.reshape(-1), C.byref(handle), pub.ctypes.data, C.addressof(ms)))
        return handle.value, pub, dict(host_sponges_ms=float(ms[0]), device_ms=float(ms[1]), call_ms=float(ms[2]))

    @staticmethod
    def _matrix_batch(what, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        if a.ndim != 3 or a.shape[1] != a.shape[2] or b.shape != a.shape:
            raise ValueError(what + ": a and b must be k x n x n")
        return a, b, a.shape[0], a.shape[1]

    def witness_matrix_batch(self, a, b):
        """The MatrixCircuit's assignments of k requests of one size, a and b [k, n, n], built in one device pass
        (zkg16_witness_matrix_batch) -> (witness handles [k], public inputs [k, 3, 4], dict of ms: host chains / device / whole call).
        Handle i holds what witness_matrix(a[i], b[i]) would; each is freed on its own."""
        a, b, k, n = self._matrix_batch("witness_matrix_batch", a, b)
        handles = np.zeros(k, dtype=np.uint64)
        pub = np.zeros((k, 3, 4), dtype=np.uint64)
        ms = (C.c_float * 3)()
        self._check(self.lib.zkg16_witness_matrix_batch(self.ctx, n, _ptr(a), _ptr(b), k, _ptr(handles), _ptr(pub), C.addressof(ms)))
        return handles, pub, _ms(ms, "host_sponges_ms", "device_ms", "call_ms")

    @staticmethod
    def _fibonacci_batch(what, a, b):
        a, b = _u64(a).reshape(-1), _u64(b).reshape(-1)
        if a.shape != b.shape:
            raise ValueError(what + ": one b per a")
        return a, b, a.shape[0]

    def witness_fibonacci_batch(self, steps, a, b):
        """The FibonacciCircuit's assignments of k requests of one round count, a and b [k] u64, built in one device pass
        (zkg16_witness_fibonacci_batch) -> (witness handles [k], public inputs [k, 3, 4] = a, b, result, dict of ms: host coefficients
        / device / whole call).  Handle i holds what circuit_load of fibonacci_circuit(a[i], b[i], steps) would; each is freed on its own."""
        a, b, k = self._fibonacci_batch("witness_fibonacci_batch", a, b)
        handles = np.zeros(k, dtype=np.uint64)
        pub = np.zeros((k, 3, 4), dtype=np.uint64)
        ms = (C.c_float * 3)()
        self._check(self.lib.zkg16_witness_fibonacci_batch(self.ctx, steps, _ptr(a), _ptr(b), k, _ptr(handles), _ptr(pub), C.addressof(ms)))
        return handles, pub, _ms(ms, "host_coeffs_ms", "device_ms", "call_ms")

    @staticmethod
    def _linear_batch(what, a, b):
        a, b = _u64(a), _u64(b)
        if a.ndim != 3 or a.shape[1] != a.shape[2] or b.shape != a.shape[:2]:
            raise ValueError(what + ": a must be k x n x n and b k x n")
        return a, b, a.shape[0], a.shape[1]

    @contextlib.contextmanager
    def _linear_solver(self, solver):
        """Option "linear_solver" set to `solver` ("forward" | "elimination") for the body and put back to what set_option last gave
        it (0 if never set).  None: the option stays as it is."""
        if solver is None:
            yield
            return
        from .circuits import linear_solver_id
        before = self._options.get("linear_solver", 0)
        self.set_option("linear_solver", linear_solver_id(solver))
        try:
            yield
        finally:
            self.set_option("linear_solver", before)

    def witness_linear_batch(self, a, b, solver=None):
        """The linear-equations assignments of k requests of one size, a [k, n, n] and b [k, n] u64, built in one device pass
        (zkg16_witness_linear_batch: the solve kernel, one wave per request, and the fill kernel) -> (witness handles [k], x [k, n, 4]
        = the handler's solutions, dict of ms: host checks / device / whole call).  Handle i holds what circuit_load of
        linear_circuit(a[i], b[i]) would; each is freed on its own.
        solver: "forward" (the reference's substitution on the lower triangle) or "elimination" (Gaussian elimination over Fr, the
        elimination kernel in the solve kernel's place: handle i holds what linear_circuit(a[i], b[i], solver="elimination") exports;
        a singular request fails the whole call with status 7) — option "linear_solver" is set for this call and restored; None
        (default): the option as the ctx has it, "forward" unless set."""
        a, b, k, n = self._linear_batch("witness_linear_batch", a, b)
        handles = np.zeros(k, dtype=np.uint64)
        x = np.zeros((k, n, 4), dtype=np.uint64)
        ms = (C.c_float * 3)()
        with self._linear_solver(solver):
            self._check(self.lib.zkg16_witness_linear_batch(self.ctx, n, _ptr(a), _ptr(b), k, _ptr(handles), _ptr(x), C.addressof(ms)))
        return handles, x, _ms(ms, "host_check_ms", "device_ms", "call_ms")

    def poseidon_hash_batch(self, elems):
        """k Poseidon hashes in one call (zkg16_poseidon_hash_batch): elems [k, n, 4] Montgomery Fr -> [k, 4], row i the bytes of
        circuits.poseidon_hash(elems[i]).  At least option "sponge_chains_min" vectors are hashed by a kernel, fewer on host threads."""
        elems = np.ascontiguousarray(elems, dtype=np.uint64)
        if elems.ndim != 3 or elems.shape[2] != 4:
            raise ValueError("poseidon_hash_batch: elems must be k x n x 4")
        out = np.zeros((elems.shape[0], 4), dtype=np.uint64)
        self._check(self.lib.zkg16_poseidon_hash_batch(self.ctx, _ptr(elems), elems.shape[1], elems.shape[0], _ptr(out)))
        return out

    def matrix_hash_batch(self, m):
        """The matrix handler's hash of k matrices of one size, m [k, n, n] u64, in one call (zkg16_matrix_hash_batch) -> [k, 4]
        Montgomery Fr: row i is hash_a of witness_matrix(m[i], .), the public input a verifier needs."""
        m = np.ascontiguousarray(m, dtype=np.uint64)
        if m.ndim != 3 or m.shape[1] != m.shape[2]:
            raise ValueError("matrix_hash_batch: m must be k x n x n")
        out = np.zeros((m.shape[0], 4), dtype=np.uint64)
        self._check(self.lib.zkg16_matrix_hash_batch(self.ctx, m.shape[1], _ptr(m), m.shape[0], _ptr(out)))
        return out

    def witness_read(self, h, n_assign):
        z = np.zeros((n_assign, 4), dtype=np.uint64)
        self._check(self.lib.zkg16_witness_read(self.ctx, h, z.reshape(-1), n_assign))
        return z

    def witness_free(self, h):
        self.lib.zkg16_witness_free(self.ctx, h)

    # ---- proofs
    def prove_resident(self, pk_h, r1cs_h, wit_h, r, s):
        proof = np.zeros(48, dtype=np.uint64)
        inf = np.zeros(3, dtype=np.uint8)
        self._check(self.lib.zkg16_prove_resident(self.ctx, pk_h, r1cs_h, wit_h, _u64(r), _u64(s), proof, inf))
        return proof, inf

    def prove_batch(self, pk_h, r1cs_h, witness_handles, rs, ss):
        """K proofs of one circuit on one resident key in one device pass (zkg16_prove_batch): witness_handles [k], rs / ss [k, 4]
        Montgomery -> (proofs [k, 48], inf [k, 3]); proof k is byte-identical to prove_resident(pk_h, r1cs_h, witness_handles[k],
        rs[k], ss[k])."""
        hs = np.ascontiguousarray(witness_handles, dtype=np.uint64).reshape(-1)
        k = hs.shape[0]
        rs, ss = _rs_ss("prove_batch", rs, ss, k, "one r and one s per witness handle")
        proofs, inf = _proof_outputs(k)
        self._check(self.lib.zkg16_prove_batch(self.ctx, pk_h, r1cs_h, hs, k, rs, ss, proofs, inf))
        return proofs, inf

    # ---- the trapdoor route: setup-and-prove without the key (zkg16_prove_trapdoor*)
    def prove_trapdoor(self, r1cs_h, wit_h, num_instance, trapdoor_mont, g1_gen, g2_gen, r, s):
        """One setup-and-prove request answered from the trapdoor, no proving key built (zkg16_prove_trapdoor) -> (proof [48], inf [3],
        vk dict shaped as setup_resident's).  Byte for byte prove_resident on setup_resident's key for the same arguments.  Only for
        callers that drew the trapdoor themselves.  An unsatisfied assignment raises Zkg16Error with status 8 (last_check names it)."""
        proofs, inf, vk = self.prove_trapdoor_batch(r1cs_h, [wit_h], num_instance, trapdoor_mont, g1_gen, g2_gen,
                                                    _u64(r).reshape(1, 4), _u64(s).reshape(1, 4), _single=True)
        return proofs[0], inf[0], vk

    def prove_trapdoor_batch(self, r1cs_h, witness_handles, num_instance, trapdoor_mont, g1_gen, g2_gen, rs, ss, _single=False):
        """k assignments of one system under the one key of the trapdoor (zkg16_prove_trapdoor_batch): rs / ss [k, 4] Montgomery ->
        (proofs [k, 48], inf [k, 3], vk dict); proof i is prove_trapdoor's for (witness_handles[i], rs[i], ss[i]).  The call's five
        times (ms: QAP evaluation, sparse product + check, dot kernel, fixed-base passes, whole call) are kept in last_trapdoor_ms."""
        hs = np.ascontiguousarray(witness_handles, dtype=np.uint64).reshape(-1)
        k = hs.shape[0]
        rs, ss = _rs_ss("prove_trapdoor_batch", rs, ss, k, "one r and one s per witness handle")
        proofs, inf = _proof_outputs(k)
        vk = dict(alpha_g1=np.zeros(12, np.uint64), beta_g2=np.zeros(24, np.uint64), gamma_g2=np.zeros(24, np.uint64),
                  delta_g2=np.zeros(24, np.uint64), gamma_abc_g1=np.zeros((num_instance, 12), np.uint64))
        ms = (C.c_float * 5)()
        trap, g1, g2 = _u64(trapdoor_mont).reshape(-1), _u64(g1_gen), _u64(g2_gen)
        tail = (_ptr(proofs), _ptr(inf), _ptr(vk["alpha_g1"]), _ptr(vk["beta_g2"]), _ptr(vk["gamma_g2"]), _ptr(vk["delta_g2"]),
                _ptr(vk["gamma_abc_g1"]), C.addressof(ms))
        if _single:
            rc = self.lib.zkg16_prove_trapdoor(self.ctx, r1cs_h, int(hs[0]), _ptr(trap), _ptr(g1), _ptr(g2), _ptr(rs), _ptr(ss), *tail)
        else:
            rc = self.lib.zkg16_prove_trapdoor_batch(self.ctx, r1cs_h, _ptr(hs) if k else None, k, _ptr(trap), _ptr(g1), _ptr(g2), _ptr(rs), _ptr(ss), *tail)
        self._check(rc)
        self.last_trapdoor_ms = _ms(ms, "qap_ms", "check_ms", "dot_ms", "points_ms", "call_ms")
        return proofs, inf, vk

    # ---- batched verification: one body per shape of entry point, whatever the form of the public inputs (_verify_args)
    def _verify_limbs(self, entry, pvk, kind, inputs, proofs, infs, rho, each):
        args, k = _verify_args(pvk, kind, inputs, proofs, infs, rho)
        ok = C.c_int(0)
        ok_each = np.zeros(k, dtype=np.uint8) if each else None
        self._check(getattr(self.lib, "zkg16_" + entry)(self.ctx, *args, C.byref(ok), _ptr(ok_each)))
        return _verify_result(ok, ok_each)

    def _verify_wire(self, entry, pvk, kind, inputs, proof_bytes, rho, each, status):
        raw, k = _wire_bytes(entry, proof_bytes)
        args, _ = _verify_args(pvk, kind, inputs, None, None, rho, k=k)
        ok = C.c_int(0)
        ok_each = np.zeros(k, dtype=np.uint8) if each else None
        st = np.zeros((k, 3), dtype=np.uint8) if status else None
        # the bytes in the place of the limbs and flags
        self._check(getattr(self.lib, "zkg16_" + entry)(self.ctx, *args[:-4], _ptr(raw) if k else None, args[-2], k, C.byref(ok), _ptr(ok_each), _ptr(st)))
        return _verify_result(ok, ok_each, st)

    def _verify_each(self, entry, pvk, kind, inputs, proofs, infs):
        args, k = _verify_args(pvk, kind, inputs, proofs, infs, np.ones((_u64(proofs).reshape(-1, 48).shape[0], 2), dtype=np.uint64))
        ok_each = np.zeros(k, dtype=np.uint8)
        self._check(getattr(self.lib, "zkg16_" + entry)(self.ctx, *args[:-2], k, _ptr(ok_each)))      # no multipliers
        return ok_each.astype(bool)

    def verify_batch(self, pvk, public_inputs, proofs, infs, rho=None, each=False):
        """K proofs under one prepared key checked together, the per-proof work in kernels (zkg16_verify_batch): public_inputs
        [k, num_instance - 1, 4] Montgomery, proofs [k, 48], infs [k, 3]; rho [k, 2]: 128-bit non-zero multipliers that whoever
        made the proofs could not predict (None: drawn from `secrets`).  -> all_valid, or (all_valid, per-proof bool array) with
        each=True.  Batches shorter than the option "verify_batch_min" are answered by the host form."""
        return self._verify_limbs("verify_batch", pvk, "limbs", (public_inputs,), proofs, infs, rho, each)

    def verify_batch_wire(self, pvk, public_inputs, proof_bytes, rho=None, each=False, status=False):
        """verify_batch from the proofs as they travel (zkg16_verify_batch_wire): proof_bytes = k x 192 compressed bytes (bytes, or
        a uint8 array), decoded on the device.  A proof that does not decode counts as invalid and leaves the others' verdicts alone.
        -> all_valid, followed by the per-proof bool array with each=True and by the [k, 3] decode statuses (A, B, C: 0 ok ... 5
        not in the subgroup, as the validating host decoder reports them) with status=True.  Batches shorter than the option
        "verify_wire_min" are decoded and answered on the host."""
        return self._verify_wire("verify_batch_wire", pvk, "limbs", (public_inputs,), proof_bytes, rho, each, status)

    def verify_each(self, pvk, public_inputs, proofs, infs):
        """What verify_prepared says of each of K proofs under one prepared key, in one device pass (zkg16_verify_each; arguments as
        verify_batch, no multipliers) -> bool array [k].  The cost does not depend on how many of the proofs are bad."""
        return self._verify_each("verify_each", pvk, "limbs", (public_inputs,), proofs, infs)

    # ---- the prime form: K prime requests of one trapdoor under the extended key (circuits.prime_vk_extend)
    def verify_prime_batch(self, pvk, xs, js, proofs, infs, rho=None, each=False):
        """verify_batch for K proofs of the prime handler made under one trapdoor (zkg16_verify_prime_batch): pvk = the prepared
        extended key (260 gamma_abc_g1 points), xs / js [k] u64; the 259 public inputs of each proof and the multiplier sums of the
        batch equation are made on the device from those 16 bytes.  Everything else as verify_batch."""
        return self._verify_limbs("verify_prime_batch", pvk, "prime", (xs, js), proofs, infs, rho, each)

    def verify_prime_batch_wire(self, pvk, xs, js, proof_bytes, rho=None, each=False, status=False):
        """verify_batch_wire for the prime form (zkg16_verify_prime_batch_wire): proof_bytes = k x 192 compressed bytes; rho is
        drawn from `secrets` when None.  Returns as verify_batch_wire."""
        return self._verify_wire("verify_prime_batch_wire", pvk, "prime", (xs, js), proof_bytes, rho, each, status)

    def prime_inputs_batch(self, xs, js, public_inputs=False):
        """The inputs kernel by itself (zkg16_prime_inputs_batch) -> (digests [k, 32] u8, n [k] u32), followed by the
        [k, 257, 4] Montgomery public inputs with public_inputs=True: circuits.prime_candidate / prime_public_inputs of each (x, j)."""
        xs, js = _u64(xs).reshape(-1), _u64(js).reshape(-1)
        k = xs.shape[0]
        if js.shape[0] != k:
            raise ValueError("prime_inputs_batch: one j per x")
        dig = np.zeros((k, 32), dtype=np.uint8)
        n = np.zeros(k, dtype=np.uint32)
        pub = np.zeros((k, 257, 4), dtype=np.uint64) if public_inputs else None
        self._check(self.lib.zkg16_prime_inputs_batch(self.ctx, _ptr(xs) if k else None, _ptr(js) if k else None, k, _ptr(dig) if k else None,
                                                      _ptr(n) if k else None, _ptr(pub) if k else None))
        return (dig, n, pub) if public_inputs else (dig, n)

    def prime_rho_sums(self, xs, js, rho, live=None):
        """The sums kernels by themselves (zkg16_prime_rho_sums): rho [k, 2], live [k] bytes or None (all) -> the 260 sums
        sum_k rho_k (1, x_k, bit_0 .. bit_255, n_k, j_k) as Python integers (unreduced)."""
        xs, js, rho = _u64(xs).reshape(-1), _u64(js).reshape(-1), _u64(rho).reshape(-1, 2)
        k = xs.shape[0]
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8).reshape(-1)
        if js.shape[0] != k or rho.shape[0] != k or (live is not None and live.shape[0] != k):
            raise ValueError("prime_rho_sums: one j, one multiplier and one live byte per x")
        sums = np.zeros((260, 4), dtype=np.uint64)
        self._check(self.lib.zkg16_prime_rho_sums(self.ctx, _ptr(xs) if k else None, _ptr(js) if k else None, _ptr(rho) if k else None,
                                                  _ptr(live) if k else None, k, _ptr(sums)))
        return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in sums]

    # ---- the u64 form: keys whose public inputs are plain 64-bit values (the linear-equations route)
    def verify_batch_u64(self, pvk, values, proofs, infs, rho=None, each=False):
        """verify_batch for a key whose public inputs are all plain u64 (zkg16_verify_batch_u64): values [k, num_instance - 1]
        uint64 in the place of the Montgomery limbs; the multiplier sums, sum_i s_i gamma_abc[i] and, when the per-proof pass runs,
        each proof's prepared input are made on the device from them.  With the option "verify_each_after" unset that pass decides
        every proof right after a failed test of the whole batch.  Everything else as verify_batch."""
        return self._verify_limbs("verify_batch_u64", pvk, "u64", (values,), proofs, infs, rho, each)

    def verify_batch_u64_wire(self, pvk, values, proof_bytes, rho=None, each=False, status=False):
        """verify_batch_wire for the u64 form (zkg16_verify_batch_u64_wire): proof_bytes = k x 192 compressed bytes; rho is drawn
        from `secrets` when None.  Returns as verify_batch_wire."""
        return self._verify_wire("verify_batch_u64_wire", pvk, "u64", (values,), proof_bytes, rho, each, status)

    def verify_each_u64(self, pvk, values, proofs, infs):
        """verify_each for the u64 form (zkg16_verify_each_u64) -> bool array [k]."""
        return self._verify_each("verify_each_u64", pvk, "u64", (values,), proofs, infs)

    def u64_rho_sums(self, values, rho, live=None):
        """The u64 form's sums kernels by themselves (zkg16_u64_rho_sums): values [k, m] uint64, rho [k, 2], live [k] bytes or None
        (all) -> the m + 1 sums sum_k rho_k (1, values[k][0], .., values[k][m - 1]) as Python integers (unreduced)."""
        values, rho = _u64(values), _u64(rho).reshape(-1, 2)
        if values.ndim != 2 or values.shape[1] == 0:
            raise ValueError("u64_rho_sums: values is [k, m] with m >= 1")
        k, m = values.shape
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8).reshape(-1)
        if rho.shape[0] != k or (live is not None and live.shape[0] != k):
            raise ValueError("u64_rho_sums: one multiplier and one live byte per row")
        sums = np.zeros((m + 1, 4), dtype=np.uint64)
        self._check(self.lib.zkg16_u64_rho_sums(self.ctx, _ptr(values) if k else None, m, _ptr(rho) if k else None, _ptr(live) if k else None, k, _ptr(sums)))
        return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in sums]

    def u64_prepared_inputs(self, gamma_abc_g1, values, idx=None):
        """The u64 form's X kernel by itself (zkg16_u64_prepared_inputs): gamma_abc_g1 [num_instance, 12] (all-zero limbs: the
        point at infinity), values [rows, num_instance - 1] uint64, idx (None: every row in order) the rows wanted, repeats allowed
        -> (points [n, 12] affine Montgomery limbs, infinity flags [n]): gamma_abc[0] + sum_c values[row][c] gamma_abc[1 + c]."""
        gabc, values = _u64(gamma_abc_g1).reshape(-1, 12), _u64(values)
        if values.ndim != 2 or values.shape[1] != gabc.shape[0] - 1:
            raise ValueError("u64_prepared_inputs: values is [rows, num_instance - 1]")
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        if idx is not None and idx.size and int(idx.max()) >= values.shape[0]:
            raise ValueError("u64_prepared_inputs: idx names a row that is not there")
        n = values.shape[0] if idx is None else idx.shape[0]
        out = np.zeros((n, 12), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.zkg16_u64_prepared_inputs(self.ctx, _ptr(gabc), gabc.shape[0], _ptr(values) if n else None, _ptr(idx) if n else None, n,
                                                       _ptr(out) if n else None, _ptr(inf) if n else None))
        return out, inf

    def final_exp_batch(self, f):
        """The verifier's final exponentiation of n Fq12 values on the device (zkg16_final_exp_batch): [n, 72] -> [n, 72], each row
        bit-equal to final_exp() of that row."""
        f = _u64(f).reshape(-1, 72)
        out = np.zeros_like(f)
        self._check(self.lib.zkg16_final_exp_batch(self.ctx, _ptr(f) if f.shape[0] else None, f.shape[0], _ptr(out) if f.shape[0] else None))
        return out

    def decompress_batch(self, group, data, validate=True):
        """n compressed points of one group back to back, decoded on the device (zkg16_points_decompress_batch) ->
        (limbs [n, 12 | 24], infinity flags [n], statuses [n]).  Nothing raises for a point that does not decode: its status says why
        (1 not compressed, 2 non-canonical infinity, 3 x not reduced, 4 not on the curve, 5 not in the subgroup) and its limbs are
        what the host decoders leave."""
        size, width = (48, 12) if group == "g1" else (96, 24)
        raw = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        if raw.size % size:
            raise ValueError("decompress_batch: a compressed %s point is %d bytes" % (group.upper(), size))
        n = raw.size // size
        out = np.zeros((n, width), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        status = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.lib.zkg16_points_decompress_batch(self.ctx, 1 if group == "g1" else 2, _ptr(raw) if n else None, n, _ptr(out) if n else None,
                                                    _ptr(inf) if n else None, 1 if validate else 0, status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0 and not status[:n].any():
            self._check(rc)
        return out, inf, status[:n].copy()

    # ---- re-randomising
    def rerandomize_batch(self, vk_or_delta, proofs, inf=None, r1=None, r2=None):
        """rerandomize_batch_host with one GPU lane per (proof, group) (zkg16_rerandomize_batch): byte for byte the host form's
        output.  Batches shorter than the option "rerandomize_min" are answered by the host form."""
        proofs, inf, k = _rerandomize_limbs(proofs, inf)
        delta, r1, r2 = _rerandomize_args(vk_or_delta, k, r1, r2)
        out = np.zeros((k, 48), dtype=np.uint64)
        oinf = np.zeros((k, 3), dtype=np.uint8)
        self._check(self.lib.zkg16_rerandomize_batch(self.ctx, _ptr(delta), _ptr(proofs) if k else None, _ptr(inf), _ptr(r1) if k else None,
                                                     _ptr(r2) if k else None, k, _ptr(out), _ptr(oinf)))
        return out, oinf

    def rerandomize_batch_wire(self, vk_or_delta, proof_bytes, r1=None, r2=None, status=True):
        """K compressed proofs (k x 192 bytes: bytes or a uint8 array) re-randomised without leaving the device between decoding
        and encoding (zkg16_rerandomize_batch_wire) -> (bytes [k, 192] uint8, statuses [k, 3]).  A proof with a point that does not
        decode or is not in the subgroup has its status set (1 .. 5, as verify_batch_wire's) and 192 zero bytes; the others are
        unaffected.  status=False: only the bytes, and such a proof raises."""
        raw, k = _wire_bytes("rerandomize_batch_wire", proof_bytes)
        delta, r1, r2 = _rerandomize_args(vk_or_delta, k, r1, r2)
        out = np.zeros((k, 192), dtype=np.uint8)
        st = np.zeros((k, 3), dtype=np.uint8) if status else None
        self._check(self.lib.zkg16_rerandomize_batch_wire(self.ctx, _ptr(delta), _ptr(raw) if k else None, _ptr(r1) if k else None, _ptr(r2) if k else None, k,
                                                          _ptr(out), _ptr(st)))
        return (out, st) if status else out

    def points_compress_batch(self, group, points, inf=None):
        """wire.points_compress on the device (zkg16_points_compress_batch): [n, 12 | 24] Montgomery limbs, optional flags -> bytes."""
        w, nb = (12, 48) if group == "g1" else (24, 96)
        pts = _u64(points).reshape(-1, w)
        n = pts.shape[0]
        inf = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
        if inf is not None and inf.shape[0] != n:
            raise ValueError("points_compress_batch: one infinity flag per point")
        out = np.zeros(n * nb, dtype=np.uint8)
        self._check(self.lib.zkg16_points_compress_batch(self.ctx, 1 if group == "g1" else 2, _ptr(pts) if n else None, _ptr(inf) if n else None, n,
                                                         _ptr(out) if n else None))
        return out.tobytes()

    def rerandomize_timings(self):
        """ms of the last rerandomize_batch / rerandomize_batch_wire: upload, decode + membership kernels (wire), the G1 kernel, the
        G2 kernel (side by side), the compress kernel (wire), read-back, total wall, and whether the host form answered."""
        names = ("upload_ms", "decode_ms", "g1_ms", "g2_ms", "compress_ms", "readback_ms", "total_ms", "host_form")
        ms = (C.c_float * 8)()
        n = self.lib.zkg16_rerandomize_timings(self.ctx, ms, 8)
        return {names[i]: float(ms[i]) for i in range(n)}

    def verify_batch_timings(self, prime=False, u64=False):
        """ms of the last verify_batch / verify_batch_wire: membership, scaling + Miller, product tree, MSM, host equation, bisecting,
        total wall, whether the host form answered, the decode kernels (verify_batch_wire only), the per-proof pass that took over
        from bisecting (0 when it did not run) and the number of range tests bisecting made.  prime=True (after verify_prime_batch /
        verify_prime_batch_wire) adds prime_inputs_ms and prime_sums_ms, the two kernels of the prime form's front (0 when the host
        form answered or the last call was not a prime call).  u64=True (after verify_batch_u64 / verify_batch_u64_wire) adds those
        and u64_sums_ms and u64_x_ms, the sums kernels and the X kernel of the u64 form's per-proof pass (0 when the host form
        answered, the last call was not a u64 call or that pass did not run); after those calls range_tests counts the test of the
        whole batch too."""
        names = ("membership_ms", "miller_ms", "product_ms", "msm_ms", "host_ms", "bisect_ms", "total_ms", "host_form", "decode_ms", "each_ms", "range_tests",
                 "prime_inputs_ms", "prime_sums_ms", "u64_sums_ms", "u64_x_ms")
        cap = 15 if u64 else 13 if prime else 11
        ms = (C.c_float * cap)()
        n = self.lib.zkg16_verify_batch_timings(self.ctx, ms, cap)
        return {names[i]: float(ms[i]) for i in range(n)}

    def miller_loop_batch(self, g1, g2, g1_inf=None, g2_inf=None):
        """n Miller loops on the device, one GPU lane per pair (zkg16_miller_loop_batch): g1 [n, 12], g2 [n, 24] -> [n, 72] (ark's
        Fq12 tower order); a pair with a point at infinity gives one.  final_exp() of a row is that pair's pairing."""
        g1 = _u64(g1).reshape(-1, 12)
        g2 = _u64(g2).reshape(-1, 24)
        if g1.shape[0] != g2.shape[0]:
            raise ValueError("miller_loop_batch: one G2 point per G1 point")
        i1, i2 = _opt_u8(g1_inf), _opt_u8(g2_inf)
        out = np.zeros((g1.shape[0], 72), dtype=np.uint64)
        self._check(self.lib.zkg16_miller_loop_batch(self.ctx, _ptr(g1), _ptr(i1), _ptr(g2), _ptr(i2), g1.shape[0], _ptr(out)))
        return out

    def point_check_batch(self, group, points, inf=None):
        """What point_check says of each of n affine points, on the device (zkg16_point_check_batch) -> bool array."""
        pts = _u64(points).reshape(-1, 12 if group == "g1" else 24)
        fl = _opt_u8(inf)
        out = np.zeros(pts.shape[0], dtype=np.uint8)
        self._check(self.lib.zkg16_point_check_batch(self.ctx, 1 if group == "g1" else 2, _ptr(pts), _ptr(fl), pts.shape[0], _ptr(out)))
        return out.astype(bool)

    def points_check_bulk(self, group, points, inf=None):
        """How many of n affine points fail point_check, and the smallest index of one, on the device by the kernels of pk_check
        (zkg16_points_check_bulk) -> (n_bad, first_bad); first_bad is 2^64 - 1 when none failed."""
        pts = _u64(points).reshape(-1, 12 if group == "g1" else 24)
        fl = _opt_u8(inf)
        n_bad, first_bad = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.zkg16_points_check_bulk(self.ctx, 1 if group == "g1" else 2, _ptr(pts) if pts.shape[0] else None, _ptr(fl), pts.shape[0],
                                                     C.byref(n_bad), C.byref(first_bad)))
        return int(n_bad.value), int(first_bad.value)

    def prove_matrix(self, pk_h, r1cs_h, a, b, r, s):
        """One matrix-handler request on resident matrices: assignment built on the device while the proof already runs
        (zkg16_prove_matrix) -> (proof, inf, public inputs [3, 4], dict of ms)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        n = a.shape[0]
        if a.shape != (n, n) or b.shape != (n, n):
            raise ValueError("prove_matrix: a and b must be n x n")
        proof = np.zeros(48, dtype=np.uint64)
        inf = np.zeros(3, dtype=np.uint8)
        pub = np.zeros((3, 4), dtype=np.uint64)
        ms = (C.c_float * 3)()
        self._check(self.lib.zkg16_prove_matrix(self.ctx, pk_h, r1cs_h, n, a.reshape(-1), b.reshape(-1), _u64(r), _u64(s), proof, inf,
                                                pub.ctypes.data, C.addressof(ms)))
        return proof, inf, pub, dict(host_sponges_ms=float(ms[0]), parts=int(ms[1]), call_ms=float(ms[2]))

    def prove_matrix_batch(self, pk_h, r1cs_h, a, b, rs, ss):
        """k matrix-handler requests of one size on one resident key, a and b [k, n, n], rs / ss [k, 4]: assignments and proofs in
        batched device passes (zkg16_prove_matrix_batch) -> (proofs [k, 48], inf [k, 3], public inputs [k, 3, 4], dict of ms).  Proof i
        is byte-identical to prove_resident on witness_matrix(a[i], b[i]) with (rs[i], ss[i])."""
        a, b, k, n = self._matrix_batch("prove_matrix_batch", a, b)
        rs, ss = _rs_ss("prove_matrix_batch", rs, ss, k)
        proofs, inf = _proof_outputs(k)
        pub = np.zeros((k, 3, 4), dtype=np.uint64)
        ms = (C.c_float * 4)()
        self._check(self.lib.zkg16_prove_matrix_batch(self.ctx, pk_h, r1cs_h, n, _ptr(a), _ptr(b), k, _ptr(rs), _ptr(ss), _ptr(proofs), _ptr(inf),
                                                      _ptr(pub), C.addressof(ms)))
        return proofs, inf, pub, _ms(ms, "host_sponges_ms", "witness_ms", "prove_ms", "call_ms")

    def prove_fibonacci_batch(self, pk_h, r1cs_h, steps, a, b, rs, ss):
        """k Fibonacci-handler requests of one round count on one resident key, a and b [k] u64, rs / ss [k, 4]: assignments and proofs
        in batched device passes (zkg16_prove_fibonacci_batch) -> (proofs [k, 48], inf [k, 3], public inputs [k, 3, 4] = a, b, result,
        dict of ms).  pk_h: a key set up on r1cs_fibonacci(steps) = r1cs_h.  Proof i is byte-identical to prove_resident on the
        circuit_load handles of fibonacci_circuit(a[i], b[i], steps) with (rs[i], ss[i])."""
        a, b, k = self._fibonacci_batch("prove_fibonacci_batch", a, b)
        rs, ss = _rs_ss("prove_fibonacci_batch", rs, ss, k)
        proofs, inf = _proof_outputs(k)
        pub = np.zeros((k, 3, 4), dtype=np.uint64)
        ms = (C.c_float * 4)()
        self._check(self.lib.zkg16_prove_fibonacci_batch(self.ctx, pk_h, r1cs_h, steps, _ptr(a), _ptr(b), k, _ptr(rs), _ptr(ss), _ptr(proofs),
                                                         _ptr(inf), _ptr(pub), C.addressof(ms)))
        return proofs, inf, pub, _ms(ms, "host_coeffs_ms", "witness_ms", "prove_ms", "call_ms")

    def prove_linear_batch(self, pk_h, r1cs_h, a, b, rs, ss, solver=None):
        """k linear-handler requests of one size on one resident key, a [k, n, n] and b [k, n] u64, rs / ss [k, 4]: assignments and
        proofs in batched device passes (zkg16_prove_linear_batch) -> (proofs [k, 48], inf [k, 3], x [k, n, 4], dict of ms).  pk_h: a
        key set up on r1cs_linear(n) = r1cs_h.  Proof i is byte-identical to prove_resident on the circuit_load handles of
        linear_circuit(a[i], b[i]) with (rs[i], ss[i]) — a proof no verifier accepts when the request's a is not lower-triangular
        enough for the handler's solver (option "check_satisfied" refuses such a batch instead).  solver: as witness_linear_batch's;
        with "elimination" proof i is prove_resident's on linear_circuit(a[i], b[i], solver="elimination") and verifies for every
        non-singular a[i]."""
        a, b, k, n = self._linear_batch("prove_linear_batch", a, b)
        rs, ss = _rs_ss("prove_linear_batch", rs, ss, k)
        proofs, inf = _proof_outputs(k)
        x = np.zeros((k, n, 4), dtype=np.uint64)
        ms = (C.c_float * 4)()
        with self._linear_solver(solver):
            self._check(self.lib.zkg16_prove_linear_batch(self.ctx, pk_h, r1cs_h, n, _ptr(a), _ptr(b), k, _ptr(rs), _ptr(ss), _ptr(proofs),
                                                          _ptr(inf), _ptr(x), C.addressof(ms)))
        return proofs, inf, x, _ms(ms, "host_check_ms", "witness_ms", "prove_ms", "call_ms")

    def prove_prime_batch(self, pk_h, r1cs_h, corr, gamma_abc0, xs, js, rs, ss, public_inputs=True):
        """k prime requests (xs[i], js[i]) on the template key in batched device passes (zkg16_prove_prime_batch).  pk_h: the key
        set up on r1cs_prime_template() = r1cs_h; corr: circuits.prime_key_corrections of its trapdoor; gamma_abc0: its
        gamma_abc_g1[0]; rs / ss [k, 4] -> (proofs [k, 48], inf [k, 3], gamma_abc0 [k, 12]: request i's gamma_abc_g1[0], public
        inputs [k, 257, 4] or None, dict of ms).  Proof and key are byte for byte those of the per-request path."""
        xs, js = _u64(xs).reshape(-1), _u64(js).reshape(-1)
        k = xs.shape[0]
        rs, ss = _rs_ss("prove_prime_batch", rs, ss, k, "one j, r and s per request")
        if js.shape[0] != k:
            raise ValueError("prove_prime_batch: one j, r and s per request")
        corr, gamma_abc0 = _u64(corr).reshape(-1), _u64(gamma_abc0).reshape(-1)
        if corr.size != 36 or gamma_abc0.size != 12:
            raise ValueError("prove_prime_batch: corr 3 x 12 limbs, gamma_abc0 12 limbs")
        proofs, inf = _proof_outputs(k)
        g0 = np.zeros((k, 12), dtype=np.uint64)
        pub = np.zeros((k, 257, 4), dtype=np.uint64) if public_inputs else None
        ms = (C.c_float * 4)()
        self._check(self.lib.zkg16_prove_prime_batch(self.ctx, pk_h, r1cs_h, _ptr(corr), _ptr(gamma_abc0), _ptr(xs), _ptr(js), k, _ptr(rs), _ptr(ss),
                                                     _ptr(proofs), _ptr(inf), _ptr(g0), _ptr(pub), C.addressof(ms)))
        return proofs, inf, g0, pub, _ms(ms, "host_inputs_ms", "witness_ms", "prove_ms", "call_ms")

    def prove(self, pk_h, r, s, r1cs, z):
        args, keep = self._csr(r1cs)
        z = _u64(z).reshape(-1, 4)
        proof = np.zeros(48, dtype=np.uint64)
        inf = np.zeros(3, dtype=np.uint8)
        self._check(self.lib.zkg16_prove(self.ctx, pk_h, _u64(r), _u64(s), *args, r1cs["num_inputs"], r1cs["num_constraints"],
                                         z, z.shape[0], proof, inf))
        return proof, inf

    def prove_partial(self, pk_h, r1cs_h, wit_h, r, s):
        part = np.zeros(72, dtype=np.uint64)
        inf = np.zeros(5, dtype=np.uint8)
        self._check(self.lib.zkg16_prove_partial(self.ctx, pk_h, r1cs_h, wit_h, _u64(r), _u64(s), part, inf))
        return part, inf

    def prove_finish(self, pk_h, r, s, partials, partial_inf):
        partials = _u64(partials).reshape(-1, 72)
        partial_inf = np.ascontiguousarray(partial_inf, dtype=np.uint8).reshape(-1, 5)
        proof = np.zeros(48, dtype=np.uint64)
        inf = np.zeros(3, dtype=np.uint8)
        self._check(self.lib.zkg16_prove_finish(self.ctx, pk_h, _u64(r), _u64(s), partials, partial_inf, partials.shape[0], proof, inf))
        return proof, inf

    # ---- stages
    def ntt(self, data, inverse=False, coset=False):
        d = _u64(data).reshape(-1, 4).copy()
        n = d.shape[0]
        log_n = n.bit_length() - 1
        if 1 << log_n != n:
            raise ValueError("ntt: length %d is not a power of two" % n)
        self._check(self.lib.zkg16_ntt(self.ctx, d, log_n, int(inverse), int(coset)))
        return d

    def msm(self, group, bases, scalars_canonical, inf=None):
        w = 12 if group == "g1" else 24
        bases = _u64(bases).reshape(-1, w)
        sc = _u64(scalars_canonical).reshape(-1, 4)
        n = min(bases.shape[0], sc.shape[0])
        inf = _opt_u8(inf)
        out = np.zeros(w, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        fn = self.lib.zkg16_msm_g1 if group == "g1" else self.lib.zkg16_msm_g2
        self._check(fn(self.ctx, _ptr(bases) if n else None, _ptr(inf), _ptr(sc) if n else None, n, out, oinf))
        return out, int(oinf[0])

    def bench_msm(self, group, bases, scalars_canonical, iters=3, inf=None):
        w = 12 if group == "g1" else 24
        bases = _u64(bases).reshape(-1, w)
        sc = _u64(scalars_canonical).reshape(-1, 4)
        n = min(bases.shape[0], sc.shape[0])
        inf = _opt_u8(inf)
        out = np.zeros(w, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        ms = C.c_float()
        self._check(self.lib.zkg16_bench_msm(self.ctx, 1 if group == "g1" else 2, _ptr(bases), _ptr(inf), _ptr(sc), n, iters,
                                             C.byref(ms), out, oinf))
        return ms.value, out, int(oinf[0])

    def bench_ntt(self, log_n, inverse=False, coset=False, iters=10):
        ms = C.c_float()
        self._check(self.lib.zkg16_bench_ntt(self.ctx, log_n, int(inverse), int(coset), iters, C.byref(ms)))
        return ms.value

    def bench_witness_map(self, r1cs_h, wit_h, iters=3):
        """ms per stand-alone witness map (3 SpMV + 6 NTT, 7 with option wm_transforms = 7) on resident inputs."""
        ms = C.c_float()
        self._check(self.lib.zkg16_bench_witness_map(self.ctx, r1cs_h, wit_h, iters, C.byref(ms)))
        return ms.value

    def witness_map(self, r1cs_h, wit_h, n_max):
        h = np.zeros((n_max, 4), dtype=np.uint64)
        log_n = C.c_size_t()
        self._check(self.lib.zkg16_witness_map(self.ctx, r1cs_h, wit_h, h, C.byref(log_n)))
        return h[: 1 << log_n.value]

    def fixed_base(self, group, base, scalars_canonical):
        w = 12 if group == "g1" else 24
        sc = _u64(scalars_canonical).reshape(-1, 4)
        n = sc.shape[0]
        out = np.zeros((n, w), dtype=np.uint64)
        oinf = np.zeros(n, dtype=np.uint8)
        fn = self.lib.zkg16_fixed_base_g1 if group == "g1" else self.lib.zkg16_fixed_base_g2
        self._check(fn(self.ctx, _u64(base), _ptr(sc), n, _ptr(out), _ptr(oinf)))
        return out, oinf

    # ---- instrumentation
    def last_timings(self):
        buf = (C.c_float * 22)()
        n = self.lib.zkg16_last_timings(self.ctx, buf, 22)
        names = ["spmv", "witness_map", "msm_sort", "msm_h", "msm_l", "msm_a", "msm_b1", "msm_b2", "host_tail", "total_wall"]
        out = {names[i]: float(buf[i]) for i in range(min(n, 10))}
        if n >= 20:
            # device times under the span names of upstream's prover (ark-groth16 prover.rs): accumulate + fix-ups / bucket reduction
            acc = dict(zip("HLA", [float(buf[10]), float(buf[11]), float(buf[12])]), B1=float(buf[13]), B2=float(buf[14]))
            red = dict(zip("HLA", [float(buf[15]), float(buf[16]), float(buf[17])]), B1=float(buf[18]), B2=float(buf[19]))
            out["device_spans"] = {
                "R1CS to QAP witness map": out["witness_map"],
                "scalar digits + bucket scatter": out["msm_sort"],
                "Compute C": {"h_accumulate": acc["H"], "h_reduce": red["H"], "l_accumulate": acc["L"], "l_reduce": red["L"]},
                "Compute A": {"accumulate": acc["A"], "reduce": red["A"]},
                "Compute B in G1": {"accumulate": acc["B1"], "reduce": red["B1"]},
                "Compute B in G2": {"accumulate": acc["B2"], "reduce": red["B2"]},
                "Finish C": out["host_tail"],
            }
        if n >= 22:     # host Horner over window sums: H's runs after the proof's last device event, the others under H's device work
            out["host_horner_h"], out["host_horner_others"] = float(buf[20]), float(buf[21])
        return out

    def kernel_timing(self, enable=True):
        """0/False off, 1/True all kernel families, 2 only the bucket accumulations"""
        self._check(self.lib.zkg16_kernel_timing(self.ctx, int(enable)))

    def kernel_stats(self, name):
        launches, ms, units = C.c_uint64(), C.c_double(), C.c_double()
        self._check(self.lib.zkg16_kernel_stats(self.ctx, name.encode(), C.byref(launches), C.byref(ms), C.byref(units)))
        return dict(launches=launches.value, ms=ms.value, units=units.value)

    def kernel_stats_reset(self):
        self.lib.zkg16_kernel_stats_reset(self.ctx)

    def set_option(self, name, value):
        self._check(self.lib.zkg16_set_option(self.ctx, name.encode(), int(value)))
        self._options[name] = int(value)


def z_costs(r1cs, z_mont, num_instance):
    """Per-index cost of the z-side MSM terms in G1 mixed additions, for shard_plan: (entries of the scalar: 0 for a zero, 1 for a
    one, one per window otherwise) x (queries whose base exists: A if the variable occurs in A or is an instance variable, L if it
    is a witness, B1 + 2.8 x B2 if it occurs in B — ark-groth16 keeps the point at infinity for the rest)."""
    z = _u64(z_mont).reshape(-1, 4)
    m = z.shape[0]
    n = m + 3
    nwin = 254 // (17 if n >= (1 << 23) else 16 if n >= (1 << 20) else 15 if n >= (1 << 17) else 13 if n >= (1 << 14) else max(4, n.bit_length() - 4)) + 1
    one = np.array([0x00000001fffffffe, 0x5884b7fa00034802, 0x998c4fefecbc4ff5, 0x1824b159acc5056f], dtype=np.uint64)      # 2^256 mod r
    is_zero = ~z.any(axis=1)
    is_one = (z == one).all(axis=1)
    entries = np.where(is_zero, 0.0, np.where(is_one, 1.0, float(nwin)))
    in_a = np.zeros(m, dtype=bool)
    in_a[np.asarray(r1cs["a"][1], dtype=np.int64)] = True
    in_a[:num_instance] = True
    in_b = np.zeros(m, dtype=bool)
    in_b[np.asarray(r1cs["b"][1], dtype=np.int64)] = True
    mult = in_a.astype(np.float32) + (np.arange(m) >= num_instance) + in_b * 3.8
    return (entries * mult).astype(np.float32)


def table_layout(kind, n, digits, stride_mode=0):
    """Entry layout of a window table (host-only zkg16_table_layout): kind "g1" / "g2", n bases, digits levels; stride_mode as option
    "table_stride" (0 = the library's choice by table size, 1 = packed 112 / 224 bytes, 2 = padded 128 / 256) -> (entry stride, bytes of the table)."""
    stride, size = C.c_size_t(0), C.c_uint64(0)
    _check_host(_lib.load().zkg16_table_layout({"g1": 1, "g2": 2}.get(kind, 0), n, digits, stride_mode, C.byref(stride), C.byref(size)))
    return stride.value, size.value


def matrix_variables(n):
    """Variables of the MatrixCircuit of size n: the constant, the three hashes and the witnesses (host-only zkg16_matrix_r1cs_dims)."""
    nc, nw = C.c_size_t(0), C.c_size_t(0)
    _check_host(_lib.load().zkg16_matrix_r1cs_dims(n, C.byref(nc), C.byref(nw), None))
    return 4 + nw.value


def matrix_stream_bounds(n, parts_wanted=0, slice_min=0):
    """The slices prove_matrix feeds a proof of size n in under options matrix_parts = parts_wanted and matrix_slice_min = slice_min
    (host-only zkg16_matrix_stream_bounds) -> list of slices + 1 permutation indices, from 0 to ceil(n^2 / 2)."""
    bounds = np.zeros(9, dtype=np.uint32)
    k = C.c_int(0)
    _check_host(_lib.load().zkg16_matrix_stream_bounds(n, int(parts_wanted), int(slice_min), bounds.ctypes.data, C.byref(k)))
    return [int(x) for x in bounds[:k.value + 1]]


def shard_plan(n_ranks, m_total, n_h, b_density=0.0, h_ranks=0, z_cost=None, window_tables=False):
    """Rank roles of one proof over n_ranks GPUs (host-only zkg16_shard_plan / zkg16_shard_plan_tables) ->
    (list of (z_lo, z_hi, h_lo, h_hi, blinding) per rank, number of ranks that run the witness map).
    z_cost: optional per-index costs (z_costs) so that the z ranges are cut by work, not by index count.
    window_tables: the shards will carry window tables (pk_precompute): the cost factors measured for that case."""
    lib = _lib.load()
    ranges = np.zeros(4 * n_ranks, dtype=np.uint64)
    blind = np.zeros(n_ranks, dtype=np.uint8)
    k = C.c_int(0)
    zc = None if z_cost is None else np.ascontiguousarray(z_cost, dtype=np.float32)
    if zc is not None and zc.shape[0] != m_total:
        raise ValueError("shard_plan: z_cost has %d entries, m_total is %d" % (zc.shape[0], m_total))
    _check_host(lib.zkg16_shard_plan_tables(n_ranks, m_total, n_h, float(b_density), h_ranks, _ptr(zc), int(bool(window_tables)), ranges, blind, C.byref(k)))
    r = ranges.reshape(n_ranks, 4)
    return [(int(r[i, 0]), int(r[i, 1]), int(r[i, 2]), int(r[i, 3]), bool(blind[i])) for i in range(n_ranks)], k.value


def combine_partials(alpha_g1, beta_g1, beta_g2, r, s, partials, partial_inf):
    """Host-only finish step (no GPU): see zkg16_combine_partials in include/zkg16.h."""
    lib = _lib.load()
    partials = _u64(partials).reshape(-1, 72)
    partial_inf = np.ascontiguousarray(partial_inf, dtype=np.uint8).reshape(-1, 5)
    proof = np.zeros(48, dtype=np.uint64)
    inf = np.zeros(3, dtype=np.uint8)
    rc = lib.zkg16_combine_partials(_u64(alpha_g1), _u64(beta_g1), _u64(beta_g2), _u64(r), _u64(s), partials, partial_inf,
                                    partials.shape[0], proof, inf)
    _check_host(rc)
    return proof, inf


def _setup(self, r1cs_h, num_instance, num_vars, domain, trapdoor_mont, g1_gen, g2_gen):
    """Groth16 setup on the device from a known trapdoor (zkg16_setup) -> (pk dict for pk_load, vk dict)."""
    nw = num_vars - num_instance
    pk = dict(a_query=np.zeros((num_vars, 12), np.uint64), a_inf=np.zeros(num_vars, np.uint8),
              b_g1_query=np.zeros((num_vars, 12), np.uint64), b_g1_inf=np.zeros(num_vars, np.uint8),
              b_g2_query=np.zeros((num_vars, 24), np.uint64), b_g2_inf=np.zeros(num_vars, np.uint8),
              h_query=np.zeros((max(domain - 1, 1), 12), np.uint64), l_query=np.zeros((max(nw, 1), 12), np.uint64),
              l_inf=np.zeros(max(nw, 1), np.uint8),
              alpha_g1=np.zeros(12, np.uint64), beta_g1=np.zeros(12, np.uint64), beta_g2=np.zeros(24, np.uint64),
              delta_g1=np.zeros(12, np.uint64), delta_g2=np.zeros(24, np.uint64))
    vk = dict(gamma_g2=np.zeros(24, np.uint64), gamma_abc_g1=np.zeros((num_instance, 12), np.uint64))
    self._check(self.lib.zkg16_setup(
        self.ctx, r1cs_h, _u64(trapdoor_mont).reshape(-1), _u64(g1_gen), _u64(g2_gen),
        pk["a_query"], _ptr(pk["a_inf"]), pk["b_g1_query"], _ptr(pk["b_g1_inf"]), pk["b_g2_query"], _ptr(pk["b_g2_inf"]),
        _ptr(pk["h_query"]), _ptr(pk["l_query"]), _ptr(pk["l_inf"]),
        pk["alpha_g1"], pk["beta_g1"], pk["beta_g2"], pk["delta_g1"], pk["delta_g2"], vk["gamma_g2"], vk["gamma_abc_g1"]))
    pk["h_query"] = pk["h_query"][:domain - 1]
    pk["l_query"], pk["l_inf"] = pk["l_query"][:nw], pk["l_inf"][:nw]
    vk.update(alpha_g1=pk["alpha_g1"], beta_g2=pk["beta_g2"], delta_g2=pk["delta_g2"])
    return pk, vk


Device.setup = _setup


def verify(vk, public_inputs_mont, proof48, inf3):
    """Host-only Groth16 verification (zkg16_verify).  vk: dict alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1 (n x 12)."""
    lib = _lib.load()
    gabc = _u64(vk["gamma_abc_g1"]).reshape(-1, 12)
    pub = _u64(public_inputs_mont).reshape(-1, 4)
    if pub.shape[0] != gabc.shape[0] - 1:          # a real exception: the C side reads num_instance - 1 inputs
        raise ValueError("verify: %d public inputs for a key with %d instance variables" % (pub.shape[0], gabc.shape[0]))
    ok = C.c_int(0)
    rc = lib.zkg16_verify(_u64(vk["alpha_g1"]), _u64(vk["beta_g2"]), _u64(vk["gamma_g2"]), _u64(vk["delta_g2"]), gabc, gabc.shape[0],
                          _ptr(pub) if pub.size else None, _u64(proof48), np.ascontiguousarray(inf3, dtype=np.uint8), C.byref(ok))
    _check_host(rc)
    return bool(ok.value)


def _setup_resident(self, r1cs_h, num_instance, trapdoor_mont, g1_gen, g2_gen):
    """Groth16 setup with the key kept on the device (zkg16_setup_resident) -> (pk handle, vk dict)."""
    vk = dict(alpha_g1=np.zeros(12, np.uint64), beta_g2=np.zeros(24, np.uint64), gamma_g2=np.zeros(24, np.uint64),
              delta_g2=np.zeros(24, np.uint64), gamma_abc_g1=np.zeros((num_instance, 12), np.uint64))
    h = C.c_uint64()
    self._check(self.lib.zkg16_setup_resident(self.ctx, r1cs_h, _u64(trapdoor_mont).reshape(-1), _u64(g1_gen), _u64(g2_gen), C.byref(h),
                                              vk["alpha_g1"], vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"], vk["gamma_abc_g1"]))
    return h.value, vk


Device.setup_resident = _setup_resident


def prove_trapdoor_host(r1cs, z, trapdoor_mont, g1_gen, g2_gen, rs, ss, threads=0):
    """The trapdoor route without a device (zkg16_prove_trapdoor_host): r1cs = the dict r1cs_load takes, z [k, num_variables, 4] (or
    [num_variables, 4] for one request), rs / ss [k, 4] -> (proofs [k, 48], inf [k, 3], vk dict shaped as setup_resident's).  The
    reference for every byte of Device.prove_trapdoor[_batch]."""
    lib = _lib.load()
    z = _u64(z)
    z = z.reshape((1,) + z.shape) if z.ndim == 2 else z
    k, nv = z.shape[0], z.shape[1]
    rs, ss = _u64(rs).reshape(-1, 4), _u64(ss).reshape(-1, 4)
    if rs.shape[0] != k or ss.shape[0] != k:
        raise ValueError("prove_trapdoor_host: one r and one s per assignment")
    ni = int(r1cs["num_inputs"])
    keep, tabs = [], []
    for i, dt in ((0, np.uint64), (1, np.uint32), (2, np.uint64)):
        arrs = [np.ascontiguousarray(r1cs[m][i], dtype=dt) for m in "abc"]
        keep += arrs
        tabs.append((C.c_void_p * 3)(*[x.ctypes.data if x.size else None for x in arrs]))
    if any(x.shape[0] != r1cs["num_constraints"] + 1 for x in keep[:3]):
        raise ValueError("prove_trapdoor_host: every row pointer has num_constraints + 1 entries")
    proofs = np.zeros((k, 48), dtype=np.uint64)
    inf = np.zeros((k, 3), dtype=np.uint8)
    vk = dict(alpha_g1=np.zeros(12, np.uint64), beta_g2=np.zeros(24, np.uint64), gamma_g2=np.zeros(24, np.uint64),
              delta_g2=np.zeros(24, np.uint64), gamma_abc_g1=np.zeros((ni, 12), np.uint64))
    trap, g1, g2 = _u64(trapdoor_mont).reshape(-1), _u64(g1_gen), _u64(g2_gen)
    _check_host(lib.zkg16_prove_trapdoor_host(C.byref(tabs[0]), C.byref(tabs[1]), C.byref(tabs[2]), ni, r1cs["num_constraints"], nv, _ptr(z), k, _ptr(trap), _ptr(g1), _ptr(g2), _ptr(rs), _ptr(ss),
                                              int(threads), _ptr(proofs), _ptr(inf), _ptr(vk["alpha_g1"]), _ptr(vk["beta_g2"]), _ptr(vk["gamma_g2"]),
                                              _ptr(vk["delta_g2"]), _ptr(vk["gamma_abc_g1"])))
    return proofs, inf, vk


def pairing_check(g1_points, g2_points, g1_inf=None, g2_inf=None, plain_final_exp=False):
    """prod e(P_i, Q_i) == 1 on the host (zkg16_pairing_check).  g1_points: n x 12, g2_points: n x 24 Montgomery limbs."""
    lib = _lib.load()
    g1 = _u64(g1_points).reshape(-1, 12)
    g2 = _u64(g2_points).reshape(-1, 24)
    if g1.shape[0] != g2.shape[0]:
        raise ValueError("pairing_check: %d G1 points against %d G2 points" % (g1.shape[0], g2.shape[0]))
    n = g1.shape[0]
    i1 = np.ascontiguousarray(g1_inf if g1_inf is not None else np.zeros(n), dtype=np.uint8)
    i2 = np.ascontiguousarray(g2_inf if g2_inf is not None else np.zeros(n), dtype=np.uint8)
    ok = C.c_int(0)
    _check_host(lib.zkg16_pairing_check(g1, i1, g2, i2, n, 1 if plain_final_exp else 0, C.byref(ok)))
    return bool(ok.value)


def scalar_mul(group, base, k_canonical):
    """[k] base on the host (zkg16_scalar_mul_g1/g2) -> (affine limbs, inf)."""
    lib = _lib.load()
    w = 12 if group == "g1" else 24
    out = np.zeros(w, dtype=np.uint64)
    inf = C.c_uint8(0)
    fn = lib.zkg16_scalar_mul_g1 if group == "g1" else lib.zkg16_scalar_mul_g2
    rc = fn(_u64(base).reshape(-1), _u64(k_canonical).reshape(-1), out, C.byref(inf))
    _check_host(rc)
    return out, int(inf.value)


def point_check(group, point):
    """Curve + prime-order-subgroup membership of one affine point (zkg16_point_check; host-only)."""
    lib = _lib.load()
    ok = C.c_int(0)
    _check_host(lib.zkg16_point_check(1 if group == "g1" else 2, _u64(point).reshape(-1), C.byref(ok)))
    return bool(ok.value)


def pvk_prepare(vk):
    """prepare_verifying_key (host-only zkg16_pvk_prepare): vk dict -> the same dict plus alpha_beta (72 u64: ark's Fq12 tower
    order) and gamma_neg_pc / delta_neg_pc (68 x 36 u64 line coefficients each)."""
    lib = _lib.load()
    ab = np.zeros(72, dtype=np.uint64)
    g = np.zeros(68 * 36, dtype=np.uint64)
    d = np.zeros(68 * 36, dtype=np.uint64)
    n = C.c_size_t(0)
    _check_host(lib.zkg16_pvk_prepare(_u64(vk["alpha_g1"]), _u64(vk["beta_g2"]), _u64(vk["gamma_g2"]), _u64(vk["delta_g2"]), ab, g, d, C.byref(n)))
    out = dict(vk)
    out.update(alpha_beta=ab, gamma_neg_pc=g.reshape(n.value, 36), delta_neg_pc=d.reshape(n.value, 36))
    return out


def verify_prepared(pvk, public_inputs_mont, proof48, inf3):
    """Groth16::verify_with_processed_vk on a prepared key (host-only zkg16_verify_prepared)."""
    lib = _lib.load()
    gabc = _u64(pvk["gamma_abc_g1"]).reshape(-1, 12)
    pub = _u64(public_inputs_mont).reshape(-1, 4)
    if pub.shape[0] != gabc.shape[0] - 1:
        raise ValueError("verify_prepared: %d public inputs for a key with %d instance variables" % (pub.shape[0], gabc.shape[0]))
    g, d = _u64(pvk["gamma_neg_pc"]).reshape(-1, 36), _u64(pvk["delta_neg_pc"]).reshape(-1, 36)
    ok = C.c_int(0)
    rc = lib.zkg16_verify_prepared(gabc, gabc.shape[0], _ptr(pub) if pub.size else None, _u64(pvk["alpha_beta"]), g, d, g.shape[0],
                                   _u64(proof48), np.ascontiguousarray(inf3, dtype=np.uint8), C.byref(ok))
    _check_host(rc)
    return bool(ok.value)


def draw_rho(k):
    """k non-zero 128-bit multipliers for a batch verification, from the operating system's generator -> [k, 2] u64."""
    import secrets
    out = np.zeros((k, 2), dtype=np.uint64)
    for i in range(k):
        v = 0
        while v == 0:
            v = secrets.randbits(128)
        out[i, 0], out[i, 1] = v & ((1 << 64) - 1), v >> 64
    return out


_FR_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def draw_rerandomizers(k):
    """k non-zero elements of Fr from the operating system's generator, a zero redrawn as ark-groth16's rerandomize_proof redraws it
    -> [k, 4] u64 Montgomery limbs."""
    import secrets
    out = np.zeros((k, 4), dtype=np.uint64)
    for i in range(k):
        v = 0
        while v == 0:
            v = secrets.randbelow(_FR_MOD)
        m = (v << 256) % _FR_MOD
        out[i] = [(m >> (64 * t)) & ((1 << 64) - 1) for t in range(4)]
    return out


def _rerandomize_args(vk_or_delta, k, r1, r2):
    """(delta_g2 [24], r1 [k, 4], r2 [k, 4]) of the three re-randomising entries; vk_or_delta: a key dict or the 24 limbs"""
    delta = _u64(vk_or_delta["delta_g2"] if isinstance(vk_or_delta, dict) else vk_or_delta).reshape(-1)
    if delta.shape[0] != 24:
        raise ValueError("rerandomize: delta_g2 is 24 limbs")
    r1 = draw_rerandomizers(k) if r1 is None else _u64(r1).reshape(-1, 4)
    r2 = draw_rerandomizers(k) if r2 is None else _u64(r2).reshape(-1, 4)
    if r1.shape[0] != k or r2.shape[0] != k:
        raise ValueError("rerandomize: one r1 and one r2 per proof")
    return delta, r1, r2


def _rerandomize_limbs(proofs, inf):
    proofs = _u64(proofs).reshape(-1, 48)
    k = proofs.shape[0]
    inf = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1, 3)
    if inf is not None and inf.shape[0] != k:
        raise ValueError("rerandomize: three infinity flags per proof")
    return proofs, inf, k


def rerandomize_batch_host(vk_or_delta, proofs, inf=None, r1=None, r2=None, threads=0):
    """K proofs of one key re-randomised on host threads (zkg16_rerandomize_batch_host; no GPU): A' = r1^-1 A, B' = r1 B + r1 r2 delta,
    C' = C + r2 A.  proofs [k, 48], inf [k, 3] or None, r1 / r2 [k, 4] Montgomery and non-zero (None: drawn from `secrets`)
    -> (proofs [k, 48], inf [k, 3]).  The new proofs verify for exactly the inputs the old ones verify for."""
    proofs, inf, k = _rerandomize_limbs(proofs, inf)
    delta, r1, r2 = _rerandomize_args(vk_or_delta, k, r1, r2)
    out = np.zeros((k, 48), dtype=np.uint64)
    oinf = np.zeros((k, 3), dtype=np.uint8)
    lib = _lib.load()
    rc = lib.zkg16_rerandomize_batch_host(_ptr(delta), _ptr(proofs) if k else None, _ptr(inf), _ptr(r1) if k else None, _ptr(r2) if k else None, k, threads,
                                          _ptr(out), _ptr(oinf))
    if rc != 0:
        detail = lib.zkg16_last_error(None).decode()
        raise Zkg16Error(rc, lib.zkg16_strerror(rc).decode() + (" — " + detail if detail else ""))
    return out, oinf


class _KeepAlive(tuple):
    def __new__(cls, items, keep):
        self = super().__new__(cls, items)
        self.keep = keep
        return self


_VERIFY_FORMS = {"limbs": "verify_batch", "prime": "verify_prime_batch", "u64": "verify_batch_u64"}


def _verify_args(pvk, kind, inputs, proofs, infs, rho, k=None):
    """The argument tuple the verification entry points share: the key (6), the form's inputs, proofs, infs, rho, k.  kind / inputs:
    "limbs" / (public_inputs [k, num_instance - 1, 4],), "prime" / (xs [k], js [k]) or "u64" / (values [k, num_instance - 1],).
    proofs = infs = None with k given: the wire form, which has no limbs yet"""
    who = _VERIFY_FORMS[kind]
    gabc = _u64(pvk["gamma_abc_g1"]).reshape(-1, 12)
    proofs = _u64(proofs).reshape(-1, 48) if proofs is not None else None
    k = proofs.shape[0] if proofs is not None else k
    infs = np.ascontiguousarray(infs, dtype=np.uint8).reshape(-1, 3) if proofs is not None else None
    if kind == "limbs":
        pub = _u64(inputs[0])
        # (k, -1, 4) cannot be inferred for an empty array: no proofs, or a key with one instance variable and so no inputs
        pub = pub.reshape(k, -1, 4) if pub.size else pub.reshape(k, 0 if k else gabc.shape[0] - 1, 4)
        if pub.shape[1] != gabc.shape[0] - 1:
            raise ValueError("verify_batch: %d public inputs per proof for a key with %d instance variables" % (pub.shape[1], gabc.shape[0]))
        inputs, there = (pub,), pub.size
    elif kind == "prime":
        inputs = tuple(_u64(a).reshape(-1) for a in inputs)
        if inputs[0].shape[0] != k or inputs[1].shape[0] != k:
            raise ValueError("verify_prime_batch: one x and one j per proof")
        there = k
    else:
        inputs = (_u64(inputs[0]),)
        if gabc.shape[0] < 2 or inputs[0].shape != (k, gabc.shape[0] - 1):
            raise ValueError("verify_batch_u64: values is [k, num_instance - 1] for a key with at least two instance variables")
        there = k
    if infs is not None and infs.shape[0] != k:
        raise ValueError("%s: one flag triple per proof" % who)
    rho = draw_rho(k) if rho is None else _u64(rho).reshape(-1, 2)
    if rho.shape[0] != k:
        raise ValueError("%s: one multiplier per proof" % who)
    g, d = _u64(pvk["gamma_neg_pc"]).reshape(-1, 36), _u64(pvk["delta_neg_pc"]).reshape(-1, 36)
    ab = _u64(pvk["alpha_beta"])
    # the arrays must outlive the call: they travel in the tuple
    keep = (gabc, ab, g, d) + inputs + (proofs, infs, rho)
    return _KeepAlive((_ptr(gabc), gabc.shape[0], _ptr(ab), _ptr(g), _ptr(d), g.shape[0]) + tuple(_ptr(a) if there else None for a in inputs)
                      + (_ptr(proofs), _ptr(infs), _ptr(rho), k), keep), k


def _wire_bytes(who, proof_bytes):
    """k x 192 compressed proof bytes (bytes, bytearray, memoryview or a uint8 array) -> (the bytes as a flat uint8 array, k)"""
    raw = np.ascontiguousarray(np.frombuffer(proof_bytes, dtype=np.uint8) if isinstance(proof_bytes, (bytes, bytearray, memoryview))
                               else np.asarray(proof_bytes, dtype=np.uint8)).reshape(-1)
    if raw.size % 192:
        raise ValueError("%s: a compressed proof is 192 bytes" % who)
    return raw, raw.size // 192


def _verify_result(ok, ok_each=None, status=None):
    """all_valid, followed by the per-proof bool array and the decode statuses where the caller asked for them"""
    out = (bool(ok.value),) + (() if ok_each is None else (ok_each.astype(bool),)) + (() if status is None else (status,))
    return out if len(out) > 1 else out[0]


def _verify_host(entry, pvk, kind, inputs, proofs, infs, rho, each, threads):
    lib = _lib.load()
    args, k = _verify_args(pvk, kind, inputs, proofs, infs, rho)
    ok = C.c_int(0)
    ok_each = np.zeros(k, dtype=np.uint8) if each else None
    _check_host(getattr(lib, entry)(*args, threads, C.byref(ok), _ptr(ok_each)))
    return _verify_result(ok, ok_each)


def verify_batch_u64_host(pvk, values, proofs, infs, rho=None, each=False, threads=0):
    """Device.verify_batch_u64's verdicts on host threads alone (zkg16_verify_batch_u64_host; threads 0 = 8; no GPU): the values are
    expanded to Montgomery limbs and verify_batch_host answers."""
    return _verify_host("zkg16_verify_batch_u64_host", pvk, "u64", (values,), proofs, infs, rho, each, threads)


def verify_prime_batch_host(pvk, xs, js, proofs, infs, rho=None, each=False, threads=0):
    """Device.verify_prime_batch's verdicts on host threads alone (zkg16_verify_prime_batch_host; threads 0 = 8; no GPU)."""
    return _verify_host("zkg16_verify_prime_batch_host", pvk, "prime", (xs, js), proofs, infs, rho, each, threads)


def verify_batch_host(pvk, public_inputs, proofs, infs, rho=None, each=False, threads=0):
    """Device.verify_batch's verdicts on host threads alone (zkg16_verify_batch_host; threads 0 = 8; no GPU)."""
    return _verify_host("zkg16_verify_batch_host", pvk, "limbs", (public_inputs,), proofs, infs, rho, each, threads)


def final_exp(f):
    """The verifier's final exponentiation of one Fq12 value (72 u64, ark's tower order; zkg16_final_exp, host-only)."""
    lib = _lib.load()
    out = np.zeros(72, dtype=np.uint64)
    _check_host(lib.zkg16_final_exp(_u64(f).reshape(-1), out))
    return out


class DeviceGroup:
    """Several Devices of this process proving one proof together (zkg16_group_create): one per GPU, or several on one GPU.
    The ranks whose key shard has an h range split the witness map's seven NTTs between them where the layout applies
    (group_layout); the group keeps its Devices alive and must be closed before them."""

    def __init__(self, devices):
        self.devices = list(devices)
        self.lib = _lib.load()
        self.group = C.c_void_p()
        arr = (C.c_void_p * len(self.devices))(*[d.ctx.value for d in self.devices])
        _check_host(self.lib.zkg16_group_create(arr, len(self.devices), C.byref(self.group)))

    def close(self):
        if self.group:
            self.lib.zkg16_group_destroy(self.group)
            self.group = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            detail = self.lib.zkg16_group_last_error(self.group).decode()
            raise Zkg16Error(rc, self.lib.zkg16_strerror(rc).decode() + (" — " + detail if detail else ""))

    def _handles(self, hs, what):
        hs = np.ascontiguousarray(hs, dtype=np.uint64)
        if hs.shape != (len(self.devices),):
            raise ValueError("%s: one handle per device (%d), got %s" % (what, len(self.devices), hs.shape))
        return hs

    def set_option(self, name, value):
        self._check(self.lib.zkg16_group_set_option(self.group, name.encode(), int(value)))

    def witness_map(self, r1cs_handles, witness_handles, n_max):
        """h of the group's witness map, gathered to the host (zkg16_witness_map_group)."""
        h = np.zeros((n_max, 4), dtype=np.uint64)
        log_n = C.c_size_t()
        self._check(self.lib.zkg16_witness_map_group(self.group, self._handles(r1cs_handles, "r1cs"), self._handles(witness_handles, "witness"),
                                                     h, C.byref(log_n)))
        return h[: 1 << log_n.value]

    def prove(self, pk_handles, r1cs_handles, witness_handles, r, s):
        """One proof over the group's ranks: per rank a key shard of one shard_plan (zkg16_prove_group) -> (proof, inf)."""
        proof = np.zeros(48, dtype=np.uint64)
        inf = np.zeros(3, dtype=np.uint8)
        self._check(self.lib.zkg16_prove_group(self.group, self._handles(pk_handles, "pk"), self._handles(r1cs_handles, "r1cs"),
                                               self._handles(witness_handles, "witness"), _u64(r), _u64(s), proof, inf))
        return proof, inf

    def last_wm(self):
        """Ranks the last call's witness map was split over; 0 = the replicated map ran (zkg16_group_last_wm)."""
        k = C.c_int(0)
        self._check(self.lib.zkg16_group_last_wm(self.group, C.byref(k)))
        return k.value

    def rank_stats(self):
        """Per rank of the last call: dict(wm_ms, exchange_bytes, h_bytes, wall_ms) (zkg16_group_rank_stats)."""
        n = len(self.devices)
        buf = (C.c_double * (4 * n))()
        got = self.lib.zkg16_group_rank_stats(self.group, buf, n)
        if got < 0 or got > n:
            self._check(got)
        return [dict(wm_ms=buf[4 * i], exchange_bytes=int(buf[4 * i + 1]), h_bytes=int(buf[4 * i + 2]), wall_ms=buf[4 * i + 3])
                for i in range(got)]


def group_layout(log_n, k, ntt_mode=1):
    """Host-only layout of the split witness map (zkg16_group_layout) -> dict(applies, n1, n2, m, unit, residues [(lo, hi)] per rank,
    rects [(src, dst, row_lo, row_hi, col_lo, col_hi, stride)] of the row-pass exchange)."""
    lib = _lib.load()
    applies = C.c_int(0)
    shape = np.zeros(4, dtype=np.uint64)
    res = np.zeros(2 * max(k, 1), dtype=np.uint64)
    n = C.c_size_t(0)
    rc = lib.zkg16_group_layout(log_n, k, ntt_mode, C.byref(applies), shape, res.ctypes.data, None, 0, C.byref(n))
    if not (rc == 1 and n.value > 0):      # the count query: BAD_ARG for "more than cap 0", with the count needed
        _check_host(rc)
    rects = np.zeros((max(n.value, 1), 7), dtype=np.uint64)
    _check_host(lib.zkg16_group_layout(log_n, k, ntt_mode, C.byref(applies), shape, res.ctypes.data, rects.ctypes.data, rects.shape[0], C.byref(n)))
    return dict(applies=bool(applies.value), n1=int(shape[0]), n2=int(shape[1]), m=int(shape[2]), unit=int(shape[3]),
                residues=[(int(res[2 * g]), int(res[2 * g + 1])) for g in range(k)],
                rects=[tuple(int(x) for x in r) for r in rects[: n.value]])


def group_h_layout(log_n, k, h_ranges, ntt_mode=1):
    """Rectangles (src, dst, row_lo, row_hi, col_lo, col_hi, stride) of the h redistribution (zkg16_group_h_layout)."""
    lib = _lib.load()
    hr = np.ascontiguousarray(h_ranges, dtype=np.uint64).reshape(-1)
    if hr.shape[0] != 2 * k:
        raise ValueError("group_h_layout: %d ranges for %d ranks" % (hr.shape[0] // 2, k))
    n = C.c_size_t(0)
    rc = lib.zkg16_group_h_layout(log_n, k, ntt_mode, hr, None, 0, C.byref(n))
    if not (rc == 1 and n.value > 0):      # the count query: BAD_ARG for "more than cap 0", with the count needed
        _check_host(rc)
    rects = np.zeros((max(n.value, 1), 7), dtype=np.uint64)
    _check_host(lib.zkg16_group_h_layout(log_n, k, ntt_mode, hr, rects.ctypes.data, rects.shape[0], C.byref(n)))
    return [tuple(int(x) for x in r) for r in rects[: n.value]]
