/* zkg16 — MI355X-native Groth16 (BLS12-381) prove hot path, C ABI.
 *
 * Drop-in boundary for the inside of `Groth16::<Bls12_381>::prove(&pk, circuit, &mut rng)` as called by
 * ArielElb/zkSnark-FinalProject:
 *     src/arkworks/backend/matrix_proof.rs:139-140      (matrix-mul + Poseidon circuit)
 *     src/arkworks/backend/fibbonaci_handler.rs:110     (Fibonacci circuit)
 *     src/arkworks/backend/prime_snark.rs:119           (Fermat-prime circuit)
 * The reference has no FFI layer of its own; the narrowest upstream seam is
 *     ark_groth16::Groth16::create_proof_with_reduction_and_matrices(pk, r, s, &matrices, num_inputs,
 *                                                                    num_constraints, &full_assignment)
 * (ark-groth16 0.4 src/prover.rs, reached from the call sites above).  `zkg16_prove` is that function; the
 * reference-side binding (Rust `extern "C"` + a `GpuGroth16::prove` wrapper) is shown in INTEGRATION.md.
 *
 * Data conventions (identical to arkworks' in-memory representation, so a Rust caller passes slices as-is):
 *   Fr  = 4 little-endian u64 limbs, Montgomery form (R = 2^256)            (ark_bls12_381::Fr)
 *   Fq  = 6 little-endian u64 limbs, Montgomery form (R = 2^384)            (ark_bls12_381::Fq)
 *   G1 affine = 12 u64: x | y                                                (G1Affine.x, .y)
 *   G2 affine = 24 u64: x.c0 | x.c1 | y.c0 | y.c1                             (G2Affine over Fq2)
 *   point at infinity: separate flag byte per point (G?Affine.infinity); coordinates then ignored
 *   "canonical" scalars = 4 LE u64 limbs of the plain residue (what `into_bigint()` yields)
 * All inputs are caller-owned and copied before the call returns; outputs are caller-allocated.
 * Every entry point returns a zkg16_status; nothing aborts or unwinds across this boundary.
 * A ctx is bound to ONE GPU (one process per GPU; multi-GPU = one ctx per rank + zkg16_prove_partial /
 * zkg16_prove_finish around a single all-gather of 5 partial points).
 * A ctx is re-entrant (actix workers call prove concurrently: src/main.rs:37-43): the proving entry points run on "lanes" — up to
 * option "lanes" (default 2) proofs at a time, each with its own streams and workspaces, all on the SAME resident key, window tables,
 * matrices and NTT tables (callers beyond that wait); a single caller always gets lane 0 and sees no difference.  Everything else
 * is serialised by the ctx mutex.  pk / r1cs / witness handles are immutable after load; freeing one while a proof on another lane
 * still uses it is safe (the memory goes back when that proof ends).
 */
#ifndef ZKG16_H
#define ZKG16_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define ZKG16_API __attribute__((visibility("default")))

typedef enum {
    ZKG16_OK = 0,
    ZKG16_ERR_BAD_ARG = 1,          /* null pointer, inconsistent lengths */
    ZKG16_ERR_DOMAIN_TOO_LARGE = 2, /* = ark SynthesisError::PolynomialDegreeTooLarge (domain > 2^32), or > build limit */
    ZKG16_ERR_HIP = 3,              /* a HIP runtime call failed; see zkg16_last_error */
    ZKG16_ERR_OOM = 4,
    ZKG16_ERR_NO_DEVICE = 5,        /* no gfx950 device visible: the product has NO CPU fallback */
    ZKG16_ERR_BAD_HANDLE = 6,
    ZKG16_ERR_UNSUPPORTED = 7,
    ZKG16_ERR_UNSATISFIED = 8       /* option "check_satisfied" or a zkg16_prove_trapdoor* call: an assignment of the call does not satisfy its R1CS; nothing was written */
} zkg16_status;

typedef struct zkg16_ctx zkg16_ctx;

/* ---- lifecycle.  device_ids/n_devices: exactly one device per ctx (n_devices == 1). */
ZKG16_API int zkg16_init(const int *device_ids, int n_devices, zkg16_ctx **out);
ZKG16_API void zkg16_destroy(zkg16_ctx *ctx);
ZKG16_API const char *zkg16_strerror(int status);
ZKG16_API const char *zkg16_last_error(zkg16_ctx *ctx); /* text of the last HIP failure on this ctx; ctx NULL: the last refusal of a host-only entry on this thread */
ZKG16_API const char *zkg16_version(void);

/* ---- proving key residency  (replaces holding `ProvingKey<Bls12_381>` on the host: matrix_proof.rs:129-140).
 * Query lengths follow ark-groth16: n_a == n_b1 == n_b2 == num_instance + num_witness, n_h == N - 1,
 * n_l == num_witness.  *_inf may be NULL (= no infinity points).  shard_index/shard_count: this ctx keeps
 * only the contiguous index range [i*n/count, (i+1)*n/count) of every query vector (1 GPU: 0, 1). */
ZKG16_API int zkg16_pk_load(zkg16_ctx *ctx,
                  const uint64_t *a_query, const uint8_t *a_inf, size_t n_a,
                  const uint64_t *b_g1_query, const uint8_t *b_g1_inf, size_t n_b1,
                  const uint64_t *b_g2_query, const uint8_t *b_g2_inf, size_t n_b2,
                  const uint64_t *h_query, const uint8_t *h_inf, size_t n_h,
                  const uint64_t *l_query, const uint8_t *l_inf, size_t n_l,
                  const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                  const uint64_t delta_g1[12], const uint64_t delta_g2[24],
                  size_t num_instance, int shard_index, int shard_count, uint64_t *pk_handle);
/* The same with explicit index ranges instead of an equal split: this ctx keeps [z_lo, z_hi) of a_query / b_g1_query /
 * b_g2_query (and the l_query entries of those variables) and [h_lo, h_hi) of h_query; `blinding` != 0 on exactly one rank of a
 * proof (its MSMs carry the r*delta, s*delta, -rs*delta terms).  A rank with an empty h range skips the witness map and the H
 * MSM, one with an empty z range (and blinding == 0) skips the four z-side MSMs: ranks may take different roles (zkg16_shard_plan). */
ZKG16_API int zkg16_pk_load_range(zkg16_ctx *ctx,
                  const uint64_t *a_query, const uint8_t *a_inf, size_t n_a,
                  const uint64_t *b_g1_query, const uint8_t *b_g1_inf, size_t n_b1,
                  const uint64_t *b_g2_query, const uint8_t *b_g2_inf, size_t n_b2,
                  const uint64_t *h_query, const uint8_t *h_inf, size_t n_h,
                  const uint64_t *l_query, const uint8_t *l_inf, size_t n_l,
                  const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                  const uint64_t delta_g1[12], const uint64_t delta_g2[24],
                  size_t num_instance, size_t z_lo, size_t z_hi, size_t h_lo, size_t h_hi, int blinding, uint64_t *pk_handle);
/* A shard cut out of a whole key that is already resident on this ctx (zkg16_setup_resident, or zkg16_pk_load with shard 0 of 1):
 * device-to-device copies only.  The source handle stays valid (free it with zkg16_pk_free when the shard is all a rank needs). */
ZKG16_API int zkg16_pk_slice(zkg16_ctx *ctx, uint64_t pk_handle, size_t z_lo, size_t z_hi, size_t h_lo, size_t h_hi, int blinding,
                   uint64_t *shard_handle);
/* Window tables for a key (or shard) that stays resident: next to every base P_i of the five queries its multiples 2^(c w) P_i
 * for the windows w = 1 .. 254/c, built on the device.  Proofs on this handle then put all digits of a scalar into ONE bucket set
 * per MSM (fewer bucket additions at the same bucket count, one reduction per MSM) — same proofs bit for bit, 6-13 % less time per
 * proof (128x128: 181 -> 171 ms, 46x46: 22.6 -> 19.7 ms), for (254/c) x the key's HBM and c * (254/c) doublings per base once.  window_bits_z covers a / b_g1 / b_g2 / l,
 * window_bits_h h_query: 0 = chosen from the query length (none under 393,216 terms), 4..24 = as given, < 0 = leave that side
 * without a table.
 * table_bytes (nullable): HBM added (the tables, zkg16_table_layout, minus the plain queries they replace).  Not part of the reference's flow (its key is rebuilt per request): for servers that keep a
 * circuit's key resident.  A second call for a side that already has its table is ZKG16_ERR_BAD_ARG. */
ZKG16_API int zkg16_pk_precompute(zkg16_ctx *ctx, uint64_t pk_handle, int window_bits_z, int window_bits_h, uint64_t *table_bytes);
/* Entry layout of a window table (host-only, no ctx, no GPU).  kind: 1 = G1, 2 = G2; n bases, digits levels (= 254 / c + 1, level 0 is
 * a copy of the query).  stride_mode as option "table_stride": 1 = packed (an entry is the two coordinates, 112 / 224 bytes, and
 * straddles 128-byte cache lines 7 times out of 8), 2 = padded to whole lines (128 / 256 bytes; one seventh more HBM), 0 = the
 * library's choice: ZKG16_TABLE_STRIDE_DEFAULT_G1 / _G2 for a table of at least ZKG16_TABLE_STRIDE_PAD_MIN_BYTES packed bytes — one
 * that cannot stay in the 256 MiB last-level cache, so its gathers are HBM requests, where whole lines were measured to pay — and
 * packed below that.
 * -> *entry_stride bytes between entries, *bytes = n x digits x stride of the whole table (either nullable).
 * zkg16_pk_precompute lays each table out by this rule with the option's value at that call (a table keeps its layout afterwards) and
 * falls back from padded to packed when only the packed tables fit the free HBM.  ZKG16_ERR_BAD_ARG: unknown kind or mode, digits < 1,
 * or a size beyond 64 bits. */
#define ZKG16_TABLE_STRIDE_PACKED_G1 112
#define ZKG16_TABLE_STRIDE_PACKED_G2 224
#define ZKG16_TABLE_STRIDE_PADDED_G1 128
#define ZKG16_TABLE_STRIDE_PADDED_G2 256
#define ZKG16_TABLE_STRIDE_DEFAULT_G1 2      /* what mode 0 means for a large table, per kind (measured: DESIGN.md 2.4) */
#define ZKG16_TABLE_STRIDE_DEFAULT_G2 2
#define ZKG16_TABLE_STRIDE_PAD_MIN_BYTES 268435456      /* 256 MiB */
ZKG16_API int zkg16_table_layout(int kind, size_t n, int digits, int stride_mode, size_t *entry_stride, uint64_t *bytes);
/* The widths of a handle's window tables (0 = that side has none). */
ZKG16_API int zkg16_pk_table_bits(zkg16_ctx *ctx, uint64_t pk_handle, int *window_bits_z, int *window_bits_h);
/* Rank roles for one proof over n_ranks GPUs (host-only, no ctx, no GPU).  ranges: n_ranks x 4 = z_lo, z_hi, h_lo, h_hi per rank;
 * blinding: n_ranks flags (exactly one set).  The first *h_ranks_out ranks run the witness map and share h_query by index range;
 * every rank gets the share of the z ranges that makes all ranks finish together under a cost model in G1 mixed additions
 * (b_density = fraction of variables present in the B queries, <= 0 for the default 0.8; h_ranks = 0 lets the model choose,
 * h_ranks = n_ranks gives the equal split of zkg16_pk_load's shard_index / shard_count).  z_cost (nullable): m_total per-index
 * costs of the z-side terms in G1 mixed additions — (0, 1 or window-count entries of the scalar) x (queries whose base is not
 * at infinity, the G2 one counted 2.8x); with it the z ranges are cut by cumulative cost instead of by index count. */
ZKG16_API int zkg16_shard_plan(int n_ranks, size_t m_total, size_t n_h, double b_density, int h_ranks, const float *z_cost,
                     uint64_t *ranges /* n_ranks x 4 */, uint8_t *blinding /* n_ranks */, int *h_ranks_out);
/* The same plan with the cost factors of shards that carry window tables (window_tables != 0; zkg16_pk_precompute on every shard). */
ZKG16_API int zkg16_shard_plan_tables(int n_ranks, size_t m_total, size_t n_h, double b_density, int h_ranks, const float *z_cost,
                            int window_tables, uint64_t *ranges, uint8_t *blinding, int *h_ranks_out);
/* Is every element of a resident key a point of its group?  What ark's ProvingKey::deserialize_compressed answers with Validate::Yes:
 * each point of the five queries satisfies the curve equation and lies in the prime-order subgroup (zkg16_point_check's rule; the
 * point at infinity passes), tested on the device where the key lies, one GPU lane per point.  Any handle: a whole key, a shard of
 * zkg16_pk_load_range / zkg16_pk_slice (the ranges it holds), with or without window tables at either entry stride.
 * Queries in the order a, b_g1, b_g2, h, l: n_bad[q] = points of query q that failed, first_bad[q] = the smallest index of one in the
 * whole key's numbering (UINT64_MAX where n_bad[q] is 0).  The three trailing blinding slots are copies of the single points and are
 * not counted.  single_mask: bit 0..4 set when alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2 is at infinity or fails
 * zkg16_point_check (host).  *ok = 1 iff nothing failed.  A bad key is an answer: ZKG16_OK with *ok = 0.
 * NOT answered: whether it is the right key (the queries against an R1CS or a verifying key, pairing relations between b_g1 and
 * b_g2 or among alpha, beta, delta).  Option "pk_validate" runs this inside zkg16_pk_load / zkg16_pk_load_range. */
ZKG16_API int zkg16_pk_check(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t n_bad[5], uint64_t first_bad[5], uint32_t *single_mask, int *ok);
/* Stage entry (tests / tools) of the same kernels: n host points of one group (1 = G1, 12 u64 each; 2 = G2, 24 u64) in the limbs of
 * zkg16_point_check_batch, inf nullable; uploaded and converted as a key's queries are.  *n_bad = points that fail
 * zkg16_point_check, *first_bad = the smallest index of one (UINT64_MAX: none).  n == 0 is ZKG16_OK with (0, UINT64_MAX). */
ZKG16_API int zkg16_points_check_bulk(zkg16_ctx *ctx, int group, const uint64_t *points, const uint8_t *inf, size_t n, uint64_t *n_bad,
                            uint64_t *first_bad);
/* The last key check on this ctx (zkg16_pk_check, or a load under option "pk_validate") and the last zkg16_points_check_bulk, in ms:
 * [0..4] the kernels of a, b_g1, b_g2, h, l (device events on the streams they ran on: they overlap, so they sum to more than the
 * call; 0 for an empty range), [5] total wall of the check with its one synchronisation (host clock); [6] the kernel of the last
 * zkg16_points_check_bulk (device events), [7] the upload and conversion in front of it (host clock).  Returns the number of
 * entries written (at most cap). */
ZKG16_API int zkg16_pk_check_timings(zkg16_ctx *ctx, float *ms, int cap);

/* ---- a proving key as bytes: ark-groth16 0.4's ProvingKey<Bls12_381>::serialize_compressed, the one object of the flow that did
 * not yet travel in arkworks' encoding (proofs and verifying keys: zkg16_points_compress and the decoders below).  Fields in
 * declaration order, a Vec as a u64 little-endian count and its items, points as zkg16_g1_decompress / zkg16_g2_decompress read them:
 *
 *   vk:  alpha_g1 48 | beta_g2 96 | gamma_g2 96 | delta_g2 96 | count 8 | gamma_abc_g1 48 x ni
 *   beta_g1 48 | delta_g1 48
 *   a_query 8 + 48 m | b_g1_query 8 + 48 m | b_g2_query 8 + 96 m | h_query 8 + 48 n_h | l_query 8 + 48 (m - ni)
 *
 * A restatement of the upstream layout, as the other mirrors: parity with bytes written by a real arkworks build is UNPINNED (the
 * crates are not vendored); what is pinned is that the host and the device forms here agree byte for byte and status for status.
 * The uncompressed encoding is not offered.  Every call is all or nothing: a refusal writes no output and leaves no handle.
 *
 * zkg16_pk_bytes_dims (host only): walks the five length prefixes and nothing else.  Each count is compared with the bytes that
 * remain before it is multiplied, so no prefix (2^63, 2^64 - 1) can overflow.  ZKG16_ERR_BAD_ARG, nothing written, zkg16_last_error(NULL)
 * naming the field: len is not exactly what the counts imply (truncated, trailing bytes), ni == 0 or ni > m, the three z-side counts
 * differ, n_l != m - ni.  zkg16_pk_bytes_size (host only): the inverse; ZKG16_ERR_BAD_ARG for ni outside 1 .. m or a size beyond size_t. */
ZKG16_API int zkg16_pk_bytes_dims(const uint8_t *bytes, size_t len, size_t *num_instance, size_t *m, size_t *n_h, size_t *n_l);
ZKG16_API int zkg16_pk_bytes_size(size_t num_instance, size_t m, size_t n_h, size_t *bytes);
/* The host forms (no ctx, up to `threads` host threads, 0 = 8), built on zkg16_points_compress and the host decoders: THE REFERENCE
 * for every byte and every status of the device forms below.  Arrays as zkg16_pk_load's (a / b_g1 / b_g2: m points, h: n_h,
 * l: m - num_instance; *_inf nullable when serialising) plus gamma_g2 and gamma_abc_g1 (num_instance points).
 * zkg16_pk_serialize_host: cap below zkg16_pk_bytes_size or a null pointer: ZKG16_ERR_BAD_ARG, out untouched.
 * zkg16_pk_deserialize_host: outputs sized by zkg16_pk_bytes_dims.  What zkg16_pk_bytes_dims refuses is refused; a point whose
 * decoder status is not 0 (1 - 4, and 5 with validate) or a single point at infinity: ZKG16_ERR_BAD_ARG, no output written, and
 * zkg16_last_error(NULL) names the entry and the status, e.g. "b_g2_query[17]: status 4": the smallest index of the first failing
 * field in file order. */
ZKG16_API int zkg16_pk_serialize_host(const uint64_t *a_query, const uint8_t *a_inf, const uint64_t *b_g1_query, const uint8_t *b_g1_inf,
                            const uint64_t *b_g2_query, const uint8_t *b_g2_inf, const uint64_t *h_query, const uint8_t *h_inf,
                            const uint64_t *l_query, const uint8_t *l_inf,
                            const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                            const uint64_t delta_g1[12], const uint64_t delta_g2[24], const uint64_t gamma_g2[24],
                            const uint64_t *gamma_abc_g1, size_t num_instance, size_t m, size_t n_h, int threads,
                            uint8_t *out, size_t cap, size_t *written);
ZKG16_API int zkg16_pk_deserialize_host(const uint8_t *bytes, size_t len, int validate, int threads,
                            uint64_t *a_query, uint8_t *a_inf, uint64_t *b_g1_query, uint8_t *b_g1_inf,
                            uint64_t *b_g2_query, uint8_t *b_g2_inf, uint64_t *h_query, uint8_t *h_inf,
                            uint64_t *l_query, uint8_t *l_inf,
                            uint64_t alpha_g1[12], uint64_t beta_g1[12], uint64_t beta_g2[24],
                            uint64_t delta_g1[12], uint64_t delta_g2[24], uint64_t gamma_g2[24], uint64_t *gamma_abc_g1);
/* A whole resident key copied back as zkg16_pk_load's arrays (limbs and infinity flags): level 0 of each query where it lies, at
 * either entry stride of a window table, without the three blinding slots, l_query in its own numbering.  With every array and
 * single point null only the dimensions are written (each nullable).  A shard: ZKG16_ERR_UNSUPPORTED. */
ZKG16_API int zkg16_pk_read(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t *a_query, uint8_t *a_inf, uint64_t *b_g1_query, uint8_t *b_g1_inf,
                  uint64_t *b_g2_query, uint8_t *b_g2_inf, uint64_t *h_query, uint8_t *h_inf, uint64_t *l_query, uint8_t *l_inf,
                  uint64_t alpha_g1[12], uint64_t beta_g1[12], uint64_t beta_g2[24], uint64_t delta_g1[12], uint64_t delta_g2[24],
                  size_t *num_instance, size_t *m, size_t *n_h);
/* zkg16_pk_serialize_host of zkg16_pk_read's arrays, byte for byte, encoded on the device where the key lies (one lane per point,
 * 0xC0 and zeros for a point at infinity anywhere) and brought back in pieces through the ctx's pinned staging ring.  The handle
 * holds neither gamma_g2 nor gamma_abc_g1 (num_instance points): the caller passes them.  Window tables are not saved
 * (zkg16_pk_precompute rebuilds them).  Before any device work, out untouched: cap below the key's size or a null pointer
 * (ZKG16_ERR_BAD_ARG), an unknown handle (ZKG16_ERR_BAD_HANDLE), a shard (ZKG16_ERR_UNSUPPORTED). */
ZKG16_API int zkg16_pk_save(zkg16_ctx *ctx, uint64_t pk_handle, const uint64_t gamma_g2[24], const uint64_t *gamma_abc_g1,
                  uint8_t *out, size_t cap, size_t *written);
/* A whole key from its bytes, decoded on the device (one lane per point; the G2 square root without an inversion) straight into the
 * key's arrays: the handle zkg16_pk_load returns for zkg16_pk_deserialize_host's arrays, word for word — blinding slots, l_query at
 * the index of its scalar, the B-side mask — usable by every call that takes a whole key.  The verifying key comes back with it
 * (gamma_abc_g1: cap_abc points of room, at least num_instance).  What zkg16_pk_bytes_dims refuses, a point of status 1 - 4
 * anywhere or a single point at infinity: ZKG16_ERR_BAD_ARG, no handle, every buffer released, no output written, zkg16_last_error
 * (of the ctx) as the host form's.  validate != 0 or option "pk_validate": zkg16_pk_check's test on the decoded key before the
 * handle exists, exactly as in zkg16_pk_load (status 5; the text is that call's), gamma_g2 and gamma_abc_g1 by zkg16_point_check. */
ZKG16_API int zkg16_pk_load_bytes(zkg16_ctx *ctx, const uint8_t *bytes, size_t len, int validate, uint64_t *pk_handle,
                        uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                        uint64_t *gamma_abc_g1, size_t cap_abc);
/* The last zkg16_pk_load_bytes / zkg16_pk_save / zkg16_pk_read on this ctx, in ms: [0] host time in the staging ring (copies into or
 * out of its pinned halves and waits for their transfers), [1..5] the decode / encode / read kernels of a, b_g1, b_g2, h, l from the
 * first piece to the last (device events; later pieces' copies overlap them), [6] gamma_abc_g1 and the single points, [7] the key
 * check of a validated load, [8] total wall time.  Returns the number of entries written (at most cap). */
ZKG16_API int zkg16_pk_bytes_timings(zkg16_ctx *ctx, float *ms, int cap);
ZKG16_API void zkg16_pk_free(zkg16_ctx *ctx, uint64_t pk_handle);

/* ---- device groups: several ctxs of ONE process (one per GPU; several may share a GPU) proving one proof together.
 * zkg16_group_create: n (1..8) distinct ctxs, kept by pointer (destroy the group before them).  Ranks on different GPUs read each
 * other's buffers: peer access is enabled here, ZKG16_ERR_UNSUPPORTED where it is unavailable.
 * zkg16_prove_group: per rank a key shard (zkg16_pk_slice / zkg16_pk_load_range of one zkg16_shard_plan(_tables) plan: the z and h
 * ranges tile the key, exactly one rank blinds), the R1CS and the assignment on that rank's ctx; every handle and dimension is
 * checked on every rank before any work.  One host thread per rank, each on a lane of its ctx; the ranks with an h range form
 * the witness-map set.  With k >= 2 of them and a two-pass domain (2^12 .. 2^24; zkg16_group_layout) they split the seven NTTs
 * between them — seven exchanges and one redistribution of h, each a gather kernel over the rectangles of zkg16_group_layout /
 * zkg16_group_h_layout — else each runs the whole witness map (as zkg16_prove_partial).  The partials are combined as
 * zkg16_prove_finish combines them: the same proof bytes as zkg16_prove_resident with the whole key.  A failing rank makes every
 * rank stop; the call returns its status (text: zkg16_group_last_error).  Group calls are serialised by the group.
 * zkg16_witness_map_group: every rank is a witness-map rank; h (N x 4 limbs) gathered to the host, rank i bringing [iN/n, (i+1)N/n).
 * zkg16_group_last_wm: ranks the last call's witness map was split over, 0 = the replicated map ran.
 * zkg16_group_rank_stats: per rank of the last call: witness-map device ms (the sum of its steps between exchanges; with option
 * "group_serial" = 1 the ranks run each step one at a time, so this is the rank's time alone on the device), bytes gathered per
 * row-pass exchange, bytes of the h redistribution, wall ms of the rank (prove: zkg16_last_timings [9]); returns the rank count. */
typedef struct zkg16_group zkg16_group;
ZKG16_API int zkg16_group_create(zkg16_ctx *const *ctxs, int n, zkg16_group **out);
ZKG16_API void zkg16_group_destroy(zkg16_group *group);
ZKG16_API const char *zkg16_group_last_error(zkg16_group *group);
ZKG16_API int zkg16_group_set_option(zkg16_group *group, const char *name, int64_t value);   /* "group_serial" (default 0) */
ZKG16_API int zkg16_prove_group(zkg16_group *group, const uint64_t *pk_handles, const uint64_t *r1cs_handles, const uint64_t *witness_handles,
                      const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3]);
ZKG16_API int zkg16_witness_map_group(zkg16_group *group, const uint64_t *r1cs_handles, const uint64_t *witness_handles, uint64_t *h_out,
                            size_t *log_n_out);
ZKG16_API int zkg16_group_last_wm(zkg16_group *group, int *k_dist);
ZKG16_API int zkg16_group_rank_stats(zkg16_group *group, double *out /* n x 4 */, int cap_ranks);
/* The split witness map's layout (host-only, no ctx, no GPU).  The two-pass NTT of 2^log_n (ntt_mode as the option) is the matrix
 * x[N2 i1 + i2]; with m = min(N1, N2) rank g of k owns the positions n with n mod m in [residues[2g], residues[2g+1]), an even split
 * in units of the pass kernels' tiles.  *applies = 0 (status OK): the replicated map runs — single-pass (<= 2^11) or three-pass
 * domains, or k above the number of units.  shape = N1, N2, m, unit.  rects (cap x 7 u64, nullable with cap 0; *n_rects = count
 * needed, ZKG16_ERR_BAD_ARG if above cap): src rank, dst rank, row lo, row hi, col lo, col hi, row stride — the positions
 * row * stride + col that dst copies from src before each row pass (dst's rows x src's columns, stride N2).
 * zkg16_group_h_layout: the same for the redistribution of h, rank g receiving [h_ranges[2g], h_ranges[2g+1]) (stride m;
 * ZKG16_ERR_UNSUPPORTED where the layout does not apply, ZKG16_ERR_BAD_ARG for ranges beyond N or overlapping). */
ZKG16_API int zkg16_group_layout(int log_n, int k, int ntt_mode, int *applies, uint64_t shape[4], uint64_t *residues /* k x 2 */,
                       uint64_t *rects, size_t cap, size_t *n_rects);
ZKG16_API int zkg16_group_h_layout(int log_n, int k, int ntt_mode, const uint64_t *h_ranges /* k x 2 */, uint64_t *rects, size_t cap,
                         size_t *n_rects);

/* ---- R1CS residency (ark_relations `ConstraintMatrices<Fr>` as CSR; matrices are per-circuit constants).
 * row_ptr: num_constraints + 1 entries; col: nnz u32; coeff: nnz x 4 limbs (Montgomery). */
ZKG16_API int zkg16_r1cs_load(zkg16_ctx *ctx,
                    const uint64_t *a_row_ptr, const uint32_t *a_col, const uint64_t *a_coeff,
                    const uint64_t *b_row_ptr, const uint32_t *b_col, const uint64_t *b_coeff,
                    const uint64_t *c_row_ptr, const uint32_t *c_col, const uint64_t *c_coeff,
                    size_t num_instance, size_t num_constraints, size_t num_variables, uint64_t *r1cs_handle);
ZKG16_API void zkg16_r1cs_free(zkg16_ctx *ctx, uint64_t r1cs_handle);

/* ---- full assignment z = instance || witness (Montgomery), n_assign x 4 limbs, uploaded once per proof. */
ZKG16_API int zkg16_witness_load(zkg16_ctx *ctx, const uint64_t *full_assignment, size_t n_assign, uint64_t *witness_handle);
ZKG16_API void zkg16_witness_free(zkg16_ctx *ctx, uint64_t witness_handle);
/* the assignment behind a handle, copied back (n_assign must match the handle's length) */
ZKG16_API int zkg16_witness_read(zkg16_ctx *ctx, uint64_t witness_handle, uint64_t *full_assignment_out, size_t n_assign);

/* ---- the hot path.  r, s: Montgomery Fr (drawn by the caller exactly as ark-groth16 does: r then s).
 * proof_out = A (12) | B (24) | C (12) affine Montgomery limbs; inf_out[3] = infinity flags of A, B, C. */
ZKG16_API int zkg16_prove_resident(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, uint64_t witness_handle,
                         const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3]);

/* K proofs of ONE circuit on ONE resident key, in one device pass.  witness_handles[k]: the full assignment of proof k
 * (num_variables of r1cs_handle); r, s: k x 4 Montgomery limbs; proofs_out: k x 48; inf_out: k x 3.
 * Proof k is byte-identical to zkg16_prove_resident(ctx, pk_handle, r1cs_handle, witness_handles[k], r + 4k, s + 4k).
 * One lane, like the other proving calls.  The witness map is one SpMV and seven transforms over the K assignments (every launch
 * with a vector index), and every MSM sorts, accumulates and reduces the K proofs' terms as ONE list whose bucket sets are the K
 * proofs' windows.  k is split into sub-batches of at most 65,535 proofs whose term lists stay under 2^31 terms and whose
 * workspaces fit the free HBM (option "batch_max" caps them).  k == 0, null pointers and lengths that do not match:
 * ZKG16_ERR_BAD_ARG; an unknown handle: ZKG16_ERR_BAD_HANDLE; a key that is not whole (a shard): ZKG16_ERR_UNSUPPORTED — all
 * checked before any work.  On any error nothing is written to proofs_out / inf_out (the proofs are staged until every
 * sub-batch has succeeded).  zkg16_last_timings / zkg16_last_term_counts then describe the whole batch (timings: [3] wait for
 * H, [7] wait for the z-side MSMs, [8] H's combination and the tails of all proofs, [21] the other MSMs' combination). */
ZKG16_API int zkg16_prove_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, const uint64_t *witness_handles,
                                size_t k, const uint64_t *r, const uint64_t *s, uint64_t *proofs_out, uint8_t *inf_out);

/* One-shot form mirroring create_proof_with_reduction_and_matrices: host pointers in, proof out
 * (uploads matrices + assignment, proves, frees). */
ZKG16_API int zkg16_prove(zkg16_ctx *ctx, uint64_t pk_handle, const uint64_t r[4], const uint64_t s[4],
                const uint64_t *a_row_ptr, const uint32_t *a_col, const uint64_t *a_coeff,
                const uint64_t *b_row_ptr, const uint32_t *b_col, const uint64_t *b_coeff,
                const uint64_t *c_row_ptr, const uint32_t *c_col, const uint64_t *c_coeff,
                size_t num_instance, size_t num_constraints,
                const uint64_t *full_assignment, size_t n_assign,
                uint64_t proof_out[48], uint8_t inf_out[3]);

/* Multi-GPU (index-range sharded pk): each rank computes h redundantly and the MSM partial sums over its shard.
 * partial_out = 4 G1 affine (H, L, A, B1 partials: 4 x 12) | 1 G2 affine (B2 partial: 24) = 72 u64;
 * partial_inf[5].  The caller all-gathers the 72-u64 records (RCCL) and any rank finishes. */
ZKG16_API int zkg16_prove_partial(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, uint64_t witness_handle,
                        const uint64_t r[4], const uint64_t s[4], uint64_t partial_out[72], uint8_t partial_inf[5]);
ZKG16_API int zkg16_prove_finish(zkg16_ctx *ctx, uint64_t pk_handle, const uint64_t r[4], const uint64_t s[4],
                       const uint64_t *partials /* n_ranks x 72 */, const uint8_t *partial_inf /* n_ranks x 5 */,
                       int n_ranks, uint64_t proof_out[48], uint8_t inf_out[3]);

/* Host-only form of the finish step (no ctx, no GPU): sums the per-rank partial records and applies the proof
 * tail  A = alpha + sum A_k,  B = beta2 + sum B2_k,  C = s*A + r*(beta1 + sum B1_k) + sum L_k + sum H_k.
 * (r*delta1, s*delta1, s*delta2 and -rs*delta1 already ride inside rank 0's partials as extra MSM terms.) */
ZKG16_API int zkg16_combine_partials(const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                           const uint64_t r[4], const uint64_t s[4],
                           const uint64_t *partials /* n_ranks x 72 */, const uint8_t *partial_inf /* n_ranks x 5 */,
                           int n_ranks, uint64_t proof_out[48], uint8_t inf_out[3]);

/* ---- Groth16 circuit-specific setup on the device from a caller-supplied trapdoor (scope row f-1).  Replaces
 * `Groth16::<Bls12_381>::setup(circuit, &mut rng)` (matrix_proof.rs:129, fibbonaci_handler.rs:107, prime_snark.rs:112-113): the caller
 * draws trapdoor = tau | alpha | beta | gamma | delta (5 x 4 limbs, Montgomery) and the generators g1, g2 from its rng as upstream's
 * generate_random_parameters_with_reduction does.  Outputs are caller-allocated with the lengths of zkg16_pk_load
 * (a/b_g1/b_g2: num_variables, h: N-1, l: num_witness) plus the verifying-key elements. */
ZKG16_API int zkg16_setup(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t trapdoor[20], const uint64_t g1_gen[12], const uint64_t g2_gen[24],
                uint64_t *a_query, uint8_t *a_inf, uint64_t *b_g1_query, uint8_t *b_g1_inf, uint64_t *b_g2_query, uint8_t *b_g2_inf,
                uint64_t *h_query, uint64_t *l_query, uint8_t *l_inf,
                uint64_t alpha_g1[12], uint64_t beta_g1[12], uint64_t beta_g2[24], uint64_t delta_g1[12], uint64_t delta_g2[24],
                uint64_t gamma_g2[24], uint64_t *gamma_abc_g1 /* num_instance x 12 */);

/* Same, but the proving key never leaves the device: returns a pk handle (as zkg16_pk_load would) plus the verifying-key
 * elements.  This is the per-request flow of the reference's handlers (setup then prove) without the host round trip. */
ZKG16_API int zkg16_setup_resident(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t trapdoor[20], const uint64_t g1_gen[12],
                         const uint64_t g2_gen[24], uint64_t *pk_handle,
                         uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                         uint64_t *gamma_abc_g1 /* num_instance x 12 */);

/* ---- Groth16 verification on the host (scope row f-3; no ctx, no GPU): `verify_with_processed_vk` of the handlers
 * (matrix_proof.rs:200-205).  gamma_abc_g1: num_instance points; public_inputs: num_instance - 1 Montgomery Fr; *ok = 1 iff
 * e(A,B) = e(alpha,beta) e(sum z_i gamma_abc_i, gamma) e(C,delta). */
ZKG16_API int zkg16_verify(const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                 const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t *public_inputs,
                 const uint64_t proof[48], const uint8_t inf[3], int *ok);

/* prepare_verifying_key (what the reference's handlers return as `pvk`: matrix_proof.rs:134-136, io.rs:62-77) and
 * verify_with_processed_vk on such a key, both host-only.  alpha_beta = e(alpha, beta) as ark's Fq12 (six Fq2 in tower order,
 * 72 u64 Montgomery limbs); *_neg_coeffs = the G2Prepared line coefficients of -gamma / -delta (*n_coeffs = 68 triples of Fq2 =
 * 68 x 36 u64 each, caller-allocated).  ark-ec's formulas are restated (un-vendored crate): self-consistent and cross-checked
 * against the plain verifier, byte parity with upstream unpinned.  Both verifiers reject proof points that are not on the curve
 * or not in the prime-order subgroup (zkg16_point_check: group 1 = G1 / 12 limbs, 2 = G2 / 24 limbs). */
ZKG16_API int zkg16_pvk_prepare(const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                      uint64_t alpha_beta[72], uint64_t *gamma_neg_coeffs, uint64_t *delta_neg_coeffs, size_t *n_coeffs);
ZKG16_API int zkg16_verify_prepared(const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t *public_inputs, const uint64_t alpha_beta[72],
                          const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                          const uint64_t proof[48], const uint8_t inf[3], int *ok);
/* n compressed G1 points (48 bytes each, the ark-serialize / zcash encoding the reference's keys and proofs travel in) -> affine
 * Montgomery limbs (n x 12) + infinity flags, strict as G1Affine::deserialize_compressed (+ the subgroup check when validate).
 * status (nullable, n ints): 0 ok, 1 not compressed, 2 non-canonical infinity, 3 x not reduced, 4 not on the curve, 5 not in the
 * subgroup; returns ZKG16_ERR_BAD_ARG if any point failed. */
ZKG16_API int zkg16_g1_decompress(const uint8_t *bytes, size_t n, uint64_t *out, uint8_t *inf, int validate, int *status);
/* The same for G2 (96 bytes = x.c1 || x.c0; out n x 24 limbs), the inverse for both groups (group 1 / 2; inf nullable), and the
 * 48-byte little-endian canonical form of Fq values (the Fq12 and line coefficients of a prepared verifying key; from-bytes
 * refuses values >= q). */
ZKG16_API int zkg16_g2_decompress(const uint8_t *bytes, size_t n, uint64_t *out, uint8_t *inf, int validate, int *status);
ZKG16_API int zkg16_points_compress(int group, const uint64_t *points, const uint8_t *inf, size_t n, uint8_t *out);
ZKG16_API int zkg16_fq_to_le_bytes(const uint64_t *limbs, size_t n, uint8_t *out);
ZKG16_API int zkg16_fq_from_le_bytes(const uint8_t *bytes, size_t n, uint64_t *out);
ZKG16_API int zkg16_point_check(int group, const uint64_t *point, int *ok);

/* ---- batched verification: k proofs under ONE prepared key, checked together.  With multipliers rho_k, all k proofs hold iff
 *     FE( prod_k ML(rho_k A_k, B_k) * ML(sum_k rho_k X_k, -gamma) * ML(sum_k rho_k C_k, -delta) ) == e(alpha, beta)^(sum_k rho_k)
 * (X_k = gamma_abc[0] + sum_i z_{k,i} gamma_abc[i]; ML the Miller loop, FE the final exponentiation) up to an error of 2^-128:
 * one final exponentiation per batch instead of one per proof.  rho: k x 2 u64, 128-bit, plain integers, each non-zero.  THE
 * CALLER DRAWS THEM (as r and s in the proving calls: this ABI draws nothing), and they must be unpredictable to whoever made the
 * proofs — fresh output of a cryptographic generator per call; with predictable multipliers forged proofs can be made to cancel.
 * public_inputs: k x (num_instance - 1) x 4 Montgomery limbs, proofs: k x 48, inf: k x 3, the key as for zkg16_verify_prepared.
 * *ok = 1 iff every proof verifies.  ok_each (nullable, k bytes): the verdict zkg16_verify_prepared gives each proof alone — when
 * the batch equation fails the bad proofs are found by bisecting over index ranges (one final exponentiation per range).
 * k == 0, null pointers, n_coeffs != 68 and any rho_k == 0 (it would wave proof k through): ZKG16_ERR_BAD_ARG before any work,
 * outputs untouched.
 * zkg16_verify_batch_host: everything on up to `threads` host threads (0 = 8); no ctx, no GPU.
 * zkg16_verify_batch: the per-proof work — the 3k membership tests, rho_k A_k, the k Miller loops on the unprepared B_k, their
 * product — in kernels on a lane of the ctx (one GPU lane per proof), sum_k rho_k C_k by the ctx's G1 MSM; the two Miller loops on
 * the key's coefficients, the final exponentiation and the bisecting stay on the host.  k above 65,536 runs in passes of that
 * many.  Batches shorter than option "verify_batch_min" (default 1024: the smallest measured K at which the kernels beat the host
 * form on eight threads, profiles/verify_batch_timing_r8.txt; 1 = always the kernels) are answered by the host form. */
ZKG16_API int zkg16_verify_batch_host(const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                            const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                            const uint64_t *public_inputs, const uint64_t *proofs, const uint8_t *inf, const uint64_t *rho, size_t k,
                            int threads, int *ok, uint8_t *ok_each);
ZKG16_API int zkg16_verify_batch(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                       const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                       const uint64_t *public_inputs, const uint64_t *proofs, const uint8_t *inf, const uint64_t *rho, size_t k,
                       int *ok, uint8_t *ok_each);
/* zkg16_verify_batch from the proofs as they travel: proof_bytes = k x 192 (A 48 | B 96 | C 48, the compressed encoding of
 * zkg16_g1_decompress / zkg16_g2_decompress).  The bytes are uploaded and decoded in a kernel, one GPU lane per point (square roots
 * and byte parsing on the device, no validation: the membership kernels test every point once), into the device proof array that
 * zkg16_verify_batch's kernels read; the decoded limbs and flags come back once (384 B per proof) for the host's share of the work.
 * A proof with a point that does not decode (status 1 to 4) is treated exactly like one that fails membership: left out of every
 * sum and product, ok_each[k] = 0, *ok = 0, the other proofs' verdicts unaffected.  decode_status (nullable, k x 3 bytes: A, B, C):
 * what the validating host decoder says of each point (5 from the membership verdicts).  When every proof decodes, *ok and ok_each
 * equal zkg16_verify_batch on the host-decoded limbs with the same rho.  Argument checks as zkg16_verify_batch, and proof_bytes
 * non-null.  Batches shorter than option "verify_wire_min" (default 256: the smallest measured K at which this call
 * beat host decoding followed by either the host form on eight threads or zkg16_verify_batch, 0.094 against 0.239 and 0.245 ms per
 * proof, each far outside the spread of the rounds; at K = 64 it lost, 0.361 against 0.270 — profiles/verify_wire_timing_r9.txt;
 * 1 = always the device) are decoded on host threads and answered by the host form. */
ZKG16_API int zkg16_verify_batch_wire(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                            const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                            const uint64_t *public_inputs, const uint8_t *proof_bytes, const uint64_t *rho, size_t k,
                            int *ok, uint8_t *ok_each, uint8_t *decode_status);
/* Each proof's own verdict in one device pass: ok_each[i] (k bytes) = what zkg16_verify_prepared says of proof i alone, for every i,
 * whatever the others are — no multipliers, the unscaled A_k, so the verdict is exact.  On a lane of the ctx, one GPU lane per proof:
 * the membership kernels of zkg16_verify_batch, then for the proofs that passed X_k = gamma_abc[0] + sum_i z_{k,i} gamma_abc[i], the
 * three-pair Miller loop ML(A_k, B_k) ML(X_k, -gamma) ML(C_k, -delta) on the key's coefficients, the final exponentiation and the
 * comparison with e(alpha, beta): a fixed number of launches per 65,536 proofs however many of them are bad.  Arguments as
 * zkg16_verify_batch without rho; k == 0, null pointers and n_coeffs != 68: ZKG16_ERR_BAD_ARG before any work, ok_each untouched.
 * zkg16_verify_batch and zkg16_verify_batch_wire run the same pass on the proofs bisecting has not decided once it has made option
 * "verify_each_after" range tests (default 32: ceil(T_each / t_range) at K = 1024 = ceil(47.72 ms / 2.156 ms) = 23, the whole
 * per-proof call against one range test of bisecting, both measured, rounded up to a power of two so that one bad proof — up to
 * 2 log2 k range tests — never reaches the pass; profiles/verify_each_timing_r10.txt; 1 = after the first range
 * test; a value above 2k never switches; 0 restores the default).  *ok and ok_each of those calls are what they were; only the time changes. */
ZKG16_API int zkg16_verify_each(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                      const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                      const uint64_t *public_inputs, const uint64_t *proofs, const uint8_t *inf, size_t k, uint8_t *ok_each);
/* Stage entry: zkg16_g1_decompress / zkg16_g2_decompress (group 1 / 2) in a kernel on a lane of the ctx, one GPU lane per point.
 * Outputs, statuses (nullable) and the return code are the host functions': limbs zero for a point of status 1 to 4,
 * ZKG16_ERR_BAD_ARG when any point failed; n == 0 is ZKG16_OK. */
ZKG16_API int zkg16_points_decompress_batch(zkg16_ctx *ctx, int group, const uint8_t *bytes, size_t n, uint64_t *out, uint8_t *inf,
                                  int validate, int *status);
/* Stage entries (tests / tools).  n Miller loops on the device, one GPU lane per pair: f_out[i] (72 u64, ark's tower order, the
 * layout of alpha_beta) = the Miller value of (g1[i], g2[i]) with ark's line scaling, one for a pair with a point at infinity (flag
 * bytes nullable); zkg16_final_exp of it is the pairing.  n membership tests on the device: ok_out[i] = what zkg16_point_check says
 * of point i (the point at infinity passes).  zkg16_final_exp: the verifier's final exponentiation, host-only.
 * zkg16_final_exp_batch: n of them on the device, one GPU lane each: out[i] (72 u64) is bit-equal to zkg16_final_exp(f[i]);
 * n == 0 is ZKG16_OK. */
ZKG16_API int zkg16_miller_loop_batch(zkg16_ctx *ctx, const uint64_t *g1, const uint8_t *g1_inf, const uint64_t *g2, const uint8_t *g2_inf, size_t n,
                            uint64_t *f_out);
ZKG16_API int zkg16_point_check_batch(zkg16_ctx *ctx, int group, const uint64_t *points, const uint8_t *inf, size_t n, uint8_t *ok_out);
ZKG16_API int zkg16_final_exp(const uint64_t f[72], uint64_t out[72]);
ZKG16_API int zkg16_final_exp_batch(zkg16_ctx *ctx, const uint64_t *f /* n x 72 */, size_t n, uint64_t *out /* n x 72 */);
/* The last zkg16_verify_batch / zkg16_verify_batch_wire / zkg16_verify_prime_batch[_wire] on this ctx, in ms: [0] membership kernels (host clock: launch to the verdicts on the host, beside
 * the Miller kernel), [1] scaling + Miller kernel (device events), [2] product tree, [3] the MSM
 * sum rho_k C_k, [4] host coefficients and the batch equation, [5] bisecting, [6] total wall; [7] = 1 when the host form answered;
 * [8] zkg16_verify_batch_wire only: the decompress kernels (device events; the host decode's wall time when the host form answered);
 * [9] the per-proof pass that took over from bisecting (device events; 0 when it did not run; its time is part of [5] too),
 * [10] the number of range tests bisecting made; [11] zkg16_verify_prime_batch[_wire] only: the inputs kernel, [12] the sums
 * kernels (device events; both 0 when the host form answered or the call was not a prime call); [13] zkg16_verify_batch_u64[_wire]
 * only: the sums kernels, [14] the X kernel of its per-proof pass (device events; 0 when the host form answered, the call was not
 * a u64 call or, for [14], the per-proof pass did not run); in those calls [10] counts the test of the whole batch too.
 * Returns the number of entries written (at most cap). */
ZKG16_API int zkg16_verify_batch_timings(zkg16_ctx *ctx, float *ms, int cap);

/* ---- re-randomising proofs (ark-groth16 0.4 Groth16::rerandomize_proof): for non-zero r1, r2 in Fr and the key's delta_g2
 *
 *     A' = r1^-1 A        B' = r1 B + (r1 r2) delta        C' = C + r2 A
 *
 * (A', B', C') verifies for exactly the public inputs (A, B, C) verifies for, and a proof that does not verify still does not:
 * both sides of the pairing equation gain e(A, delta)^r2.  Nothing is drawn here: r1, r2 are the caller's, k x 4 Montgomery limbs
 * each, as r and s of zkg16_prove_batch.  proofs k x 48 limbs (A 12 | B 24 | C 12), inf k x 3 flags (nullable: none set).
 * A point is the point at infinity when its flag is set or all its limbs are zero (zkg16_verify_prepared's rule); an output at
 * infinity is zero limbs with its flag set (0xC0 and zeros on the wire).  A = O gives A' = O and C' = C; B = O gives
 * B' = (r1 r2) delta; C = O gives C' = r2 A.  The limb forms do not test membership, like zkg16_verify_prepared's key points: what
 * they return for a point that is on no curve, or for limbs that are not below q, is unspecified (nothing traps).
 * ZKG16_ERR_BAD_ARG before any work, outputs untouched: k == 0, a null pointer (inf excepted), a delta_g2 of all-zero limbs, any
 * r1 or r2 that is zero or whose limbs are not below r — zkg16_last_error (of the ctx; of NULL for the host form, per thread)
 * names the proof index and which multiplier.
 *
 * zkg16_rerandomize_batch_host: no ctx and no GPU, on up to `threads` host threads (0 = 8), by the kernels' own arithmetic compiled
 * for the host: the reference for every byte the device produces.
 * zkg16_rerandomize_batch: on a lane of the ctx, one GPU lane per (proof, group), in passes of at most 65,536 proofs (option
 * "rerandomize_pass" lowers that); byte for byte the host form's output.  Batches shorter than option "rerandomize_min" are
 * answered by the host form (default 256, the measured crossover: see zkg16_set_option).
 * zkg16_rerandomize_batch_wire: proof_bytes k x 192 compressed bytes in, bytes_out k x 192 out, nothing but bytes crossing the
 * bus: decoded by the decompress kernels, every decoded point tested by the membership kernels, re-randomised, encoded by the
 * compress kernel.  A proof with a point that does not decode or is not in the subgroup gets the validating host decoder's status
 * (1 to 5, as decode_status of zkg16_verify_batch_wire) in status (k x 3, nullable) and 192 zero bytes out; the other proofs are
 * unaffected, and the return code is ZKG16_OK.  With status null and any such proof: ZKG16_ERR_BAD_ARG (bytes_out is written). */
ZKG16_API int zkg16_rerandomize_batch_host(const uint64_t delta_g2[24], const uint64_t *proofs, const uint8_t *inf, const uint64_t *r1, const uint64_t *r2,
                                           size_t k, int threads, uint64_t *proofs_out, uint8_t *inf_out);
ZKG16_API int zkg16_rerandomize_batch(zkg16_ctx *ctx, const uint64_t delta_g2[24], const uint64_t *proofs, const uint8_t *inf, const uint64_t *r1,
                                      const uint64_t *r2, size_t k, uint64_t *proofs_out, uint8_t *inf_out);
ZKG16_API int zkg16_rerandomize_batch_wire(zkg16_ctx *ctx, const uint64_t delta_g2[24], const uint8_t *proof_bytes, const uint64_t *r1, const uint64_t *r2,
                                           size_t k, uint8_t *bytes_out, uint8_t *status);
/* Stage entry: the device form of zkg16_points_compress, byte for byte (the flag alone says infinity; inf nullable).  n == 0: ZKG16_OK. */
ZKG16_API int zkg16_points_compress_batch(zkg16_ctx *ctx, int group, const uint64_t *points, const uint8_t *inf, size_t n, uint8_t *out);
/* The last zkg16_rerandomize_batch / zkg16_rerandomize_batch_wire on this ctx, in ms (device events unless said): [0] upload,
 * [1] decompress + membership kernels (wire only), [2] the G1 kernel, [3] the G2 kernel (the two run side by side), [4] the compress
 * kernel (wire only), [5] read-back, [6] total wall (host clock); [7] = 1 when the host form answered (then only [6] is set).  A
 * refused call leaves the entries as they were.  Returns the number of entries written (at most cap). */
ZKG16_API int zkg16_rerandomize_timings(zkg16_ctx *ctx, float *ms, int cap);

/* ---- the prime form: K proofs of the prime handler made under ONE trapdoor (zkg16_prove_prime_batch), verified together.
 * Request i's own key is the template's with gamma_abc_g1[0] + n_i V_n - j_i V_j in front, so no two requests share a key — but
 * everything that differs is a function of (x, j).  Under the EXTENDED key — the template's 258 gamma_abc_g1 points, then V_n, then
 * -V_j (num_instance = 260) — request i has the 259 short public inputs x_i, bit_0 .. bit_255 of SHA-256(x_i + j_i), n_i = that
 * digest mod 2^20, j_i, and X_i = gamma_abc_ext[0] + sum z_i gamma_abc_ext[i] is exactly the X of its own key: one key, no key
 * data per proof, and the Miller, membership, product, per-proof and decompress kernels of zkg16_verify_batch unchanged.
 * zkg16_prime_vk_extend (host only): out (260 x 12) = gamma_abc_g1 (258 x 12) | V_n | -V_j from corr = U | V_n | V_j
 * (zkg16_prime_key_corrections); nulls or a correction at infinity (zero limbs): ZKG16_ERR_BAD_ARG.
 * zkg16_prime_ext_inputs (host only): out (259 x 4, Montgomery) = zkg16_prime_public_inputs(x, j) followed by n and j.
 * zkg16_verify_prime_batch_host: zkg16_verify_batch_host on those inputs; no ctx, no GPU.
 * zkg16_verify_prime_batch / zkg16_verify_prime_batch_wire: zkg16_verify_batch / _wire with the inputs made on the device from
 * xs, js (k u64 each; 16 bytes per proof instead of 8.3 KB of limbs): a SHA-256 kernel (one GPU lane per request), the 260
 * multiplier sums sum_k rho_k z_{k,i} of the member proofs as plain integers in a second kernel (no reduction on the device: every
 * sum stays below 2^224; the host reduces once and cross-checks s_0 against its own sum), and, when the per-proof pass takes over
 * from bisecting, each listed proof's 259 scalars written on the device.  The host expands inputs (from the 32-byte digests it then
 * downloads) only when bisecting runs.  num_instance must be 260 and k below 2^32, else ZKG16_ERR_BAD_ARG before any work; argument
 * checks, undecodable proofs, membership failures, ok_each, decode_status and the options "verify_batch_min" / "verify_wire_min" /
 * "verify_each_after" are exactly those of zkg16_verify_batch / _wire (below the thresholds the host form answers).  A candidate
 * the prover would refuse (n < 2, a zero base) is not an error here: its verdict is the equation's. */
ZKG16_API int zkg16_prime_vk_extend(const uint64_t *gamma_abc_g1 /* 258 x 12 */, const uint64_t corr[36], uint64_t *out /* 260 x 12 */);
ZKG16_API int zkg16_prime_ext_inputs(uint64_t x, uint64_t j, uint64_t *out /* 259 x 4 */);
ZKG16_API int zkg16_verify_prime_batch_host(const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                                  const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                                  const uint64_t *xs, const uint64_t *js, const uint64_t *proofs, const uint8_t *inf, const uint64_t *rho,
                                  size_t k, int threads, int *ok, uint8_t *ok_each);
ZKG16_API int zkg16_verify_prime_batch(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                             const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                             const uint64_t *xs, const uint64_t *js, const uint64_t *proofs, const uint8_t *inf, const uint64_t *rho,
                             size_t k, int *ok, uint8_t *ok_each);
ZKG16_API int zkg16_verify_prime_batch_wire(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                                  const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                                  const uint64_t *xs, const uint64_t *js, const uint8_t *proof_bytes /* k x 192 */, const uint64_t *rho,
                                  size_t k, int *ok, uint8_t *ok_each, uint8_t *decode_status);
/* Stage entries (tests / tools).  zkg16_prime_inputs_batch: digests (k x 32) and n_out (k) = zkg16_prime_candidate's digest and n
 * of each (x, j), byte for byte; public_inputs (nullable, k x 257 x 4) = zkg16_prime_public_inputs.  zkg16_prime_rho_sums: sums
 * (260 x 4 u64, plain integers, unreduced) = sum_k rho_k (1, x_k, bit_0 .. bit_255, n_k, j_k) over the proofs with live[k] != 0
 * (live null: all).  k == 0: ZKG16_OK, nothing written. */
ZKG16_API int zkg16_prime_inputs_batch(zkg16_ctx *ctx, const uint64_t *xs, const uint64_t *js, size_t k, uint8_t *digests, uint32_t *n_out,
                             uint64_t *public_inputs);
ZKG16_API int zkg16_prime_rho_sums(zkg16_ctx *ctx, const uint64_t *xs, const uint64_t *js, const uint64_t *rho, const uint8_t *live, size_t k,
                         uint64_t *sums);

/* ---- the u64 form: K proofs under one key whose public inputs are all plain 64-bit values (the linear-equations route: its
 * n^2 + n inputs a[0][*], b[0], a[1][*], b[1], ... are the row-major matrix [a | b]).  values = k x (num_instance - 1) u64,
 * row-major: 8 bytes per input where zkg16_verify_batch takes 32, and nothing is converted on the host unless bisecting runs.
 * zkg16_verify_batch_u64_host: the values expanded to Montgomery limbs, then zkg16_verify_batch_host; no ctx, no GPU.  It is the
 * reference for every verdict of the calls below.
 * zkg16_verify_batch_u64 / zkg16_verify_batch_u64_wire: zkg16_verify_batch / _wire with the inputs' share of the work on the device.
 * The values go up once; the num_instance multiplier sums s_0 = sum rho_k, s_{1+c} = sum_k rho_k values[k][c] of the member proofs
 * are taken in a kernel as plain integers (rho < 2^128, values < 2^64, k < 2^32: every sum stays below 2^224 < r, nothing is
 * reduced on the device); sum_i s_i gamma_abc_g1[i] is one G1 MSM of the ctx over the key's points with those sums as scalars,
 * and the test of the whole batch takes that point — the host walks neither K x (num_instance - 1) inputs nor num_instance scalar
 * multiplications.  The host cross-checks s_0 against its own sum of the multipliers; on a mismatch the device sums are refused,
 * the verdicts come from host-expanded inputs and the call reports ZKG16_ERR_HIP.  Narrower ranges (bisecting) are computed on
 * the host from inputs expanded on demand.
 * The per-proof pass (zkg16_verify_each_u64, and the take-over from bisecting) makes X_k = gamma_abc[0] + sum_c values[k][c]
 * gamma_abc[1 + c] with each proof spread over L lanes (the smallest power of two >= min(num_instance - 1, 64)), one shared
 * doubling chain of 64 steps per lane; the Miller and final-exponentiation kernels of zkg16_verify_each follow unchanged.
 * In these entries the test of the whole batch counts as the first range test and an UNSET option "verify_each_after" means 1: the
 * per-proof pass decides every member proof right after that test fails (each further range test costs num_instance host scalar
 * multiplications here; the default of 32 was derived at num_instance = 4).  A value the caller set is honoured (a value above
 * 2k bisects to the end).  Below "verify_batch_min" / "verify_wire_min" the host form answers; those thresholds were measured
 * for zkg16_verify_batch / _wire at num_instance = 4 and are reused here, this form's own crossover is not measured.
 * num_instance < 2, null values and k >= 2^32: ZKG16_ERR_BAD_ARG before any work, outputs untouched; every other argument check,
 * undecodable proofs, membership failures, ok_each, decode_status and passes of 65,536 proofs as zkg16_verify_batch / _wire / _each. */
ZKG16_API int zkg16_verify_batch_u64_host(const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                                const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                                const uint64_t *values /* k x (num_instance - 1) */, const uint64_t *proofs, const uint8_t *inf,
                                const uint64_t *rho, size_t k, int threads, int *ok, uint8_t *ok_each);
ZKG16_API int zkg16_verify_batch_u64(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                           const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                           const uint64_t *values, const uint64_t *proofs, const uint8_t *inf, const uint64_t *rho, size_t k,
                           int *ok, uint8_t *ok_each);
ZKG16_API int zkg16_verify_batch_u64_wire(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                                const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                                const uint64_t *values, const uint8_t *proof_bytes /* k x 192 */, const uint64_t *rho, size_t k,
                                int *ok, uint8_t *ok_each, uint8_t *decode_status);
ZKG16_API int zkg16_verify_each_u64(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t alpha_beta[72],
                          const uint64_t *gamma_neg_coeffs, const uint64_t *delta_neg_coeffs, size_t n_coeffs,
                          const uint64_t *values, const uint64_t *proofs, const uint8_t *inf, size_t k, uint8_t *ok_each);
/* Stage entries (tests / tools).  zkg16_u64_rho_sums: sums ((m + 1) x 4 u64, plain integers, unreduced) = sum_k rho_k
 * (1, values[k][0 .. m)) over the proofs with live[k] != 0 (live null: all); m >= 1, k < 2^32; k == 0: ZKG16_OK, nothing written.
 * zkg16_u64_prepared_inputs: x_out[j] (12 u64, affine Montgomery limbs; zeros with inf_out[j] = 1 for the point at infinity) =
 * gamma_abc_g1[0] + sum_c values[idx[j]][c] gamma_abc_g1[1 + c], j < n (idx null: row j; idx entries index rows of values, which
 * must hold them all); gamma_abc_g1 with all-zero limbs = the point at infinity; n == 0: ZKG16_OK, nothing written. */
ZKG16_API int zkg16_u64_rho_sums(zkg16_ctx *ctx, const uint64_t *values, size_t m, const uint64_t *rho, const uint8_t *live, size_t k,
                       uint64_t *sums /* (m + 1) x 4 */);
ZKG16_API int zkg16_u64_prepared_inputs(zkg16_ctx *ctx, const uint64_t *gamma_abc_g1, size_t num_instance, const uint64_t *values,
                              const uint32_t *idx, size_t n, uint64_t *x_out /* n x 12 */, uint8_t *inf_out /* n */);

/* prod_i e(P_i, Q_i) == 1 ?  Host-only (no ctx, no GPU).  g1: n x 12 limbs, g2: n x 24 limbs, flag bytes nullable.
 * flags: ZKG16_PAIRING_PLAIN_FINAL_EXP = final exponentiation as one plain power by (q^12-1)/r (slow cross-check of the
 * default Frobenius + |z|-chain path).  The building block of zkg16_verify; mirrors ark-ec's `Pairing::multi_pairing`
 * followed by the `== one` test of verifier.rs. */
#define ZKG16_PAIRING_PLAIN_FINAL_EXP 1
ZKG16_API int zkg16_pairing_check(const uint64_t *g1, const uint8_t *g1_inf, const uint64_t *g2, const uint8_t *g2_inf, size_t n,
                        int flags, int *ok);

/* ---- host-side circuit synthesis (row a2: stays on the host; no ctx, no GPU).  C++ mirrors of the reference's circuits with
 * the same allocation order (variable k here = variable k in arkworks):
 *   MatrixCircuit     src/arkworks/matrix_proof_of_work/constraints.rs:78-128 (+ Poseidon hasher.rs:17-40, hashing_utils.rs:15-877)
 *   FibonacciCircuit  src/arkworks/constraints/fibbonaci.rs:22-48
 * zkg16_circuit_export yields exactly the arguments of zkg16_r1cs_load / zkg16_witness_load. */
typedef struct zkg16_circuit zkg16_circuit;
ZKG16_API int zkg16_circuit_matrix(size_t n, const uint64_t *a /* n*n, row-major */, const uint64_t *b, zkg16_circuit **out);
/* Only the assignment z (instance || witness, n_assign x 4 limbs) of that circuit for these inputs: the matrices of the
 * MatrixCircuit depend on n alone, so a caller that kept them from one zkg16_circuit_matrix call needs only this per request. */
ZKG16_API int zkg16_circuit_matrix_witness(size_t n, const uint64_t *a, const uint64_t *b, uint64_t *z, size_t n_assign);
ZKG16_API int zkg16_circuit_fibonacci(uint64_t a, uint64_t b, size_t steps, zkg16_circuit **out);
/*   PrimeCircuit      src/arkworks/prime_snark/prime_circut.rs:92-146 (+ fermat_circut.rs, utils/hasher.rs, utils/modulo.rs): SHA-256 of
 *                     x + j, the digest mod 2^20, three hashed Fermat bases, 20-step square-and-multiply with witnessed quotients.
 *                     The SHA-256 / Boolean / comparison gadgets come from un-vendored crates upstream and are restated here:
 *                     values (digests, modpows, satisfaction, verification) are checked, the constraint LAYOUT is unpinned.
 * zkg16_prime_search = the handler's loop over check_if_next_is_prime (backend/prime_snark.rs:57-70). */
ZKG16_API int zkg16_prime_search(uint64_t x, uint64_t i_max, uint64_t *j_out, uint32_t *prime_out, uint8_t digest_out[32], int *found);
ZKG16_API int zkg16_prime_candidate(uint64_t x, uint64_t j, uint8_t digest_out[32], uint32_t *n_out, uint32_t bases_out[3],
                          uint8_t r_bytes_out[32], int *is_prime);
ZKG16_API int zkg16_circuit_prime(uint64_t x, uint64_t j, zkg16_circuit **out);
/* The PrimeCircuit's 257 public inputs (x, then the digest bits) without building the circuit: out = 257 x 4 limbs, Montgomery. */
ZKG16_API int zkg16_prime_public_inputs(uint64_t x, uint64_t j, uint64_t *out);
ZKG16_API void zkg16_circuit_free(zkg16_circuit *c);
ZKG16_API int zkg16_circuit_dims(const zkg16_circuit *c, size_t *num_instance, size_t *num_witness, size_t *num_constraints, size_t nnz[3]);
ZKG16_API int zkg16_circuit_is_satisfied(const zkg16_circuit *c);
ZKG16_API int zkg16_circuit_export(const zkg16_circuit *c, uint64_t *const row_ptr[3], uint32_t *const col[3], uint64_t *const coeff[3],
                         uint64_t *full_assignment /* (num_instance + num_witness) x 4 */);
/* The public inputs (instance assignment without the leading one): (num_instance - 1) x 4 limbs; cap = room in elements. */
ZKG16_API int zkg16_circuit_public_inputs(const zkg16_circuit *c, uint64_t *out, size_t cap);
/* Load a synthesized circuit straight onto the device: *r1cs_handle as from zkg16_r1cs_load and *witness_handle as from
 * zkg16_witness_load of zkg16_circuit_export's arrays (same bytes on the device), staged through pinned memory the ctx keeps — the
 * request path of the handlers whose circuits are re-synthesized per request (PrimeCircuit, Fibonacci). */
ZKG16_API int zkg16_circuit_load(zkg16_ctx *ctx, const zkg16_circuit *c, uint64_t *r1cs_handle, uint64_t *witness_handle);
/* ---- the MatrixCircuit's assignment built ON THE DEVICE (scope row f-4 "on GPU"; csrc/witness.hip).  The reference re-synthesises
 * the circuit inside its timed `Groth16::prove` (matrix_proof.rs:138-145, constraints.rs:78-128): per request only the
 * assignment changes, 75 % of which are the S-box products of 3 ceil(n^2/2) Poseidon permutations (hashing_utils.rs:737-802).
 * The host runs the three native sponges (sequential by construction: hasher.rs:17-27) and keeps the state in front of every
 * permutation; kernels write z in place — a, b as Fr, the n^3 products, 265 values per permutation — into a buffer
 * zkg16_prove_resident reads.  *witness_handle: as from zkg16_witness_load of zkg16_circuit_matrix_witness's output (same bytes).
 * public_inputs (nullable): hash_a | hash_b | hash_c, Montgomery.  timings_ms (nullable, 3 floats): host sponges, device
 * (upload + kernels), whole call. */
ZKG16_API int zkg16_witness_matrix(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, uint64_t *witness_handle,
                         uint64_t public_inputs[12], float *timings_ms);
/* One request of the matrix handler on a key and matrices that are resident: assignment + proof, overlapped — the host sponges feed
 * the device in parts (option "matrix_parts", default five growing slices) and the z-side MSMs run on the parts that exist while the sponges
 * still compute the rest; same proof bytes as zkg16_witness_matrix + zkg16_prove_resident.  r1cs_handle / pk_handle must be the
 * MatrixCircuit of size n (else ZKG16_ERR_BAD_ARG).  public_inputs (nullable): hash_a | hash_b | hash_c.  timings_ms (nullable, 3):
 * host sponges (wall, overlapped with the device), parts used, whole call. */
ZKG16_API int zkg16_prove_matrix(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t n, const uint64_t *a, const uint64_t *b,
                       const uint64_t r[4], const uint64_t s[4], uint64_t proof_out[48], uint8_t inf_out[3], uint64_t public_inputs[12],
                       float *timings_ms);
/* The slices zkg16_prove_matrix would feed a proof of size n in under option values "matrix_parts" = parts_wanted (0..8) and
 * "matrix_slice_min" = slice_min (0 = the default, 512; else 1..2^20), host only (no ctx, no GPU; the one function the proof itself
 * calls): *slices_out = the slice count, bounds_out[0 .. slices] = the first permutation of every slice, then ceil(n^2/2); the words
 * behind them are zero.  The proof has slices + 1 parts: part 0 is what needs a and b alone, part 1 + s the S-box values of slice s of
 * every sponge, the last part also the three hashes.  parts_wanted 1 describes the one slice of a proof that does not overlap.  n
 * outside 2..1024, an option value out of range or a null pointer: ZKG16_ERR_BAD_ARG, nothing written. */
ZKG16_API int zkg16_matrix_stream_bounds(size_t n, int parts_wanted, int slice_min, uint32_t bounds_out[9], int *slices_out);
/* The streamed assignment of zkg16_prove_matrix alone, part by part (diagnostics for tests): the stream object, its attachment and its
 * produce(k) calls are the proof's own, under the ctx's "matrix_parts" and "matrix_slice_min"; no MSM and no witness map runs.  The
 * assignment buffer is filled with 0xFF bytes first (an all-ones word is at least r: no stored Fr equals it); after every part the
 * ctx's stream is drained and the buffer read back.  part_of_out[n_assign + 3]: the device's part map (the three trailing entries are
 * the r, s, -rs slots); all 255 under "matrix_parts" 1, which builds none.  first_valid_out[n_assign]: the first part after which entry
 * i differs from the fill, 255 = never written.  z_out[n_assign][4]: the finished assignment, the bytes of
 * zkg16_circuit_matrix_witness.  *parts_out: the parts produced.  n_assign must be the circuit's variable count (num_witness + 4 of
 * zkg16_matrix_r1cs_dims); that, n outside 2..1024 or a null pointer: ZKG16_ERR_BAD_ARG.  On any error no output is written. */
ZKG16_API int zkg16_diag_matrix_stream(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, uint8_t *part_of_out,
                                       uint8_t *first_valid_out, uint64_t *z_out, size_t n_assign, int *parts_out);
/* Its host-only half (no ctx, no GPU): states (nullable) = 3 hashes x ceil(n^2/2) permutations x 3 Fr, the sponge state in
 * front of each permutation (after its two elements were absorbed); hashes = hash_a | hash_b | hash_c. */
ZKG16_API int zkg16_matrix_sponge_states(size_t n, const uint64_t *a, const uint64_t *b, uint64_t *states, uint64_t hashes[12]);
/* The same for k requests of one size on a pool of host threads (no ctx, no GPU).  a, b: k x n^2, request-major.  threads: 0 = 8; the
 * value is capped at 16 and at 3k (the 3k chains are the tasks: a chain is sequential, the c chains are handed out first).  Request
 * i's states (nullable: k x 3 x ceil(n^2/2) x 12) and hashes (k x 12) are byte for byte those of zkg16_matrix_sponge_states(n, a_i,
 * b_i).  n outside 2..1024, k == 0, threads < 0 or a null a / b / hashes: ZKG16_ERR_BAD_ARG, nothing written. */
ZKG16_API int zkg16_matrix_sponge_states_batch(size_t n, const uint64_t *a, const uint64_t *b, size_t k, int threads, uint64_t *states,
                                               uint64_t *hashes);
/* zkg16_witness_matrix for k requests of one size in ONE upload, two launches and one synchronisation: the chains of all requests run
 * first, before the ctx is locked, on option "matrix_batch_threads" host threads; the device then reads one array of all a | b, one
 * of all entering states and the k instance triples out of pinned staging the ctx keeps, and writes the k assignments — which share
 * one allocation, returned when the last of the k handles is freed — through a table of their addresses.  witness_handles[i]: the
 * bytes of zkg16_witness_matrix(n, a_i, b_i), usable wherever a witness handle is.  public_inputs (nullable): k x 12.  timings_ms
 * (nullable, 3): host chains (wall), device (uploads + kernels), whole call.  Arguments as zkg16_witness_matrix, and k == 0 or k
 * assignments beyond a size_t: ZKG16_ERR_BAD_ARG, before any work.  All or nothing: on any error no handle is registered and neither
 * witness_handles nor public_inputs is written. */
ZKG16_API int zkg16_witness_matrix_batch(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, size_t k, uint64_t *witness_handles,
                                         uint64_t *public_inputs, float *timings_ms);
/* k requests of the matrix handler on one resident key: a, b (k x n^2) in, k proofs and their public inputs out.  Proof i is byte for
 * byte zkg16_prove_resident's on zkg16_witness_matrix(n, a_i, b_i) with (r + 4i, s + 4i).  One lane.  The work goes in sub-batches sized
 * as zkg16_prove_batch's with the assignment itself (32 B per variable) added per proof, capped by option "batch_max"; per sub-batch the
 * host chains, the batched witness pass, then the batched proof, after which its assignments are released — no witness handle ever
 * exists.  pk_handle / r1cs_handle must be a whole key and the MatrixCircuit of size n (ZKG16_ERR_BAD_HANDLE, ZKG16_ERR_UNSUPPORTED
 * for a shard, else ZKG16_ERR_BAD_ARG, as k == 0 and null pointers): all checked before any work.  On any error nothing is written
 * (proofs and public inputs are staged until every sub-batch has succeeded).  public_inputs (nullable): k x 12.  timings_ms (nullable,
 * 4): host chains (summed wall), witness passes (device), proving (zkg16_last_timings[9] summed), whole call.  zkg16_last_timings /
 * zkg16_last_term_counts describe the batch as after zkg16_prove_batch. */
ZKG16_API int zkg16_prove_matrix_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t n, const uint64_t *a,
                                       const uint64_t *b, size_t k, const uint64_t *r, const uint64_t *s, uint64_t *proofs_out /* k x 48 */,
                                       uint8_t *inf_out /* k x 3 */, uint64_t *public_inputs, float *timings_ms);
/* ---- the MatrixCircuit's R1CS of size n WITHOUT synthesising it constraint by constraint (csrc/matrix_plan.hpp): the sponge rows are
 * copies of one template per permutation class with renamed variables, matrix_mul's rows have a closed form.  _dims / _host: host
 * loops (the reference the device kernel is tested against; same arrays as zkg16_circuit_matrix + zkg16_circuit_export);
 * zkg16_r1cs_matrix: the same arrays written by a kernel straight into HBM -> an r1cs handle as from zkg16_r1cs_load, with nothing
 * but the templates (a few hundred KB) crossing PCIe instead of 3.7 GB at 128x128.  zkg16_r1cs_read copies a handle's arrays back. */
ZKG16_API int zkg16_matrix_r1cs_dims(size_t n, size_t *num_constraints, size_t *num_witness, size_t nnz[3]);
ZKG16_API int zkg16_matrix_r1cs_host(size_t n, uint64_t *const row_ptr[3], uint32_t *const col[3], uint64_t *const coeff[3]);
ZKG16_API int zkg16_r1cs_matrix(zkg16_ctx *ctx, size_t n, uint64_t *r1cs_handle);
ZKG16_API int zkg16_r1cs_read(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t *const row_ptr[3], uint32_t *const col[3], uint64_t *const coeff[3],
                    size_t *num_instance, size_t *num_constraints, size_t *num_variables, size_t nnz[3]);
/* ---- the PrimeCircuit of candidate (x, j) WITHOUT synthesising it (csrc/prime_program.hpp): a witness program and the R1CS, recorded
 * once per process from one sequential build.  Every entry refuses the candidates zkg16_circuit_prime refuses (ZKG16_ERR_UNSUPPORTED).
 * _host: host loops, the references of the device entries (same bytes as zkg16_circuit_prime + zkg16_circuit_export; z: n_assign =
 * num_instance + num_witness entries x 4 limbs, Montgomery).  _dims: the dimensions depend on j only (C has one non-zero fewer at j = 0).
 * zkg16_r1cs_prime: an r1cs handle as from zkg16_r1cs_load of those arrays — a device-to-device copy of the template the ctx keeps
 * resident (uploaded on first use, freed by zkg16_destroy) plus four coefficients.  zkg16_witness_prime: a witness handle with the bytes
 * of zkg16_witness_load of that z — the host computes the program's inputs (a few hundred field elements), kernels evaluate the bits. */
ZKG16_API int zkg16_prime_witness_host(uint64_t x, uint64_t j, uint64_t *z, size_t n_assign);
ZKG16_API int zkg16_prime_r1cs_dims(uint64_t j, size_t *num_instance, size_t *num_witness, size_t *num_constraints, size_t nnz[3]);
ZKG16_API int zkg16_prime_r1cs_host(uint64_t x, uint64_t j, uint64_t *const row_ptr[3], uint32_t *const col[3], uint64_t *const coeff[3]);
ZKG16_API int zkg16_r1cs_prime(zkg16_ctx *ctx, uint64_t x, uint64_t j, uint64_t *r1cs_handle);
ZKG16_API int zkg16_witness_prime(zkg16_ctx *ctx, uint64_t x, uint64_t j, uint64_t *witness_handle);
/* ---- K prime requests on ONE key.  Two candidates' R1CS differ in four coefficients of column 0 (the constant-one variable): n three
 * times in A, -j once in C.  The TEMPLATE is the j >= 1 form with those four set to zero; for one trapdoor a candidate's key differs
 * from the template's in a_query[0] and gamma_abc_g1[0] only:
 *     a_query[0] = template's + n U,    gamma_abc_g1[0] = template's + n V_n - j V_j,
 *     U = [u] g1, V_n = [beta u / gamma] g1, V_j = [w / gamma] g1,  u = L_r1(tau) + L_r2(tau) + L_r3(tau), w = L_r4(tau),
 * r1..r3 the rows of A's patched coefficients, r4 the row of C's, L_i the Lagrange polynomials of the domain.
 * zkg16_prime_r1cs_template_host (no ctx): the template arrays, with the dimensions of zkg16_prime_r1cs_dims(1, ...), and r1..r4.
 * zkg16_r1cs_prime_template: an r1cs handle holding those bytes (a device-to-device copy of the resident template), marked as the
 * template — the only handle zkg16_prove_prime_batch takes.  zkg16_prime_key_corrections (host only; the trapdoor is not kept):
 * corr_out = U | V_n | V_j as affine Montgomery limbs, inf_out their infinity flags.
 * zkg16_witness_prime_batch: zkg16_witness_prime for k candidates in one upload, two launches and one synchronisation; handle i holds
 * the bytes of zkg16_witness_prime(xs[i], js[i]); the k assignments share one allocation, returned when the last handle is freed.  All
 * or nothing: a refused candidate gives ZKG16_ERR_UNSUPPORTED, no handle is registered and nothing is written. */
ZKG16_API int zkg16_prime_r1cs_template_host(uint64_t *const row_ptr[3], uint32_t *const col[3], uint64_t *const coeff[3], uint64_t patch_rows[4]);
ZKG16_API int zkg16_r1cs_prime_template(zkg16_ctx *ctx, uint64_t *r1cs_handle);
ZKG16_API int zkg16_prime_key_corrections(const uint64_t trapdoor[20], const uint64_t g1_gen[12], uint64_t corr_out[36], uint8_t inf_out[3]);
ZKG16_API int zkg16_witness_prime_batch(zkg16_ctx *ctx, const uint64_t *xs, const uint64_t *js, size_t k, uint64_t *witness_handles);
/* k prime requests on the template key (zkg16_setup_resident of the template handle) in batched device passes: per sub-batch (sized
 * as zkg16_prove_batch's with the assignment added per proof; option "batch_max") the batched assignment, then the batched proof
 * with request i's n added to A z in rows r1..r3 and -j to C z in row r4 before the transforms, and n U added to its A on the host.
 * Proof i is byte for byte zkg16_prove_resident's on zkg16_r1cs_prime / zkg16_witness_prime(xs[i], js[i]) under the key
 * zkg16_setup_resident gives that R1CS for the same trapdoor and generators, with (r + 4i, s + 4i); gamma_abc0_out[12 i ..] is that
 * key's gamma_abc_g1[0] (every other verifying-key element is the template's).  corr: zkg16_prime_key_corrections' output (no
 * infinity among them); gamma_abc0_template: the template key's gamma_abc_g1[0].  public_inputs (nullable): k x 257 x 4
 * (zkg16_prime_public_inputs).  timings_ms (nullable, 4): host inputs (prime_inputs, summed wall), assignment passes (device),
 * proving (zkg16_last_timings[9] summed), whole call.  One lane.  Checked before any work: unknown handles (ZKG16_ERR_BAD_HANDLE), a
 * shard key (ZKG16_ERR_UNSUPPORTED), an r1cs handle that is not the template, a key that does not fit it, k == 0 or null pointers
 * (ZKG16_ERR_BAD_ARG), a refused candidate anywhere in the batch (ZKG16_ERR_UNSUPPORTED).  On any error nothing is written. */
ZKG16_API int zkg16_prove_prime_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, const uint64_t corr[36],
                                      const uint64_t gamma_abc0_template[12], const uint64_t *xs, const uint64_t *js, size_t k,
                                      const uint64_t *r, const uint64_t *s, uint64_t *proofs_out /* k x 48 */, uint8_t *inf_out /* k x 3 */,
                                      uint64_t *gamma_abc0_out /* k x 12 */, uint64_t *public_inputs /* nullable, k x 257 x 4 */,
                                      float *timings_ms /* nullable, 4 */);
/* ---- K Fibonacci requests on ONE key.  The FibonacciCircuit's matrices depend on `steps` alone (fibbonaci.rs:22-48: a, b and result
 * occur only in the assignment), so one key per round count serves every request of that count, with no template and no corrections.
 * A request's assignment is five elements: 1, a, b, result, 0; result = c_a a + c_b b with two coefficients that depend on `steps`
 * alone.  steps above ZKG16_FIBONACCI_STEPS_MAX: ZKG16_ERR_BAD_ARG in every entry below.
 * zkg16_fibonacci_results_host (no ctx, no GPU): a, b = k u64; out[4 i ..] = the `result` input of zkg16_circuit_fibonacci(a[i], b[i],
 * steps) as Montgomery limbs — the value in Fr, by the additive chain, request by request: the reference the kernel is tested against.
 * k == 0 or a null pointer: ZKG16_ERR_BAD_ARG, nothing written.
 * zkg16_r1cs_fibonacci: the circuit's matrices as an r1cs handle with no request in hand — the arrays of zkg16_circuit_fibonacci +
 * zkg16_circuit_export for any (a, b), built by the host mirror and uploaded (steps + 1 rows: a kernel would not pay).
 * zkg16_witness_fibonacci_batch: k assignments in ONE upload (16 bytes of input and one address per request), one launch and one
 * synchronisation; handle i holds byte for byte the assignment zkg16_circuit_export gives for (a[i], b[i], steps) and is usable
 * wherever a witness handle is.  The assignments share one allocation, returned when the last handle is freed.  public_inputs
 * (nullable): k x 12 limbs, a | b | result.  timings_ms (nullable, 3): host coefficients, device (upload + kernel + read-back), whole
 * call.  All or nothing: on any error no handle is registered and nothing is written. */
#define ZKG16_FIBONACCI_STEPS_MAX ((size_t)0x0FFFFFFF) /* 2^28 - 1 */
ZKG16_API int zkg16_fibonacci_results_host(size_t steps, const uint64_t *a, const uint64_t *b, size_t k, uint64_t *out /* k x 4 */);
ZKG16_API int zkg16_r1cs_fibonacci(zkg16_ctx *ctx, size_t steps, uint64_t *r1cs_handle);
ZKG16_API int zkg16_witness_fibonacci_batch(zkg16_ctx *ctx, size_t steps, const uint64_t *a, const uint64_t *b, size_t k,
                                            uint64_t *witness_handles, uint64_t *public_inputs, float *timings_ms);
/* k requests of the Fibonacci handler on one resident key: a, b (k u64 each) in, k proofs and their public inputs out.  Proof i is byte
 * for byte zkg16_prove_resident's on the assignment above with (r + 4i, s + 4i).  One lane.  The work goes in sub-batches sized as
 * zkg16_prove_batch's, capped by option "batch_max"; per sub-batch the batched assignment pass, then the batched proof, after which its
 * assignments are released — no witness handle ever exists.  Checked before any work, in this order: k == 0 or a null pointer
 * (ZKG16_ERR_BAD_ARG), an unknown handle (ZKG16_ERR_BAD_HANDLE), a shard key (ZKG16_ERR_UNSUPPORTED), a key that does not fit the
 * r1cs handle or an r1cs handle whose dimensions are not those of the FibonacciCircuit of `steps` (ZKG16_ERR_BAD_ARG).  On any error
 * nothing is written (proofs and public inputs are staged until every sub-batch has succeeded).  public_inputs (nullable): k x 12,
 * a | b | result.  timings_ms (nullable, 4): host coefficients, assignment passes (device), proving (zkg16_last_timings[9] summed),
 * whole call.  zkg16_last_timings / zkg16_last_term_counts describe the batch as after zkg16_prove_batch. */
ZKG16_API int zkg16_prove_fibonacci_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t steps, const uint64_t *a,
                                          const uint64_t *b, size_t k, const uint64_t *r, const uint64_t *s, uint64_t *proofs_out /* k x 48 */,
                                          uint8_t *inf_out /* k x 3 */, uint64_t *public_inputs, float *timings_ms);
/* ---- the linear-equations route (backend/linear_equations.rs:43-106, constraints/linear_equations_constraints.rs:39-61) and K of its
 * requests on ONE key.  A request is a square system: a = n x n u64 row-major, b = n u64.  The handler's solver (:20-41) starts from
 * x = 0 and sets x[i] = (b[i] - sum_j a[i][j] x[j]) / a[i][i] for i = 0 .. n-1, so only the terms j < i contribute: x solves L x = b
 * with L the lower triangle of a, diagonal included.  The circuit claims a x = b, so a request whose a has non-zero entries above the
 * diagonal is in general UNSATISFIED by the handler's own assignment — by design of the reference; option "linear_solver" = 1, below,
 * solves the system the circuit claims instead — (failing rows: the equality rows i (n + 1) + n of the i with
 * (U x)_i != 0, U the strict upper triangle): zkg16_r1cs_check and option "check_satisfied" report it.  a[i][i] == 0, a panic upstream
 * (inverse().unwrap()), is ZKG16_ERR_UNSUPPORTED here, before any other work.
 * Layout, with NI = 1 + n (n + 1) instance values first (ark's ConstraintMatrices): a_ij at 1 + i (n + 1) + j, b_i at 1 + i (n + 1) + n;
 * witness w in column NI + w, NW = n (2 n + 1): per row i the sum's seed 0 at w = i (2 n + 1), the copy of x_j at i (2 n + 1) + 1 + 2 j and
 * the product a_ij x_j at i (2 n + 1) + 2 + 2 j.  NC = n (n + 1) constraints: row i (n + 1) + j is a_ij * x-copy = product; row i (n + 1) + n
 * is (-b_i + seed + sum_j product_ij) * 1 = 0.  The matrices depend on n alone, so one key per n serves every request.
 * n == 0, n > ZKG16_LINEAR_N_MAX, k == 0 or a null pointer: ZKG16_ERR_BAD_ARG in every entry below; every entry is all or nothing — on
 * any error no handle is registered and no output byte is written.
 * zkg16_circuit_linear (no ctx, no GPU): the host mirror, for zkg16_circuit_dims / _export / _is_satisfied / _public_inputs / _load.
 * zkg16_linear_solve_host (no ctx, no GPU): the solver for k requests, x_out[(i n + j) 4 ..] = x_j of request i as Montgomery limbs:
 * the reference the kernels are tested against.
 * zkg16_linear_r1cs_dims: the dimensions and non-zero counts (2 n^2 + 2 n, n^2 + n, n^2) with no request in hand (outputs nullable).
 * zkg16_r1cs_linear: the matrices as an r1cs handle with no request in hand, written on the host from the closed form above and
 * uploaded once per n — byte for byte the arrays of zkg16_circuit_linear + zkg16_circuit_export for any (a, b).
 * zkg16_witness_linear_batch: k assignments in ONE upload (8 bytes per input value), two launches whatever k is (the solve: one
 * 64-lane wave per request; the fill: one lane per element of an assignment) and one synchronisation.  Handle i holds byte for byte
 * the assignment zkg16_circuit_export gives for request i and is usable wherever a witness handle is.  The assignments share one
 * allocation, returned when the last handle is freed.  x_out (nullable): k x n x 4 limbs.  timings_ms (nullable, 3): host checks,
 * device (upload + kernels + read-back), whole call.  A zero diagonal entry in any request: ZKG16_ERR_UNSUPPORTED, zkg16_last_error
 * names the request and the row.
 * Option "linear_solver" (zkg16_set_option; per ctx): 0 (default) is the solver above, the reference's behaviour, and every entry, error
 * and byte is as described.  1 solves a x = b itself, by Gaussian elimination over Fr with row pivoting (any non-zero entry of the column
 * among the rows left; division-free row updates p row_i - a_ic row_c, then the n pivots inverted at once, then the back substitution by
 * columns), so a request with ANY a that is non-singular mod r is satisfied and its proof verifies; for a lower-triangular a with a
 * non-zero diagonal x and every byte are those of solver 0.  zkg16_witness_linear_batch and zkg16_prove_linear_batch read the option: under 1
 * the zero-diagonal check is skipped, the solve launch is wit_linear_elim_kernel (one 256-lane workgroup per request; the n x (n + 1)
 * working matrix in LDS for n <= option "linear_elim_lds_max", 64 by default, else in a global workspace of 32 n (n + 1) bytes per
 * workgroup, which zkg16_prove_linear_batch's sub-batch sizing counts per request), and its k status words are read back at the call's
 * (sub-batch's) one synchronisation: 0, or 1 + c with c the smallest column index for which columns 0..c of a are linearly dependent
 * mod r — a value no pivot order changes.  Any singular request: ZKG16_ERR_UNSUPPORTED, nothing written, no handle registered,
 * zkg16_last_error names the first such request and c.  The order of the other argument checks is unchanged.
 * zkg16_linear_solve_general_host (no ctx, no GPU): the same elimination (the kernel's phase functions on one lane) for k requests;
 * status_out (nullable, k) is written whenever the arguments are good, x_out only when every request was solved, else
 * ZKG16_ERR_UNSUPPORTED.  zkg16_circuit_linear_general: zkg16_circuit_linear with the eliminated x as the assignment (the same matrices);
 * a singular a: ZKG16_ERR_UNSUPPORTED. */
#define ZKG16_LINEAR_N_MAX ((size_t)1024)
ZKG16_API int zkg16_circuit_linear(size_t n, const uint64_t *a /* n x n */, const uint64_t *b /* n */, zkg16_circuit **out);
ZKG16_API int zkg16_linear_solve_host(size_t n, const uint64_t *a /* k x n x n */, const uint64_t *b /* k x n */, size_t k,
                                      uint64_t *x_out /* k x n x 4 */);
ZKG16_API int zkg16_circuit_linear_general(size_t n, const uint64_t *a /* n x n */, const uint64_t *b /* n */, zkg16_circuit **out);
ZKG16_API int zkg16_linear_solve_general_host(size_t n, const uint64_t *a /* k x n x n */, const uint64_t *b /* k x n */, size_t k,
                                              uint64_t *x_out /* k x n x 4 */, uint32_t *status_out /* k */);
ZKG16_API int zkg16_linear_r1cs_dims(size_t n, size_t *num_instance, size_t *num_witness, size_t *num_constraints, size_t nnz[3]);
ZKG16_API int zkg16_r1cs_linear(zkg16_ctx *ctx, size_t n, uint64_t *r1cs_handle);
ZKG16_API int zkg16_witness_linear_batch(zkg16_ctx *ctx, size_t n, const uint64_t *a, const uint64_t *b, size_t k, uint64_t *witness_handles,
                                         uint64_t *x_out, float *timings_ms);
/* k requests of the linear handler on one resident key.  Proof i is byte for byte zkg16_prove_resident's on the assignment above with
 * (r + 4i, s + 4i).  One lane.  The work goes in sub-batches sized as zkg16_prove_batch's with the assignment and its input added per
 * proof, capped by option "batch_max"; per sub-batch the batched assignment pass, then the batched proof, after which its assignments
 * are released — no witness handle ever exists.  Option "check_satisfied" applies as to the other batch entries: a batch holding a
 * request the solver leaves unsatisfied returns ZKG16_ERR_UNSATISFIED, writes nothing, and zkg16_last_check names it.  Checked before
 * any work, in this order: k == 0, n == 0, n > ZKG16_LINEAR_N_MAX or a null pointer (ZKG16_ERR_BAD_ARG), an unknown handle
 * (ZKG16_ERR_BAD_HANDLE), a shard key (ZKG16_ERR_UNSUPPORTED), a key that does not fit the r1cs handle or an r1cs handle whose
 * dimensions are not those of the n-system (ZKG16_ERR_BAD_ARG), a zero diagonal entry in any request (ZKG16_ERR_UNSUPPORTED,
 * zkg16_last_error names the request and the row).  x_out (nullable): k x n x 4.  timings_ms (nullable, 4): host checks, assignment
 * passes (device), proving (zkg16_last_timings[9] summed), whole call. */
ZKG16_API int zkg16_prove_linear_batch(zkg16_ctx *ctx, uint64_t pk_handle, uint64_t r1cs_handle, size_t n, const uint64_t *a, const uint64_t *b,
                                       size_t k, const uint64_t *r, const uint64_t *s, uint64_t *proofs_out /* k x 48 */,
                                       uint8_t *inf_out /* k x 3 */, uint64_t *x_out, float *timings_ms);
/* ---- does an assignment satisfy its R1CS?  (A z)_i * (B z)_i == (C z)_i for every constraint row i < num_constraints, compared as fully
 * reduced residues.  The proving calls prove whatever they are handed: an unsatisfied assignment gives a well-formed proof that no
 * verifier accepts (arkworks' prover debug_asserts cs.is_satisfied(); prime_snark.rs:123-128 asserts it on every request).  The witness
 * map begins with the three sparse products written side by side, so the check is ONE kernel over rows a proof computes anyway
 * (csrc/r1cs_check_dev.cuh; r1cs_check_kernel in csrc/poly.hip): a lane per row forms the Montgomery product and compares, a block
 * folds its verdicts by ballot, and a block with a failing row makes one atomic add and one atomic min on two 64-bit words per
 * assignment, which are read back once per call.  Rows at or beyond num_constraints (the instance rows, the padding) are no rows of the
 * system and are not looked at; the verdict does not depend on the coefficient dictionary or the row order of the sparse product.
 * Every entry: *n_bad (required) = failing rows, *first_bad (nullable) = the smallest failing row, UINT64_MAX when none.  Null
 * pointers, k == 0 and lengths that do not match: ZKG16_ERR_BAD_ARG; unknown handles: ZKG16_ERR_BAD_HANDLE; all checked before any
 * work, and the outputs are then untouched.
 * zkg16_r1cs_check_host: no ctx, no GPU — the reference of the device entries and the check for callers without a device.  Arrays as
 * for zkg16_r1cs_load (col / coeff of a matrix without non-zeros may be null), z: num_variables x 4 limbs.  A decreasing row pointer or
 * a column >= num_variables: ZKG16_ERR_BAD_ARG.
 * zkg16_r1cs_check: one sparse product and the kernel, on the witness map's own vectors.  It counts as a use of the r1cs handle exactly
 * as a witness map does (zkg16_r1cs_spmv_state's spmv_uses: the dictionary and the row order are built on the second use).
 * zkg16_r1cs_check_batch: k assignments of one system; per sub-batch one batched sparse product and one launch.  A sub-batch is what
 * fits the witness map's four vectors per assignment into 60 % of the free HBM — never more than zkg16_prove_batch would take — at
 * most 65,535, capped by option "batch_max".
 * zkg16_prime_check_batch: k prime requests on the TEMPLATE handle (zkg16_r1cs_prime_template; any other handle: ZKG16_ERR_BAD_ARG).
 * The assignments are built as zkg16_prove_prime_batch builds them, then the batched sparse product, then each request's n and -j
 * added at the template's four patch rows, then the kernel: request i's verdict is zkg16_r1cs_check's on zkg16_r1cs_prime /
 * zkg16_witness_prime(xs[i], js[i]).  A refused candidate anywhere: ZKG16_ERR_UNSUPPORTED before any device work.
 * zkg16_r1cs_check[_batch] on a template handle is ZKG16_ERR_UNSUPPORTED: the template is no request's system.
 * Inside the proving calls: option "check_satisfied" (zkg16_set_option) launches the same kernel right after the sparse product (and
 * the patch) of the proof's own witness map, on the same stream, before the first transform — no second sparse product.  The verdict
 * is read where the proof's results are collected; if any assignment of the call failed, the call returns ZKG16_ERR_UNSATISFIED and
 * writes nothing.  It applies to zkg16_prove_resident, zkg16_prove, zkg16_prove_partial (ranks with an h range), zkg16_prove_matrix,
 * zkg16_prove_batch, zkg16_prove_matrix_batch and zkg16_prove_prime_batch.  Group calls (zkg16_prove_group, zkg16_witness_map_group)
 * never check, whatever the option says.  Off (the default) nothing changes: no launch, no allocation, the same bytes.
 * zkg16_last_check: the per-proof verdicts of the last proving call that checked, attributed to the ctx as zkg16_last_timings
 * attributes its times (the lane of the proof that finished last): *k_out (nullable) = proofs of that call (0: it did not check), up
 * to cap of them written to n_bad / first_bad (either nullable).  Returns the number written. */
ZKG16_API int zkg16_r1cs_check_host(const uint64_t *const row_ptr[3], const uint32_t *const col[3], const uint64_t *const coeff[3],
                          size_t num_constraints, size_t num_variables, const uint64_t *z, uint64_t *n_bad, uint64_t *first_bad);
ZKG16_API int zkg16_r1cs_check(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, uint64_t *n_bad, uint64_t *first_bad);
ZKG16_API int zkg16_r1cs_check_batch(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t *witness_handles, size_t k,
                           uint64_t *n_bad /* k */, uint64_t *first_bad /* nullable, k */);
ZKG16_API int zkg16_prime_check_batch(zkg16_ctx *ctx, uint64_t r1cs_template_handle, const uint64_t *xs, const uint64_t *js, size_t k,
                            uint64_t *n_bad /* k */, uint64_t *first_bad /* nullable, k */);
ZKG16_API int zkg16_last_check(zkg16_ctx *ctx, uint64_t *n_bad, uint64_t *first_bad, size_t cap, size_t *k_out);

/* ---- The trapdoor route: setup-and-prove requests answered without the proving key.
 * THIS IS NOT A WAY TO PROVE UNDER SOMEONE ELSE'S KEY.  It is for callers that drew the trapdoor themselves — every handler of the
 * reference does, proves once and drops the key — and who could therefore forge a proof of any statement anyway.  What it saves is
 * building and consuming a proving key nobody else ever reads.  With u_k, v_k, w_k the QAP column values at tau and
 * lg_k = (beta u_k + alpha v_k + w_k) / delta, a SATISFIED assignment z has
 *   S_u = sum z_k u_k   S_v = sum z_k v_k   S_w = sum z_k w_k   S_l = sum_{k >= num_instance} z_k lg_k
 *   a = alpha + S_u + r delta     b = beta + S_v + s delta     c = S_l + (S_u S_v - S_w) / delta + s a + r b - r s delta
 *   A = a G1   B = b G2   C = c G1
 * (h(tau) Z(tau) = S_u S_v - S_w because h Z = a b - c as polynomials).  These are the group elements the key route computes, and
 * affine coordinates are unique: proof i is byte for byte
 *   zkg16_prove_resident(zkg16_setup_resident(r1cs, trapdoor, g1_gen, g2_gen), r1cs, witness_handles[i], r + 4 i, s + 4 i)
 * and alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1 are zkg16_setup_resident's.  A log of 0 is the point at infinity (limbs 0,
 * flag 1), as zkg16_prove_resident writes one.
 * The identity needs a satisfied z (arkworks' h is not the quotient otherwise), so satisfaction is ALWAYS checked (one sparse product
 * and zkg16_r1cs_check's kernel over the k assignments): if any assignment fails the call returns ZKG16_ERR_UNSATISFIED, writes
 * nothing, and zkg16_last_check names the requests — where the key route would emit a proof no verifier accepts.
 * One trapdoor per call: the batch form is k assignments of one system under one key, the single form is the batch form with k = 1.
 * Per call: the QAP evaluation once (zkg16_setup's first stage), per pass of at most 65,535 requests (option "trapdoor_pass") the
 * check and one kernel for the four dot products, then the O(1) tail per request on the host and num_instance + 3 k + 7 fixed-base
 * points (one G1 and one G2 pass).  Outputs are written only when every pass has succeeded.  The call takes one lane.
 * timings_ms (nullable, 5): QAP evaluation, sparse product + check, dot kernel, fixed-base passes (device events), whole call (host).
 * Checked before any device work, outputs untouched: null pointers or k == 0 (ZKG16_ERR_BAD_ARG), unknown handles
 * (ZKG16_ERR_BAD_HANDLE), a prime template handle (ZKG16_ERR_UNSUPPORTED: no request's system, as in zkg16_r1cs_check), a witness
 * whose length is not the system's num_variables, a zero trapdoor entry (zkg16_setup refuses those too) or a tau with tau^N = 1
 * (ZKG16_ERR_BAD_ARG; zkg16_last_error says which entry).
 * zkg16_prove_trapdoor_host: no ctx, no GPU, up to `threads` host threads (0 = 8) — the reference for every byte of the device
 * forms.  Arrays as for zkg16_r1cs_check_host, z: k x num_variables x 4.  L_j(tau) = (Z(tau) / N) omega^j / (tau - omega^j) with a
 * batch inversion, column sums by a plain loop, the check is zkg16_r1cs_check_host's, points by the host scalar multiplication.  Its
 * refusals' text: zkg16_last_error(NULL). */
ZKG16_API int zkg16_prove_trapdoor(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, const uint64_t trapdoor[20],
                         const uint64_t g1_gen[12], const uint64_t g2_gen[24], const uint64_t r[4], const uint64_t s[4],
                         uint64_t proof_out[48], uint8_t inf_out[3],
                         uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                         uint64_t *gamma_abc_g1 /* num_instance x 12 */, float *timings_ms /* nullable, 5 */);
ZKG16_API int zkg16_prove_trapdoor_batch(zkg16_ctx *ctx, uint64_t r1cs_handle, const uint64_t *witness_handles, size_t k,
                               const uint64_t trapdoor[20], const uint64_t g1_gen[12], const uint64_t g2_gen[24],
                               const uint64_t *r /* k x 4 */, const uint64_t *s /* k x 4 */,
                               uint64_t *proofs_out /* k x 48 */, uint8_t *inf_out /* k x 3 */,
                               uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                               uint64_t *gamma_abc_g1 /* num_instance x 12 */, float *timings_ms /* nullable, 5 */);
ZKG16_API int zkg16_prove_trapdoor_host(const uint64_t *const row_ptr[3], const uint32_t *const col[3], const uint64_t *const coeff[3],
                              size_t num_instance, size_t num_constraints, size_t num_variables,
                              const uint64_t *z /* k x num_variables x 4 */, size_t k,
                              const uint64_t trapdoor[20], const uint64_t g1_gen[12], const uint64_t g2_gen[24],
                              const uint64_t *r /* k x 4 */, const uint64_t *s /* k x 4 */, int threads,
                              uint64_t *proofs_out /* k x 48 */, uint8_t *inf_out /* k x 3 */,
                              uint64_t alpha_g1[12], uint64_t beta_g2[24], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                              uint64_t *gamma_abc_g1 /* num_instance x 12 */);
/* native Poseidon sponge hash of n Fr elements (Montgomery) — the public inputs hash_a/b/c of the matrix handler */
ZKG16_API int zkg16_poseidon_hash(const uint64_t *elems, size_t n, uint64_t out[4]);
/* k hashes in one call.  elems: k vectors of n Fr each (Montgomery), back to back; out[4 i ..] is byte for byte
 * zkg16_poseidon_hash(elems + 4 n i, n).  _host (no ctx, no GPU): on the pool of zkg16_matrix_sponge_states_batch (threads: 0 = 8, capped at
 * 16 and at k).  The ctx form takes a lane; with at least option "sponge_chains_min" chains (k) a kernel walks them, one GPU lane per
 * chain, else it answers with the host form on "matrix_batch_threads" threads.  zkg16_matrix_hash_batch[_host]: the reference's
 * hash_matrix endpoint for k matrices m of n^2 u64 each: hashes[4 i ..] = hash_a of zkg16_matrix_sponge_states(n, m_i, .) — the value
 * a verifier needs as a public input.  k == 0, n == 0, null pointers, threads < 0 and, for the matrix forms, n outside 2..1024:
 * ZKG16_ERR_BAD_ARG before any work; on any error the output is untouched. */
ZKG16_API int zkg16_poseidon_hash_batch_host(const uint64_t *elems, size_t n, size_t k, int threads, uint64_t *out);
ZKG16_API int zkg16_poseidon_hash_batch(zkg16_ctx *ctx, const uint64_t *elems, size_t n, size_t k, uint64_t *out);
ZKG16_API int zkg16_matrix_hash_batch_host(size_t n, const uint64_t *m, size_t k, int threads, uint64_t *hashes);
ZKG16_API int zkg16_matrix_hash_batch(zkg16_ctx *ctx, size_t n, const uint64_t *m, size_t k, uint64_t *hashes);

/* ---- stage entry points (tests / bench; host buffers) ----------------------------------------- */
/* ark-poly Radix2EvaluationDomain<Fr>: in-place, natural order; inverse => ifft (incl. 1/N);
 * coset => offset g = 7 (coset_fft = g^i then fft; coset_ifft = ifft then g^-i). */
ZKG16_API int zkg16_ntt(zkg16_ctx *ctx, uint64_t *data, size_t log_n, int inverse, int coset);
/* ark-ec VariableBaseMSM::msm_bigint: sum scalars[i] * bases[i]; result affine. */
ZKG16_API int zkg16_msm_g1(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical,
                 size_t n, uint64_t out_affine[12], uint8_t *out_inf);
ZKG16_API int zkg16_msm_g2(zkg16_ctx *ctx, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical,
                 size_t n, uint64_t out_affine[24], uint8_t *out_inf);
/* LibsnarkReduction::witness_map_from_matrices: h (N x 4 limbs, Montgomery), N = 2^log_n. */
ZKG16_API int zkg16_witness_map(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, uint64_t *h_out, size_t *log_n_out);
/* ark-ec FixedBase::msm: out[i] = [scalars[i]] base (used by the known-trapdoor setup in tests/bench). */
ZKG16_API int zkg16_fixed_base_g1(zkg16_ctx *ctx, const uint64_t base[12], const uint64_t *scalars_canonical, size_t n,
                        uint64_t *out_affine /* n x 12 */, uint8_t *out_inf /* n */);
ZKG16_API int zkg16_fixed_base_g2(zkg16_ctx *ctx, const uint64_t base[24], const uint64_t *scalars_canonical, size_t n,
                        uint64_t *out_affine /* n x 24 */, uint8_t *out_inf /* n */);
/* One scalar multiplication on the host (no ctx, no GPU): [k] base, k canonical.  What a caller uses to derive its own
 * generators (upstream: `E::G1::rand`), where a device pass would be all latency. */
ZKG16_API int zkg16_scalar_mul_g1(const uint64_t base[12], const uint64_t k_canonical[4], uint64_t out_affine[12], uint8_t *out_inf);
ZKG16_API int zkg16_scalar_mul_g2(const uint64_t base[24], const uint64_t k_canonical[4], uint64_t out_affine[24], uint8_t *out_inf);

/* ---- device-resident stage benches (inputs uploaded once, op repeated on device) ---------------- */
ZKG16_API int zkg16_bench_ntt(zkg16_ctx *ctx, size_t log_n, int inverse, int coset, int iters, float *ms_per_iter);
ZKG16_API int zkg16_bench_witness_map(zkg16_ctx *ctx, uint64_t r1cs_handle, uint64_t witness_handle, int iters, float *ms_per_iter);
ZKG16_API int zkg16_bench_msm(zkg16_ctx *ctx, int group /*1|2*/, const uint64_t *bases, const uint8_t *inf,
                    const uint64_t *scalars_canonical, size_t n, int iters, float *ms_per_iter,
                    uint64_t *out_affine, uint8_t *out_inf);

/* ---- instrumentation --------------------------------------------------------------------------- */
/* Times of the last prove on this ctx, in ms (returns the number of entries written, up to 22):
 * [0] unused, [1] witness map (device; upstream span "R1CS to QAP witness map"), [2] scalar digits + bucket scatter of both scalar
 * vectors (device), [3..7] host-observed completion gaps of H, L, A, B1, B2 in collection order (NOT a breakdown: the first gap
 * holds most of the device time), [8] host tail ("Finish C"), [9] total wall;
 * [10..14] device time of the bucket accumulation + fix-ups of H, L, A, B1, B2 and [15..19] of their bucket reductions, from event
 * pairs on the streams they ran on: upstream's "Compute C" = H + L, "Compute A", "Compute B in G1", "Compute B in G2"
 * (ark-groth16 prover.rs).  MSMs overlap each other and the witness map, so the device times sum to more than [9];
 * [20] host time of combining H's window sums (after the proof's last device event), [21] of the other four MSMs' (under H's device work). */
ZKG16_API int zkg16_last_timings(zkg16_ctx *ctx, float *ms, int cap);
/* Lengths of the sorted (scalar, window) term lists of the last proof on this ctx = mixed additions of each MSM that walks the list:
 * [0] the z list (A and L), [1] the B list (B1 and B2; 0 = they used the z list), [2] the h list.  Synchronises the ctx. */
ZKG16_API int zkg16_last_term_counts(zkg16_ctx *ctx, uint64_t counts[3]);
/* G1 accumulation waves per SIMD (2 or 4) the last proof's term lists ran at: [0] z list, [1] B list, [2] h list; 0 = not built. */
ZKG16_API int zkg16_last_acc_waves(zkg16_ctx *ctx, int waves[3]);
/* Waves of the bucket-accumulation kernels one SIMD holds at once (their register use decides): [0] G1, [1] G2.  The grid of an
 * accumulation may be sized for more waves per SIMD than that (zkg16_last_acc_waves): the extra ones run as a second round. */
ZKG16_API int zkg16_acc_resident_waves(zkg16_ctx *ctx, int waves[2]);
/* What the last zkg16_msm_g1 / zkg16_msm_g2 / zkg16_bench_msm / zkg16_diag_msm_tabled / zkg16_diag_msm_rounds call on this ctx ran as (diagnostics for tests):
 * out = { c, nwin, entries, seg_len, fixup_items, fixup_chains, bit_sliced, two_level_k }.  c: window bits; nwin: windows;
 * entries: length of the sorted (scalar, window) term list; seg_len: entries per lane the accumulation kernel read; fixup_items /
 * fixup_chains: work items queued for spilled buckets longer than four segments (one per 1024 segments), and how many of those
 * buckets needed more than one item; bit_sliced: weight bits of the bit-sliced bucket reduction, 0 = another form ran;
 * two_level_k: chunk size of the bit-sliced or the work-efficient reduction, 0 = the classic form ran.  Copies four words from the
 * device when called; the MSM and prove paths record nothing for it.  All zero before the first such call and again after a proof
 * that ran on the ctx's first lane (it takes over the workspace and slot the words live in); entries and what follows are zero
 * after a call with n = 0.  A null out: ZKG16_ERR_BAD_ARG. */
ZKG16_API int zkg16_last_msm_state(zkg16_ctx *ctx, uint32_t out[8]);
/* The bucket scatter alone on raw digit codes (diagnostics for tests): codes[nwin][n] in the digit kernel's format, (|d| - 1) << 1 |
 * negate with |d| - 1 < 2^(c-1), or ~0 for digit 0.  Runs the scatter the MSM plans run, in a workspace of its own (the ctx's term
 * lists, slots and zkg16_last_msm_state are left as they were), and copies out: entries_xy = the sorted list as (x, y) pairs of 32-bit
 * words, x = position << 1 | negate, y = window * 2^(c-1) + bucket (room for nwin * n pairs; *length are written); win_totals[nwin] =
 * entries per window — for more than 32 windows the differences of the scatter's own window prefix; *length = the list's length as
 * the device summed it.  n == 0: *length = 0, win_totals zero, ZKG16_OK.  c - 1 > 24 or n >= 2^31: the scatter refuses
 * (ZKG16_ERR_HIP, zkg16_last_error names the limit).  nwin < 1, c < 2, nwin * n >= 2^31 or a null pointer: ZKG16_ERR_BAD_ARG.
 * Synchronises the ctx's stream; on any error no output is written. */
ZKG16_API int zkg16_diag_bucket_sort(zkg16_ctx *ctx, const uint32_t *codes, size_t n, int nwin, int c, uint32_t *entries_xy,
                                     uint32_t *win_totals, uint64_t *length);
/* The sorted term list of batch vectors of n canonical scalars (scalars[batch][n][4]) as the proofs build it (diagnostics for tests):
 * digits, scatter (or the rocPRIM sort under option "sort_mode" 1) and bucket offsets, in workspaces of its own.  window_bits and
 * tabled go to the plan as they are (a tabled plan takes up to 24 bits; a width the plan does not take = chosen by size).  mask_mode
 * 0: no mask; 1: scalars i with mask[i] != 0 count as zero in the digit kernel; 2: the full list, then the stable compaction that
 * drops their terms (what B1 / B2 of a key with window tables use).  plan_out = { c, windows of the list, digits per scalar,
 * total buckets tb }; entries_xy = the first offsets[tb] entries (x = position << 1 | negate, position = i on a plain key and
 * digit * n + i with tables; y = global bucket id), at most entries_cap pairs; offsets = the tb + 1 bucket boundaries, at most
 * offsets_cap words; *length = offsets[tb].  n == 0: plan_out only, *length = 0.  A buffer too small for the plan, batch < 1, a
 * mask_mode outside 0..2, mask_mode != 0 without a mask or a null pointer: ZKG16_ERR_BAD_ARG.  Synchronises the ctx's stream; on any
 * error no output is written. */
ZKG16_API int zkg16_diag_term_list(zkg16_ctx *ctx, const uint64_t *scalars_canonical, size_t n, int batch, int window_bits, int tabled,
                                   const uint8_t *mask, int mask_mode, uint32_t plan_out[4], uint32_t *entries_xy, size_t entries_cap,
                                   uint32_t *offsets, size_t offsets_cap, uint64_t *length);
/* One MSM on window tables, run as a proof runs one query of a key that carries them (diagnostics for tests).  group: 1 = G1, 2 = G2;
 * bases[n] with their infinity mask (nullable) as zkg16_msm_g1 takes them; scalars[batch][n][4] canonical; window_bits 2..24, taken as
 * they are; stride_mode 1 = packed table entries, 2 = padded to whole cache lines (zkg16_table_layout); last_of_proof 0 | 1 = what the
 * proof sets for the MSM whose reduction is its tail.  Builds the table [254 / c + 1][n] with the routine zkg16_pk_precompute calls,
 * the tabled term list of the batch (vector v = window v of one plan) in the workspace of zkg16_msm_g1, accumulates and reduces on
 * that entry's slot and combines every vector's window on the host: out_affine[batch][12 | 24], out_inf[batch].  table_out /
 * table_inf (both or neither): the table, read at its stride and converted to the ABI's form, table_out[levels][n][12 | 24] and
 * table_inf[levels][n].  zkg16_last_msm_state reports this call, nwin reading as batch.  n == 0: every output is the point at
 * infinity, no table is written, the state is { c, batch, 0, ... }.  A null pointer (inf excepted), one table pointer without the
 * other, a group outside 1..2, batch < 1, window_bits outside 2..24, a stride_mode outside 1..2, last_of_proof outside 0..1 or
 * batch * 2^(c-1) >= 2^32: ZKG16_ERR_BAD_ARG.  batch * n * (254 / c + 1) >= 2^31: refused as the plan refuses it (ZKG16_ERR_HIP), before
 * anything is read.  Synchronises the ctx's stream; on any error no output is written. */
ZKG16_API int zkg16_diag_msm_tabled(zkg16_ctx *ctx, int group, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical,
                                    size_t n, int batch, int window_bits, int stride_mode, int last_of_proof, uint64_t *out_affine,
                                    uint8_t *out_inf, uint64_t *table_out, uint8_t *table_inf);
/* One MSM on a plain key fed in rounds, run as a proof on a streamed assignment (zkg16_prove_matrix) runs one z-side query (diagnostics
 * for tests).  group, bases, inf and scalars[n][4] as zkg16_diag_msm_tabled takes them, one vector; part_of[n]: the part each scalar
 * belongs to; parts 1..255; window_bits 2..20, taken as they are.  For k = 0 .. parts - 1: the term list of the scalars with part_of[i]
 * == k (the others count as zero) in the workspace of zkg16_msm_g1, accumulated as round k on that entry's slot — round 0 into the
 * MSM's bucket array, every later round into a second one, its fix-ups, then the bucket-wise sum of the two — and round_entries_out[k]
 * = the length of that round's list.  Then one reduction and one collection: out_affine[12 | 24], *out_inf.  A scalar whose label is
 * parts or more takes part in no round.  zkg16_last_msm_state reports the last round.  n == 0: the point at infinity, every count
 * zero.  A null pointer (inf excepted), a group outside 1..2, parts outside 1..255 or window_bits outside 2..20: ZKG16_ERR_BAD_ARG.
 * n * (254 / c + 1) >= 2^31: refused as the plan refuses it (ZKG16_ERR_HIP), before anything is read.  Synchronises the ctx's stream;
 * on any error no output is written. */
ZKG16_API int zkg16_diag_msm_rounds(zkg16_ctx *ctx, int group, const uint64_t *bases, const uint8_t *inf, const uint64_t *scalars_canonical,
                                    size_t n, const uint8_t *part_of, int parts, int window_bits, uint64_t *out_affine, uint8_t *out_inf,
                                    uint32_t *round_entries_out /* parts */);
/* Which sparse product an r1cs handle's witness maps run (diagnostics; takes the handle's own lock, launches nothing):
 * out = { dict_state, ndict, perm_ok, spmv_uses }.  dict_state: 0 = the coefficient dictionary has not been tried yet (the handle
 * has run fewer than two witness maps: plain kernel, rows in natural order), 1 = the dictionary is in use (ndict distinct
 * coefficients, 1..1024; 16-bit indices), 2 = this handle keeps the plain kernel (more than 1024 distinct coefficients, or fewer
 * than 4096 non-zeros; ndict = 0).  perm_ok: 1 = the rows are walked in length-class order (built with the dictionary, from 4096
 * constraints on; either kernel uses it).  spmv_uses: witness maps counted on the handle until the structures were built.  A null
 * out or an unknown handle: ZKG16_ERR_BAD_ARG, out untouched. */
ZKG16_API int zkg16_r1cs_spmv_state(zkg16_ctx *ctx, uint64_t r1cs_handle, uint32_t out[4]);
/* The lanes of the most recent proofs: rows of (lane, start ms, end ms) on the host's steady clock, oldest first; returns the number of
 * rows written (<= cap_rows).  Two rows with different lanes and intersecting intervals = two proofs in flight at once. */
ZKG16_API int zkg16_lane_log(zkg16_ctx *ctx, double *rows, int cap_rows);
/* Live HIP-event timing of individual kernels (bench.py's roofline leg).  enable: 0 off, 1 every kernel family, 2 only the
 * bucket-accumulation launches (five event pairs per proof instead of ~60).  stats are accumulated per kernel name since
 * the last reset. */
ZKG16_API int zkg16_kernel_timing(zkg16_ctx *ctx, int enable);
ZKG16_API int zkg16_kernel_stats(zkg16_ctx *ctx, const char *kernel_name, uint64_t *launches, double *total_ms,
                       double *units /* kernel-specific work units, e.g. bucket additions */);
ZKG16_API void zkg16_kernel_stats_reset(zkg16_ctx *ctx);
/* Tuning / A-B switches; none of them changes a result (tests/test_gpu_parity.py toggles every one and compares proofs).
 *   "window_bits"    MSM window bits c for every plan (0 = by size: 13 / 15 / 16 / 17; <= 20)      "window_bits_h"  the H MSM's plan only
 *   "reduce_chunk"   buckets per lane in the bucket reduction (0 = 8)                   "reduce_mode"    1 = work-efficient two-level form,
 *                    2 = that form except for the proof's last MSM, 4 = classic everywhere, 5 = bit-sliced wherever it applies,
 *                    6 = the default without the bit-sliced form, 0 = default (bit-sliced for bucket sets up to 2^19, else 2 from 16-bit windows on)
 *   "sort_mode"      0 = hand-written wave-ballot bucket scatter (default), 1 = rocPRIM radix sort
 *   "acc_pipeline"   bit 0 / 1: G1 / G2 accumulation gathers the next base behind the last (inlined) product; 4 = off, 0 = default (both)
 *   "wm_concurrent"  0 = witness map in order on the main stream (default: own stream)  "fixup_aux"      1 = fix-ups on the reduction stream
 *   "g1_waves"       G1 accumulation waves per SIMD in the resident round (0 = 2)       "min_seg"        shortest per-lane run (0 = adaptive)
 *   "ntt_mode"       0 = saturated-limb butterflies (first version), 1 = unsaturated (default), 3 = unsaturated, but 2^23 and
 *                    2^24 by three passes over 2048-point tiles instead of two over 4096-point tiles
 *   "ntt_radix"      1 (default; also 0) = the last seven butterfly stages of a tile by lane exchanges, 3 = the top seven as well,
 *                    2 = every stage through the LDS, 4 = two stages per LDS trip
 *   "fuse_pointwise" 1 (default) = the point-wise product fused into the load of the witness map's last transform, 0 = its own pass
 *   "wm_transforms"  6 (default; also 0) = the witness map's C only inverse-transformed and subtracted on the last transform's store,
 *                    7 = arkworks' seven transforms (C to the coset and back)
 *   "collect_threads" host combination of the z-side MSMs' window sums: 0 = own threads for plain keys, 1 = always, 2 = never
 *   "fixed_base_bits" window width of the setup's fixed-base multiplications (0 = by batch size; 16 / 18 / 20 = two-level tables)
 *   "g2_lazy"        G2 accumulation's Fq2 products: 0 / 1 (default) two fused two-product reductions with operands parked in LDS, 2 = Karatsuba
 *   "g2_split"       G2 accumulation: 1 (default) = every Fq2 value split over a pair of lanes, two waves per SIMD; 0 = one lane per point
 *                    (same proofs byte for byte; "acc_pipeline" bit 1, "g2_lazy" = 2 and "acc_debug" keep their one-lane loops)
 *   "g2_split_form"  the split loop's field products: 0 / 2 (default) = inlined, 1 = device-function calls
 *   "g1_inline"      G1 accumulation (plain loop): 0 / 1 (default) every field product inlined, no call; 2 = products as device-function calls
 *   "acc_lazy"       the default G1 / G2 accumulation loops: 1 (default) = mixed additions without the carry passes their results do not
 *                    need, 0 = the earlier additions (same sums; for A/B runs)
 *   "table_stride"   entry layout of the window tables zkg16_pk_precompute builds from now on (zkg16_table_layout): 0 (default) = padded to
 *                    whole cache lines for tables of at least 256 MiB, packed below; 1 = packed; 2 = padded.  An existing table keeps its layout
 *   "lanes"          proofs this ctx runs at a time (1..8, default 2): see the note on re-entrancy at the top
 *   "matrix_parts"   zkg16_prove_matrix: slices of the host sponges the proof is fed in (0 = five growing slices, k = k equal ones; 1 = assignment first, then the proof)
 *   "matrix_slice_min" zkg16_prove_matrix: the slice count is lowered until a slice holds at least this many permutations (0 = the default,
 *                    512; else 1..2^20; at least 1 keeps every slice non-empty).  zkg16_matrix_stream_bounds gives the slices of a size
 *   "batch_max"      zkg16_prove_batch / zkg16_prove_matrix_batch: proofs per device pass (0 = as many as fit, else 1..65535)
 *   "matrix_batch_threads" zkg16_witness_matrix_batch / zkg16_prove_matrix_batch: host threads of the sponge chains (0 = 8, else 1..16)
 *   "matrix_batch_grid" cap on either grid dimension of the batched witness kernels (0 = 65535, else 1..65535): beyond it they loop
 *   "linear_solver"  zkg16_witness_linear_batch / zkg16_prove_linear_batch: 0 (default) = the reference's forward substitution on the lower
 *                    triangle of a, 1 = Gaussian elimination with row pivoting (see the linear-equations route above).  The default is 0
 *                    because 0 is what the reference computes, unsatisfied assignments for dense a included
 *   "linear_elim_lds_max" wit_linear_elim_kernel: the largest n whose working matrix lies in LDS (0 = the default, 64; else 1..64); above it
 *                    the matrix lies in a global workspace
 *   "sponge_chains_min" zkg16_witness_matrix_batch / zkg16_prove_matrix_batch (3K chains per call or sub-batch) and zkg16_poseidon_hash_batch /
 *                    zkg16_matrix_hash_batch (k chains): calls with at least this many Poseidon sponge chains walk them on the device, one
 *                    GPU lane per chain (the S-box values written as it goes, the hashes read back once; timings_ms[0] = 0); fewer run on
 *                    the host pool.  1 = always the device, any value above 2^32 = never, 0 = the default, which is NEVER:
 *                    measured (profiles/sponge_chains_timing.txt; t_perm = 0.714 ms per permutation of a lone wave) the device
 *                    beat 8 host threads in zkg16_witness_matrix_batch from 3072 chains (K = 1024: 3.7x at n = 8, 16 and 32) and in
 *                    zkg16_matrix_hash_batch from 1024 chains (1.3x; 5.2x at 4096), but in zkg16_prove_matrix_batch, whose chain count is that
 *                    of a sub-batch, only at n = 8 and by 6 %, and it lost at n = 32 by 1.4x.  The default must win on every entry at
 *                    every measured size; none does.  Callers of the first two entries with that many chains set 3072
 *   "check_satisfied" 0 (default) = the proving calls prove whatever they are handed; 1 = they check their assignments on the device
 *                    and return ZKG16_ERR_UNSATISFIED, writing nothing, when one fails (zkg16_r1cs_check above; zkg16_last_check); any
 *                    other value: ZKG16_ERR_BAD_ARG.  The one option that can change what a call returns — for assignments no verifier accepts
 *   "pk_validate"    0 (default) = zkg16_pk_load / zkg16_pk_load_range copy the key they are handed; 1 = they run zkg16_pk_check on the
 *                    uploaded key before the handle exists: a key with a bad point returns ZKG16_ERR_BAD_ARG, *pk_handle is not
 *                    written, the key's device buffers are released and zkg16_last_error names the query and the index
 *                    (e.g. "h_query[63]") or the single point; any other value: ZKG16_ERR_BAD_ARG
 *   "sponge_chain_segment" permutations of a chain per launch of the chain kernel (0 = 256, else 1..65535): the state is carried between launches
 *   "rerandomize_min" zkg16_rerandomize_batch[_wire]: shorter batches are answered by the host form (1 = always the device, 0 restores
 *                    the default).  Default 256: the smallest measured K at which both device forms beat the host form on eight
 *                    threads in every round, 0.092 (limbs) and 0.109 (wire) against 0.163 ms per proof; at K = 64 they lost, 0.367 and
 *                    0.432 against 0.168: a device call costs 24 to 28 ms whatever K is (profiles/rerandomize_timing.txt)
 *   "rerandomize_pass" zkg16_rerandomize_batch[_wire]: proofs per kernel launch (0 = 65,536, else 1..65,536; tests lower it to run
 *                    several passes at small k)
 *   "trapdoor_pass"  zkg16_prove_trapdoor_batch: requests per device pass (0 = 65,535, else 1..65,535; tests lower it to run several
 *                    passes at small k)
 *   "pk_bytes_piece" zkg16_pk_load_bytes / zkg16_pk_save / zkg16_pk_read: points per piece of a query (0 = 524,288, else 1..524,288).
 *                    Each query is cut into pieces on its own; two pieces are in flight, so the default keeps the staging beside
 *                    the key at 96 MiB of HBM (two pieces of G2 bytes), under 256 MiB.  Tests lower it to reach several pieces at small keys
 * Unknown names return ZKG16_ERR_UNSUPPORTED. */
ZKG16_API int zkg16_set_option(zkg16_ctx *ctx, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* ZKG16_H */
