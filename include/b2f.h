/*
 * b2f.h -- C ABI of the MI355X (gfx950) BLAKE2f Table16 witness-fill and constraint-eval
 * engine. Plain pointers and sizes only; no torch or HIP types in the signatures
 * (`stream` is an opaque hipStream_t, NULL = the default stream).
 *
 * Drop-in point: the reference's gadget boundary `Blake2fInstructions<F>`
 * (blake2f-circuit/src/blake2f.rs:40-72), implemented by `Table16Chip`
 * (blake2f-circuit/src/blake2f/table16.rs:338-384), whose region drivers
 * `CompressionConfig::{initialize_with_iv, initialize_with_state, compress, digest}`
 * (table16/compression.rs:1078-1149) assign the trace cell by cell; and the batch entry the
 * reference sketches, `Blake2fChip::construct(config, Vec<Blake2fWitness>)` +
 * `chip.load(&mut layouter)` checked by `MockProver::run(k, ..).verify()`
 * (blake2f.rs:250-303, commented out there). One b2f_fill call assigns every region of a
 * batch of independent compressions; one b2f_eval call is the MockProver check of the
 * resulting trace. The trace contract is docs/LAYOUT.md (LAYOUT v1).
 *
 * Threading: one context per device, externally synchronized, and used on ONE stream at a
 * time: a context owns per-call scratch (half-round states, tile index, lookup scratch) that
 * every stream-ordered call reuses, so two `*_dev` calls of one context in flight on two
 * streams race on it. Use one context per concurrent stream. `*_dev` calls are
 * stream-ordered and asynchronous; b2f_sync() waits and returns any device-side error raised
 * since the previous b2f_sync (errors are sticky until then). Host-pointer calls block.
 * Everything a context owns -- scratch, the cached domain tables, the pinned staging blocks, the
 * status words -- is ordered by the stream its calls were issued on and by nothing else: the
 * library never orders one caller stream behind another, and a stream created non-blocking is
 * not ordered behind the null stream either. To move a context from stream A to stream B, call
 * b2f_sync(ctx, A) after the last call on A and before the first call on B (any other wait for
 * A's completion serves, but only b2f_sync collects A's errors); the cached tables and warm
 * scratch are then used on B as they are. b2f_sync takes the stream the calls were issued on:
 * it waits for that stream alone, then reads and clears the error word from the host, so no
 * call of the context may be in flight on any stream while it runs. A call may block the host
 * where its comment says so: when a context-owned block has to grow (it waits for `stream`
 * first), and until the previous call's staged upload has run (the permutation and the
 * evaluation / opening calls stage their host arrays in one pinned block each). No
 * call aborts; errors come back as B2F_* status codes with a message in b2f_last_error().
 * They map onto halo2's plonk::Error at a Rust call site: B2F_ERR_ROWS ->
 * NotEnoughRowsAvailable, the others -> Synthesis.
 */
#ifndef B2F_H
#define B2F_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B2F_API __attribute__((visibility("default")))

#define B2F_NUM_ADVICE 10      /* a_0..a_9, table16.rs:281-309 */
#define B2F_NUM_GATES 16       /* selector bits, docs/LAYOUT.md §4 */
#define B2F_CODE_LOOKUP 16
#define B2F_CODE_COPY 17
#define B2F_CODE_FIXED 18   /* fixed-column cell differs from the keygen structure */
#define B2F_CODE_LAYOUT 19  /* the row map was rejected: nothing was checked */
#define B2F_CODE_CHECK 20   /* an internal cross-check failed (B2F_ERR_CHECK, a library defect):
                               the verdict is not trustworthy, whatever the witness */
#define B2F_MAX_ROUNDS (1u << 20)

/* Status codes */
#define B2F_OK 0
#define B2F_ERR_ARG 1       /* null pointer, misaligned buffer, total_rows % 4 != 0 */
#define B2F_ERR_ROUNDS 2    /* rounds > B2F_MAX_ROUNDS */
#define B2F_ERR_ROWS 3      /* buffers hold fewer rows than the batch needs */
#define B2F_ERR_HIP 4       /* HIP runtime error */
#define B2F_ERR_LAYOUT 5    /* offsets are not the prefix sums of R(rounds_i) */
#define B2F_ERR_INPUT 6     /* malformed EIP-152 input (length != 213 or f not 0/1) */
#define B2F_ERR_FIELD 7     /* (at b2f_sync) a grand product's denominator product is zero: a
                               challenge collides with a cell value, its z column is meaningless;
                               or an NTT's or a quotient call's omega is not a primitive
                               root of unity of its domain; or the vanishing divide met X^n = 1 */
#define B2F_ERR_CHECK 8     /* (at b2f_sync) an internal cross-check failed -- a library defect:
                               the lookup's permuted columns do not multiply to the product of
                               its input columns (its columns are wrong), or the fused pass's
                               long-instance segment list overflowed (its verdict reads unclean) */

/* One EIP-152 compression: the reference's Blake2fWitness{rounds, h, m, t, f}
 * (blake2f.rs:208-239), 216 bytes, naturally aligned. f must be 0 or 1. */
typedef struct {
    uint64_t h[8];
    uint64_t m[16];
    uint64_t t[2];
    uint32_t rounds;
    uint32_t f;
} b2f_input;

/* MockProver-equivalent verdict (docs/LAYOUT.md §6). first_failure = min over all failures
 * of (row << 8) | code (code = selector bit 0..15, B2F_CODE_LOOKUP, B2F_CODE_COPY,
 * B2F_CODE_FIXED), UINT64_MAX when every constraint holds.
 * fixed_failures: rows whose fixed cell (selector mask | k_0 << 16) differs from the one the
 * keygen structure of the row map puts there (b2f_fill_fixed_dev): halo2 fixes selectors and
 * constants at keygen, so a trace checked under a caller-altered fixed column is rejected even
 * when its advice is consistent with the altered selectors.
 * A rejected row map (B2F_ERR_LAYOUT) leaves rows_checked = 0 and first_failure =
 * B2F_CODE_LAYOUT: the report never reads clean for a batch that was not checked. A failed
 * internal cross-check (B2F_ERR_CHECK) does the same with B2F_CODE_CHECK, so a library defect
 * never reads as a witness layout failure. */
typedef struct {
    uint64_t gate_failures[B2F_NUM_GATES];
    uint64_t lookup_failures;
    uint64_t copy_failures;
    uint64_t first_failure;
    uint64_t rows_checked;
    uint64_t fixed_failures;
} b2f_eval_report;

typedef struct b2f_ctx b2f_ctx;

B2F_API int b2f_version(void);

/* Rows of one instance, R(rounds) = 228 + 416*rounds (LAYOUT.md §5). Replaces the SHA row
 * map of compression_util.rs:32-205. Returns 0 when rounds > B2F_MAX_ROUNDS. */
B2F_API uint64_t b2f_layout_rows(uint32_t rounds);

/* offsets[0..n]: row offset of every instance region, i.e. where each `assign_region` of
 * compression.rs:1084/1120/1140 lands in the batch. Host function. */
B2F_API int b2f_layout_offsets(const b2f_input* in, size_t n, uint64_t* offsets);

/* halo2 advice-column index of a_i in the reference's allocation order
 * (table16.rs:281-294: a_5, a_3, a_4, a_6, a_7, a_8, a_9, a_0, a_1, a_2); -1 if i > 9. */
B2F_API int b2f_halo2_column_index(int a_i);

/* Parse one 213-byte EIP-152 precompile input (rounds u32 BE | h 64 B | m 128 B | t 16 B |
 * f 1 B; words little-endian), the format of the reference KAT (blake2f.rs:193-247). */
B2F_API int b2f_parse_eip152(const uint8_t* raw, size_t len, b2f_input* out);

/* Context bound to one HIP device (owns scratch, events, the device status words). */
B2F_API b2f_ctx* b2f_create(int device);
B2F_API void b2f_destroy(b2f_ctx* ctx);
B2F_API const char* b2f_last_error(const b2f_ctx* ctx);

/* Witness fill, device pointers. Replaces CompressionConfig::{initialize_with_iv,
 * compress, digest} (compression.rs:1078-1149) with their helpers
 * (compression_util.rs:208-890, subregion_initial.rs:11-155, SpreadVar::with_lookup
 * spread_table.rs:257-285, AssignedBits::assign_bits table16.rs:136-167) for n instances.
 *   d_in        n records (16-B aligned)
 *   d_offsets   n+1 row offsets (b2f_layout_offsets)
 *   total_rows  rows of the buffers (>= offsets[n], multiple of 4); rows past offsets[n]
 *               are written as zeros
 *   d_advice    column-major uint32 [10][total_rows] (16-B aligned); cell a_c of row r at
 *               d_advice[c * total_rows + r]
 *   d_fixed     uint32 [total_rows]: selector mask (bits 0..15) | constant k_0 << 16
 *   d_h_out     n * 8 uint64 compression outputs h' (may be NULL)
 * Asynchronous on `stream`. */
B2F_API int b2f_fill_dev(b2f_ctx* ctx, const b2f_input* d_in, size_t n,
                         const uint64_t* d_offsets, uint64_t total_rows, uint32_t* d_advice,
                         uint32_t* d_fixed, uint64_t* d_h_out, void* stream);

/* Constraint evaluation over a trace, device pointers: the `MockProver::verify` of
 * blake2f.rs:301-302 -- every gate of compression.rs:604-1056 (as re-derived in
 * LAYOUT.md §4), the spread lookup of spread_table.rs:443-453 on every row, and every
 * copy constraint (`copy_advice`). d_report is overwritten. Asynchronous on `stream`. */
B2F_API int b2f_eval_dev(b2f_ctx* ctx, const uint32_t* d_advice, const uint32_t* d_fixed,
                         const uint64_t* d_offsets, size_t n, uint64_t total_rows,
                         b2f_eval_report* d_report, void* stream);

/* Fused witness fill + constraint evaluation, device pointers: the same trace, h' and
 * verdict as b2f_fill_dev followed by b2f_eval_dev on that trace (MockProver::run then
 * ::verify, blake2f.rs:301-302), in one pass: every cell is checked while it is still on the
 * CU, so the trace is written once and never read back. Arguments as b2f_fill_dev plus the
 * report (overwritten). Asynchronous on `stream`. */
B2F_API int b2f_fill_eval_dev(b2f_ctx* ctx, const b2f_input* d_in, size_t n,
                              const uint64_t* d_offsets, uint64_t total_rows, uint32_t* d_advice,
                              uint32_t* d_fixed, uint64_t* d_h_out, b2f_eval_report* d_report,
                              void* stream);

/* b2f_fill_eval_dev with flags; flags = 0 is that call. The fixed column (selector mask and
 * k_0) is a function of the row map alone -- keygen output, what b2f_fill_fixed_dev writes, no
 * witness in it -- so a prover that runs many witnesses of one circuit shape through the same
 * buffers need not write it again:
 *   B2F_FIXED_RESIDENT  the caller states that d_fixed already holds this row map's column,
 *                       written by an earlier fused call of `ctx` with the same d_fixed,
 *                       d_offsets, n and total_rows, and that nothing has written it (or the row
 *                       map) since. The call may then leave d_fixed unwritten: 40 instead of
 *                       44 bytes stored per row. Advice, h' and report are what the full call
 *                       gives; the fixed cells are still formed and checked on the CU.
 * The library honours the flag only where its own record agrees: the context's last full fused
 * write with the inject hook off (the call was issued without error, and no b2f_fill_dev,
 * b2f_fill_fixed_dev or failing b2f_sync of this context came after it) had exactly these four
 * arguments, and the hook is off. Otherwise the call silently runs in full and renews the record;
 * under the hook it runs in full and clears it. The record knows nothing of writes made outside
 * these calls: those are what the caller's statement covers. The diagnostics build ignores the
 * flag. Unknown flag bits: B2F_ERR_ARG. Timed as B2F_KERNEL_FILL_EVAL. */
#define B2F_FIXED_RESIDENT 1u
B2F_API int b2f_fill_eval_dev_ex(b2f_ctx* ctx, const b2f_input* d_in, size_t n,
                                 const uint64_t* d_offsets, uint64_t total_rows, uint32_t* d_advice,
                                 uint32_t* d_fixed, uint64_t* d_h_out, b2f_eval_report* d_report,
                                 uint32_t flags, void* stream);

/* Test hook: which kernel the last b2f_fill_eval_dev[_ex] call of `ctx` launched: *out = 0 the
 * full one (every column written), 1 the advice-only one (B2F_FIXED_RESIDENT honoured). Host
 * state only: no synchronize. */
B2F_API int b2f_debug_fused_path(b2f_ctx* ctx, uint32_t* out);

/* Test hook for the fused path: XOR `mask` into cell (row, col) as b2f_fill_eval_dev assigns
 * it (col 0..9 = a_col, 10 = the fixed column), so both the trace it writes and the trace it
 * checks carry the fault; row = UINT64_MAX turns it off (the default). Lets tests prove the
 * fused verdict equals b2f_eval_dev's / the oracle's on the trace actually written. */
B2F_API int b2f_debug_inject(b2f_ctx* ctx, uint64_t row, uint32_t col, uint32_t mask);

/* Test hook: which path the last b2f_eval_dev call of `ctx` took, after a device synchronize:
 * *out = 0 the fast clean-check pass found the trace clean (its report stands), 1 the pass
 * flagged something and the exact eval kernel wrote the report, 2 no fast pass ran (the exact
 * kernel alone). Lets tests prove a clean trace costs the fast pass only. */
B2F_API int b2f_debug_eval_path(b2f_ctx* ctx, uint32_t* out);

/* Diagnostics: eval-kernel phase cycle totals (s_memtime deltas summed over workgroups) of
 * the EVAL_CLOCK variant since the previous call; out[8 * wave + phase], phases:
 * stage+lookups, barrier 1, prefetch issue, G-table build, gate pass, copies, per-quad paths,
 * barrier 2. That variant exists only in the diagnostics build of this ABI (libb2f_diag.so,
 * selected there by B2F_DIAG_EVAL=23); the product library (libb2f.so) reads no environment,
 * launches only the full kernels and returns zeros here. Clears the totals. */
B2F_API int b2f_debug_clock(b2f_ctx* ctx, uint64_t* out);

/* Keygen structure (halo2 keygen_vk / keygen_pk over Value::unknown() witnesses,
 * benchmarking/src/blake2f_circuit_bench.rs:54-55; SURVEY.md §8(b) "Semantics to preserve"):
 * the fixed column of a batch from its row map alone, no witness -- selector masks and the
 * IV constants k_0 (LAYOUT.md §4/§5), zeros past offsets[n]. Equal to the d_fixed that
 * b2f_fill_dev writes for any witness of the same rounds. B2F_ERR_LAYOUT (at b2f_sync) for an
 * invalid row map. d_fixed 16-byte aligned, total_rows a multiple of 4. Asynchronous. */
B2F_API int b2f_fill_fixed_dev(b2f_ctx* ctx, const uint64_t* d_offsets, size_t n,
                               uint64_t total_rows, uint32_t* d_fixed, void* stream);

/* The copy constraints (equality pairs, `copy_advice` sites: table16.rs:431-433,
 * compression_util.rs:398-416,548-574) of one instance of `rounds` rounds, as keygen records
 * them: writes min(count, cap) quadruples (dst_row, dst_col, src_row, src_col), rows relative
 * to the instance, columns a_0..a_9 (b2f_halo2_column_index maps them to halo2's order), and
 * returns count = 24 + 576 * rounds + 96 (0 if rounds > B2F_MAX_ROUNDS). Host function. */
B2F_API uint64_t b2f_copy_constraints(uint32_t rounds, uint32_t* out4, uint64_t cap);

/* Wait for `stream` and return the first device-side error of the calls issued since the
 * previous b2f_sync (B2F_ERR_LAYOUT / B2F_ERR_ROUNDS from fill/eval, B2F_ERR_FIELD from the
 * lookup / permutation grand products, the root checks of the NTT and the quotient calls and the
 * vanishing divide), then clear it. */
B2F_API int b2f_sync(b2f_ctx* ctx, void* stream);

/* Host-pointer conveniences (allocate, copy, run, copy back; blocking). b2f_fill sizes the
 * trace to exactly offsets[n] rows; advice must hold 10*offsets[n] and fixed offsets[n]. */
B2F_API int b2f_fill(b2f_ctx* ctx, const b2f_input* in, size_t n, uint32_t* advice,
                     uint32_t* fixed, uint64_t* h_out);
B2F_API int b2f_eval(b2f_ctx* ctx, const uint32_t* advice, const uint32_t* fixed,
                     const uint64_t* offsets, size_t n, uint64_t total_rows,
                     b2f_eval_report* report);

/* Multi-block chaining (the reference gadget's Blake2f::update /
 * finalize, blake2f.rs:101-168): writes the b2f_input records of one block step for messages
 * 0 .. n-1 -- h from the previous step's outputs h' (d_h_prev, n x 8; the initial state for the
 * first block), the block's 16 message words (d_blocks, n x 16), the byte counter after the
 * block (d_t, n x 2), the final-block flag (d_f, n; non-zero = 1) and `rounds` (12 for
 * BLAKE2b). A host orders its messages by block count so that the messages still running at
 * a step are a prefix (b2f/hasher.py). Asynchronous on `stream`. */
B2F_API int b2f_chain_inputs_dev(b2f_ctx* ctx, const uint64_t* d_h_prev, const uint64_t* d_blocks,
                                 const uint64_t* d_t, const uint32_t* d_f, uint32_t rounds,
                                 size_t n, b2f_input* d_out, void* stream);

/* Fp export: advice cells as elements of the prover's scalar field,
 * the form halo2's prover keeps its advice columns in. Two fields:
 *   pallas::Base (pasta_curves 0.5.1 Fp, halo2_proofs 0.3.0's own field),
 *     p = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001;
 *   BN254 Fr (halo2curves 0.3.2 bn256::Fr, the field of the reference's circuit test and KZG
 *     bench: blake2f.rs:283,293, blake2f_circuit_bench.rs:10,34),
 *     r = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001.
 * Rows [row_begin, row_begin + nrows) of the ten advice columns are written in halo2 column
 * order (b2f_halo2_column_index): element of a_i at row row_begin + r goes to
 * d_out[(h * out_rows + r) * 4 + limb], h = b2f_halo2_column_index(i), 4 little-endian u64
 * limbs. out_rows >= nrows is the column stride (rows past nrows are not written; a prover
 * zero-fills to 2^k). `form`:
 *   B2F_FP_MONTGOMERY        x * 2^256 mod p (the in-memory Fp of pasta_curves)
 *   B2F_FP_CANONICAL         x as a 32-byte little-endian integer (PrimeField::to_repr)
 *   B2F_FP_BN254_MONTGOMERY  x * 2^256 mod r (the in-memory bn256::Fr of halo2curves)
 *   B2F_FP_BN254_CANONICAL   x as a 32-byte little-endian integer
 * (bit 1 selects the field, bit 0 Montgomery form). d_out must be 16-byte aligned.
 * Asynchronous on `stream`. */
#define B2F_FP_CANONICAL 0
#define B2F_FP_MONTGOMERY 1
#define B2F_FP_BN254_CANONICAL 2
#define B2F_FP_BN254_MONTGOMERY 3
B2F_API int b2f_export_fp_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                              uint64_t row_begin, uint64_t nrows, uint32_t form,
                              uint64_t* d_out, uint64_t out_rows, void* stream);

/* The fixed column as the prover's fixed columns (keygen data): the trace keeps the sixteen
 * selectors and k_0 packed in one u32 per row (mask | k_0 << 16, docs/LAYOUT.md §2); this writes
 * B2F_NUM_FIXED_FP = 17 field columns of rows [row_begin, row_begin + nrows) to
 * d_out[(c * out_rows + r) * 4 + limb]: c = 0..15 selector bit c as the field's 0 or 1, c = 16
 * k_0 = q >> 16. `form` is any B2F_FP_*; rows past nrows are not written; arguments, alignment
 * and errors as b2f_export_fp_dev (nrows < 2^38). One B2F_KERNEL_EXPORT region. Asynchronous. */
#define B2F_NUM_FIXED_FP 17
B2F_API int b2f_export_fixed_fp_dev(b2f_ctx* ctx, const uint32_t* d_fixed, uint64_t total_rows,
                                    uint64_t row_begin, uint64_t nrows, uint32_t form,
                                    uint64_t* d_out, uint64_t out_rows, void* stream);

/* The spread table as the prover's table columns (SpreadTableChip::load, spread_table.rs:470-508;
 * rows from SpreadTableConfig::generate, spread_table.rs:574-600): column c = 0 tag, 1 dense,
 * 2 spread, row x < 2^16 holds (tag(x), x, spread(x)), rows 2^16 .. usable_rows - 1 the
 * layouter's fill_from_row default (row 0's values: zero). Written to
 * d_out[(c * out_rows + row) * 4 + limb] in `form` (any B2F_FP_*), 2^16 <= usable_rows < 2^32,
 * out_rows >= usable_rows, d_out 16-byte aligned. Keygen data (halo2 fixes it in the proving
 * key); the lookup-columns call computes the compressed table internally. Asynchronous. */
B2F_API int b2f_spread_table_dev(b2f_ctx* ctx, uint64_t usable_rows, uint32_t form, uint64_t* d_out,
                                 uint64_t out_rows, void* stream);

/* Lookup-argument prover columns of the spread lookup
 * (spread_table.rs:443-453), as halo2_proofs 0.3.0's lookup prover builds them
 * (plonk/lookup/prover.rs: commit_permuted, permute_expression_pair, commit_product), for
 * n_circuits circuits cut from the trace: circuit c covers trace rows d_row_begin[c] ..
 * + usable_rows - 1 (rows past total_rows read as zero rows, i.e. table row 0), and the
 * table columns hold the 2^16 spread-table rows then the row-0 default up to usable_rows
 * (the layouter's fill_from_row). usable_rows = 2^k - blinding_factors - 1 is the caller's,
 * in [2^16, 2^31]. Challenges theta, beta, gamma: canonical field elements (4 LE u64 limbs).
 * Output, per circuit c and column j, d_out[((c * 5 + j) * out_rows + row) * 4 + limb]:
 *   j = 0  A:  compressed input   theta^2 a_0 + theta a_1 + a_2   (rows < usable_rows)
 *   j = 1  S:  compressed table                                     (rows < usable_rows)
 *   j = 2  A': permuted input (ascending canonical order)           (rows < usable_rows)
 *   j = 3  S': permuted table (A'[i] == S'[i] or A'[i] == A'[i-1])  (rows < usable_rows)
 *   j = 4  z:  lookup grand product, z[0] = 1                       (rows <= usable_rows)
 * in `form` (any B2F_FP_* form: pasta Fp or BN254 Fr, Montgomery or canonical; the
 * challenges are canonical elements of that field); out_rows >= usable_rows + 1, blinding
 * rows are the prover's. d_first_bad[c] receives the first circuit row whose (a_0, a_1, a_2)
 * is not a table row (halo2's ConstraintSystemFailure), UINT64_MAX if none; that circuit's
 * columns are then meaningless. Asynchronous on `stream`. */
B2F_API int b2f_lookup_columns_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                                   const uint64_t* d_row_begin, uint32_t n_circuits,
                                   uint64_t usable_rows, const uint64_t theta[4],
                                   const uint64_t beta[4], const uint64_t gamma[4], uint32_t form,
                                   uint64_t* d_out, uint64_t out_rows, uint64_t* d_first_bad,
                                   void* stream);

/* Keygen's permutation mapping of one instance of `rounds` rounds (halo2_proofs 0.3.0
 * plonk/permutation/keygen.rs Assembly::copy replayed over b2f_copy_constraints in synthesis
 * order, each copy as copy(destination, source)): for permutation column j (= a_{j+1}, the
 * enable_equality order of table16.rs:312-314) and instance row i < R = b2f_layout_rows(rounds),
 * out[j * R + i] = (c' << 29) | r' names the cell the permutation maps (j, i) to. Writes
 * min(8 R, cap) words, returns 8 R (0 for rounds > B2F_MAX_ROUNDS). Host function. */
B2F_API uint64_t b2f_permutation_mapping(uint32_t rounds, uint32_t* out, uint64_t cap);

/* Permutation-argument prover columns (halo2_proofs 0.3.0 plonk/permutation: build_pk's
 * permutation polynomials and prover.rs commit) of the equality columns a_1..a_8 for one
 * circuit made of the instances with host row map h_offsets[0..n] (trace rows of the batch in
 * d_advice; circuit row = trace row - h_offsets[0]), in a domain of 2^k rows:
 *   d_sigma (nullable): sigma_j(w^i) = delta^c' w^r' for (c', r') the mapped cell, at
 *     d_sigma[(j * out_rows + i) * 4 + limb], j < 8, every row i < 2^k (identity past the
 *     instances);
 *   d_z: for each set c of chunk_len columns (cs.degree() - 2 in halo2) the grand product
 *     z_c[0] = z_{c-1}[usable_rows] (1 for c = 0),
 *     z_c[i + 1] = z_c[i] prod_{j in c} (v_j(i) + beta delta^j w^i + gamma)
 *                          / (v_j(i) + beta sigma_j(w^i) + gamma),   i < usable_rows,
 *     at d_z[(c * out_rows + i) * 4 + limb], rows 0 ..= usable_rows (the blinding rows after
 *     them are the prover's). v_j(i) is the cell of a_{j+1} (zero past the instances).
 * usable_rows = 2^k - blinding_factors - 1 >= h_offsets[n] - h_offsets[0]; omega = the
 * domain's generator (F::ROOT_OF_UNITY squared S - k times), delta = F::DELTA, beta, gamma:
 * canonical elements of the field chosen by `form` (any B2F_FP_*; outputs in that form).
 * out_rows >= usable_rows + 1 (and >= 2^k with d_sigma); 16-byte aligned outputs. A valid
 * trace closes: z_last[usable_rows] = 1. Asynchronous on `stream` after a short host setup
 * (mapping patterns cached per rounds in the context; the instance table goes up by an async
 * copy from pinned staging). The host waits only for the previous call's table upload, and for
 * the whole stream only when a device buffer has to grow (a new `rounds`, more instances, a
 * larger k or a smaller chunk_len than before). Scratch: ceil(8 / chunk_len) column sets of
 * 3 x 32 B per usable row plus O(2^k / 1024) tables. */
B2F_API int b2f_permutation_columns_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                                        const uint64_t* h_offsets, size_t n, uint32_t k,
                                        uint64_t usable_rows, const uint64_t omega[4],
                                        const uint64_t delta[4], const uint64_t beta[4],
                                        const uint64_t gamma[4], uint32_t chunk_len, uint32_t form,
                                        uint64_t* d_sigma, uint64_t* d_z, uint64_t out_rows,
                                        void* stream);

/* The permutation z columns of n_circuits circuits in one call (halo2's create_proof takes a
 * slice of circuits and draws one beta, gamma for all of them; the shape of
 * b2f_lookup_columns_dev). h_offsets[0..n] is the host row map of the instances in d_advice, as
 * for b2f_permutation_columns_dev; h_circuit_first[0..n_circuits] holds strictly increasing
 * instance indices, h_circuit_first[n_circuits] <= n: circuit c is made of the instances
 * [h_circuit_first[c], h_circuit_first[c + 1]) and its row 0 is trace row
 * h_offsets[h_circuit_first[c]] (instances before the first and after the last boundary belong to
 * no circuit). k, usable_rows, omega, delta, beta, gamma, chunk_len and form are shared. With
 * sets = ceil(8 / chunk_len), column set s of circuit c goes to
 *   d_z[((c * sets + s) * out_rows + i) * 4 + limb],  rows 0 ..= usable_rows,
 * bit for bit what b2f_permutation_columns_dev writes for that circuit alone with d_sigma = NULL:
 * every circuit's first set starts at 1, its sets chain, cells past its instances are zero and
 * map to themselves. There is no sigma argument: sigma is keygen data, computed once per circuit
 * shape by b2f_permutation_sigma_dev. The circuits run in groups of
 * clamp(2^24 / usable_rows, 1, n_circuits) (and at most 65,535 / sets), so the scratch is that
 * many times the single call's per-circuit scratch whatever n_circuits is; the coset tables are
 * built once per call and one instance table goes up for all circuits (same host setup and
 * waits as the single call). B2F_ERR_ROWS names the first circuit that uses more than
 * usable_rows rows. A zero denominator product in any circuit reports B2F_ERR_FIELD at b2f_sync;
 * the other circuits' columns are written all the same. One call is one B2F_KERNEL_PERM region.
 * Asynchronous on `stream`. */
B2F_API int b2f_permutation_columns_batch_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                                              const uint64_t* h_offsets, size_t n,
                                              const uint64_t* h_circuit_first, uint32_t n_circuits,
                                              uint32_t k, uint64_t usable_rows, const uint64_t omega[4],
                                              const uint64_t delta[4], const uint64_t beta[4],
                                              const uint64_t gamma[4], uint32_t chunk_len, uint32_t form,
                                              uint64_t* d_z, uint64_t out_rows, void* stream);

/* Keygen's permutation polynomials alone (halo2_proofs 0.3.0 plonk/permutation/keygen.rs
 * build_pk: the sigma columns depend on the circuit's structure, not on a witness): the same
 * d_sigma that b2f_permutation_columns_dev writes for the row map h_offsets[0..n], domain 2^k,
 * omega, delta and `form` -- sigma_j(w^i) = delta^c' w^r' at d_sigma[(j * out_rows + i) * 4 +
 * limb], j < 8, every row i < 2^k. A prover computes it once per circuit shape and then calls
 * b2f_permutation_columns_dev with d_sigma = NULL per proof (the z columns never read sigma).
 * h_offsets[n] - h_offsets[0] < 2^k, out_rows >= 2^k, d_sigma 16-byte aligned. Asynchronous on
 * `stream` after the same short host setup. */
B2F_API int b2f_permutation_sigma_dev(b2f_ctx* ctx, const uint64_t* h_offsets, size_t n, uint32_t k,
                                      const uint64_t omega[4], const uint64_t delta[4], uint32_t form,
                                      uint64_t* d_sigma, uint64_t out_rows, void* stream);

/* Batched NTT of prover columns (halo2's EvaluationDomain::lagrange_to_coeff, coeff_to_lagrange
 * and coeff_to_extended), n = 2^k rows, n_cols columns in one call. Column c of the input is
 * d_in[(c * in_rows + i) * 4 + limb] (the layout every prover-column call here writes): rows
 * i < in_len are read, rows in_len .. n - 1 are taken as zero (coeff_to_extended's padding, no
 * padded copy) and never read. Column c of the output is d_out[(c * out_rows + i) * 4 + limb]:
 * all n rows are written in natural order, rows >= n are not touched. omega (the generator of the
 * 2^k domain) and shift (non-zero) are canonical elements of the field `form` selects (any
 * B2F_FP_*); data is in `form` on both sides, inputs reduced (< p), outputs fully reduced.
 *   B2F_NTT_FORWARD  out[i] = sum_j in[j] (shift omega^i)^j: coefficients to evaluations on the
 *                    coset shift <omega>. shift = 1 is coeff_to_lagrange; coeff_to_extended is
 *                    k = the extended k, in_len = 2^k_circuit, shift = F::ZETA.
 *   B2F_NTT_INVERSE  out[j] = shift^-j n^-1 sum_i in[i] omega^(-i j): the exact inverse of the
 *                    forward map for the same omega and shift. shift = 1 is lagrange_to_coeff.
 * The caller passes the domain's own omega and shift in both directions; omega^-1, n^-1 and
 * shift^-1 are derived on the device. Twiddle and shift-power tables are built on the device once
 * per (field, k, direction, omega, shift) and cached in the context (8 domains, replaced
 * round-robin), so a repeated call builds nothing.
 * B2F_ERR_ARG: a null pointer, d_in or d_out not 16-byte aligned, k outside [1, 28] (BN254's
 * 2-adicity; one limit for both fields), n_cols == 0, in_len == 0, direction > 1, form > 3, omega
 * or shift >= p, shift == 0, or any overlap of [d_in, d_in + n_cols in_rows 32) with
 * [d_out, d_out + n_cols out_rows 32) (no in-place transform). B2F_ERR_ROWS: in_len > 2^k,
 * in_rows < in_len or out_rows < 2^k. Nothing is launched on either. B2F_ERR_FIELD at b2f_sync
 * when omega^(2^(k-1)) != -1 (omega is not a primitive 2^k-th root of unity): the outputs are then
 * meaningless; the next call works normally. Asynchronous on `stream`; one call is one
 * B2F_KERNEL_NTT region. n_cols may exceed 65,535 (the call launches column groups). */
#define B2F_NTT_FORWARD 0
#define B2F_NTT_INVERSE 1
B2F_API int b2f_ntt_columns_dev(b2f_ctx* ctx, const uint64_t* d_in, uint64_t in_rows,
                                uint64_t in_len, uint32_t n_cols, uint32_t k,
                                const uint64_t omega[4], const uint64_t shift[4],
                                uint32_t direction, uint32_t form, uint64_t* d_out,
                                uint64_t out_rows, void* stream);

/* The custom-gate, permutation and lookup terms of the quotient numerator on the extended coset,
 * and the division by the vanishing polynomial (the gates of docs/LAYOUT.md §4; halo2_proofs
 * 0.3.0 plonk/permutation/prover.rs and plonk/lookup/prover.rs Committed::construct,
 * EvaluationDomain::divide_by_vanishing_poly). The term calls fold into a caller-supplied
 * accumulator; halo2's order is the gates, then the permutation, then each lookup.
 * Shared conventions: columns are d[(c * rows + i) * 4 + limb] in `form` (any B2F_FP_*; the
 * canonical forms convert at load and store, inputs reduced); n = 2^k, n_ext = 2^ext_k,
 * 1 <= k < ext_k <= 28, rot = 2^(ext_k - k); extended row i is the point X_i = shift omega_ext^i
 * and a rotation by r circuit rows reads extended row (i + r rot) mod n_ext; usable_rows =
 * 2^k - blinding_factors - 1 as in the column calls; omega_ext, shift, delta and the challenges
 * are canonical elements of the field of `form`. The fold: h = h_in (zero when d_h_in is NULL),
 * then h = h y + e_t for each term in order, i.e. h_out = y^T h_in + sum_t y^(T-1-t) e_t. d_h_in
 * == d_h_out is allowed (a row reads only its own h); any other overlap of h_out with h_in or
 * with an input block is B2F_ERR_ARG. Common errors, nothing launched on either: B2F_ERR_ARG for a
 * null or misaligned (16 B) pointer, k or ext_k out of range, form > 3, an element >= p, shift ==
 * 0; B2F_ERR_ROWS for usable_rows >= 2^k, rows < n_ext, out_rows < 2^k. Asynchronous on `stream`;
 * each call is one B2F_KERNEL_QUOTIENT region.
 *
 * b2f_lagrange_selectors_dev (keygen data): three Lagrange-form columns over 2^k rows at
 * d_out[(c * out_rows + i) * 4 + limb]: c = 0 l_0 (1 at row 0), 1 l_last (1 at row usable_rows),
 * 2 l_active = 1 - l_last - l_blind (1 on rows < usable_rows), zero elsewhere; rows >= 2^k are
 * not touched. Two b2f_ntt_columns_dev calls take them to the coset like any other column. */
B2F_API int b2f_lagrange_selectors_dev(b2f_ctx* ctx, uint32_t k, uint64_t usable_rows, uint32_t form,
                                       uint64_t* d_out, uint64_t out_rows, void* stream);

/* Custom-gate terms. d_advice: the ten advice columns in halo2 order (the block
 * b2f_export_fp_dev writes, extended); d_fixed: the seventeen columns of b2f_export_fixed_fp_dev,
 * extended; both with stride rows >= n_ext. x@j of extended row i is row (i + j rot) mod n_ext
 * (a true mod: 11 rot may exceed n_ext). Each term is q_g p with q_g fixed column g; T = 74, in
 * ascending selector bit g, within a gate in the order of docs/LAYOUT.md §4 with "for all k"
 * expanded k = 0..3 outermost (a_i = advice column b2f_halo2_column_index(i), k_0 = fixed
 * column 16; docs/LAYOUT.md §4.1 has the same list):
 *   0  (2)  a_7@0 - a_1@0 - 2^16 a_1@1;  a_8@0 - a_1@2 - 2^16 a_1@3
 *   1  (8)  per k, k1 = (k+1)&3, k2 = (k+2)&3:  a_7@3k - a_1@(3k1+1) - 2^8 a_1@3k2;
 *           a_8@3k - a_2@(3k1+1) - 2^16 a_2@3k2
 *   2  (8)  per k, k3 = (k+3)&3:  a_7@2k - a_6@2k3 - 2 a_1@2k;  a_8@2k - a_6@2k3 - 4 a_2@2k
 *   3  (2)  sum_k 2^16k (a_3@k + a_4@k + a_5@k - a_1@k) - 2^64 a_9@0;  a_9@0 (a_9@0 - 1)(a_9@0 - 2)
 *   4  (12) per k:  a_3@3k + a_4@3k - a_2@3k - 2^16 a_2@(3k+1) - 2 a_2@(3k+2);  a_0@3k;  a_0@(3k+1)
 *   5  (2)  sum_k 2^16k (a_3@k + a_4@k - a_1@k) - 2^64 a_9@0;  a_9@0 (a_9@0 - 1)
 *   6  (4)  per k:  a_3@2k + a_4@2k - a_2@2k - 2 a_2@(2k+1)
 *   7  (2)  as 3
 *   8  (12) per k:  a_3@2k + a_4@2k - a_2@2k - 2^30 a_6@2k - 2 a_2@(2k+1);  a_0@2k (a_0@2k - 1);
 *           a_6@2k (a_6@2k - 1)
 *   9  (2)  as 5
 *   10 (4)  as 6
 *   11 (2)  a_7@0 - a_1@0 - 2^16 a_1@2;  a_8@0 - a_1@4 - 2^16 a_1@6
 *   12 (4)  as 6
 *   13 (4)  per k:  a_3@2k + a_4@2k + a_5@2k - a_2@2k - 2 a_2@(2k+1)
 *   14 (1)  a_1@0 - k_0@0
 *   15 (5)  a_5@0 (a_5@0 - 1);  per k:  a_1@k - 65535 a_5@0
 * Gates with the same polynomials are separate terms. The largest degree is 4 (bit 3 with its
 * selector), the lookup's, so ext_k = k + 2 serves all three term calls. No omega and no shift:
 * the gates never use X_i. halo2's keygen would combine simple selectors into fewer fixed
 * columns; that is not modelled. Errors, nothing launched: B2F_ERR_ARG for a null or misaligned
 * pointer, k or ext_k out of range, form > 3, y >= p, a forbidden overlap; B2F_ERR_ROWS for
 * rows < n_ext. */
B2F_API int b2f_quotient_gates_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, const uint64_t* d_advice,
                                   const uint64_t* d_fixed, uint64_t rows, const uint64_t y[4],
                                   const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form, void* stream);

/* Permutation terms. All blocks are on the extended coset with stride rows >= n_ext: d_l the
 * three selector columns; d_advice the ten advice columns in halo2 order, the block
 * b2f_export_fp_dev writes (v_j = column b2f_halo2_column_index(j + 1), j < 8; the two columns
 * outside the permutation are not read); d_sigma the eight sigma columns; d_z the sets =
 * ceil(8 / chunk_len) grand-product columns (1 <= chunk_len <= 8). Terms per row, T = 2 sets + 1:
 *   l_0 (1 - z_0)
 *   l_last (z_last^2 - z_last),                  z_last = set sets - 1
 *   l_0 (z_s - z_{s-1}(w^usable_rows X)),        s = 1 .. sets - 1
 *   l_active (z_s(w X) prod_{j in s} (v_j + beta sigma_j + gamma)
 *             - z_s prod_{j in s} (v_j + beta delta^j X_i + gamma)),   s = 0 .. sets - 1
 * (j runs over all eight columns across the sets; the last set may be short). X_i comes from a
 * two-level power table built on the device once per (field, ext_k, omega_ext, shift) and cached
 * in the context (4 domains, replaced round-robin). B2F_ERR_FIELD at b2f_sync when
 * omega_ext^(n_ext / 2) != -1. */
B2F_API int b2f_quotient_permutation_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, uint64_t usable_rows,
                                         const uint64_t* d_l, const uint64_t* d_advice,
                                         const uint64_t* d_sigma, const uint64_t* d_z, uint32_t chunk_len,
                                         uint64_t rows, const uint64_t omega_ext[4], const uint64_t shift[4],
                                         const uint64_t delta[4], const uint64_t beta[4],
                                         const uint64_t gamma[4], const uint64_t y[4],
                                         const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form,
                                         void* stream);

/* Lookup terms. d_lookup holds the five columns A, S, A', S', z in the order
 * b2f_lookup_columns_dev writes them, extended (stride rows). Terms per row, T = 5:
 *   l_0 (1 - z)
 *   l_last (z^2 - z)
 *   l_active (z(w X) (A' + beta) (S' + gamma) - z (A + beta) (S + gamma))
 *   l_0 (A' - S')
 *   l_active (A' - S') (A' - A'(w^-1 X))
 * A and S are passed compressed: the theta-combination is linear, so the extension of the
 * compressed column is the polynomial halo2 evaluates, provided its blinding rows are the
 * compression of the advice (and table) blinding rows. There is no theta argument. */
B2F_API int b2f_quotient_lookup_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, const uint64_t* d_l,
                                    const uint64_t* d_lookup, uint64_t rows, const uint64_t beta[4],
                                    const uint64_t gamma[4], const uint64_t y[4], const uint64_t* d_h_in,
                                    uint64_t* d_h_out, uint32_t form, void* stream);

/* divide_by_vanishing_poly: h_out[i] = h_in[i] (X_i^n - 1)^-1 over the n_ext rows, in place
 * allowed. The divisor has period rot in i: rot values are inverted on the device once per
 * (field, k, ext_k, omega_ext, shift) and cached in the context (4 domains, replaced round-robin).
 * B2F_ERR_FIELD at b2f_sync when X_i^n = 1 for some i (e.g. shift = 1: the outputs are then
 * meaningless) or omega_ext^(n_ext / 2) != -1; the next call works normally. */
B2F_API int b2f_quotient_divide_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, const uint64_t omega_ext[4],
                                    const uint64_t shift[4], const uint64_t* d_h_in, uint64_t* d_h_out,
                                    uint32_t form, void* stream);

/* The opening step over coefficient columns: multi-point evaluation, linear folds and Kate division
 * (halo2_proofs 0.3.0 arithmetic.rs eval_polynomial and kate_division; the evaluations and the
 * x^n fold of the h pieces in plonk/prover.rs; the x_1, x_2 and x_4 folds and the divisions of
 * poly/multiopen/prover.rs). Field arithmetic only: the transcript, the commitments and the final
 * IPA / KZG opening stay with the caller. The pieces of h are the columns of the inverse NTT's
 * output (b2f_ntt_columns_dev, shift = ZETA) viewed with rows = n.
 * Shared conventions: a column block is d[(c * rows + i) * 4 + limb] in `form` (any B2F_FP_*;
 * inputs reduced, outputs fully reduced and in the same form: every pass is linear in the column
 * data with Montgomery-form multipliers, which gives a canonical column exactly what converting at
 * load and store would); len <= rows coefficients per column are read, at i < len, and rows >= len
 * are never read or written; points and scalars are canonical host elements < p; every host array
 * is consumed before the call returns; scratch belongs to the context; pointers are 16-byte
 * aligned; no output may overlap an input. Errors, nothing launched and the next good call works:
 * B2F_ERR_ARG for a null or misaligned pointer, form > 3, len == 0 (or > 2^32), n_cols == 0,
 * n_queries == 0 / n_out == 0, a column or point index out of range, an h_first that does not
 * start at 0 or decreases, an element >= p, a forbidden overlap; B2F_ERR_ROWS for len > rows or
 * out_rows < len. Asynchronous on `stream`; each call is one B2F_KERNEL_QUOTIENT region.
 *
 * b2f_poly_eval_dev: d_out[q] = sum_{i < len} col[c_q][i] pt[p_q]^i for the query q =
 * (h_queries[2 q], h_queries[2 q + 1]) = (column, point index), as n_queries elements in `form`.
 * Queries come in any order and may repeat. The queries are grouped by column on the host and a
 * column is read once per call, however many queries name it: a workgroup keeps a tile of 1,024
 * coefficients in registers while it loops over the column's points; the tile sums are combined
 * by a second launch. The power tables of the points are built on the device. */
B2F_API int b2f_poly_eval_dev(b2f_ctx* ctx, const uint64_t* d_cols, uint64_t rows, uint64_t len, uint32_t n_cols,
                              const uint64_t* h_points, uint32_t n_points, const uint32_t* h_queries,
                              uint64_t n_queries, uint32_t form, uint64_t* d_out, void* stream);

/* Output column o = sum_{j in [h_first[o], h_first[o + 1])} h_scalar[j] * column h_col[j], over
 * i < len, at d_out[(o * out_rows + i) * 4 + limb]; an empty range gives zeros. h_first has
 * n_out + 1 entries, h_col and h_scalar nnz = h_first[n_out]. Every challenge fold of the step is
 * one of these: q = q x_1 + poly over a point set (scalars x_1^(m-1) .. 1), the x_2 and x_4 folds,
 * and h(X) = sum_i x^(n i) h_i(X) (the host supplies the powers). One pass: an output row reads
 * each of its inputs once. */
B2F_API int b2f_poly_combine_dev(b2f_ctx* ctx, const uint64_t* d_cols, uint64_t rows, uint64_t len,
                                 uint32_t n_cols, const uint32_t* h_first, const uint32_t* h_col,
                                 const uint64_t* h_scalar, uint32_t n_out, uint32_t form, uint64_t* d_out,
                                 uint64_t out_rows, void* stream);

/* Output column c is halo2's kate_division applied to column c for the points h_points[h_first[c]]
 * .. h_points[h_first[c + 1] - 1] in turn (h_first: n_cols + 1 entries): with m_c points, the
 * floor quotient by prod (X - pt_j), remainders discarded. Its len - m_c coefficients are written
 * and rows len - m_c <= i < len are written zero (halo2 resizes to n); m_c = 0 copies the column,
 * m_c >= len gives all zeros. One division is q_{len-1} = 0, q_{i-1} = a_i + z q_i, a suffix
 * recurrence with a constant multiplier: per point, one launch forms the tile sums (the evaluation
 * kernel's), one scans them into carries, one applies them; a chain of several points repeats the
 * three, ping-ponging through context scratch. */
B2F_API int b2f_kate_divide_dev(b2f_ctx* ctx, const uint64_t* d_cols, uint64_t rows, uint64_t len,
                                uint32_t n_cols, const uint32_t* h_first, const uint64_t* h_points,
                                uint32_t form, uint64_t* d_out, uint64_t out_rows, void* stream);

/* The commitments: a batched variable-base multi-scalar multiplication on the curve whose scalar
 * field `form` names: Vesta (y^2 = x^3 + 5 over pasta Fq, group order pasta Fp) for forms 0/1,
 * BN254 G1 (y^2 = x^3 + 3 over bn256::Fq, group order bn256::Fr) for forms 2/3. This is halo2's
 * commit / commit_lagrange of a column against the parameters' points (g, g_lagrange);
 * b2f_group_ntt_dev derives g_lagrange from g; choosing g and the blinding term's generator stay
 * with the caller (the transcript: b2f_transcript_*_dev; the IPA opening: b2f_ipa_open_dev).
 * d_scalars is a column block d[(c * rows + i) * 4 + limb] in `form` (any B2F_FP_*, reduced: the
 * blocks every other prover call produces); rows >= len are never read. d_bases holds n_bases >=
 * len affine points shared by all columns, a point being (x, y), each coordinate four
 * little-endian u64 limbs in base-field Montgomery form (R = 2^256), 64 bytes, the identity all
 * zero: d_bases[i * 8 + 0..3] = x, [i * 8 + 4..7] = y. A (0, 0) base contributes nothing. Points
 * are NOT checked to be on the curve: off-curve input gives a meaningless point and never an
 * out-of-range access. d_out receives n_cols affine points in the same layout, d_out[c * 8 + ..],
 * the identity as all zeros; the affine form is canonical, so the result is bit-exact whatever
 * the order of summation.
 * Pippenger's bucket method: signed c-bit digits, a radix sort by (column, window, bucket), bucket
 * sums by a levelled reduction in which no lane adds more than 32 points in a row whatever the
 * scalars' distribution, window sums by running sums, Horner over the windows and one inversion
 * per output (B2F_ERR_CHECK at b2f_sync if that inversion fails: a library defect). Columns and
 * rows are processed in passes of at most 2^24 digits and 2^20 buckets, so scratch (the context's)
 * is bounded: b2f_msm_plan reports it. Asynchronous on `stream`; pointers are 16-byte aligned; one
 * B2F_KERNEL_QUOTIENT region per call. Errors, nothing launched and the next good call works:
 * B2F_ERR_ARG for a null or misaligned pointer, form > 3, len == 0 or len > 2^28, n_cols == 0,
 * d_out overlapping an input; B2F_ERR_ROWS for len > rows or len > n_bases; B2F_ERR_HIP for
 * runtime failures, scratch growth included. */
/* out[c] = sum_{i < len} scalar[c][i] * base[i], c < n_cols */
B2F_API int b2f_msm_dev(b2f_ctx* ctx, const uint64_t* d_scalars, uint64_t rows, uint64_t len,
                        uint32_t n_cols, const uint64_t* d_bases, uint64_t n_bases, uint32_t form,
                        uint64_t* d_out, void* stream);
/* host only: the plan b2f_msm_dev would use (window bits, windows, columns per group, scratch bytes);
 * B2F_ERR_ARG where the call would refuse len, n_cols or form. Any output pointer may be null. */
B2F_API int b2f_msm_plan(uint64_t len, uint32_t n_cols, uint32_t form, uint32_t* window_bits,
                         uint32_t* windows, uint32_t* group, uint64_t* scratch_bytes);

/* Commitments of columns cut from u32 cells where they lie: the advice columns of the trace and the
 * packed fixed column. halo2 commits an advice column in Lagrange form (commit_lagrange against
 * g_lagrange), so the scalars are the raw cells followed by the blinding rows the caller drew; a
 * cell of `bits` bits is ceil((bits + 1) / c) signed c-bit digits where a field element is
 * ceil(256 / c), and nothing is widened to 32 bytes on the way.
 * One column is a b2f_cell_column: scalar i (i < len) is
 *   i < avail ? (d_cells[offset + i] >> shift) & (2^bits - 1) : 0
 * Cells have no form: they are integers. d_tail (may be null, then tail_rows == 0; tail_rows <= 64)
 * is a block d[(c * tail_rows + t) * 4 + limb] of full scalars in `form`, reduced, multiplying bases
 * len .. len + tail_rows - 1. `form`, d_bases and d_out are as b2f_msm_dev defines them: n_cols affine
 * points out, bit-exact. h_cols is a HOST array of n_cols b2f_cell_column (passed as void*: 24 bytes
 * each); the call copies what it needs before it returns, so the caller may overwrite or free it at
 * once. The passes are b2f_msm_dev's (sort, levelled bucket reduction, window sums) over each
 * column's own windows, then windows * c doublings of Horner per column; the tail's scalar
 * multiplications run on a side stream of the context beside them and are joined back before the one
 * affine conversion. Asynchronous on `stream`; scratch is the context's (b2f_msm_cells_plan reports
 * it); one B2F_KERNEL_QUOTIENT region per call. Errors, nothing launched and the next good call
 * works: B2F_ERR_ARG for a null or misaligned pointer (d_cells, d_bases, d_out, d_tail 16-byte
 * aligned), form > 3, len == 0 or len > 2^28, n_cols == 0 or n_cols > 4096, tail_rows > 64, d_tail
 * non-null with tail_rows == 0 or the reverse, bits == 0, bits > 32 or shift + bits > 32, d_out
 * overlapping an input; B2F_ERR_ROWS for offset + min(avail, len) > n_cells in any column or
 * len + tail_rows > n_bases; B2F_ERR_HIP for runtime failures, scratch growth included. */
typedef struct {
  uint64_t offset; /* index of the column's first cell in d_cells */
  uint64_t avail;  /* cells from `avail` on read as zero and are never loaded */
  uint32_t shift;  /* 0..31 */
  uint32_t bits;   /* 1..32, shift + bits <= 32 */
} b2f_cell_column; /* 24 bytes */
/* out[c] = sum_{i < len} scalar_c(i) base[i] + sum_{t < tail_rows} tail[c][t] base[len + t] */
B2F_API int b2f_msm_cells_dev(b2f_ctx* ctx, const uint32_t* d_cells, uint64_t n_cells,
                              const void* h_cols, uint32_t n_cols, uint64_t len,
                              const uint64_t* d_tail, uint64_t tail_rows,
                              const uint64_t* d_bases, uint64_t n_bases, uint32_t form,
                              uint64_t* d_out, void* stream);
/* host only: the plan b2f_msm_cells_dev would use: the window bits, the digits it recodes (len times
 * the sum over the columns of ceil((bits + 1) / c)) and the scratch bytes; B2F_ERR_ARG where the call
 * would refuse the descriptors, n_cols, len, tail_rows or form. Any output pointer may be null. */
B2F_API int b2f_msm_cells_plan(const void* h_cols, uint32_t n_cols, uint64_t len,
                               uint64_t tail_rows, uint32_t form, uint32_t* window_bits,
                               uint64_t* digits, uint64_t* scratch_bytes);
/* host only: the descriptors of one circuit's ten advice columns, the circuit being trace rows
 * row_begin .. row_begin + usable_rows - 1 of a trace of total_rows rows (d_cells = d_advice,
 * n_cells = 10 * total_rows), in halo2 column order: entry b2f_halo2_column_index(i) describes a_i
 * (offset i * total_rows + row_begin, shift 0, bits 32). avail = min(usable_rows, total_rows -
 * row_begin), 0 for row_begin >= total_rows: a circuit that runs past the trace reads zero rows there,
 * as b2f_lookup_columns_dev defines. out10 holds 10 b2f_cell_column. Returns 10, or 0 (nothing
 * written) for total_rows % 4 != 0, usable_rows == 0 or a null out10. */
B2F_API uint32_t b2f_advice_cell_columns(uint64_t total_rows, uint64_t row_begin, uint64_t usable_rows,
                                         void* out10);
/* host only: the same for the B2F_NUM_FIXED_FP = 17 fixed columns over the packed fixed column
 * (d_cells = d_fixed, n_cells = total_rows), in b2f_export_fixed_fp_dev's order: c < 16 selector bit
 * c (shift c, bits 1), c = 16 k_0 (shift 16, bits 16); every offset is row_begin. Returns 17, or 0. */
B2F_API uint32_t b2f_fixed_cell_columns(uint64_t total_rows, uint64_t row_begin, uint64_t usable_rows,
                                        void* out17);

/* The rounds of the inner product argument's opening (halo2's pasta backend:
 * poly/commitment/prover.rs::create_proof's loop) over three device vectors of length len = 2^j:
 * the coefficients p and the powers b, scalars d[i * 4 + limb] in `form` (any B2F_FP_*, reduced), and
 * the generators G, points in b2f_msm_dev's layout (64 bytes, base-field Montgomery coordinates, the
 * identity all zero, not checked to be on the curve). Forms 0/1 are Vesta, forms 2/3 BN254 G1. With
 * half = len / 2, one round is
 *   L = <p[half..], G[..half]>         R = <p[..half], G[half..]>          (b2f_ipa_round_dev)
 *   value_l = <p[half..], b[..half]>   value_r = <p[..half], b[half..]>
 *   caller: L += [value_l z] U + [l_rand] W, the same for R; writes both; squeezes u
 *   p[i] += p[half+i] u^-1   b[i] += b[half+i] u   G[i] = affine(G[i] + [u] G[half+i])   (b2f_ipa_fold_dev)
 * and after log2(len) rounds c = p[0]. For these three calls the transcript, the blinding scalars
 * and the U / W terms stay with the caller and every challenge is a host argument (canonical limbs);
 * b2f_ipa_open_dev below queues the whole loop, caller's lines included, on a device transcript.
 * All three calls are asynchronous on `stream`, take 16-byte aligned pointers, use the context's
 * scratch and are one B2F_KERNEL_QUOTIENT region each. Errors, nothing launched and the next good
 * call works: B2F_ERR_ARG for a null or misaligned pointer, form > 3, a len that is not a power of
 * two in [2, 2^28] (powers: len == 0 or > 2^28), h_x >= p, h_u >= p or h_u == 0, d_lr or d_values
 * overlapping an input or each other, the three vectors overlapping each other; B2F_ERR_HIP for
 * runtime failures, scratch growth included; B2F_ERR_CHECK at b2f_sync if an affine conversion's
 * inversion fails on a non-identity point (a library defect, as for b2f_msm_dev). */
/* d_b[i] = x^i, i < len, in `form` */
B2F_API int b2f_ipa_powers_dev(b2f_ctx* ctx, const uint64_t h_x[4], uint64_t len, uint32_t form,
                               uint64_t* d_b, void* stream);
/* d_lr[0..7] = L, d_lr[8..15] = R (affine, the identity as zeros: bit-exact); d_values[0..3] =
 * value_l, d_values[4..7] = value_r (fully reduced, in `form`). Reads all len elements of the three
 * vectors and writes nothing else. A round of len <= b2f_ipa_direct_max_len() is one launch; a
 * longer one is a single two-column Pippenger pass plus a tiled inner product. */
B2F_API int b2f_ipa_round_dev(b2f_ctx* ctx, const uint64_t* d_p, const uint64_t* d_b,
                              const uint64_t* d_g, uint64_t len, uint32_t form, uint64_t* d_lr,
                              uint64_t* d_values, void* stream);
/* The three collapses in place on i < half; elements at i >= half are read and never written. u^-1 is
 * formed on the host. */
B2F_API int b2f_ipa_fold_dev(b2f_ctx* ctx, uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len,
                             const uint64_t h_u[4], uint32_t form, void* stream);
/* host only: the longest round b2f_ipa_round_dev runs as one direct launch (a power of two) */
B2F_API uint64_t b2f_ipa_direct_max_len(void);

/* The Fiat-Shamir transcript on the device: halo2's Blake2bWrite with Challenge255 (halo2_proofs
 * 0.3.0 transcript.rs), so that a challenge can stay where the previous call left it. The hash is
 * BLAKE2b with a 64-byte digest, no key and the personalisation "Halo2-Transcript".
 *   common_point(P)    absorbs the byte 1, then x and y of the affine point as 32 little-endian
 *                      bytes each, canonical (write_point hashes the same bytes)
 *   common_scalar(s)   absorbs the byte 2, then 32 little-endian bytes of the canonical scalar
 *   squeeze_challenge  absorbs the byte 0 into the running state, finalises a COPY of it, reads the
 *                      64 digest bytes as a 512-bit little-endian integer and reduces it modulo
 *                      the scalar field's r (from_uniform_bytes); the running state goes on
 * The state is B2F_TRANSCRIPT_BYTES of device memory, 16-byte aligned, and its layout is part of
 * this ABI, so a host with a BLAKE2b of its own can export a transcript it began or import one the
 * device moved on. As uint64_t words:
 *   0..7    h (after init: the IV xor the parameter block 0x01010040 and the personalisation)
 *   8..9    t, the bytes compressed so far, low word first (a multiple of 128)
 *   10..25  the 128-byte block buffer; bytes at and past the count are zero in every state these
 *           calls write (an imported state need not keep that)
 *   26      the bytes in the buffer, 0..128 (a larger value is read as 128)
 *   27..31  zero
 * A full buffer is compressed only when the next byte arrives: BLAKE2's lazy last block, whose
 * compression carries the final flag. So the bytes absorbed so far are t + word 26.
 * d_points holds n affine points in b2f_msm_dev's layout (64 bytes, base-field Montgomery
 * coordinates), absorbed in order; `form` selects the curve (0/1 Vesta, 2/3 BN254 G1). The
 * identity (all zero), which halo2 refuses to write, absorbs the byte 1 and 64 zero bytes, so the
 * state stays defined, and reports B2F_ERR_FIELD at b2f_sync. d_scalars holds d[i * 4 + limb] in
 * `form`, reduced. d_challenge receives four canonical limbs of the form's scalar field whatever
 * the form: how every challenge is passed in this ABI (and what b2f_ipa_open_dev's d_z takes).
 * One workgroup: its lanes convert a chunk of 256 elements to bytes in LDS, one lane hashes.
 * Asynchronous on `stream`; one B2F_KERNEL_QUOTIENT region per call. B2F_ERR_ARG, with nothing
 * launched and the next good call working: a null or misaligned (16 B) pointer, form > 3, n == 0
 * or n > 2^20, the state overlapping the data or the challenge. */
#define B2F_TRANSCRIPT_BYTES 256
B2F_API int b2f_transcript_init_dev(b2f_ctx* ctx, uint64_t* d_state, void* stream);
B2F_API int b2f_transcript_absorb_points_dev(b2f_ctx* ctx, uint64_t* d_state, const uint64_t* d_points,
                                             uint64_t n, uint32_t form, void* stream);
B2F_API int b2f_transcript_absorb_scalars_dev(b2f_ctx* ctx, uint64_t* d_state, const uint64_t* d_scalars,
                                              uint64_t n, uint32_t form, void* stream);
B2F_API int b2f_transcript_squeeze_dev(b2f_ctx* ctx, uint64_t* d_state, uint32_t form,
                                       uint64_t* d_challenge, void* stream);

/* The whole opening loop in one queued call: with k = log2(len), for j = 0 .. k - 1 on the
 * current length (len, len / 2, .., 2)
 *   1  L, R, value_l, value_r as b2f_ipa_round_dev forms them (the same launches)
 *   2  L_j = L + [value_l z] U + [l_rand_j] W,  R_j = R + [value_r z] U + [r_rand_j] W, affine, to
 *      d_lr[16 j .. 16 j + 7] and d_lr[16 j + 8 .. 16 j + 15]
 *   3  L_j then R_j absorbed as points into the transcript at d_state; u_j squeezed to
 *      d_u[4 j ..], canonical
 *   4  f += l_rand_j u_j^-1 + r_rand_j u_j, u_j^-1 formed on the device
 *   5  the three folds of b2f_ipa_fold_dev with u_j and u_j^-1 read from device memory
 * and then c = p[0]; c, then f, absorbed as scalars (write_scalar twice); d_cf[0..3] = c,
 * d_cf[4..7] = f, both in `form`. No host step lies between the rounds: the call returns once
 * everything is queued. d_p, d_b, d_g: as for the three calls above, folded in place. d_z: four
 * canonical limbs on the device (a squeeze's output). d_rand: 2k scalars in `form`, reduced,
 * l_rand_0, r_rand_0, l_rand_1, ..: the randomness is the caller's. d_cf[4..7] on entry: the
 * starting f, in `form`. h_u_point, h_w_point: HOST affine points in b2f_msm_dev's layout, read
 * before the call returns; their multiples come from the cached tables of
 * b2f_fixed_base_mul_dev (two entries of its cache, built on the first call with a base), one
 * table entry per lane summed in LDS, so the blinding adds no doubling chain to a round. Choosing
 * g, U and W, the s_poly masking before the loop and the byte encoding of the proof stay with the
 * caller. Errors: B2F_ERR_ARG, nothing launched and the next good call working, for what the three
 * calls refuse, a null or misaligned pointer, U or W the identity, or any buffer the call writes
 * (the vectors, the state, d_lr [128 k bytes], d_u [32 k], d_cf [64]) overlapping another buffer
 * of the call; B2F_ERR_FIELD at b2f_sync if an L_j or R_j is the identity or a u_j is zero (halo2
 * fails there too; the outputs are then meaningless); B2F_ERR_CHECK and B2F_ERR_HIP as above. One
 * B2F_KERNEL_QUOTIENT region. */
B2F_API int b2f_ipa_open_dev(b2f_ctx* ctx, uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len,
                             const uint64_t h_u_point[8], const uint64_t h_w_point[8],
                             const uint64_t* d_z, const uint64_t* d_rand, uint64_t* d_state,
                             uint32_t form, uint64_t* d_lr, uint64_t* d_u, uint64_t* d_cf, void* stream);

/* The group NTT: the discrete Fourier transform of n = 2^k curve points over the 2^k domain of the
 * curve's scalar field. This is what turns the parameters' g into g_lagrange (halo2's
 * g_to_lagrange in Params::new / ParamsKZG::setup: best_fft over the points with omega^-1, every
 * point times n^-1, batch-normalised), the bases the Lagrange-form commitments (b2f_msm_cells_dev,
 * b2f_msm_dev of a Lagrange column) multiply against: g_lagrange = inverse(g). Hash-to-curve for
 * the IPA's g and a KZG ceremony's points stay with the caller (b2f_fixed_base_mul_dev builds g for
 * a caller who knows tau).
 * d_in holds n points in b2f_msm_dev's layout (64 bytes, base-field Montgomery coordinates, the
 * identity all zero, not checked to be on the curve: off-curve input gives meaningless points and
 * never an out-of-range access). `form` only selects the curve: forms 0/1 are Vesta, forms 2/3
 * BN254 G1. omega is the 2^k domain's generator as canonical limbs of that curve's scalar field, as
 * for b2f_ntt_columns_dev, in both directions; omega^-1 and n^-1 are derived by the library.
 *   B2F_NTT_FORWARD  out[i] = sum_j [omega^(i j)] in[j]
 *   B2F_NTT_INVERSE  out[i] = [n^-1] sum_j [omega^(-i j)] in[j]: the exact inverse of the forward map
 * d_out receives n affine points in the same layout, the identity as all zeros; the affine form is
 * canonical, so the result is bit-exact whatever the order of summation. d_out == d_in is allowed
 * (the transform then runs in place); any other overlap is refused.
 * Radix-2 stages in place in d_out, the points affine between stages, one launch per stage; the
 * stage whose twiddle is 1 multiplies nothing and, for the inverse, carries the n multiplications
 * by n^-1. The n / 2 twiddles are rebuilt on every call in the context's scratch. Asynchronous on
 * `stream`; pointers are 16-byte aligned; one B2F_KERNEL_QUOTIENT region per call; all byte offsets
 * are 64-bit. Errors: B2F_ERR_ARG, with nothing launched and the next good call working, for a null
 * or misaligned pointer, k outside [1, 28], direction > 1, form > 3, omega >= r, or d_in and d_out
 * overlapping without being equal; B2F_ERR_FIELD at b2f_sync when omega^(2^(k-1)) != -1 (the outputs
 * are then meaningless; the next call works normally); B2F_ERR_CHECK at b2f_sync if an affine
 * conversion's inversion fails on a non-identity point (a library defect, as for b2f_msm_dev);
 * B2F_ERR_HIP for runtime failures, scratch growth included. */
B2F_API int b2f_group_ntt_dev(b2f_ctx* ctx, const uint64_t* d_in, uint32_t k, const uint64_t omega[4],
                              uint32_t direction, uint32_t form, uint64_t* d_out, void* stream);
/* host only: the full-width scalar multiplications the inverse direction performs, n + (n / 2)(k - 1)
 * (n by n^-1 and n / 2 in each of the k - 1 stages with twiddles, those by the twiddle 1 included; the
 * forward direction performs the (n / 2)(k - 1) alone), and the scratch bytes of either direction;
 * B2F_ERR_ARG where the call would refuse k or form. Either output pointer may be null. */
B2F_API int b2f_group_ntt_plan(uint32_t k, uint32_t form, uint64_t* scalar_muls, uint64_t* scratch_bytes);

/* Batched fixed-base scalar multiplication: len multiples of one point. With s_i = tau^i
 * (b2f_ipa_powers_dev) and B the curve's generator this is g of halo2's ParamsKZG::setup(k, rng),
 * g[i] = [tau^i] G, whose g_lagrange b2f_group_ntt_dev then derives: the UNSAFE set-up, for a caller
 * who knows tau (tests, benches, development). A production prover loads a ceremony's points;
 * [tau] G2, the pairing and hash-to-curve for the IPA's g stay with the caller.
 * h_base is a HOST affine point in b2f_msm_dev's layout (64 bytes, base-field Montgomery
 * coordinates, all zero for the identity), read before the call returns. It is NOT checked to be on
 * the curve: an off-curve base gives meaningless points and never an out-of-range access. `form`
 * selects the curve and the scalars' form as for b2f_msm_dev: forms 0/1 are Vesta, forms 2/3 BN254
 * G1, Montgomery scalars are converted at load. d_scalars holds len reduced scalars d[i * 4 + limb]
 * (what b2f_ipa_powers_dev writes). d_out receives len affine points in the same layout, the identity
 * as all zeros; the affine form is canonical, so the result is bit-exact. Scalar 0 gives the
 * identity; the identity base gives all identities.
 * A scalar is recoded to `windows` signed digits of `window_bits` bits and the output is the sum of
 * one table entry per non-zero digit (mixed additions, then one inversion per output). The table,
 * [j 2^(w window_bits)] B for every window w and 1 <= j <= 2^(window_bits - 1), table_points affine
 * points, is built on the device in the context's scratch on the first call with a base and cached
 * per (curve, base): four entries, replaced round-robin, the key compared on the host, so a repeated
 * call with the same base builds nothing. Asynchronous on `stream`; pointers are 16-byte aligned; one
 * B2F_KERNEL_QUOTIENT region per call (the table build, when there is one, inside it); all byte
 * offsets are 64-bit. Errors: B2F_ERR_ARG, with nothing launched and the next good call working, for
 * a null or misaligned pointer, form > 3, len == 0 or len > 2^28, or d_out overlapping d_scalars;
 * B2F_ERR_CHECK at b2f_sync if an affine conversion's inversion fails on a non-identity point (a
 * library defect for an on-curve base, as for b2f_msm_dev); B2F_ERR_HIP for runtime failures,
 * scratch growth included. */
/* out[i] = [s_i] B, i < len */
B2F_API int b2f_fixed_base_mul_dev(b2f_ctx* ctx, const uint64_t h_base[8], const uint64_t* d_scalars,
                                   uint64_t len, uint32_t form, uint64_t* d_out, void* stream);
/* host only: the digit width, the digits of a scalar, the table's points (windows *
 * 2^(window_bits - 1): signed digits store half of them) and the scratch bytes of one cached table;
 * B2F_ERR_ARG, nothing written, where the call would refuse len or form. Any output pointer may be
 * null. */
B2F_API int b2f_fixed_base_plan(uint64_t len, uint32_t form, uint32_t* window_bits, uint32_t* windows,
                                uint64_t* table_points, uint64_t* scratch_bytes);

/* The advice queries of the chip: the (halo2 advice column, rotation) pairs the sixteen gates read
 * (the list at b2f_quotient_gates_dev), as a set, sorted by column then rotation; writes
 * min(count, cap) pairs (column, rotation) and returns count. These are the evaluations of advice
 * columns a prover owes for the custom gates (the permutation and lookup arguments add their
 * own); the fixed columns are all read at rotation 0. halo2 records queries in the order the
 * gates first make them; that order is not modelled, as the combination of selectors is not.
 * Host function. */
B2F_API uint64_t b2f_gate_queries(uint32_t* pairs, uint64_t cap);

/* Per-kernel timing with HIP events recorded on the launch stream around every kernel the
 * fill/eval calls launch (no host synchronization while recording). b2f_set_timing(ctx, 1)
 * clears the log and starts recording; b2f_kernel_times waits for the recorded events and
 * returns, per kernel kind, the summed duration (ms) and the launch count, then clears the
 * log. Kinds: */
#define B2F_KERNEL_RECORD 0 /* BLAKE2f compression + half-round states (fill, part 1) */
#define B2F_KERNEL_FILL 1   /* trace expansion (fill, part 2) */
#define B2F_KERNEL_EVAL 2   /* constraint evaluation */
#define B2F_KERNEL_EXPORT 3 /* Fp export */
#define B2F_KERNEL_FILL_EVAL 4 /* fused trace expansion + constraint evaluation */
#define B2F_KERNEL_LOOKUP 5 /* lookup-argument prover columns (all passes of one call) */
#define B2F_KERNEL_PERM 6   /* permutation-argument prover columns (all passes of one call) */
#define B2F_KERNEL_PERM_SIGMA 7 /* permutation keygen: the sigma columns (b2f_permutation_sigma_dev) */
#define B2F_KERNEL_NTT 8    /* NTT of prover columns (table build and all passes of one call) */
#define B2F_KERNEL_QUOTIENT 9 /* quotient terms, the vanishing divide, the Lagrange selectors and the
                                 evaluation / opening calls; the commitments (b2f_msm_dev, b2f_msm_cells_dev);
                                 the IPA rounds (b2f_ipa_*_dev); the group NTT (b2f_group_ntt_dev); the
                                 fixed-base multiples (b2f_fixed_base_mul_dev); the transcript
                                 (b2f_transcript_*_dev) and the one-call opening (b2f_ipa_open_dev) */
#define B2F_NUM_KERNELS 10
/* total_ms and count must each hold b2f_num_kernels() entries (= B2F_NUM_KERNELS of the
 * header the library was built with; it grew from 7 to 8 with B2F_KERNEL_PERM_SIGMA, to 9
 * with B2F_KERNEL_NTT and to 10 with B2F_KERNEL_QUOTIENT): a caller
 * built against another header sizes its buffers from the query, so the library never writes
 * past them. */
B2F_API int b2f_num_kernels(void);
B2F_API int b2f_set_timing(b2f_ctx* ctx, int enable);
B2F_API int b2f_kernel_times(b2f_ctx* ctx, double* total_ms, uint32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* B2F_H */
