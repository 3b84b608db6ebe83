/* bpg.h -- C ABI of libbpg.so, the MI355X (gfx950) block-proof hot path.
 *
 * Drop-in boundary for the path BASELINE.json names: the three entry points of
 * plonky_block_proof_gen (reference: plonky_block_proof_gen/src/proof_gen.rs:39-43, :61-65,
 * :85-89), its prover/verifier state (prover_state.rs:17-20,80-100; verifier_state.rs:19-23,
 * 46-52,56-71) and, one level down, the kernel-shaped operations that a patched
 * PolynomialBatch::from_values / MerkleTree::new / compute_quotient_polys / fri_proof would call
 * (upstream plonky2 @ 265d46a9 -- not in the reference tree; the only in-tree anchors are the call
 * sites proof_gen.rs:44-52, :66-75, :97-103).  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add.
 *
 * Conventions
 *  - plain C types only; device buffers are raw HIP device pointers (uint64_t*), streams are
 *    hipStream_t passed as void* (NULL = the null stream);
 *  - field elements are little-endian u64, canonical (< p = 2^64 - 2^32 + 1) on output; extension
 *    elements are two consecutive u64 (c0, c1), digests four;
 *  - every function returns 0 (BP_OK) or a negative bp_status; the message is in bp_last_error()
 *    (thread-local).  Nothing throws or aborts across the ABI (reference convention:
 *    Result<_, ProofGenError(String)>, proof_gen.rs:16-36);
 *  - inputs are caller-owned and read-only for the call; outputs returned through uint8_t** are
 *    library-allocated and released with bp_free_buffer (reference: results by value, children
 *    borrowed, proof_gen.rs:62-64,86-88);
 *  - a bp_state is immutable after bp_state_build and may be used from many threads at once
 *    (reference: &ProverState shared, proof_gen.rs:40).
 */
#ifndef BPG_H
#define BPG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  BP_OK = 0,
  BP_ERR_ABORTED = -1,       /* abort flag observed (proof_gen.rs:42,51) */
  BP_ERR_INVALID_INPUT = -2, /* malformed IR / proof bytes, non-contiguous children */
  BP_ERR_RANGE = -3,         /* trace taller/shorter than the configured table range (constants.rs:6-18) */
  BP_ERR_DEVICE = -4,        /* HIP error, no gfx950 device, out of device memory */
  BP_ERR_VERIFY = -5,        /* verifier rejected (verifier_state.rs:56-71) */
  BP_ERR_UNSUPPORTED = -6
} bp_status;

const char* bp_last_error(void);
const char* bp_version(void);
/* number of visible HIP devices; negative on error.  Does not initialise a context. */
int bp_device_count(void);
/* Makes host threads SLEEP while they wait for this device (hipDeviceScheduleBlockingSync) instead of
 * spinning.  A prover stream per host thread needs this to use more streams than the host has cores.
 * The mode is decided ONCE per device, by whoever comes first -- this call, or the first worker the
 * library creates on the device (bp_state_build, bp_stark_prove_air) -- and is never changed
 * afterwards: later calls return BP_OK and do nothing.  The mode can only be switched on a device the
 * PROCESS has not used yet (switching it under queues that already carried work makes a later hipFree or
 * hipDeviceSynchronize hang on this ROCm): on a device that is already in use the call leaves the mode
 * alone, and the library's prover threads then wait with a loop of their own -- poll the event, sleep an
 * eighth of the time waited so far between polls -- instead of the runtime's spinning wait (measured on
 * 16 streams: within 1 % of the interrupt-driven rate at 10 % of a core per thread; the runtime's wait
 * keeps every thread at 100 %).  A process that uses the device through another library (PyTorch, ...)
 * may still call this first thing to get interrupt-driven waits. */
int bp_use_blocking_sync(int device);
/* What was decided for the device: 0 nothing yet, 1 host waits sleep, 2 the device was already in use (or
 * configured otherwise) and keeps its mode. */
int bp_host_wait_mode(int device);

/* ------------------------------------------------------------------------------------------
 * L0 -- kernel-shaped operations on device buffers.
 *
 * Data layout in HBM: matrices are COLUMN-MAJOR, column c at base +
 * c*col_stride elements.  "values" are in natural row order.  "coeffs" are stored in
 * BIT-REVERSED order (position bitrev_n(j) holds coefficient j).  LDE evaluations are
 * "coset-major": position t*n + m holds the evaluation at 7 * w_{n*2^r}^(t + 2^r*m); the Merkle
 * leaf index of that row is bitrev_r(t)*n + bitrev_n(m), i.e. exactly upstream's
 * reverse_index_bits order.
 * ------------------------------------------------------------------------------------------ */

/* Buffers of the L0 entries.  A column stride (in elements) may be any value >= the column's length, so a call can
 * work on a slice of a wider arena: the words between the end of one column and the start of the next are never read
 * as data and never written, and nothing before the first column or after the last is touched.  Every output and
 * scratch buffer is written within the size stated for it and nowhere else; input buffers of out-of-place calls are
 * left as they are.  Bad arguments -- a null pointer, a stride shorter than the column, overlapping buffers, too many
 * columns -- are refused with BP_ERR_INVALID_INPUT (bp_last_error() says which) before anything is launched or
 * written. */

/* The K2 entries take at most this many columns per call (the kernels index columns by grid.y); a wider matrix
 * goes in several calls on column ranges. */
#define BP_NTT_MAX_COLS 65535u

/* K2.  plonky2_field fft/ifft semantics on a batch of columns, in place.
 *   dir = BP_NTT_FWD_BR2NAT: coefficients (bit-reversed order) -> values (natural)
 *   dir = BP_NTT_INV_NAT2BR: values (natural) -> coefficients (bit-reversed), includes 1/n
 *   dir = BP_NTT_FWD_NAT / BP_NTT_INV_NAT: natural in, natural out (adds one permutation pass)
 * Inputs may be any u64 (reduced mod p on the way in), outputs are canonical.  n_cols <= BP_NTT_MAX_COLS. */
enum { BP_NTT_FWD_BR2NAT = 0, BP_NTT_INV_NAT2BR = 1, BP_NTT_FWD_NAT = 2, BP_NTT_INV_NAT = 3 };
int bp_ntt_batch(uint64_t* d_cols, uint32_t log_n, uint32_t n_cols, uint64_t col_stride, int dir,
                 void* stream);

/* K2.  The inverse transform out of place (what PolynomialBatch::from_values does first: the values stay, the
 * coefficients, bit-reversed and scaled by 1/n, go to d_coeffs_out).  The two buffers (first column to the end of the
 * last, pad words included) must not overlap, or be the same pointer WITH THE SAME STRIDE (in place: the same
 * columns); the same pointer with two different strides is refused, as is any other overlap.
 * n_cols <= BP_NTT_MAX_COLS. */
int bp_intt_batch(const uint64_t* d_values, uint64_t in_stride, uint64_t* d_coeffs_out, uint64_t out_stride,
                  uint32_t log_n, uint32_t n_cols, void* stream);

/* K2.  PolynomialBatch::from_values / from_coeffs low-degree extension.
 *   d_in: n_cols columns of n values (natural) or, if from_coeffs, n coefficients (bit-reversed);
 *   d_coeffs_out (nullable if from_coeffs): n_cols x n coefficients, bit-reversed; not overlapping d_in, or the same
 *   pointer as d_in with coeffs_stride == in_stride (in place; the same pointer with another stride is refused);
 *   d_lde_out: n_cols x (n << rate_bits), coset-major, overlapping neither.  Strides in elements.
 * Inputs may be any u64 (reduced mod p on the way in), outputs are canonical; overlapping buffers are refused
 * with BP_ERR_INVALID_INPUT.  n_cols <= BP_NTT_MAX_COLS. */
int bp_lde_batch(const uint64_t* d_in, uint64_t in_stride, uint64_t* d_coeffs_out, uint64_t coeffs_stride,
                 uint64_t* d_lde_out, uint64_t lde_stride, uint32_t log_n, uint32_t rate_bits,
                 uint32_t n_cols, int from_coeffs, void* stream);

/* Measurement aid: plain 8-byte-per-lane streaming copy of n words (calibrates PMC byte counters). */
int bp_debug_copy_u64(const uint64_t* d_in, uint64_t* d_out, uint64_t n, void* stream);

/* K1 self-check: every device form of the Goldilocks arithmetic (types.rs:10 fixes the field) on n
 * operand pairs, for tests against big-integer arithmetic.  d_a/d_b: any u64 values (non-canonical
 * allowed); d_out: 15 planes of n canonical words: a*b by the one-element carry chain, in groups of
 * four, in groups of three, by the compiler form; a+b; a-b; the unreduced dot-product accumulator
 * (2*a*b + a*b[first of its group of four]); 7*a; a^-1; the two components of the extension product
 * (a, b) * (b, a^b); then the interleaved group forms the NTT butterflies use: a + canon(b), a - canon(b),
 * canon(a), canon(b). */
int bp_debug_field_ops(const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n, void* stream);
/* The lazily reduced forms of the same arithmetic -- those that return ANY 64-bit representative of the residue -- on n
 * operand pairs, the words stored exactly as the form returns them (NOT canonical), so that a test can see which
 * representative a form hands on.  d_a/d_b: any u64 values; d_out: 12 planes of n words: a*b by the one-element carry
 * chain (plane 0), by the groups of four (1..4: the pair in every slot of its group) and of three (5..7), a + canon(b)
 * (8), a - canon(b) (9), 7*a (10), a^7 by the one-element S-box (11). */
int bp_debug_lazy_forms(const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, uint64_t n, void* stream);
/* The weights with which the quotient of AIR 8 folds its Poseidon gate (csrc/plonk_hash_fold.hpp: the MDS layers act on
 * the alpha powers, once per quotient, not on every row's state) for one pair of canonical challenges, exactly as a
 * quotient's launch leaves them on the device.  d_out: 238 words: for pair p < 118 (the wire of constraint 90 + p and
 * the S-box output that goes with it) the words 2p, 2p + 1 = -C_0[p], -C_1[p], the S-box output's weights under the two
 * challenges; then K_0, K_1.  The call returns when the words are there.  bp_debug_plonk_hash_fold_host: host only, the
 * same words by the recurrences. */
int bp_debug_plonk_hash_fold(const uint64_t alphas[2], uint64_t* d_out, void* stream);
int bp_debug_plonk_hash_fold_host(const uint64_t alphas[2], uint64_t* out);
/* The multiplications by 2^(12k), k = 1..7, of the NTT's shift-only 16-point DFTs (gl::mul_pow2_n) on n words
 * (any u64).  d_out: 21 planes of n canonical words, plane 3(k-1) + f: a * 2^(12k) by the groups of four (f = 0), the
 * groups of three (f = 1) and the one-element form (f = 2). */
int bp_debug_mul_pow2(const uint64_t* d_a, uint64_t* d_out, uint64_t n, void* stream);

/* Tuning knob: the size (rows / nodes / candidates of one launch) from which the hashing kernels put 64 Poseidon
 * states on a wave.  Matrix-core form (default): four sets of 16 states per wave from this size up, two from half of
 * it, one below.  With bp_tune_poseidon_mx(0): one lane per state from this size up, the quad-cooperative kernels
 * (4 lanes per state, DPP exchange) below.  Results are identical either way.  0 (default) = automatic: 2^19 (2^17
 * without the matrix-core form) while fewer than 6 provers (bp_generate_*_proof calls) are at work on the device,
 * 2^13 under load.  A caller that drives the L0 entry points from many streams itself should set 2^13: the library
 * cannot see that load. */
void bp_tune_quad_threshold(uint64_t n_perms);
/* Merkle levels of at most 2048 nodes: 1 (default) = fused, up to 7 levels per launch (LDS hand-down, one-set
 * matrix-core permutation; +2.8 % on the 256-txn block, +3..5 % on 16- and 32-txn shards: fewer launches on every
 * proof's critical path); 0 = one launch per level; -1 = fused only while fewer than 6 provers are at work on the
 * device.  Results are identical. */
void bp_tune_merkle_fused(int mode);
/* With the fused tail on: levels of up to 2^k parents (k = 8..24; 0 = none) also go nine at a time through
 * merkle_subtree_wide_kernel (256 parents per workgroup, four-set waves while a level has 64 or more of them).
 * Results are identical. */
void bp_tune_merkle_wide(int log2_parents);
/* 1 (default): hashing launches at or above the quad threshold use the matrix-core form of the permutation
 * (csrc/poseidon_mx.cuh: the MDS layer as int8 MFMAs on the byte planes of the state); 0: one lane per state.
 * Results are identical either way. */
void bp_tune_poseidon_mx(int on);
/* Sets of 16 states a wave of the matrix-core form carries: 4, 2 or 1 (fewer sets = more waves for the same launch);
 * 0 (default) = by launch size: 4 from the quad threshold up, 2 from half of it, else 1.  Results are identical. */
void bp_tune_poseidon_mx_sets(int sets);
/* The four-set matrix-core kernels take the partial rounds in groups: within a group only the next S-box input (an
 * affine form of the untouched words and the earlier S-box outputs, evaluated by int8 MFMAs on their bytes) is
 * recombined per round, the twelve words once per group (csrc/poseidon_mx.cuh, grp; tools/poseidon_group_model.py).
 * Non-zero (default): all 22 partial rounds in three groups, 8 + 8 + 6; 0: every round by itself.  Results are
 * identical either way. */
void bp_tune_poseidon_grouped(int on);
/* The load-dependent choices -- Poseidon sets per wave by launch size, K5 and the FRI alpha-combination in one pass
 * without partial sums -- follow the number of bp_generate_*_proof calls at work on the device (six or more =
 * loaded): -1 (default).  0 / 1: stated by a caller that drives the L0 / L0.5 entry points from its own threads (the
 * library cannot see that load), or by a test that pins both paths.  Results are identical. */
void bp_tune_assume_loaded(int mode);
/* The recursion-shaped proofs of a transaction -- level k of its seven per-table chains (proof_gen.rs:44-52 proves all
 * tables in one call; upstream shrinks each table's proof through a chain of fixed-shape circuits) -- are proved in
 * lock-step, up to n (1..8, default 8) proofs per batch: seven transcripts stepped together, every kernel launch and every
 * host wait shared.  1 = one proof at a time (round 3's behaviour, for A/B runs).  Results are identical. */
void bp_tune_rec_batch(int n);
/* A prover that is alone on the device (a lone transaction, the last one of a shard) spreads its transaction's seven
 * trace commitments -- which do not depend on each other -- over the streams of up to three idle workers of the state
 * (1, default); 0 = always on the prover's own stream; n > 1 = also while up to n provers are at work (measured: no gain,
 * profiles/r5_block_size_series.txt).  Results are identical. */
void bp_tune_side_lanes(int n);
/* Inside bp_prove_shard / bp_prove_shard_gi / bp_aggregate_proofs a transaction's root proof and the tree's aggregation
 * proofs ride in the spare slot of other transactions' lock-step batches, and what is left at the end of a tree is proved
 * a batch at a time (1, default); 0 = every node is proved where it is started, one proof per chain of launches.  Read
 * once per call.  Results are identical.  (Not listed by bp_debug_tune_state; bp_tune_reset puts it back.) */
void bp_tune_rec_riders(int on);
/* Transactions a thread of bp_prove_shard / bp_prove_shard_gi starts at a time (1 .. 8; 1 = one transaction per thread;
 * 0, the default = by the state: 3 where bp_state_build found fewer hardware queues (GPU_MAX_HW_QUEUES) than the state
 * has prover streams, else 1 -- profiles/txn_groups_ab.txt).
 * A thread that takes n transactions leases n provers whose arenas are neighbours in device memory -- fewer when fewer
 * neighbours are idle at that moment, never waiting for them -- and proves table t of all its transactions as lock-step
 * batches wherever their shapes agree, t = 0..6, every transaction on its own transcript; the recursion chains and the
 * roots follow (bp_tune_rec_group).  bp_config.arena_bytes remains the memory of ONE transaction: a group
 * uses the arenas of the provers it leases, and nothing that is provable alone fails because it was grouped (a batch
 * that would pass a limit is split).  Read once per call.  Results are identical, byte for byte.  (Not listed by
 * bp_debug_tune_state; bp_tune_reset puts it back.) */
void bp_tune_txn_group(int n);
/* How a group's recursion follows its table proofs: 0 (default) = level k of the seven chains of ALL the transactions the
 * lease granted is one lock-step batch -- 7 g proofs on 7 g transcripts, and the riders that fit, 24 at most; a batch
 * that would pass a limit (24 proofs, 672 query indices, the mailbox) is split, never failed --, then level k + 1, then
 * each transaction's root; 1 = one transaction's recursion after the other (batches of seven and a rider: the schedule
 * before this knob, kept for A/B runs).  A lone transaction is the same either way.  Read once per call.  Results are
 * identical, byte for byte.  (Not listed by bp_debug_tune_state; bp_tune_reset puts it back.) */
void bp_tune_rec_group(int mode);
/* Host only: out[b] (b < n) = how many lock-step batches of exactly b recursion-shaped proofs this process has proved
 * since the last reset (sizes beyond n - 1 are not reported; 25 words hold every size); reset != 0 clears the counters
 * after reading them.  out may be null when n is 0 (reset only). */
int bp_debug_rec_batch_histogram(uint64_t* out, uint32_t n, int reset);
/* The witness of a recursion circuit's Poseidon rows (the sponge over its public-input list, its children's Merkle paths,
 * the sponges over their opened rows: independent pieces) is made on the host; a prover that is alone on the device makes
 * the pieces of a lock-step batch on up to n threads (default 7; 1 = on the prover's own thread).  Results are identical. */
void bp_tune_witness_threads(int n);
/* How the library's prover threads wait for the device: 0 (default) = the runtime's wait where it sleeps
 * (bp_host_wait_mode 1), the library's own poll-and-sleep wait where the runtime's would spin (mode 2: a device the
 * process had already used when the library came to it); 1 = always the runtime's wait; 2 = always poll and sleep. */
void bp_tune_host_wait(int mode);
/* The CPU permutation of the Fiat-Shamir transcript (K7 stays on the host): 0 (default) = the AVX2 form of the MDS
 * layer where the CPU has it, 1 = always the scalar form.  Same values either way (tests). */
void bp_tune_host_poseidon(int mode);
/* Host only: that permutation over n states of 12 words (any u64 in, canonical out), in place. */
int bp_debug_poseidon_host(uint64_t* states, size_t n);
/* Measurement knob: 1 = while the device is loaded the quotient kernel spreads the units of the SYNTHETIC AIR over
 * workgroup rows until the launch has 256 workgroups, as it does for the AIRs of the real tables; 0 (default): one pass. */
void bp_tune_k5_spread(int on);
/* Host only: the operand images of one group of K partial rounds starting at round r0 as the device gets them
 * (csrc/poseidon_group.hpp); tests/test_mx_tables.py pins them to tools/poseidon_group_model.py.
 * out_ops: bp_debug_poseidon_group_ops(K) x 1024 bytes, out_cform: 64 i32, out_cmain: 96 i32. */
uint32_t bp_debug_poseidon_group_ops(uint32_t K);
int bp_debug_poseidon_group_tables(uint32_t K, uint32_t r0, uint8_t* out_ops, int32_t* out_cform, int32_t* out_cmain,
                                   int32_t* out_max_plane_sum);

/* Tuning knob for K2: 0 (default; also any other value) = automatic, 1 = never, 2 = wherever a split form exists:
 * transform a 2^13 / 2^14-point block with TWO workgroups that each do half of the stage coupling its halves while
 * loading (csrc/ntt.hip).  Only the inverse direction (values -> coefficients) has a split form; the forward
 * transforms and coset LDEs are not affected.  Results are identical either way. */
void bp_tune_ntt_split(int mode);
/* NTT blocks as three radix-16 passes whose 16-point DFTs are int8 MFMAs on the bytes of the elements
 * (csrc/ntt_mx.cuh): 0 = never (the VALU butterfly kernels everywhere), 1 = 2^12- and 2^13-point blocks, 2 = 2^14-point
 * blocks too, 3 (default, and any value out of range) = 2^13-point blocks while fewer than 6 provers are at work on
 * the device.  Alone on the chip the form is level to +17 %; under the multi-stream block run its register footprint loses 12 %
 * (DESIGN.md section 7).  Results are identical either way. */
void bp_tune_ntt_mx(int mode);
/* Every bp_tune_* knob back to its default (csrc/tune.hpp holds them). */
void bp_tune_reset(void);
/* Host only: the current value of every knob as "name=value\n" lines in a fixed order, NUL-terminated, into buf
 * (cap bytes; BP_ERR_INVALID_INPUT if it does not fit: 512 is plenty). */
int bp_debug_tune_state(char* buf, size_t cap);
/* Host only (no GPU needed): the constants the matrix-core kernels run on, as the device gets them, so that CPU tests
 * can pin them to an independent derivation.  NTT (csrc/ntt_mx.cuh): kind 0 = DIF / 1 = DIT matrix, inverse = root
 * direction; out_a 8192 bytes ([row block 8][lane 64][16] int8, K-chunk 0), out_c 128 i32, out_tw256 4096 u64,
 * out_tw16 256 u64.  Poseidon (csrc/poseidon_mx.cuh): the C-operand table, 30 x 4 x 24 u32. */
int bp_debug_ntt_mx_tables(int kind, int inverse, uint8_t* out_a, int32_t* out_c, uint64_t* out_tw256,
                           uint64_t* out_tw16);
int bp_debug_poseidon_mx_cin(uint32_t* out);

/* K3.  Poseidon-Goldilocks permutation (width 12) on n states of 12 words, in place. */
int bp_poseidon_perm_batch(uint64_t* d_states, uint64_t n, void* stream);

/* K4.  MerkleTree::new(leaves, cap_height) over the rows of a coset-major LDE matrix.
 *   n_leaves = n << rate_bits rows of n_cols elements; leaf digest = hash_or_noop(row).
 *   d_lde: column c at d_lde + c * lde_stride (elements; >= n << rate_bits, refused otherwise);
 *   d_digests: level-order buffer of bp_merkle_digest_words(log_leaves, cap_height) words
 *   (leaf digests in leaf-index order first, ..., the 2^cap_height cap digests last). */
uint64_t bp_merkle_digest_words(uint32_t log_leaves, uint32_t cap_height);
int bp_merkle_commit(const uint64_t* d_lde, uint64_t lde_stride, uint32_t n_cols, uint32_t log_n,
                     uint32_t rate_bits, uint32_t cap_height, uint64_t* d_digests, void* stream);

struct bp_stark_cfg;
/* K5.  The AIRs the library can prove (csrc/air.hpp).  What upstream expresses as `impl Stark for ...`
 * (eval_packed_generic / eval_ext, evaluated by plonky2_evm's compute_quotient_polys, reached from
 * proof_gen.rs:44-52; the seven zkEVM tables of prover_state.rs:85-93, Keccak range constants.rs:12) is here an
 * air_id: 0 = the synthetic AIR of DESIGN.md section 4 (any width), 1 = keccak_f, one round of Keccak-f[1600] per
 * row on 2431 columns, written from FIPS 202 (not upstream's column layout), 2 = logic, one AND / OR / XOR of two
 * 256-bit words per row on 524 columns, 3 = memory, a log of reads and writes sorted by (address, timestamp) on 45
 * columns, 4 = arithmetic, ADD / SUB / LT / GT on 256-bit words with a carry chain on 309 columns, 5 = byte_packing,
 * a big-endian byte sequence and the word it spells on 299 columns, 6 = keccak_sponge, the absorbing side of
 * Keccak-256 (XOR into the rate, chaining, pad10*1) on 2414 columns, 7 = arithmetic_mul, x * y = z + 2^256 w on 1217
 * columns (likewise their own layouts; a transaction's arithmetic table is proven by AIR 4 or by AIR 7: bp_ir_set_arithmetic_mul_air), 8 = plonk, a
 * PLONK-shaped circuit as a table: 135 wires (80 routed), 84 preprocessed constant columns (two gate selectors, two gate
 * constants, 80 sigmas), arithmetic and S-box gates, public inputs bound to the first row and the copy-constraint
 * permutation argument (Z + nine partial products per challenge set) as its auxiliary columns; degree 9, rate_bits 3 -- the
 * proof system of upstream's recursion circuits (CircuitData::prove), not their gate set and not a verifier circuit.  bp_air_describe returns the shape and
 * the constraint list of an AIR as families (first index, count, kind, degree); the list is followed by the constraints
 * of the table's auxiliary columns, its cross-table lookups (csrc/air.hpp, namespace ctl): n_cols / 8 unfiltered running
 * products for the synthetic AIR (a load placeholder), filter + carried input + two filtered running products for
 * keccak_f (the looked side of keccak_sponge -> keccak_f), two filtered running products for keccak_sponge (the looking
 * side), two for byte_packing (the looking side of byte_packing -> memory), a filter and two for memory (the looked
 * side), one constant product for the tables no lookup is built for. */
typedef struct bp_air_family {
  uint32_t first_index, count;
  uint32_t kind;   /* 0 all rows, 1 transition (x (X - g^(n-1))), 2 first row (x L_0), 3 last row (x L_(n-1)) */
  uint32_t degree; /* in the trace polynomials, before the selector */
} bp_air_family;
typedef struct bp_air_desc {
  uint32_t air_id;
  char name[24];
  uint32_t fixed_n_cols;      /* 0: the AIR takes any width */
  uint32_t n_const_max;       /* preprocessed constant columns it can use */
  uint32_t degree;            /* constraint degree: rate_bits must give 2^rate_bits >= degree - 1 */
  uint32_t n_cols, n_aux;     /* for the width asked about */
  uint32_t n_air_constraints, n_ctl_constraints;
  uint32_t n_units;           /* independently evaluable slices of the list (the kernel's grid.y granularity) */
  uint32_t n_families;
  bp_air_family families[24]; /* interleaved families (synthetic AIR, CTL) list the index of their first member */
} bp_air_desc;
uint32_t bp_air_count(void); /* the BUILT-IN AIRs (9); registered programs, below, are not counted */
int bp_air_describe(uint32_t air_id, uint32_t n_cols, uint32_t n_const, uint32_t deg_pow, bp_air_desc* out);

/* Run-time AIRs.  A table's constraints can also be given as DATA: a straight-line program of field operations, which
 * the library validates, registers under an air_id of its own and interprets with one routine (csrc/air_program.hpp)
 * in the three places a built-in AIR is compiled into: the quotient kernel, the CPU verifier and the trace checker.
 * A host that has a constraint system as code traces its evaluation once into such a program.
 *
 * The program: little-endian u64 words.
 *   word 0      magic "BPGAIRP1" (0x3150524941475042)
 *   1 .. 9      n_cols (8 .. 65536), n_const (preprocessed constant columns, 0 .. 4096), n_public (0 .. 4), degree (1 .. 9:
 *               the declared constraint degree; deg_pow of the table's bp_stark_cfg is 1 up to degree 3, else 3),
 *               n_constraints (1 .. 65536), n_families (1 .. 24), n_regs (1 .. 64), n_units (1 .. 256), n_code (1 .. 2^20)
 *   then        n_families x (first_index, count, kind, degree), bp_air_family's fields: the families cover the index
 *               range [0, n_constraints) in order, exactly once (first_index = where the family before ends, count >= 1);
 *               kind 0 .. 3, degree 1 .. the program's; the kind of a constraint is its family's
 *   then        n_units + 1 code offsets: unit u is code words [off[u], off[u + 1]); off[0] = 0, off[n_units] = n_code,
 *               off[u] < off[u + 1]: no unit is empty.
 *               Units are what the kernels spread over grid.y; registers do not live across units.
 *   The program is exactly these 10 + 4 n_families + n_units + 1 + n_code words.
 *   then        n_code code words:  op | dst << 8 | a << 16 | b << 40  (8 / 8 / 24 / 24 bits)
 *                 0 loc dst, a = column      1 nxt dst, a = column (next row)      2 cst dst, a = constant column
 *                 3 pub dst, a = j           4 x dst (the evaluation point)        5 imm dst, the NEXT word = a constant < p
 *                 6 add dst, a, b            7 sub dst, a, b  (a - b)              8 mul dst, a, b     (a, b: registers)
 *                 9 emit: dst = the kind of constraint a's family, a = constraint index, b = register: adds the
 *                   register to constraint a.  An index may be emitted several times (partial sums add), in any order.
 *               dst is a register below n_regs for every operation but emit; an operation above 9 is refused, and so
 *               is an imm whose constant word is not inside its unit; a field an operation does not use (b of a load,
 *               a and b of x and imm) is not looked at.
 * n_regs is bounded by where the device keeps the registers: LDS, 2 KiB a register per 256-lane workgroup, sized from
 * the program's n_regs (64 registers = 128 KiB of the CU's 160 always fit; fewer registers = more workgroups per CU).
 * bp_air_register refuses, with BP_ERR_INVALID_INPUT and a message "word <offset>: ...": bad magic or sizes, a register
 * read before its unit writes it, column / register / constraint indices out of range, a non-canonical immediate, a
 * constraint never emitted, families that do not tile the list, an emit whose kind is not its family's, and a DEGREE
 * violation: degrees are propagated (loc / nxt / cst / x = 1, pub / imm = 0, add / sub = max, mul = sum), every emit
 * must stay within its family's degree and every family within the program's.  A FIRST-ROW or LAST-ROW family is held
 * to less: degree <= 2 in a program of degree <= 3, <= 8 otherwise.  Those constraints are multiplied by L_0 / L_(n-1), of
 * degree n - 1, so a family of degree d leaves a quotient of degree (d + 1)(n - 1) - n, and the 2^rate_bits n quotient
 * coefficients (rate_bits 1 / 3) hold that only for d <= 2^rate_bits: above it an honest proof is rejected.
 *
 * The id: 0x80000000 | (the first four bytes of Keccak-256 of the program's bytes, little-endian) & 0x7fffffff -- the
 * same in every process, so header word 14 of a proof names the program to a verifier elsewhere.  Registering the same
 * program again returns the same id; a different program whose id is taken is refused, never aliased.
 * bp_air_describe answers for a registered id from the program's own tables (n_cols / n_const / deg_pow are ignored).
 * Every entry that takes an air_id takes a registered one: bp_quotient_scratch_words, bp_quotient_eval,
 * bp_air_check_trace(_host), bp_stark_verify_air(_pub), bp_stark_prove_trace.  A registered AIR without ports has the
 * auxiliary column of a table no lookup is built for (one constant running product, as AIR 4 and AIR 7); pub = four
 * words when n_public > 0.  Not built: a registered AIR as one of a transaction's seven tables, and compiling a program
 * to a native kernel at run time.  The program goes to a device once, at its first use there.
 *
 * Lookup ports: the format "BPGAIRP2" (0x3250524941475042).  "BPGAIRP1" stays valid and untouched.  A PORT is a filter f
 * and a tuple t_0 .. t_(n_tuple - 1) of expressions over the row: the rows where f = 1 send (a looking port) or expose
 * (a looked port) their tuple to another table, which bp_stark_prove_table_set links it to.  "BPGAIRP2" is "BPGAIRP1" with
 *   word 10     n_ports (0 .. 8), after the nine header words above (n_units counts the constraint units only; n_regs
 *               covers both kinds of unit)
 *   then        the family table, as above
 *   then        n_ports words: n_tuple of port l (1 .. 128)
 *   then        n_units + n_ports + 1 code offsets: the constraint units, then PORT UNIT l = unit n_units + l
 *   then        n_code code words, with one more operation:
 *                 10 port: dst = slot, a = port index, b = register.  Slot 0 adds the register to the port's filter f,
 *                    slot 1 + j to tuple element t_j.  Partial sums add, in any order, as with emit.
 *   The program is exactly these 11 + 4 n_families + n_ports + n_units + n_ports + 1 + n_code words.
 * Port units may load and compute but not emit; constraint units may not port; port unit l names port l only; every
 * slot 0 .. n_tuple of a port is written at least once and none beyond.
 * What follows from a port is derived by the library, so a program cannot get the product argument wrong.  With the
 * challenge set c = (beta_c, gamma_c), v_c = sum_j beta_c^j t_j and term_c = 1 + f (gamma_c + v_c - 1):
 *   auxiliary columns: 2 n_ports; port l has z_(l,0), z_(l,1) at columns 2l, 2l + 1, z_c[i] = prod_(i' >= i) term_c[i']
 *               (backwards, as every running product here).  n_ports = 0 keeps the single constant product.
 *   constraints: 5 per port after the program's own, at n_constraints + 5l, in AIR 3's order:
 *               all rows f f - f; then for c = 0, 1: transition z_c - z_c' term_c, last row z_c - term_c.
 *               bp_air_describe reports them (n_aux, n_ctl_constraints, five families per port with the degrees
 *               max(1, 2 deg f), 1 + deg f + deg t, max(1, deg f + deg t); where n_families + 5 n_ports > 24 three
 *               interleaved families stand for all ports instead -- (n_constraints, n_ports, all rows),
 *               (n_constraints + 1, 2 n_ports, transition), (n_constraints + 2, 2 n_ports, last row), members of port l
 *               at + 5l and, the second of a port's two, 2 further -- with the largest degree among the ports).
 *   refused:    2 deg f > degree; 1 + deg f + max_j deg t_j > degree; deg f + max_j deg t_j above the first-row / last-row
 *               bound stated above (z - term is a last-row constraint); more than 21 families in a program with ports
 *               (bp_air_desc.families holds both lists); a slot never written or beyond n_tuple; port outside a port unit, or for another port;
 *               emit in a port unit; n_ports > 8; n_tuple outside 1 .. 128.  Each with the word offset, as above.
 * The trace checker is unchanged: it checks the AIR's own constraints only, ports dropped, as for the built-in tables.
 * bp_stark_prove_trace on a program with ports proves it alone: its ports are linked to nothing, their constraints are
 * checked; bp_quotient_eval (d_aux_lde: 2 n_ports columns) and bp_stark_verify_air(_pub) take the id as any other.
 *
 * Log ports and range checks: the format "BPGAIRP3" (0x3350524941475042).  "BPGAIRP1" and "BPGAIRP2" stay valid and
 * untouched: bytes, ids, digests, proofs.  "BPGAIRP3" is "BPGAIRP2" word for word except the port-table word of port l,
 * which is  n_tuple | kind << 32  (any other bit set is refused):
 *   kind 0      a product port, exactly the one above
 *   kind 1      a LOG port whose filter is a bit
 *   kind 2      a LOG port whose filter is a MULTIPLICITY: any field value (the looked side of a range table, which
 *               answers many looking rows with one row; or a looking side that sends a tuple several times)
 * Sizes, limits and the port-unit rules are unchanged, and the id is taken from the bytes as before, so the kinds are part
 * of the digest a table set's transcript observes.  What the library derives from a log port l, with
 * d_c = gamma_c + v_c:
 *   auxiliary columns: the same two, at 2l and 2l + 1: s_(l,c)[i] = sum_(i' >= i) f[i'] / d_c[i'] (backwards, like
 *               every running column here; no helper column; n_aux = 2 n_ports whatever the kinds)
 *   constraints: the same five slots at n_constraints + 5l: slot 0, all rows, f f - f for kind 1 and identically zero
 *               for kind 2; then for c = 0, 1: transition (s_c - s_c') d_c - f, last row s_c d_c - f.
 *               bp_air_describe reports them as for product ports, with the degrees max(1, 2 deg f) for slot 0 (1 for
 *               kind 2's zero slot) and max(1 + deg t, deg f) for the transition and the last-row slots.
 *   refused:    kind 3 or a stray bit in the port word; max(1 + max_j deg t_j, deg f) > degree; the same quantity above
 *               the first-row / last-row bound (s d - f is a last-row constraint: a degree-3 program takes linear tuples
 *               only); for kind 1 also 2 deg f > degree.  Each with the word offset, as above.
 * What a link of log ports MEANS (bp_stark_prove_table_set): for every tuple value, the sum of f over the looking rows
 * that carry it equals the sum of f over the looked rows that carry it.  That every sent tuple is IN the looked table
 * follows only when the looking filters are bits -- a filter of 1 on one row and p - 1 on another sends a tuple the table
 * does not hold and still balances -- which is why kind 1 exists and why the library, not the program's author, adds
 * f f - f.  A range check of k-bit limbs: the limb columns go out through kind-1 ports with tuple (limb), the table
 * exposes a constant column 0 .. 2^k - 1 through a kind-2 port whose filter is a trace column of multiplicities
 * (bp_range_multiplicities makes it); the link may stay inside one table.
 * A pole: a row where d_c = 0 contributes 0 when f = 0 there; where f != 0 the sum has no value, and the prover (or
 * bp_air_port_products) fails with BP_ERR_VERIFY naming the port, the challenge set and the smallest such row.  With
 * challenges drawn from a transcript that is a 2^-64-ish event per row. */
int bp_air_register(const uint64_t* program, size_t n_words, uint32_t* air_id_out);
int bp_air_unregister(uint32_t air_id);
int bp_air_program_digest(uint32_t air_id, uint8_t out[32]); /* Keccak-256 of the registered bytes */

/* K5.  Constraint / quotient evaluation on the extended domain: what compute_quotient_polys does for one table.
 * shape: log_n, n_cols, n_const, deg_pow, rate_bits of the table (the other fields must make a valid
 * configuration: use the values of the proof the quotient belongs to).  The three LDE matrices are
 * column-major and coset-major with column stride n << rate_bits (d_aux_lde: bp_air_desc.n_aux columns; d_const_lde may
 * be NULL when n_const == 0).  ctl = beta0, gamma0, beta1, gamma1; alphas = the two constraint challenges.
 * d_scratch: bp_quotient_scratch_words(air_id, shape) words.  d_qvals_out: [2][n << rate_bits], coset-major:
 * position t*n + m = quotient value at x = 7 * w_{n 2^r}^(t + 2^r m), already divided by Z_H.  Row j of the output is
 *   ( sum_i alphas[j]^(T - 1 - i) * sel_i(x) * c_i(x) ) / Z_H(x),   Z_H(x) = x^n - 1,
 * over the T = n_air_constraints + n_ctl_constraints constraints of bp_air_describe's list in index order (what
 * starky's consumer acc = acc * alpha + c leaves), c_i evaluated on the row at t*n + m with the NEXT row at
 * t*n + ((m + 1) mod n) -- the same coset -- and sel_i by the kind of i's family: 1 (all rows), x - g^-1 (transition),
 * L_0(x) = Z_H(x) / (n (x - 1)) (first row), L_(n-1)(x) = Z_H(x) / (n (g x - 1)) (last row), g = w_n.  The entry takes no
 * public inputs: pub(j) reads zero here (bp_stark_prove_trace and the verifier pass a table's own).
 * One kernel serves every AIR; the random linear combination stays in registers, and a table tall enough to fill
 * the chip is evaluated in one pass without partial sums in HBM. */
uint64_t bp_quotient_scratch_words(uint32_t air_id, const struct bp_stark_cfg* shape);
int bp_quotient_eval(uint32_t air_id, const struct bp_stark_cfg* shape, const uint64_t* d_trace_lde,
                     const uint64_t* d_aux_lde, const uint64_t* d_const_lde, const uint64_t ctl[4],
                     const uint64_t alphas[2], uint64_t* d_scratch, uint64_t* d_qvals_out, void* stream);

/* The running products of a registered program's ports on the trace domain, without a proof around them: what the prover
 * commits as the table's auxiliary columns.  air_id: a registered program with ports (anything else: BP_ERR_INVALID_INPUT).
 * shape, d_trace, stride, d_consts, pub: as bp_air_check_trace's.  ctl = beta0, gamma0, beta1, gamma1.
 * d_aux_out: 2 n_ports columns x 2^log_n words, column stride 2^log_n: port l's z_0 at column 2l, z_1 at 2l + 1; for a
 * log port ("BPGAIRP3") the running sums s_0, s_1 in the same places.  A pole of a log port: BP_ERR_VERIFY (above); the
 * call waits for the stream when the program has a log port. */
int bp_air_port_products(uint32_t air_id, const struct bp_stark_cfg* shape, const uint64_t* d_trace, uint64_t stride,
                         const uint64_t* d_consts, const uint64_t pub[4], const uint64_t ctl[4], uint64_t* d_aux_out, void* stream);

/* Multiplicities for a range-check lookup: over n_cols column-major columns (column c at d_values + c * stride, n_rows
 * words each) counts how often every value of [0, 2^log_range) occurs on the rows the filter keeps, and ADDS the counts
 * to d_mult (2^log_range words: zero them for a fresh count, or call several times to count several groups of columns).
 * d_filter: n_rows words of 0 / 1, one per row for all columns, or NULL = every row.  log_range: 1 .. 24.
 * A value >= 2^log_range on a kept row: BP_ERR_RANGE, and *first_bad (a host word) is the smallest col * n_rows + row
 * that holds one (the in-range values have been counted); otherwise *first_bad = UINT64_MAX.  Values on rows the filter
 * drops are not looked at.  Counts are integer adds: the result does not depend on any order.  The call waits for the
 * stream.  Up to 2^13 values (bp_tune_range_lds_log) are counted in per-workgroup LDS histograms, more with global
 * atomics; a wave adds its most common value once. */
int bp_range_multiplicities(const uint64_t* d_values, uint64_t stride, uint32_t n_cols, uint64_t n_rows, const uint64_t* d_filter,
                            uint32_t log_range, uint64_t* d_mult, uint64_t* first_bad, void* stream);
/* bp_range_multiplicities counts in LDS up to 2^log_range values: 1 .. 14 (default 13); anything else = the default.
 * Results are identical.  (Not listed by bp_debug_tune_state; bp_tune_reset puts it back.) */
void bp_tune_range_lds_log(int log_range);

/* Test entry: the auxiliary columns (bp_air_desc.n_aux of them: helper columns, then the running products; column
 * stride 2^log_n) the prover commits for a BUILT-IN table with a lookup side (AIR 1, 2, 3, 5, 6), from a trace of column
 * stride 2^log_n.  What bp_air_port_products is compared with. */
int bp_debug_air_aux(uint32_t air_id, const struct bp_stark_cfg* shape, const uint64_t* d_trace, const uint64_t ctl[4],
                     uint64_t* d_aux_out, void* stream);

/* The AIR trace checker: which rows of a witness violate which constraints of its AIR, without proving it (upstream's
 * debugging aid check_constraints).  The AIR is evaluated on the TRACE domain: row i with the next row (i + 1) mod n and
 * x = w_n^i; all-rows constraints on every row, transition constraints on every row but n - 1, first-row constraints
 * on row 0, last-row constraints on row n - 1.  Only the AIR's own constraints are checked: not the lookup constraints
 * of its auxiliary columns, not AIR 8's copy constraints.
 * shape: validated exactly as bp_quotient_eval's (a fixed-width AIR's own width; a valid configuration).  d_trace:
 * canonical words, column-major, n_cols columns x 2^log_n rows, column stride `stride` (>= 2^log_n).  d_consts:
 * n_const columns, column stride 2^log_n (AIR 0 with constant columns, AIR 8: bp_plonk_constants), else NULL.  pub:
 * AIR 8's four public inputs, else NULL.
 * Out: *n_violated_rows = how many rows violate a constraint; rows_out[0 .. min(that, max_rows)) = the first of them in
 * row order; viol_out = the violations of those rows in row order, then constraint index (at most max_viol written);
 * *n_viol = how many those rows have in all.  value = the constraint's value before its row selector (the sum of what
 * the evaluator emits for that index); family = its index into bp_air_describe's families, kind its kind.
 * The device entry marks the rows with a kernel (the constraints folded with fresh random challenges, one bit per row)
 * and names the constraints of the first max_rows of them on the host; it allocates its own scratch and returns after
 * the stream has drained.  The _host entry takes host pointers and does everything on the CPU, row by row. */
typedef struct bp_air_violation {
  uint32_t row, constraint, family, kind;
  uint64_t value;
} bp_air_violation;
int bp_air_check_trace(uint32_t air_id, const struct bp_stark_cfg* shape, const uint64_t* d_trace, uint64_t stride,
                       const uint64_t* d_consts, const uint64_t pub[4], uint32_t max_rows, uint64_t* n_violated_rows,
                       uint32_t* rows_out, bp_air_violation* viol_out, uint32_t max_viol, uint32_t* n_viol, void* stream);
int bp_air_check_trace_host(uint32_t air_id, const struct bp_stark_cfg* shape, const uint64_t* trace, uint64_t stride,
                            const uint64_t* consts, const uint64_t pub[4], uint32_t max_rows, uint64_t* n_violated_rows,
                            uint32_t* rows_out, bp_air_violation* viol_out, uint32_t max_viol, uint32_t* n_viol);

/* Witness of AIR 1 (generate_traces is inside the reference's call too, proof_gen.rs:44-52): n = 2^log_n rows x 2431
 * columns (the last one, the lookup's filter, zero), column-major, row r = round r % 24 of permutation r / 24.  d_inputs: [ceil(n / 24)][25] input lanes
 * (any u64; lane x + 5y), or NULL to draw them from `seed` (splitmix64(seed ^ (lane << 32) ^ permutation)). */
int bp_keccak_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of AIR 2 (the logic table: one AND / OR / XOR of two 256-bit words per row): n = 2^log_n rows x 524 columns
 * (the last one, the filter of the lookup keccak_sponge -> logic, zero), column-major.  d_inputs: [n][9] = operation code (0 none = a padding row, 1 and, 2 or, 3 xor;
 * only the low two bits of the word count), then the four 64-bit
 * words of operand 0 and of operand 1, least significant first; or NULL to draw them from `seed`
 * (code = splitmix64(seed ^ (0xFF << 32) ^ row) & 3, word w of operand j = splitmix64(seed ^ ((1 + 4 j + w) << 32) ^ row)). */
int bp_logic_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of AIR 3 (the memory table: a log of reads and writes sorted by address, then timestamp): n = 2^log_n rows x
 * 45 columns (the last one, the lookup's filter, zero), column-major.  d_inputs: [n][11] = is_read, address (< 2^32), timestamp (< 2^32), eight 32-bit value
 * limbs, ALREADY SORTED (the kernel derives the address_changed flag and the gap bits from neighbouring rows; a log
 * that is out of order, or whose reads do not return the previous value, gives a witness the verifier rejects); or NULL
 * for a log drawn from `seed` (four operations per address; csrc/stark_kernels.hip, memory_trace_kernel).
 * Any u64 is accepted.  Outside the ranges above the kernel does what the oracle does: is_read is bit 0 of its word;
 * address, timestamp and value limbs are stored reduced mod p; address_changed compares the 64-bit words; the gap is
 * the 64-bit difference (address' - address - 1 across a change, timestamp' - timestamp - 1 within) taken modulo 2^32.
 * The witness is then rejected at that row (the gap constraint) unless the difference of the STORED values, minus one,
 * is that 32-bit number in the field, i.e. unless the true gap fits: an address step from 3 to 2^32 proves (gap
 * 2^32 - 4), a timestamp step of 2^32 + 1, equal timestamps on one address or a descending address do not
 * (tests/witness_edges.py, tests/test_witness_edges.py, tests/test_gpu_witness_edges.py). */
int bp_memory_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of AIR 4 (the additive part of the arithmetic table: ADD / SUB / LT / GT on 256-bit words as sixteen 16-bit
 * limbs with a carry chain): n = 2^log_n rows x 309 columns, column-major.  d_inputs: [n][9] = operation code (0 none,
 * 1 add, 2 sub, 3 lt, 4 gt; any other 64-bit value: none), then the four 64-bit words of x and of y, least significant first; or NULL to draw them
 * from `seed` (code = splitmix64(seed ^ (0xFE << 32) ^ row) % 5, words as in bp_logic_trace). */
int bp_arithmetic_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of AIR 5 (the byte-packing table: a big-endian sequence of 1..32 bytes and the 256-bit word it spells, what
 * MLOAD_32BYTES / MSTORE_32BYTES move): n = 2^log_n rows x 299 columns, column-major.  d_inputs: [n][6] = word 0:
 * is_read (bit 0) | timestamp << 8; word 1: len (low byte; 0 = a padding row; above 32: 32) | address << 8 -- the 32-bit
 * address and timestamp of the memory operation that moves the word (the lookup byte_packing -> memory sends
 * (is_read, address, timestamp, value limbs) to the memory table; zero when the caller does not care; bits 1..7 of word
 * 0 and bits 40..63 of both words are ignored) --; then the 32
 * byte slots as four 64-bit words (slot i = byte i % 8 of word i / 8; slots from len on are ignored); or NULL to draw
 * them from `seed` (address = row, timestamp = 2 + row). */
int bp_byte_packing_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of AIR 6 (the Keccak sponge table: the absorbing side of Keccak-256, one 136-byte block per row): n =
 * 2^log_n rows x 2414 columns, column-major.  d_inputs: [n][44] = flags (1 full block, 2 final block, 0 or 3 padding row; the low two bits count),
 * message bytes in the block, the block as absorbed (17 words, pad10*1 included), the 25 lanes of the state before the
 * block -- bp_keccak256_sponge_rows makes them for a message; or NULL for one single-block message per row drawn from
 * `seed`.  The kernel computes the XOR and the permutation of every row. */
int bp_keccak_sponge_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of AIR 7 (the multiplicative half of the arithmetic table, a table of its own here: x * y = z + 2^256 w as a
 * 32-column schoolbook product over 16-bit limbs with 21-bit carries; the largest carry any operands produce is
 * 0xFFFEF, out of column 15 of (2^256 - 1)^2, so bit 20 of every carry is zero): n = 2^log_n rows x 1217 columns, column-major.
 * d_inputs: [n][9] = is_mul (bit 0 of the word; 0 = a padding row), the four 64-bit words of x and of y; or NULL to draw them from `seed`. */
int bp_arithmetic_mul_trace(const uint64_t* d_inputs, uint64_t seed, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* Witness of the DIVISION table: DIV and MOD on 256-bit words, one operation per row.  The table has no built-in air_id:
 * its AIR is a constraint program shipped with the Python package (proof_protocol_decoder_amd/arithmetic_div.py, which
 * registers it with bp_air_register; AIRS.md section 2, "Division (a shipped program)", lists the columns).  Every row
 * proves: there are q, r in [0, 2^256) with q y + r = x OVER THE INTEGERS (no wrap modulo 2^256); r < y unless y = 0; res = 0
 * when y = 0 (the EVM's x / 0 = x % 0 = 0), else q under is_div and r under is_mod; at most one flag is set, a row with
 * neither is a padding row (res = 0), and the filter g of the table's one product port, which exposes (is_div, is_mod, the
 * sixteen 16-bit limbs of x, of y, of res), may be 1 only on a row with a flag.
 * n = 2^log_n rows (log_n 4 .. 26, as bp_arithmetic_mul_trace) x 1650 columns, column-major.  d_inputs: [n][9] = word 0:
 * the operation in its low byte (1 div, 2 mod, anything else a padding row, whose other words are ignored) | exposed << 8
 * (bit 8: the row's g; bits 9 .. 63 are ignored); then the four 64-bit words of x and of y, least significant first.  Any
 * u64 is accepted and every 256-bit operand is a valid one: this table has no input a verifier must reject.  There is no
 * seeded draw: d_inputs == NULL is BP_ERR_INVALID_INPUT.
 * Carries: product column k (16-bit limbs) is sum_{i+j=k} q_i y_j + r_k + c_{k-1} = x_k + 2^16 c_k.  q y <= x < 2^256 lets
 * q and y have at most 17 limbs between them, so a column holds at most 8 products that are not zero and c_k <
 * (8 (2^16 - 1)^2 + 2^16 - 1) / (2^16 - 1) = 8 (2^16 - 1) + 1 < 2^19: 19 bits a carry, all of them needed (q = y =
 * 2^128 - 1, r = y - 1 reaches 0x7FFF7 out of column 7).  Only c_0 .. c_14 are columns: c_15 = floor((q y + r) / 2^256) = 0, and columns 16 .. 30 are
 * the one constraint sum_{i+j>=16} q_i y_j = 0 (a sum of non-negative integers below 2^39). */
int bp_arithmetic_div_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* The column map bp_arithmetic_div_trace stores by, 18 words (n_words: the room in `out`, at least 18): n_cols, then the
 * first column of is_div, is_mod, g, z, inv, the x / y / res / q limbs, the x / y / q / r / d bits, the carry bits, the
 * bits per carry, the first column of the r + d + 1 carry bits.  No device is needed.  The program in arithmetic_div.py
 * states the same map a second time; its register() compares the two and refuses to go on when they differ. */
int bp_arithmetic_div_layout(uint32_t* out, size_t n_words);
/* Witness of the MODULAR table: ADDMOD and MULMOD on 256-bit words, one operation per row.  Like the division table it has
 * no built-in air_id: its AIR is a constraint program shipped with the Python package (proof_protocol_decoder_amd/
 * arithmetic_mod.py, which registers it with bp_air_register; AIRS.md section 2, "Modular (a shipped program)", lists the
 * columns).  Every row proves: with U = a + b under is_addmod, U = a b under is_mulmod and U = 0 on a row with neither flag
 * -- OVER THE INTEGERS, 257 and 512 bits, never reduced modulo 2^256 on the way -- there are q in [0, 2^512) and r in
 * [0, 2^256) with U = q M + r, where M = m + z 2^256 and z = [m = 0]; r < m unless m = 0; res = (1 - z) r, which is (a + b)
 * mod m or (a b) mod m, and 0 when m = 0 (the EVM's convention); at most one flag is set, a row with neither is a padding row
 * (res = 0), and the filter g of the table's one product port, which exposes (is_addmod, is_mulmod, the sixteen 16-bit limbs
 * of a, of b, of m, of res: 66 elements), may be 1 only on a row with a flag.
 * The M convention: a zero modulus is divided by as 2^256, so the honest witness there is q = U >> 256, r = U mod 2^256, and
 * no constraint has to switch the left side off (which would cost a degree).
 * n = 2^log_n rows (log_n 4 .. 26) x 2560 columns, column-major.  d_inputs: [n][13] = word 0: the operation in its low byte
 * (1 addmod, 2 mulmod, anything else a padding row, whose other words are ignored) | exposed << 8 (bit 8: the row's g; bits
 * 9 .. 63 are ignored); then the four 64-bit words of a, of b and of m, least significant first.  Any u64 is accepted and
 * every 256-bit operand is a valid one.  There is no seeded draw: d_inputs == NULL is BP_ERR_INVALID_INPUT.
 * Carries: over 16-bit limbs, column k = 0 .. 31 is L_k - R_k + c_{k-1} = 2^16 c_k with L_k = is_mulmod sum_{i+j=k} a_i b_j +
 * is_addmod (a_k + b_k), R_k = sum_{i+j=k} q_i M_j + r_k (M_16 = z), c_{-1} = 0 and no c_31; the products of columns 32 .. 47
 * are the one constraint sum_{i+j>=32} q_i M_j = 0.  The carries are SIGNED: c_k is the left side's own unsigned carry minus
 * the right side's.  The left side has at most 16 products in a column; q M <= U < 2^512 lets q and M have at most 33 limbs
 * between them, so the right side has at most 16 that are not zero: both carries are at most 16 (2^16 - 1) + 1 and
 * |c_k| < 2^20.  The columns hold c_k + 2^20 in 21 bits.  MULMOD (2^256 - 2, 2^255, 2^256 - 1) reaches -0xEFFF1 and MULMOD
 * (2^256 - 1, 2^256 - 1, 0) reaches +0xFFFEF. */
int bp_arithmetic_mod_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* The column map bp_arithmetic_mod_trace stores by, 21 words (n_words: the room in `out`, at least 21): n_cols, then the
 * first column of is_addmod, is_mulmod, g, z, inv, the a / b / m / res / q limbs, the a / b / m / q / r / d bits, the carry
 * bits, the bits per carry, the offset the carry columns add (2^20), the first column of the r + d + 1 carry bits.  No
 * device is needed.  arithmetic_mod.py states the same map a second time; its register() refuses to go on when they differ. */
int bp_arithmetic_mod_layout(uint32_t* out, size_t n_words);
/* Witness of the SHIFT table: SHL, SHR and SAR on 256-bit words, one operation per row.  Like the division and modular tables
 * it has no built-in air_id: its AIR is a constraint program shipped with the Python package (proof_protocol_decoder_amd/
 * arithmetic_shift.py, which registers it with bp_air_register; AIRS.md section 2, "Shift (a shipped program)", lists the
 * columns).  A row holds a shift count s and a value x, both 256-bit words, in the EVM's operand order (shift, value).  Every
 * row proves, OVER THE INTEGERS and with n = s when s < 256: under is_shl res = (x 2^n) mod 2^256, and 0 when s >= 256; under
 * is_shr res = floor(x / 2^n), and 0 when s >= 256; under is_sar, with sign = bit 255 of x, res = floor(x / 2^n) + sign (2^256 -
 * 2^(256 - n)), and sign (2^256 - 1) when s >= 256.  THE WHOLE s DECIDES, not its low byte: z = [s < 256] is proven from the
 * limbs 1 .. 15 and bits 8 .. 15 of limb 0, so a count masked to eight bits has no witness.  At most one flag is set, a row
 * with none is a padding row (the kernel writes s = x = res = 0 there), and the filter g of the table's one product port,
 * which exposes (is_shl, is_shr, is_sar, the sixteen 16-bit limbs of s, of x, of res: 51 elements), may be 1 only on a row with
 * a flag.  Every tuple element is range-checked by the table: s and x by their bits, res as one of the limbs of y (below).
 * The shift: with l = bits 0 .. 3 of s and W = 2^l (SHL) or 2^(16 - l) (SHR, SAR), x_k W = lo_k + 2^16 hi_k per limb, both halves
 * 16 bits, both sides below 2^32; y_k = lo_k + hi_(k-1) (left) or hi_k + lo_(k+1), y_15 = hi_15 + fill (2^16 - W) (right), with
 * fill = is_sar sign, every y_k below 2^16 without a carry; then res_k is the limb of y at the signed limb offset of bits 4 ..
 * 7 of s, zero below limb 0 and 0xFFFF fill above limb 15, and 0xFFFF fill throughout when s >= 256.
 * n = 2^log_n rows (log_n 4 .. 26) x 1143 columns, column-major.  d_inputs: [n][9] = word 0: the operation in its low byte
 * (1 shl, 2 shr, 3 sar, anything else a padding row, whose other words are ignored) | exposed << 8 (bit 8: the row's g; bits
 * 9 .. 63 are ignored); then the four 64-bit words of s and of x, least significant first.  Any u64 is accepted and every
 * 256-bit operand is a valid one.  There is no seeded draw: d_inputs == NULL is BP_ERR_INVALID_INPUT. */
int bp_arithmetic_shift_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* The column map bp_arithmetic_shift_trace stores by, 19 words (n_words: the room in `out`, at least 19): n_cols, then the
 * first column of is_shl, is_shr, is_sar, g, z, inv, fill, W, the s / x / res / y limbs, the one-hot l (16 columns), the
 * one-hot e (31 columns, offset d at + 15 + d), the s / x / lo / hi bits.  No device is needed.  arithmetic_shift.py states
 * the same map a second time; its register() refuses to go on when they differ. */
int bp_arithmetic_shift_layout(uint32_t* out, size_t n_words);
/* Witness of the SIGNED table: SDIV and SMOD on 256-bit words, one operation per row.  Like the other three shipped tables it
 * has no built-in air_id: its AIR is a constraint program shipped with the Python package (proof_protocol_decoder_amd/
 * arithmetic_sdiv.py, which registers it with bp_air_register; AIRS.md section 2, "Signed (a shipped program)", lists the
 * columns).  A row holds x, y and res as 256-bit words in two's complement.  With sx, sy their bits 255 and X = x - sx 2^256,
 * Y = y - sy 2^256, every row proves OVER THE INTEGERS: under is_sdiv res = 0 when Y = 0, else trunc(X / Y) mod 2^256, the
 * quotient ROUNDED TOWARD ZERO (not floored: -7 / 2 is -3), so SDIV(-2^255, -1) is the word 2^255; under is_smod res = 0 when
 * Y = 0, else (X - Y trunc(X / Y)) mod 2^256, the remainder with THE SIGN OF X (not of Y: -7 % 2 is -1); at most one flag is
 * set, a row with neither has res = 0 (the kernel writes the all-zero row with z = 1 there), and the filter g of the table's
 * one product port, which exposes (is_sdiv, is_smod, the sixteen 16-bit limbs of x, of y, of res: 50 elements, the division
 * table's tuple), may be 1 only on a row with a flag.  Every tuple element is range-checked by the table, by bits of its own.
 * How: ax = |X| and ay = |Y|, both at most 2^255, are tied to x and y by a conditional negation over the 16-bit limbs
 * (v_k + w_k + c_{k-1} = 2^16 c_k where the sign is set, w_k = v_k where it is not; sixteen carry bits a chain); q ay + r = ax
 * and r < ay unless y = 0 are the division table's columns, carries and bounds on the magnitudes (19 bits a carry, still all
 * needed: |X| = (2^127 - 1)(2^128 - 1) + 2^128 - 2 over |Y| = 2^128 - 1 reaches 0x77FF8 out of column 7); the magnitude m = 0
 * (y = 0), q (is_sdiv), r (is_smod) and the sign neg = sx xor sy (is_sdiv), sx (is_smod) are columns, and a third such
 * negation gives res from m under neg.  Its last carry bit is free: m + res = 2^256 c_15 has res = m = 0 when c_15 = 0, so
 * -0 = 0 needs no zero test of its own.
 * n = 2^log_n rows (log_n 4 .. 26) x 2499 columns, column-major.  d_inputs: [n][9], bp_arithmetic_div_trace's format = word 0:
 * the operation in its low byte (1 sdiv, 2 smod, anything else a padding row, whose other words are ignored) | exposed << 8
 * (bit 8: the row's g; bits 9 .. 63 are ignored); then the four 64-bit words of x and of y, least significant first.  Any u64
 * is accepted and every 256-bit operand is a valid one.  There is no seeded draw: d_inputs == NULL is BP_ERR_INVALID_INPUT. */
int bp_arithmetic_sdiv_trace(const uint64_t* d_inputs, uint32_t log_n, uint64_t* d_trace_out, void* stream);
/* The column map bp_arithmetic_sdiv_trace stores by, 27 words (n_words: the room in `out`, at least 27): n_cols, then the
 * first column of is_sdiv, is_smod, g, z, inv, neg, the x / y / res / q / ay / m limbs, the x / y / res / ax / ay / q / r / d
 * bits, the carry bits, the bits per carry, the first column of the r + d + 1 carry bits and of the carry bits of x + ax, of
 * y + ay and of m + res.  No device is needed.  arithmetic_sdiv.py states the same map a second time; its register() refuses
 * to go on when they differ. */
int bp_arithmetic_sdiv_layout(uint32_t* out, size_t n_words);
/* Witness of the EXPONENTIATION table: EXP on 256-bit words, ONE EXPONENT BIT PER ROW.  Like the other four shipped tables it
 * has no built-in air_id: its AIR is a constraint program shipped with the Python package (proof_protocol_decoder_amd/
 * arithmetic_exp.py, which registers it with bp_air_register; AIRS.md section 2, "Exponentiation (a shipped program)", lists
 * the columns).  It is the first shipped program whose statement spans rows: an operation is a chain of rows(e) = max(1, bit
 * length of the exponent e) CONSECUTIVE rows, binary exponentiation from the least significant bit.  A row holds the running
 * square p, the running result r, the exponent e still to consume and the chain's final result res.  With bit = e's bit 0
 * every row proves OVER THE INTEGERS m = r p mod 2^256 and s = p p mod 2^256 (truncated schoolbook products over sixteen
 * 16-bit limbs, sixteen carries of 20 bits each, the last one -- discarded -- range-checked like the rest) and out = bit ? m :
 * r; a row whose flag `last` is 0 is followed by p' = s, r' = out, e' = e >> 1, res' = res; a `last` row has e < 2 and res =
 * out; a `first` row has r = 1; the trace's last row has last = 1.  So r p^e = base^exponent mod 2^256 on a first row and after
 * every step, and the row exposed by the table's one product port -- (the sixteen limbs of p, of e, of res: 48 elements), its
 * filter g allowed on a first row only -- states res = base^exponent mod 2^256, THE WHOLE 256-BIT EXPONENT deciding and 0^0 =
 * 1.  A padding row is all zero except last = 1.
 * n = 2^log_n rows (log_n 4 .. 26) x 2003 columns, column-major.  d_ops: [n_ops][9] = word 0: the operation in its low byte
 * (1 exp; any other byte turns the operation's rows into padding rows, its other words ignored) | exposed << 8 (bit 8: the g of
 * the operation's first row; bits 9 .. 63 are ignored); then the four 64-bit words of the base and of the exponent, least
 * significant first.  d_starts: [n_ops + 1], the exclusive prefix sum of the operations' rows(e) -- starts[0] = 0, starts[n_ops]
 * <= n, computed by the caller; rows from starts[n_ops] on are padding.  n_ops = 0 gives an all-padding trace and reads neither
 * array.  One lane per row finds its operation in d_starts by binary search and replays the operation's steps; it reads
 * d_ops[op] for op < n_ops and d_starts[k] for k <= n_ops only and writes its own row only, whatever the arrays hold, and takes
 * `last` from the exponent, so wrong prefix sums yield a trace the checker refuses, not a wrong statement.  NULL d_trace_out,
 * log_n outside 4 .. 26, n_ops > n, and with n_ops > 0 a NULL d_ops or d_starts are BP_ERR_INVALID_INPUT before any launch. */
int bp_arithmetic_exp_trace(const uint64_t* d_ops, uint32_t n_ops, const uint32_t* d_starts, uint32_t log_n, uint64_t* d_trace_out,
                            void* stream);
/* The column map bp_arithmetic_exp_trace stores by, 17 words (n_words: the room in `out`, at least 17): n_cols, then the first
 * column of g, first, last, the p / e / res / r / out limbs, the p / r / e / m / s bits, the carry bits of r p and of p p, the
 * bits per carry.  No device is needed.  arithmetic_exp.py states the same map a second time; its register() refuses to go on
 * when they differ. */
int bp_arithmetic_exp_layout(uint32_t* out, size_t n_words);

/* AIR 8 (plonk): the 85 preprocessed constant columns of the fixed circuit (selectors, gate constants drawn from `seed`,
 * the Poseidon-row selector, the 80 sigmas of its copy permutation), n = 2^log_n rows, column-major, for a circuit that
 *   - hashes a public-input list of pi_len words (1..104) in Poseidon-gate rows 4.. (one permutation per row), and
 *   - walks n_paths Merkle paths of path_depth levels each in Poseidon-gate rows 17.. (n_paths x path_depth <= 96): path p
 *     starts at list words path_pi0 + 8p .. + 3 (a leaf digest) and must arrive at list words path_pi0 + 8p + 4 .. + 7 (a
 *     cap entry); every recursion circuit of the prover state walks one path per child proof (merkle_proofs::
 *     verify_merkle_proof_to_cap of the child's first query into its trace oracle).  Arithmetic rows start at
 *     the first multiple of four past the Merkle rows (20 without paths) and one group of four must fit (2^log_n >= 32);
 * and the circuit's witness, 135 wires: free wires drawn from `seed`, the list pi hashed in rows 4.., its hash in row 0
 * (the four public inputs) and, through copy constraints, in the first arithmetic row; `paths` (NULL when n_paths = 0):
 * per path 1 + 4 path_depth + leaf_len words -- the leaf's position (bit l = "the node of level l is a right child"), the
 * sibling digests from the leaf upward, then (leaf_len > 0: the aggregation and block circuits of a prover state whose
 * recursion shape has the rows for it) the leaf_len words of the opened row, which the circuit hashes in ceil(leaf_len / 8)
 * Poseidon rows per path right after the Merkle rows; their digest is the path's first node and the list's leaf digest.  A witness whose path does not arrive at the list's cap entry is written as it
 * is: its proof is what a verifier rejects.  bp_plonk_trace returns after the stream has run it. */
typedef struct bp_plonk_layout {
  uint32_t pi_len, n_paths, path_depth, path_pi0;
  uint32_t leaf_len; /* 0, or the words of the row each path's leaf digest is the hash of (> 8): the circuit then hashes it too */
} bp_plonk_layout;
int bp_plonk_constants(uint64_t seed, uint32_t log_n, const bp_plonk_layout* layout, uint64_t* d_consts_out, void* stream);
int bp_plonk_trace(const uint64_t* d_consts, uint64_t seed, const uint64_t* pi, const bp_plonk_layout* layout, const uint64_t* paths,
                   uint32_t log_n, uint64_t* d_trace_out, void* stream);

/* K6.  One FRI fold (plonky2 fri::prover::fri_committed_trees: reduce_with_powers(beta) + coset_fft on the
 * folded domain), done in the evaluation domain.  d_values: the layer's n_l << rate_bits extension values
 * (c0, c1 interleaved) on shift * <w_{n_l 2^r}>, coset-major (position t*n_l + m = point index t + 2^r m).
 * d_out: the next layer, (n_l / 2^arity_bits) << rate_bits values on shift^(2^arity_bits) * <...>, same
 * layout.  arity_bits must be 4 (ConstantArityBits(4, 5)). */
int bp_fri_fold(const uint64_t* d_values, uint32_t log_nl, uint32_t rate_bits, uint32_t arity_bits, uint64_t shift,
                const uint64_t beta[2], uint64_t* d_out, void* stream);

/* K8.  Openings (plonky2_evm StarkOpeningSet::new / PolynomialBatch eval): every column polynomial of a
 * bit-reversed coefficient matrix (as bp_lde_batch leaves it; column stride in words) evaluated at one
 * or two extension-field points z0, z1 (z1 may be NULL).  d_pw_scratch: 4 << log_n words.
 * d_out: 4 words per column = (p(z0).c0, p(z0).c1, p(z1).c0, p(z1).c1); the z1 pair is zero when z1 is NULL. */
int bp_openings(const uint64_t* d_coeffs, uint64_t stride, uint32_t log_n, uint32_t n_cols, const uint64_t z0[2],
                const uint64_t z1[2], uint64_t* d_pw_scratch, uint64_t* d_out, void* stream);

/* K9.  Proof-of-work grind (plonky2 fri::prover::fri_proof_of_work): the SMALLEST nonce w such that the
 * Poseidon permutation of `state` with word `pos` (a rate word, < 8) replaced by w has `bits` leading
 * zero bits in output word 7.  Upstream accepts any witness; the minimum makes results reproducible.
 * Synchronous: *nonce_out is valid on return. */
int bp_pow_grind(const uint64_t state[12], uint32_t pos, uint32_t bits, uint64_t* nonce_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * L0.5 -- one table proof on the synthetic AIR: K2-K9 end to end.
 * This is what plonky2_evm's prove_single_table does for one STARK table (reached from
 * proof_gen.rs:44-52); it exists in the ABI so the whole per-table path can be parity-tested
 * against the oracle.  Transcript prologue: observe constants cap (if n_const), observe trace cap,
 * draw 4 CTL challenges.  The witness is generated on the device from (seed, const_seed).
 * *out receives orc-identical proof words (little-endian u64), *out_len their byte length.
 * Accepted (anything else is BP_ERR_INVALID_INPUT before any device work): arity_bits = 4, cap_height 0..8 with
 * log_n + rate_bits >= cap_height (equal: the cap is the leaf level, queries open rows without a path), final_poly_bits
 * 0..8.  A polynomial of 2^d coefficients is folded while d > final_poly_bits, d >= arity_bits and the folded layer's
 * tree still holds a cap (d + rate_bits >= cap_height + arity_bits): the final polynomial (header word 10) has at most
 * 2^10 coefficients -- a tall cap, not final_poly_bits, is what allows the longest.
 * ------------------------------------------------------------------------------------------ */
typedef struct bp_stark_cfg {
  uint32_t log_n, n_cols, n_const, deg_pow, rate_bits, cap_height, num_queries, pow_bits, arity_bits,
      final_poly_bits;
} bp_stark_cfg;
int bp_stark_prove_synthetic(const bp_stark_cfg* cfg, uint64_t seed, uint64_t const_seed, int device,
                             uint8_t** out, size_t* out_len);
/* The same for any built-in AIR (bp_stark_prove_synthetic = air_id 0).  air_id 1 .. 7: n_cols = 2431 / 524 / 45 / 309 / 299 / 2414 / 1217,
 * n_const = 0, deg_pow = 1, rate_bits = 1; const_seed is ignored.  The air_id is header word 14 of the proof. */
int bp_stark_prove_air(uint32_t air_id, const bp_stark_cfg* cfg, uint64_t seed, uint64_t const_seed, int device,
                       uint8_t** out, size_t* out_len);
/* The same table proof from the CALLER's trace on device `device`: canonical words, column-major, n_cols columns x
 * 2^log_n rows, column stride `stride` (>= 2^log_n) -- for a built-in air_id (the bytes are bp_stark_prove_air's when
 * the trace is bp_*_trace(seed)'s) and for a registered one (bp_air_register), which bp_stark_prove_air refuses: there
 * is no witness generator to draw from a seed.  d_consts: n_const columns, stride 2^log_n, or NULL; pub: the four
 * public inputs (AIR 8, programs with n_public > 0), or NULL.  The trace must be complete when the call is made (the
 * library proves on a stream of its own) and is not modified. */
int bp_stark_prove_trace(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* d_trace, uint64_t stride,
                         const uint64_t* d_consts, const uint64_t* pub, int device, uint8_t** out, size_t* out_len);
/* The CPU verifier (csrc/verifier.cpp, what VerifierState::verify runs per proof, verifier_state.rs:56-71) on one
 * table proof of bp_stark_prove_air: same transcript prologue.  const_cap: the 2^cap_height x 4 words of the
 * constants commitment when n_const > 0, else NULL.  Host only; BP_ERR_VERIFY + bp_last_error() on rejection. */
int bp_stark_verify_air(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* const_cap, const uint8_t* proof,
                        size_t len);
/* AIR 8 (plonk) binds four public inputs to its first row: the hash of the proof's public-input list, which the circuit
 * computes in its hash rows.  A lone table proof (bp_stark_prove_air(8, ...)) has the four-word list
 * bp_stark_public_input_list(seed); bp_stark_public_inputs = its hash, what the verifier is given (pub = NULL: four zeros,
 * what every other AIR has). */
void bp_stark_public_inputs(uint64_t seed, uint64_t out[4]);
void bp_stark_public_input_list(uint64_t seed, uint64_t out[4]);
int bp_stark_verify_air_pub(uint32_t air_id, const bp_stark_cfg* cfg, const uint64_t* const_cap, const uint64_t* pub,
                            const uint8_t* proof, size_t len);
/* Table sets: several caller traces, linked port to port, proven on ONE transcript and verified as ONE statement.
 * A member is a registered program with ports, or a built-in AIR with a lookup side, whose ports are its product
 * columns in order (port l = auxiliary columns first_product + 2l + c); filters and tuples as AIRS.md section 3 states:
 *   AIR 1 keccak_f       port 0 (looked): filter g (column 2430); tuple = 50 input limbs, 50 output limbs of the permutation
 *   AIR 2 logic          port 0 (looked): filter g (column 523); tuple = is_and, is_or, is_xor, 8 limbs of input 0, of
 *                        input 1, of the result (27)
 *   AIR 3 memory         port 0 (looked): filter g (column 44); tuple = is_read, address, timestamp, 8 value limbs (11)
 *   AIR 5 byte_packing   port 0 (looking): filter = the row has a length; tuple = is_read, address, timestamp, 8 value limbs
 *   AIR 6 keccak_sponge  port 0 (looking): filter is_full + is_final; tuple = 34 xored rate limbs, 16 capacity limbs, 50
 *                        updated state limbs.  Ports 1 .. 5 (looking, limb group m = port - 1): the same filter; tuple =
 *                        0, 0, 1, limbs 8m .. 8m + 7 of the rate before, of the block, of the xored rate (limbs past the
 *                        34th are zero)
 * The filter column g of a built-in member is whatever the caller's trace holds.  "Looking" and "looked" only say which
 * side of a link a port is on: the identity is symmetric.  A link states, for both challenge sets,
 *   prod over its looking ports of z(first row) = z_looked(first row):
 * the multiset of tuples the looking ports send on their filtered rows is the multiset the looked port exposes.
 * A link of LOG ports (a registered "BPGAIRP3" program's kinds 1 and 2) states the sum instead,
 *   sum over its looking ports of s(first row) = s_looked(first row)
 * (what that means: "Log ports and range checks" above).  A link's ports are all product ports or all log ports -- the
 * ports of a built-in member are product ports -- else it is refused with BP_ERR_INVALID_INPUT naming the link and the
 * port, before a device is touched.  Both ends of a link may be in the same table: a table that range-checks itself.
 * At most 8 tables and 16 links; every port of every member is in exactly one link (an unlinked port or a port named
 * twice is refused, before a device is touched).
 * Transcript: a fresh challenger observes the statement -- "BPGTSET1", n_tables, n_links; per table air_id, log_n,
 * n_cols, n_const, rate_bits and, for a registered id, the eight 32-bit little-endian words of the program's Keccak-256
 * digest; per link n_looking, its looking (table, port) pairs, the looked pair -- then per table the constants cap (if
 * any), the trace cap and four public inputs (zeros without), draws the four lookup challenges, and is threaded through
 * the table proofs in order.  Every trace is committed before the challenges exist.
 * After the proofs every link is checked on the first-row openings: an unbalanced link fails with BP_ERR_VERIFY and a
 * message naming the link's index and both ends, unless flags has BP_SET_SKIP_LINK_CHECK (the container is returned
 * anyway: for showing a verifier an unbalanced set).
 * The container (u64 words): "BPGTSET1" (0x3154455354475042), n_tables, n_links, beta0, gamma0, beta1, gamma1; per link
 * n_looking, its (table, port) pairs, the looked pair; per table air_id, log_n, n_cols, n_words and the proof words.
 * bp_stark_verify_table_set: the statement is the VERIFIER's -- tables (d_trace, stride, d_consts are ignored; pub is
 * read), const_caps (n_tables pointers, NULL where a table has no constant columns; the array may be NULL when none
 * has) and links are the caller's own, never read from the container, whose shape must agree with them.  It re-derives
 * the transcript, compares the challenges, verifies each table from the transcript state it was proven at and checks
 * every link.  Registered members must be registered in the verifying process.  Host only. */
typedef struct bp_set_table {
  uint32_t air_id;
  bp_stark_cfg cfg;
  const uint64_t* d_trace;
  uint64_t stride;
  const uint64_t* d_consts;
  const uint64_t* pub;
} bp_set_table;
typedef struct bp_set_port {
  uint32_t table, port;
} bp_set_port;
typedef struct bp_set_link {
  uint32_t n_looking;
  bp_set_port looking[8];
  bp_set_port looked;
} bp_set_link;
#define BP_SET_SKIP_LINK_CHECK 1u
int bp_stark_prove_table_set(const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links,
                             uint32_t flags, int device, uint8_t** out, size_t* out_len);
int bp_stark_verify_table_set(const bp_set_table* statement, uint32_t n_tables, const uint64_t* const* const_caps,
                              const bp_set_link* links, uint32_t n_links, const uint8_t* proof, size_t len);
/* The pre-flight of a set: what is wrong with its witness, found without proving it (the analogue of
 * bp_check_txn_witness).  The statement and its refusals are bp_stark_prove_table_set's, refused before a device is
 * touched with the same statuses and texts under this entry's name; strides, constants and public inputs are read as the
 * prover reads them.  Nothing is committed or proven; the call returns after the device has finished.
 * BP_OK exactly when bp_stark_prove_table_set on the same arguments would return a container that
 * bp_stark_verify_table_set accepts (up to the soundness error stated below); otherwise BP_ERR_VERIFY, and
 * bp_last_error() names the first finding in this order: tables in index order (a member that violates its OWN AIR: row,
 * constraint and family, in bp_check_txn_witness's words), then links in index order, a bad filter before an unbalanced
 * tuple, both named by table, port and row.  Either way *out holds everything found: every table and every link is
 * checked, not just the first that fails.
 * table[t]: bp_air_check_trace's answer for the member (max_rows = max_viol = 8).
 * link[k], with a port's (f, tuple) on a row being what its port unit computes (next row wrapping at the last row,
 * x = w^i), or for a built-in member the filter and tuple listed above (Keccak-f's input read 23 rows up):
 *   A TUPLE VALUE is the tuple with trailing zeros stripped: (a, b) and (a, b, 0) are one value, as they are to the
 *     proof, whose compression sum_j beta^j t_j cannot tell them apart.  Ends of different tuple lengths may be linked.
 *   BALANCE: for every tuple value, the sum of f over the looking rows that carry it is congruent mod p to the sum of f
 *     over the looked rows that carry it -- the meaning of a log link above; on a product link the filters are bits, the
 *     sums are counts below 2^31 and the congruence is the multiset equality.
 *   n_unbalanced: the tuple values for which that fails.  first_looking_end / first_looking_row: the smallest (end index,
 *     row), lexicographically, among the looking rows with f != 0 that carry an unbalanced value; first_looked_row: the
 *     smallest such row of the looked end; -1 where there is none.  n_looking / n_looked: the rows with f != 0.
 *   BAD FILTER: a row with f outside {0, 1} on an end whose port demands a bit -- a registered program's product port or
 *     kind-1 log port; not a kind-2 port (a multiplicity), not a built-in member (its filter is its own AIR's matter,
 *     reported under table[]).  The smallest (end, row) is reported with the value; the row enters the balance with its f.
 *   holds: balanced and no bad filter.
 * There are no poles here: the balance is over tuples, not over 1 / (gamma + v), so the pre-flight never fails the way
 * bp_air_port_products can.
 * How: the balance is computed on the device (csrc/set_check.hip).  Per call four fresh random challenges; a row's tuple
 * is compressed to v_0, v_1 under two of them and accumulated in a hash table keyed by v_0 (S = sum of +-f,
 * S_1 = sum of +-f v_1, exact integer sums: the report is a function of the inputs alone).  A value balances iff S = S_1 = 0.
 * Two distinct tuple values collide in v_0 with probability about n_tuple N^2 / 2^64 (N rows in the link); a collision of
 * balanced values leaves both sums zero, so there is NO false alarm at any size; a false pass (and a miscount of
 * n_unbalanced by merging) needs that collision and, for the pass, S_1 = 0 on top of it: a second, independent
 * 2^-64-sized coincidence.  Scratch: one allocation of 64 bytes x the power of two >= twice the rows of the largest
 * link's ends; if the device cannot give it, BP_ERR_DEVICE naming the bytes. */
typedef struct bp_set_table_report {
  uint64_t n_violated_rows;      /* of the member's OWN constraints (bp_air_check_trace) */
  uint32_t n_viol, reserved;
  bp_air_violation viol[8];      /* the first rows', row order */
} bp_set_table_report;
typedef struct bp_set_link_report {
  uint32_t holds;                /* balanced and no bad filter on any of its ends */
  uint32_t is_log;
  uint64_t n_looking, n_looked;  /* rows with f != 0 on each side */
  uint64_t n_unbalanced;         /* tuple values whose two sides differ */
  int32_t  first_looking_end;    /* index into link.looking; -1: none */
  int32_t  bad_filter_end;       /* 0 .. n_looking-1: link.looking[i]; n_looking: the looked end; -1: none */
  int64_t  first_looking_row, first_looked_row, bad_filter_row;   /* -1: none */
  uint64_t bad_filter_value;
} bp_set_link_report;
typedef struct bp_set_report { bp_set_table_report table[8]; bp_set_link_report link[16]; } bp_set_report;
int bp_check_table_set(const bp_set_table* tables, uint32_t n_tables, const bp_set_link* links, uint32_t n_links,
                       int device, bp_set_report* out);
/* bp_stark_prove_synthetic keeps one worker (stream + device arena, up to ~100 GB for a 2^20 x 2432
 * table) parked per device between calls, because re-allocating it costs more than the proof.
 * This frees the parked workers. */
void bp_release_cached_memory(void);
void bp_free_buffer(uint8_t* buf);

/* ------------------------------------------------------------------------------------------
 * L1 -- the reference's public API for this path, byte-for-byte shaped.
 *
 *   reference (Rust)                                              this ABI
 *   ProverStateBuilder::default() / set_<t>_circuit_size / build   bp_config_default, bp_state_build
 *     (prover_state.rs:34-53, 55-75, 80-100; constants.rs:6-18)
 *   generate_txn_proof(&ProverState, TxnProofGenIR, abort)         bp_generate_txn_proof
 *     (proof_gen.rs:39-56)
 *   generate_agg_proof(&ProverState, &lhs, &rhs)                   bp_generate_agg_proof
 *     (proof_gen.rs:61-79; is_agg()/intern()/public_values(): proof_types.rs:55-74)
 *   generate_block_proof(&ProverState, Option<&parent>, &agg)      bp_generate_block_proof
 *     (proof_gen.rs:85-110)
 *   VerifierState::from(&ProverState) / build_verifier / verify    bp_verifier_state_*, bp_verify_block_proof
 *     (verifier_state.rs:34-42, 46-52, 56-71)
 *
 * The zkEVM tables and recursion circuits behind those calls are upstream-only, so
 * the work performed is the synthetic txn proof of SURVEY.md section 8(d): 7 table STARKs (one per
 * AllStark table, positional order arithmetic, byte_packing, cpu, keccak, keccak_sponge, logic,
 * memory -- prover_state.rs:85-93), a 3-deep recursion-shaped chain per table and a root proof;
 * an aggregation / block proof is one recursion-shaped proof bound to its children's digests.
 * Byte formats (the reference fixes none: proof_types.rs:12,25,35,46 only derive serde) are defined
 * in DESIGN.md section 6: little-endian u64 words throughout.
 * ------------------------------------------------------------------------------------------ */
#define BP_NUM_TABLES 7

typedef struct bp_config {
  /* per-table supported log2 trace heights, Range<usize> lo..hi, hi exclusive (constants.rs:6-18) */
  uint32_t table_log_lo[BP_NUM_TABLES], table_log_hi[BP_NUM_TABLES];
  /* StarkConfig::standard_fast_config(): rate_bits 1, cap_height 4, 84 queries, 16 PoW bits,
   * ConstantArityBits(4, 5)  [UPSTREAM-UNVERIFIED values, runtime parameters here].  bp_state_build refuses
   * (BP_ERR_INVALID_INPUT, before it looks for a device) a cap taller than the smallest table's tree
   * (table_log_lo + stark_rate_bits < stark_cap_height) or than the recursion shape's, and, with rec_air_id = 8, a
   * shape whose circuits do not fit 2^rec_log_n rows: every Merkle path a circuit walks needs at least one level
   * (table_log_lo + stark_rate_bits > stark_cap_height, rec_log_n + rec_rate_bits > stark_cap_height) and one row per
   * level -- seven paths in the root circuit, 96 Merkle rows at most. */
  uint32_t stark_rate_bits, stark_cap_height, stark_num_queries, stark_pow_bits, arity_bits, final_poly_bits;
  /* CircuitConfig::standard_recursion_config() shaped proofs: 2^13 rows x 135 wires, rate_bits 3, 28 queries; 84
   * preprocessed constant columns (4 gate constants + 80 sigmas) for the PLONK-shaped circuit, which is the default */
  uint32_t rec_log_n, rec_n_cols, rec_n_const, rec_rate_bits, rec_num_queries, rec_pow_bits;
  uint32_t shrink_depth; /* recursion-shaped proofs per table before the root (3; at least 1: the root circuit walks paths of the recursion shape) */
  uint32_t rec_air_id;   /* what the recursion-shaped proofs are proofs OF: 0 = the synthetic AIR on rec_n_cols x rec_n_const
                          * columns (rounds 1-3; 82 constants); 8 (default) = the PLONK-shaped circuit of AIR 8 (csrc/air.hpp: gates by constants,
                          * public inputs bound in-circuit, copy constraints by the permutation argument), which needs
                          * rec_n_cols = 135 and rec_n_const = 84 -- the proof system of upstream's recursion circuits
                          * (prove_aggregation / prove_block, proof_gen.rs:66-75, 97-103), still not a verifier circuit */
  int32_t device;        /* HIP device index */
  uint32_t n_workers;    /* concurrent provers (one HIP stream + arena each) */
  uint64_t arena_bytes;  /* device arena per worker.  A table height inside its configured range is PROVABLE when
                          * the table's working set -- about 8 * 2^log_n * width * (2 + 2^rate_bits) * 1.3 bytes: values,
                          * coefficients, LDE, digests and FRI scratch -- fits here; otherwise the call returns
                          * BP_ERR_DEVICE ("device arena exhausted").  The default ranges are the reference's
                          * (constants.rs:6-18, up to 2^30 rows), the arena is the deployment's choice: 5-6 GiB
                          * holds the S1 transfer-txn shapes, a 2^20 x 2432 table needs ~100 GiB. */
} bp_config;

typedef struct bp_state bp_state;                   /* ProverState (prover_state.rs:17-20) */
typedef struct bp_verifier_state bp_verifier_state; /* VerifierState (verifier_state.rs:19-23) */

void bp_config_default(bp_config* cfg);
int bp_state_build(const bp_config* cfg, bp_state** out); /* "very expensive call" in the reference */
void bp_state_free(bp_state* s);
uint64_t bp_state_device_bytes(const bp_state* s);
/* What bp_state_build found about the environment the state runs in, as text ("" when there is nothing to say; valid
 * until bp_state_free).  Two things are reported.  (1) RUN-TIME PREREQUISITE: one prover = one HIP stream, and ROCm
 * multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues -- 4 unless the environment variable says
 * otherwise, read once when the HIP runtime starts.  With fewer queues than n_workers the provers share queues and
 * serialise; export GPU_MAX_HW_QUEUES >= n_workers (bench.py: 32) before the process's first HIP call.  (2) The
 * host-wait mode the device was left in (bp_host_wait_mode 2: the library's own poll-and-sleep wait is in use). */
const char* bp_state_warnings(const bp_state* s);
/* the configuration the state was built with */
int bp_state_config(const bp_state* s, bp_config* out);

/* abort_flag: nullable; polled between kernel stages (Option<Arc<AtomicBool>>, proof_gen.rs:42). */
int bp_generate_txn_proof(const bp_state* s, const uint8_t* ir, size_t ir_len, const volatile int32_t* abort_flag,
                          uint8_t** out, size_t* out_len);
/* generate_txn_proof (proof_gen.rs:39-56) for a transaction whose Keccak table attests GIVEN hashing work: the
 * IR must carry the Keccak-AIR flag (bp_ir_set_keccak_air) and keccak_inputs are the states that go into the
 * table's permutations (n_perms x 25 lanes; at most 2^log_n / 24 rounded up; the rest of the table is permutations
 * of the all-zero state).  The decoder side derives them from GenerationInputs with bp_keccak256_permutation_inputs
 * over signed_txn and contract_code (decoding.rs:131-145; block_driver.irs_from_generation_inputs). */
int bp_generate_txn_proof_keccak(const bp_state* s, const uint8_t* ir, size_t ir_len, const uint64_t* keccak_inputs,
                                 size_t n_perms, const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len);
/* The general form: witness data for any table that has an AIR, instead of a witness drawn from the seed (the decoder
 * side derives it from GenerationInputs: proof_protocol_decoder_amd/block_driver.py).  A table is given data when its
 * has_* field is non-zero (n may be 0: a table of padding only) and its IR flag is set (bp_ir_set_*_air).  Items beyond
 * n are padding: Keccak permutations of the all-zero state, rows without an operation, and for the memory log reads of
 * the last address at later and later times.  Layouts as for the bp_*_trace entry points, [n][words of an item]: the
 * table above bp_ir_set_*_air lists them (byte_sequences with the address and timestamp of the memory operation each
 * names when the memory table is real too: bp_byte_packing_trace).  When the sponge table and the
 * logic table are both proven by their AIRs the logic table's FIRST rows are not the caller's: rows 5 p + m are the XOR of
 * limbs 8 m .. 8 m + 7 of sponge row p's rate with its block (the lookup keccak_sponge -> logic), for the min(sponge rows,
 * logic rows / 5) sponge rows the table has room for; logic_ops (or seeded operations) follow them, and more operations
 * than fit behind them are BP_ERR_INVALID_INPUT.
 * Given data is CHECKED: the prover does not validate a witness and nothing downstream verifies the table proofs (upstream's
 * root circuit would), so the table proof made from caller-given data is verified on the host before the call goes on;
 * data that does not satisfy the table's AIR (a log that is not a memory, sponge rows that do not chain, ...) returns
 * BP_ERR_VERIFY.  (bp_generate_txn_proof_keccak likewise; every set of permutation inputs satisfies the Keccak-f AIR.) */
typedef struct bp_txn_witness {
  const uint64_t* keccak_inputs;   size_t n_perms;           int has_keccak;
  const uint64_t* logic_ops;       size_t n_logic_ops;       int has_logic;
  const uint64_t* memory_log;      size_t n_memory_ops;      int has_memory;
  const uint64_t* arithmetic_ops;  size_t n_arithmetic_ops;  int has_arithmetic;
  const uint64_t* byte_sequences;  size_t n_byte_sequences;  int has_byte_packing;
  const uint64_t* sponge_rows;     size_t n_sponge_rows;     int has_keccak_sponge;
} bp_txn_witness;
int bp_generate_txn_proof_witness(const bp_state* s, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data,
                                  const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len);
/* What upstream's `prove` yields before the recursion starts (its AllProof; reached from proof_gen.rs:44-52): the seven
 * table proofs of the transaction on their ONE transcript, with the public values and the lookup challenges -- the part of
 * bp_generate_txn_proof that the recursion-shaped proofs then digest.  data: nullable, as for
 * bp_generate_txn_proof_witness.  Bytes (little-endian u64 words): "BPGTABLS", 7, the 13 public values, the four lookup
 * challenges, then per table: air_id, log_n, n_cols, n_words and the table's STARK proof.
 * bp_verify_txn_table_proofs is upstream's verify_proof(all_stark, all_proof, config) on the CPU: every table proof against
 * the shared transcript AND the cross-table lookups between the tables that are proven with their AIRs (csrc/air.hpp,
 * namespace ctl: keccak_sponge -> keccak_f -- what the sponge table hashes is what the Keccak-f table permutes --,
 * byte_packing -> memory -- the word a sequence spells is the memory operation it names): for both challenge sets the looking and the looked running products agree at the first row.  cfg: the STARK parameters only.
 * The same lookup check runs inside every bp_generate_txn_proof* call (upstream's root circuit does it in-circuit): tables
 * that do not form one statement end the call with BP_ERR_VERIFY. */
int bp_generate_txn_table_proofs(const bp_state* s, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data,
                                 const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len);
/* bp_generate_txn_table_proofs for n transactions (IR i at irs + i * ir_stride; data nullable, and so is every
 * data[i]), table t of the transactions whose shapes agree proved in lock-step on one group of provers (bp_tune_txn_group
 * says how; the knob itself is not read, the caller has formed the group).  outs[i] / out_lens[i] are the blobs the single
 * call gives, byte for byte; on a failure -- the first failing transaction's status and message -- nothing is handed out. */
int bp_generate_txn_table_proofs_group(const bp_state* s, const uint8_t* irs, size_t ir_stride, uint32_t n,
                                       const bp_txn_witness* const* data, const volatile uint8_t* abort_flag, uint8_t** outs,
                                       size_t* out_lens);
int bp_verify_txn_table_proofs(const bp_config* cfg, const uint8_t* table_proofs, size_t len);
/* The same with the STATEMENT fixed by the verifier, as upstream's verify_proof has it (all_stark is the verifier's): ir
 * = the transaction's IR; a table whose header names another AIR, height or width than the IR does (e.g. a Keccak-f
 * table relabelled as synthetic, which would drop its constraints and both of its lookups), or public values other than
 * the IR's, is BP_ERR_VERIFY.  bp_verify_txn_table_proofs alone takes air_id / log_n / n_cols and the public values
 * from the blob, i.e. from the prover: its caller must compare that header with what it expects. */
int bp_verify_txn_table_proofs_for(const bp_config* cfg, const uint8_t* ir, size_t ir_len, const uint8_t* table_proofs,
                                   size_t len);
/* The transaction witness pre-flight: what bp_generate_txn_proof_witness would say about the same inputs, without
 * committing or proving anything.  The seven traces are built by the prover's own code (the same refusals, statuses
 * BP_ERR_INVALID_INPUT / BP_ERR_RANGE); every table proven by its AIR is checked row by row (bp_air_check_trace), and
 * the lookups that exist between them (keccak_sponge -> keccak_f, byte_packing -> memory, keccak_sponge -> logic) as
 * links: the tables proven by an AIR are the members, as contiguous traces, and the balance is bp_check_table_set's, by
 * its code (csrc/set_check.hip, one set of fresh challenges per call) and with its soundness.  A bp_witness_lookup's
 * fields are the bp_set_link_report's of the same names, as "Table sets" above defines them; the looking ends of
 * keccak_sponge -> logic are the sponge table's ports 1 .. 5 in order, and first_looking_row is the row of the smallest
 * (end, row) -- the end is not reported.  Status: BP_OK when the prover would accept the data, BP_ERR_VERIFY when it would
 * not -- a given table that violates its AIR (its row and constraint in the message), else the first lookup that does
 * not hold (its first unmatched rows) -- and out holds everything found either way.  Takes one of the state's workers,
 * as a proof call does, on whose stream everything runs.  Scratch: one allocation of 64 bytes x the power of two >= twice
 * the rows of the largest lookup's ends, beside the worker's arena; if the device cannot give it, BP_ERR_DEVICE naming the
 * bytes.
 * Until the lookups were checked as links, their terms were downloaded and matched greedily in a map on the host.  A
 * report differs from that one in two places only.  (1) A tuple value that a looking rows and b looked rows carry with
 * 0 < b < a: the greedy match named the (b + 1)-th looking row (with 0 < a < b: the (a + 1)-th looked row), the balance
 * names the value's first row on both sides.  Where a value is on one side only, or everything balances, the two agree.  (2) keccak_sponge -> logic:
 * first_looking_row was the smallest row over the five ends and is the row of the smallest (end, row); through this
 * entry that lookup balances by construction (the logic table's first rows are derived from the sponge trace), so no
 * input shows it. */
typedef struct bp_witness_table {
  uint32_t checked;            /* 1: the table is proven by its AIR and was checked */
  uint32_t given;              /* 1: made from the caller's data (0: drawn from the seed or derived) */
  uint64_t n_violated_rows;
  uint32_t n_viol;             /* violations in viol[] (the first rows', row order) */
  bp_air_violation viol[8];
} bp_witness_table;
typedef struct bp_witness_lookup {
  uint32_t checked;            /* 1: both tables are proven by their AIRs */
  uint32_t holds;
  uint64_t n_looking, n_looked;  /* rows with f != 0 on each side (keccak_sponge -> logic: over the five ends) */
  int64_t first_looking_row;   /* first looking row whose tuple the looked table does not expose; -1: none */
  int64_t first_looked_row;    /* first looked row nobody asks for; -1: none */
} bp_witness_lookup;
typedef struct bp_witness_report {
  bp_witness_table table[7];   /* by table index (prover_state.rs:85-93) */
  bp_witness_lookup lookup[3]; /* keccak_sponge -> keccak_f, byte_packing -> memory, keccak_sponge -> logic */
} bp_witness_report;
int bp_check_txn_witness(const bp_state* s, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data,
                         bp_witness_report* out);
/* the same for bp_generate_txn_proof_keccak's inputs */
int bp_check_txn_witness_keccak(const bp_state* s, const uint8_t* ir, size_t ir_len, const uint64_t* keccak_inputs,
                                size_t n_perms, bp_witness_report* out);
/* Test entry, host only (no state, no device): what the prover and the pre-flight make of an IR and its witness data
 * (data: nullable) before they touch the GPU -- per table the AIR, width and height the IR's flags select, whether the
 * table is made from the caller's data and how many items of how many words it holds (the table above bp_ir_set_*_air);
 * per lookup of air::ctl::pairs() its two sides and whether it exists for these tables; the sponge rows whose XORs the
 * logic table holds first and the rows the seeded sponge table may absorb in (UINT32_MAX: all).  Every refusal that
 * depends only on the IR, the shapes and which tables are given is this call's too, with the same status and message. */
typedef struct bp_txn_plan_table {
  uint32_t air_id, n_cols, log_n, given, item_words;
  uint64_t capacity;
} bp_txn_plan_table;
typedef struct bp_txn_plan_lookup {
  uint32_t active, looking_table, looking_air, looked_table, looked_air;
} bp_txn_plan_lookup;
typedef struct bp_txn_plan {
  bp_txn_plan_table table[7];
  bp_txn_plan_lookup lookup[3];
  uint32_t logic_covered, sponge_row_limit;
} bp_txn_plan;
int bp_debug_txn_plan(const bp_config* cfg, const uint8_t* ir, size_t ir_len, const bp_txn_witness* data, bp_txn_plan* out);
/* the same call taking the reference's own flag: Arc<AtomicBool> is ONE byte, `flag.as_ptr()` binds here directly */
int bp_generate_txn_proof_u8(const bp_state* s, const uint8_t* ir, size_t ir_len, const volatile uint8_t* abort_flag,
                             uint8_t** out, size_t* out_len);
int bp_generate_agg_proof(const bp_state* s, const uint8_t* lhs, size_t lhs_len, int lhs_is_agg,
                          const uint8_t* rhs, size_t rhs_len, int rhs_is_agg, uint8_t** out, size_t* out_len);
/* parent may be NULL (checkpoint heights, proof_gen.rs:83-84). *b_height = block number of the proof. */
int bp_generate_block_proof(const bp_state* s, const uint8_t* parent, size_t parent_len, const uint8_t* agg,
                            size_t agg_len, uint8_t** out, size_t* out_len, uint64_t* b_height);

int bp_verifier_state_from_prover(const bp_state* s, bp_verifier_state** out);
int bp_verifier_state_build(const bp_config* cfg, bp_verifier_state** out);
/* verifier-only deployment: the three circuit caps (root, agg, block), 4 << stark_cap_height words each */
int bp_verifier_state_from_caps(const bp_config* cfg, const uint64_t* caps, bp_verifier_state** out);
void bp_verifier_state_free(bp_verifier_state* v);
/* CPU only.  BP_ERR_VERIFY with a reason in bp_last_error() when rejected. */
int bp_verify_block_proof(const bp_verifier_state* v, const uint8_t* proof, size_t len);
/* same check for txn / agg containers (not in the reference API; used by tests and the block driver) */
int bp_verify_proof(const bp_verifier_state* v, const uint8_t* proof, size_t len);

/* Serialise a TxnProofGenIR for the synthetic workload; out: BP_IR_WORDS u64. */
#define BP_IR_WORDS 25
#define BP_PV_WORDS 13
int bp_ir_encode(uint64_t block_number, uint64_t txn_number_before, uint64_t gas_used_before,
                 uint64_t gas_used_after, const uint64_t state_root_before[4], uint64_t seed,
                 const uint32_t table_log_n[BP_NUM_TABLES], const uint32_t table_width[BP_NUM_TABLES],
                 uint64_t out_words[BP_IR_WORDS]);
/* A dummy entry (protocol_decoder/src/decoding.rs:484-520, used to pad blocks of 0 or 1 transactions to the two
 * entries an aggregation needs, :304-347): proven like a transaction, but its public values do not
 * advance -- txn_number_after = txn_number_before, gas unchanged, state_root_after = state_root_before. */
int bp_ir_encode_dummy(uint64_t block_number, uint64_t txn_number, uint64_t gas_used, const uint64_t state_root[4],
                       uint64_t seed, const uint32_t table_log_n[BP_NUM_TABLES],
                       const uint32_t table_width[BP_NUM_TABLES], uint64_t ir_out[BP_IR_WORDS]);
/* bp_ir_set_<x>_air marks an encoded IR (a flag above the version byte of word 1) so that one of the transaction's
 * tables is proven with its AIR instead of the synthetic one; the table's width must then be the AIR's.  Tables by their
 * position in upstream's order (prover_state.rs:85-93); the witness is drawn from the seed unless bp_txn_witness gives it:
 *
 *   table          index  setter                        AIR                 flag    width  witness item (u64 words)
 *   arithmetic       0    bp_ir_set_arithmetic_air      4 arithmetic        0x800    309   9: operation, x, y
 *                         bp_ir_set_arithmetic_mul_air  7 arithmetic_mul    0x4000  1217   9: is_mul, x, y (x * y = z + 2^256 w per row)
 *   byte_packing     1    bp_ir_set_byte_packing_air    5 byte_packing      0x1000   299   6: a sequence
 *   cpu              2    -- (always synthetic)
 *   keccak           3    bp_ir_set_keccak_air          1 keccak_f          0x100   2431   25: a permutation's input lanes; one per 24 rows
 *   keccak_sponge    4    bp_ir_set_keccak_sponge_air   6 keccak_sponge     0x2000  2414   44: bp_keccak256_sponge_rows
 *   logic            5    bp_ir_set_logic_air           2 logic             0x200    524   9: operation, in0, in1
 *   memory           6    bp_ir_set_memory_air          3 memory            0x400     45   11: a log entry, sorted by (address, timestamp)
 *
 * A table of 2^log_n rows holds one item per row, the Keccak table ceil(2^log_n / 24).  The arithmetic table is proven by
 * ONE AIR: AIR 4 or, instead, AIR 7 (the multiplicative half of upstream's arithmetic table). */
int bp_ir_set_keccak_air(uint64_t ir[BP_IR_WORDS], int on);
int bp_ir_set_logic_air(uint64_t ir[BP_IR_WORDS], int on);
int bp_ir_set_memory_air(uint64_t ir[BP_IR_WORDS], int on);
int bp_ir_set_arithmetic_air(uint64_t ir[BP_IR_WORDS], int on);
int bp_ir_set_arithmetic_mul_air(uint64_t ir[BP_IR_WORDS], int on);
int bp_ir_set_byte_packing_air(uint64_t ir[BP_IR_WORDS], int on);
int bp_ir_set_keccak_sponge_air(uint64_t ir[BP_IR_WORDS], int on);
/* public values of a proof container: txn_before, txn_after, gas_before, gas_after, root_before[4],
 * root_after[4], block_number */
int bp_proof_public_values(const uint8_t* proof, size_t len, uint64_t pv_out[BP_PV_WORDS], int* kind_out);

/* ------------------------------------------------------------------------------------------
 * Next row: Erigon compact block-witness decoder + state-trie root
 * (protocol_decoder/src/compact/compact_prestate_processing.rs:1240-1281 process_compact_prestate,
 * compact_to_partial_trie.rs:37-165).  Host-only (it is CPU parsing in the reference too).
 * Pinned by the reference's own golden vectors (complex_test_payloads.rs:14-30 and
 * compact_prestate_processing.rs:1439,1483-1492).  Any out-pointer may be NULL.
 * n_accounts_missing_storage counts account leaves whose non-empty storage root has no extracted
 * storage trie (the invariant the reference's test harness asserts, complex_test_payloads.rs:73-90).
 * ------------------------------------------------------------------------------------------ */
int bp_compact_decode(const uint8_t* witness, size_t len, uint8_t* header_version, uint8_t state_root[32],
                      uint32_t* n_accounts, uint32_t* n_storage_tries, uint32_t* n_code,
                      uint32_t* n_accounts_missing_storage);
/* The reference's FULL output of the same call (ProcessedCompactOutput{header, witness_out{tries{state,
 * storage}, code}}, compact_prestate_processing.rs:1243-1281), release with bp_free_buffer:
 *   "BPGCWIT1" | version:u8 | state: len:u32 trie | n_storage:u32 (hashed_addr[32] len:u32 trie)* |
 *   n_code:u32 (code_hash[32] len:u32 bytes)*
 * Storage tries are keyed by HASHED ACCOUNT ADDRESS (the re-keying of compact_to_partial_trie.rs:167-190), lists
 * in ascending key order, integers little-endian.  A trie is its nodes in preorder, one tag byte each:
 *   0x00 empty | 0x01 hash[32] | 0x02 mask:u16 vlen:u32 value child* (present children, nibble order) |
 *   0x03 nkey:u8 nibble[nkey] child | 0x04 nkey:u8 nibble[nkey] vlen:u32 value
 * (leaf values are what the reference inserts: rlp(AccountRlp) for accounts, rlp(value) for storage slots). */
int bp_compact_decode_full(const uint8_t* witness, size_t len, uint8_t** out, size_t* out_len);
/* one instruction per text line; release with bp_free_buffer */
int bp_compact_instructions(const uint8_t* witness, size_t len, uint8_t** text_out, size_t* text_len);
void bp_keccak256(const uint8_t* data, size_t len, uint8_t out[32]);
/* Keccak-256 of `data` and the 25-lane state (lane index x + 5y) that goes into each of its permutations
 * (len / 136 + 1 of them): the rows the Keccak table of a transaction that hashes `data` has to contain.
 * states_out (room for max_perms x 25 words) and digest_out may be NULL; *n_perms_out is always set.  Host only. */
int bp_keccak256_permutation_inputs(const uint8_t* data, size_t len, uint8_t digest_out[32], uint64_t* states_out,
                                    size_t max_perms, size_t* n_perms_out);
/* The same hash as rows of the Keccak sponge table (bp_keccak_sponge_trace): 44 words per 136-byte block.  rows_out
 * may be NULL to count. */
int bp_keccak256_sponge_rows(const uint8_t* data, size_t len, uint8_t digest_out[32], uint64_t* rows_out, size_t max_rows,
                             size_t* n_rows_out);

/* ------------------------------------------------------------------------------------------
 * Next row: the txn IR producer, BlockTrace::into_txn_proof_gen_ir
 * (protocol_decoder/src/processed_block_trace.rs:38-50, 210-332; decoding.rs:81-177, 179-292, 304-347, 356-428):
 * compact pre-image + per-txn account traces -> one GenerationInputs per transaction (minimal partial tries,
 * deltas replayed over the block's trie state, roots after), padded to >= 2 entries with dummies, withdrawals on
 * the last dummy.  Host-only, sequential by nature.  Unpinned by the reference (it has no test for this path);
 * pinned here by invariants (tests/test_decoding.py).  All integers little-endian, U256 as 32 bytes big-endian.
 *
 * in  = "BPGTRAC1" | witness: len:u32 bytes | n_txn:u32 txn* | checkpoint_state_trie_root[32] |
 *       block_metadata: len:u32 bytes | block_hashes: len:u32 bytes (both opaque upstream types, copied through) |
 *       n_withdrawals:u32 (address[20] amount[32])* | n_code:u32 (code_hash[32] len:u32 bytes)*  (CodeHashResolveFunc as a table)
 * txn = n_traces:u32 trace* | byte_code: len:u32 bytes | new_txn_trie_node_byte | new_receipt_trie_node_byte | gas_used:u64
 * trace = address[20] flags:u8 [balance[32]] [nonce[32]] [n:u32 slot[32]*] [n:u32 (slot[32] value[32])*] [code_hash[32] | len:u32 code]
 *       flags: 1 balance, 2 nonce, 4 storage_read, 8 storage_written, 16 code_usage read, 32 code_usage write, 64 self_destructed
 * out = "BPGGENI1" | n:u32 ir* | final_state_root[32]
 * ir  = txn_number_before[32] gas_used_before[32] gas_used_after[32] | has_signed_txn:u8 signed_txn: len:u32 bytes |
 *       n:u32 (address[20] amount[32])* withdrawals | tries: state, transactions, receipts (each len:u32 trie),
 *       n:u32 (hashed_addr[32] len:u32 trie)* storage | trie_roots_after: state[32] transactions[32] receipts[32] |
 *       checkpoint_state_trie_root[32] | n:u32 (code_hash[32] len:u32 bytes)* contract_code | block_metadata | block_hashes
 * Release with bp_free_buffer.
 * ------------------------------------------------------------------------------------------ */
int bp_decode_block_trace(const uint8_t* trace, size_t len, uint8_t** out, size_t* out_len);

/* ------------------------------------------------------------------------------------------
 * GenerationInputs as the prover's input (csrc/gi.cpp).  The reference's generate_txn_proof consumes
 * TxnProofGenIR = GenerationInputs (plonky_block_proof_gen/src/proof_gen.rs:39-43, protocol_decoder/src/types.rs:48,
 * fields as populated at decoding.rs:131-145): ONE entry of what BlockTrace::into_txn_proof_gen_ir emits.  Here: one
 * entry of a "BPGGENI1" buffer (bp_decode_block_trace; a host holding a single GenerationInputs wraps it as a
 * one-entry buffer).  The library derives the 25-word IR -- txn number, gas and the state-root public
 * value threaded entry to entry (bp_gi_chain: what the entries before left; decoding.rs:106-154 threads the same
 * three), the witness seed = Keccak-256(signed_txn | trie roots after | withdrawals) -- and, for the tables proven
 * with their AIRs, the witness of the entry's OWN hashing work: Keccak-256 of signed_txn and of every contract_code
 * entry (and of the hash-referenced nodes of its partial tries) as Keccak-f permutations, sponge rows, and the
 * memory log / byte-packing sequences of the same bytes (AIRS.md section 3).  Table heights grow to hold that work.
 * ------------------------------------------------------------------------------------------ */
#define BP_GI_KECCAK_AIR 1u         /* table 3 proven with the Keccak-f AIR over the entry's hashing work */
#define BP_GI_KECCAK_TRIE_NODES 2u  /* ... which includes the hashing of the entry's partial tries */
#define BP_GI_MEMORY_AIR 4u         /* table 6: the memory log of the hashed bytes */
#define BP_GI_BYTE_PACKING_AIR 8u   /* table 1: the byte-packing sequences of the hashed bytes */
#define BP_GI_KECCAK_SPONGE_AIR 16u /* table 4: the sponge rows absorbing the same strings */
#define BP_GI_LOGIC_AIR 32u         /* table 5: the logic AIR, holding the sponge rows' XORs first (keccak_sponge -> logic; needs the sponge flag) */
typedef struct bp_gi_options {
  uint64_t block_number;
  uint32_t table_log_n[BP_NUM_TABLES];  /* base heights (the tables that hold given work grow beyond them as needed) */
  uint32_t table_width[BP_NUM_TABLES];  /* widths of the tables that stay synthetic */
  uint32_t flags;                       /* BP_GI_* */
} bp_gi_options;
typedef struct bp_gi_chain {            /* where an entry starts: what the entries before it left */
  uint64_t txn_number, gas_used, state_root[4];
} bp_gi_chain;
int bp_gi_count(const uint8_t* geni, size_t len, uint32_t* n_entries);
/* chain before entry 0: counters 0, state root = the first entry's state-trie root folded into four field elements */
int bp_gi_chain_start(const uint8_t* geni, size_t len, bp_gi_chain* chain);
/* the IR of entry `entry` given the chain before it (heights as the prover will use them); *chain moves past the entry */
int bp_gi_entry_ir(const uint8_t* geni, size_t len, uint32_t entry, const bp_gi_options* opt, bp_gi_chain* chain,
                   uint64_t ir_out[BP_IR_WORDS]);
/* generate_txn_proof(&ProverState, GenerationInputs, Option<Arc<AtomicBool>>): entry `entry`, the chain before it in
 * *chain (moved past the entry on success).  abort_flag as in bp_generate_txn_proof_u8. */
int bp_generate_txn_proof_gi(const bp_state* s, const uint8_t* geni, size_t len, uint32_t entry, const bp_gi_options* opt,
                             bp_gi_chain* chain, const volatile uint8_t* abort_flag, uint8_t** out, size_t* out_len);

/* ------------------------------------------------------------------------------------------
 * The shard scheduler (csrc/gi.cpp): all txn proofs of a CONTIGUOUS slice (aggregation needs contiguous ranges,
 * proof_types.rs:23-24) and its aggregation tree on a pool of threads; every aggregation starts the moment both of its
 * children exist and goes AHEAD of the transactions still waiting for a thread.  The reference leaves this to its
 * scheduler (docs/usage_seq_diagrams.md:8-20); bench.py's headline rate is measured through bp_prove_shard.
 * bp_aggregation_plan: entry k = node n + k = (left, right) node ids, leaves are 0..n-1, the last entry is the root;
 *   shape 0 = balanced (adjacent pairs level by level, an odd tail carried up), 1 = pairs then a left-to-right chain.
 *   pairs: room for 2 (n - 1) ids or NULL; returns n - 1, or UINT32_MAX for n = 0 / an unknown shape.
 * bp_run_shard: the scheduler over caller-supplied work (how the CPU tests drive it, and how a host with another
 *   prover behind the same tree would): leaf(ctx, i) makes leaf i, agg(ctx, ...) merges two children; buffers are
 *   malloc()ed by the callee and owned by the scheduler.  root_out: the slice's one proof (the leaf itself when
 *   n = 1).  leaf_out / leaf_len: NULL, or room for n pointers / lengths -- the leaves are then handed to the caller
 *   too (each released with bp_free_buffer).  The first failing node ends the call with its status and message.
 * n_threads = 0: the state's n_workers (bp_run_shard: 1). */
typedef struct bp_shard_options {
  uint32_t n_threads;
  uint32_t tree_shape;
} bp_shard_options;
typedef int (*bp_shard_leaf_fn)(void* ctx, uint32_t index, uint8_t** out, size_t* out_len);
typedef int (*bp_shard_agg_fn)(void* ctx, const uint8_t* lhs, size_t lhs_len, int lhs_is_agg, const uint8_t* rhs, size_t rhs_len,
                               int rhs_is_agg, uint8_t** out, size_t* out_len);
uint32_t bp_aggregation_plan(uint32_t n, uint32_t shape, uint32_t* pairs);
int bp_run_shard(uint32_t n, const bp_shard_options* opt, bp_shard_leaf_fn leaf, bp_shard_agg_fn agg, void* ctx,
                 const volatile uint8_t* abort_flag, uint8_t** root_out, size_t* root_len, uint8_t** leaf_out, size_t* leaf_len);
/* irs: n IRs, ir_stride bytes apart (>= BP_IR_WORDS * 8) */
int bp_prove_shard(const bp_state* s, const uint8_t* irs, size_t ir_stride, uint32_t n, const bp_shard_options* opt,
                   const volatile uint8_t* abort_flag, uint8_t** root_out, size_t* root_len, uint8_t** txn_out, size_t* txn_len);
/* n proofs made elsewhere (txn or aggregation proofs, contiguous in this order: the sub-block proofs gathered from the
 * other ranks) folded into one along the same plan */
int bp_aggregate_proofs(const bp_state* s, const uint8_t* const* proofs, const size_t* lens, uint32_t n, const bp_shard_options* opt,
                        uint8_t** out, size_t* out_len);
/* entries [first, first + n) of a decoded block */
int bp_prove_shard_gi(const bp_state* s, const uint8_t* geni, size_t len, uint32_t first, uint32_t n, const bp_gi_options* gi,
                      const bp_shard_options* opt, const volatile uint8_t* abort_flag, uint8_t** root_out, size_t* root_len,
                      uint8_t** txn_out, size_t* txn_len);

/* state root after one synthetic txn (host-side helper for building a chain of IRs) */
int bp_state_root_after(const uint64_t root_before[4], uint64_t seed, uint64_t txn_number, uint64_t out[4]);

/* Optional HIP-event timing of kernel families on their own streams (bench.py roofline leg).
 * family 0: LDE coset NTT (LDS-resident DIT), 1: inverse NTT (DIF); total_alg_bytes uses the
 * algorithmic byte counts of SURVEY.md section 8(d).  family 2: Merkle leaf hashing (integer-ALU
 * bound): the third output counts Poseidon PERMUTATIONS instead of bytes.  The other HBM-class kernels of
 * section 8(d): 3 FRI fold (16 M (1 + 1/16)), 4 openings (8 n C), 5 FRI alpha-combination (8 n C), 6 auxiliary
 * running products (8 n per column read or written), 7 + air_id the quotient kernel K5 of that AIR (every LDE
 * element read once, two quotient columns written). */
void bp_profile_enable(int on);
void bp_profile_reset(void);
int bp_profile_read(int family, uint64_t* launches, double* total_ms, double* total_alg_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BPG_H */
