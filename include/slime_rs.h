/*
 * slime_rs.h — C-ABI of the MI355X-native Reed-Solomon shard codec that
 * replaces encryptio/slime's internal/rs and internal/rs/gf (Go) behind their
 * unchanged Go API.  Field: GF(p), p = 2^32 - 5, 32-bit symbols
 * (internal/rs/doc.go:1-2, internal/rs/gf/map.go:7).
 *
 * Two layers:
 *   1. Go-API entry points (host memory in, host memory out).  Each one is
 *      what the cgo shim of the corresponding Go function binds (see
 *      INTEGRATION.md).  They validate exactly like the reference and return
 *      a status code; slime_rs_status_string() gives the reference's panic
 *      text, which the shim re-raises with panic().
 *   2. Device-resident batch API (new, additive): plans + layouts over
 *      objects already in HBM, launched on a caller-supplied hipStream_t.
 *      This is the hot path the benchmark measures.
 *
 * Every compute entry point runs on the GPU (HIP kernels for gfx950). There is
 * no CPU fallback: without a usable device they return SLIME_RS_ERR_NO_DEVICE.
 * Host-only entry points (matrix construction, gf scalars) need no device.
 * All functions are thread-safe.
 */
#ifndef SLIME_RS_H
#define SLIME_RS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------
 * Codes 1..8 correspond one-to-one to the reference's panics; the strings
 * returned by slime_rs_status_string() are the reference's exact messages. */
enum slime_rs_status {
  SLIME_RS_OK = 0,
  SLIME_RS_ERR_VARYING_LENGTH = 1, /* "CreateParity called on data chunks of varying length" vector.go:21 */
  SLIME_RS_ERR_LEN_MISMATCH = 2,   /* "RecoverData: len(chunks) != len(indices)"            vector.go:52 */
  SLIME_RS_ERR_EMPTY = 3,          /* "RecoverData: len(chunks) == 0"                       vector.go:56 */
  SLIME_RS_ERR_NO_INDICES = 4,     /* "RecoverData: No indices given"                       vector.go:66 */
  SLIME_RS_ERR_SINGULAR_NONZERO = 5, /* "Couldn't ensure nonzero m[i][i]"                   matrix.go:68 */
  SLIME_RS_ERR_SINGULAR_ONE = 6,   /* "Couldn't ensure one m[i][i]"                         matrix.go:77 */
  SLIME_RS_ERR_SINGULAR_ZERO = 7,  /* "Couldn't ensure zero m[i][j]"                        matrix.go:92 */
  SLIME_RS_ERR_INDEX_RANGE = 8,    /* Go runtime "index out of range" panic                  */
  SLIME_RS_ERR_INVALID_ARG = 9,    /* C-ABI misuse (null pointer, bad shape)                  */
  SLIME_RS_ERR_NO_DEVICE = 10,     /* no usable HIP device: compute calls fail loudly         */
  SLIME_RS_ERR_HIP = 11,           /* HIP runtime error (detail in slime_rs_last_error())     */
  SLIME_RS_ERR_MAPPING_FALLBACK = 12, /* no candidate mapping fits (only with a bounded search) */
  SLIME_RS_ERR_BAD_HASH = 13       /* "bad checksum after reconstruction" (ErrBadHash) multi_store.go:26,244-249 */
};

/* Reference panic message (codes 1..8) or a short description. Static storage. */
const char *slime_rs_status_string(int status);
/* Detail of the last failure on the calling thread ("" if none).  Meaningful
 * only on the thread that made the failing call, before its next call: the
 * *_ex forms return the detail of the call itself instead. */
const char *slime_rs_last_error(void);
/* Library version string. */
const char *slime_rs_version(void);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int slime_rs_device_count(void);

/* Device of a host-memory entry point (CreateParity ... reconstruct, the
 * MapToGF codec).  SLIME_RS_ANY_DEVICE: the library's device pool picks the
 * visible GPU with the fewest calls in flight (ties round-robin), so
 * concurrent callers spread over every GPU of the node (objects are
 * independent: no data exchange between GPUs). */
#define SLIME_RS_ANY_DEVICE (-1)
/* Pin the calling OS thread's host entry points to `device`
 * (SLIME_RS_ANY_DEVICE, the default, returns them to the pool).  Thread-local:
 * callers whose threads migrate between calls (Go) use the *_ex forms. */
int slime_rs_select_device(int device);
/* The calling thread's selection (SLIME_RS_ANY_DEVICE if none): lets a scope
 * that selects a device restore the one it found. */
int slime_rs_selected_device(void);

/* Per-call context of the *_ex entry points, for callers that must not depend
 * on thread-local state between calls (cgo: a goroutine may run consecutive
 * C calls on different OS threads, and concurrent goroutines share threads).
 * Replaces, for these callers, slime_rs_select_device and
 * slime_rs_last_error. */
typedef struct slime_rs_call {
  int device;        /* device ordinal, or SLIME_RS_ANY_DEVICE (the pool picks) */
  char *detail;      /* optional: receives this call's failure detail, NUL-terminated ("" on success) */
  size_t detail_cap; /* bytes at detail (0: no detail wanted) */
} slime_rs_call_t;
/* Kernel form for shards/chunks under 4 GiB (process-wide): 1 =
 * software-pipelined kernels (default), 0 = the non-pipelined forms that
 * larger shards always take.  mode < 0 queries.  Results are identical; the
 * parity tests run both. */
int slime_rs_kernel_pipeline(int mode);
/* Work schedule of the pipelined kernels for k <= 32 (process-wide): 1 =
 * dynamic, waves take units
 * of work from ticket counters, except inside a graph capture, where the
 * static kernels are captured (default); 2 = dynamic inside captures too --
 * the captured launch keeps a counter set for the graph's life (returned to
 * the library when the graph and its execs are destroyed), so a graph holding
 * one must not be replayed by two execs at the same time; 0 = static shares
 * per wave.  mode < 0 queries.  Results are identical; the parity tests run
 * every mode. */
int slime_rs_kernel_schedule(int mode);
/* Wide codes (k >= 33, or 17 <= k <= 32 with k x rows >= 128; up to 32 output
 * rows and k <= 112) on the matrix cores (process-wide): 1 = the exact
 * int8-limb kernel on v_mfma_i32_16x16x64_i8 (default), 0 = the VALU kernels.
 * mode < 0 queries.  Results are identical; the parity tests run both. */
int slime_rs_kernel_matrix_cores(int mode);
/* Second pass of the fused byte encode (writeChunks on device) for need <= 10
 * (process-wide).  The first pass assumes MapToGF's mapping 0; the units it
 * encoded before an object's first word >= p must be redone with 1<<31.
 * 0 = by object size (default): objects of 1 GiB and more (uniform bytes
 * switch in 27% of them) have the first pass also store each mapping-0
 * column's need top bits (need/8 bytes a column of device scratch), and the
 * second pass corrects those units' parity from the bits and the parity
 * itself instead of re-reading the data; smaller objects re-encode the units.
 * 1 = always correct, 2 = always re-encode.  mode < 0 queries.  Results are
 * identical; the parity tests run every mode. */
int slime_rs_switch_bits(int mode);

/* ==== internal/rs/gf ===================================================== */

/* gf.MaxVal = 1<<32 - 5  (internal/rs/gf/map.go:7) */
#define SLIME_GF_MAXVAL 4294967291u
uint32_t slime_gf_max_val(void);
/* gf.MInverse (internal/rs/gf/gf.go:5): in^(p-2) mod p. Host-only. */
uint32_t slime_gf_minverse(uint32_t in);
/* gf.Raise (internal/rs/gf/gf.go:46): x^n mod p, Raise(x,0) = 1. Host-only. */
uint32_t slime_gf_raise(uint32_t x, uint32_t n);

/* gf.MapToGF (internal/rs/gf/map.go:15).  out must hold (len+3)/4 words.
 * Mapping 0 if every big-endian word is < p, else 1<<31 if that fits, else
 * the first fitting value from the library's random candidate stream (the
 * reference draws rand.Uint32(); see slime_gf_seed).  Host memory: runs on
 * the host cores where the bytes are (slime_gf_codec_placement). */
int slime_gf_map_to_gf(const uint8_t *in, uint64_t len, uint32_t *mapping, uint32_t *out);
/* gf.MapToGFWith (internal/rs/gf/map.go:74). out holds (len+3)/4 words. */
int slime_gf_map_to_gf_with(const uint8_t *in, uint64_t len, uint32_t n, uint32_t *out);
/* gf.MapFromGF (internal/rs/gf/map.go:103). out holds 4*count bytes. */
int slime_gf_map_from_gf(uint32_t n, const uint32_t *in, uint64_t count, uint8_t *out);
/* Where the three host-memory codec calls above run (process-wide): 0 = on
 * the host cores, in
 * place on the caller's buffers (AVX2 passes split over the library's copy
 * pool; default -- the codec is a byte swap, an XOR and a compare, and the
 * bytes are in host memory); 1 = through the GPU codec kernels and the pinned
 * staging ring (two PCIe crossings per call).  Device-resident buffers and
 * the fused object entry points always use the GPU codec.  mode < 0 queries.
 * Results are identical; the parity tests run both. */
int slime_gf_codec_placement(int mode);
/* The host codec's instruction set ("avx2" or "scalar"; env
 * SLIME_RS_CODEC_ISA=scalar forces the portable form) and the threads its
 * passes use (the library's copy pool plus the calling thread). */
int slime_gf_codec_info(const char **isa, int *threads);
/* Seed the MapToGF fallback candidate stream (default: std::random_device,
 * like the reference's crypto-seeded math/rand, main.go:128-136). */
void slime_gf_seed(uint64_t seed);

/* ==== internal/rs: matrices (host-only, exact) =========================== */

/* vandermondeMatrix (internal/rs/matrix.go:8): out is (d+p) x d row-major. */
int slime_rs_vandermonde_matrix(int d, int p, uint32_t *out);
/* ParityMatrix (internal/rs/matrix.go:27): out is (d+p) x d row-major. */
int slime_rs_parity_matrix(int d, int p, uint32_t *out);
/* ParityMatrixCached (internal/rs/matrixcache.go:11): *out points at a shared,
 * read-only (d+p) x d matrix that lives for the life of the process. */
int slime_rs_parity_matrix_cached(int d, int p, const uint32_t **out);
/* solveSubIdentity (internal/rs/matrix.go:35), in place on rows x cols. */
int slime_rs_solve_sub_identity(uint32_t *m, int rows, int cols);
/* invertMatrix (internal/rs/matrix.go:112): inv = m^-1, both d x d. */
int slime_rs_invert_matrix(const uint32_t *m, int d, uint32_t *inv);

/* ==== internal/rs: Go-API data entry points (host memory, GPU compute) ===== */

/* CreateParity (internal/rs/vector.go:18).  data[i] points at lens[i] words;
 * out receives lens[0] words (the shim handles Go's `out` reuse rule). */
int slime_rs_create_parity(const uint32_t *const *data, const uint64_t *lens, int ndata, int index,
                           uint32_t *out);
/* All total-ndata parity rows in one pass (the batched form of the
 * reference's per-row loop, multi_store.go:528-531): out[i] receives row
 * ndata+i, each lens[0] words. */
int slime_rs_create_parities(const uint32_t *const *data, const uint64_t *lens, int ndata, int total,
                             uint32_t *const *out);
/* RecoverData (internal/rs/vector.go:50).  chunks[i] has lens[i] words and
 * code-row index indices[i]; out[0..nchunks-1] each receive lens[0] words of
 * data rows 0..nchunks-1.  Only the erased data rows (those not among
 * indices) are computed on the GPU; a surviving data row's inverse row is a
 * unit row, so its output is that chunk mod p, written on the host.  Output
 * rows may overlap the chunks (an in-place repair): survivors an output
 * overlaps are read from copies taken first. */
int slime_rs_recover_data(const uint32_t *const *chunks, const uint64_t *lens, int nchunks, const int *indices,
                          int nindices, uint32_t *const *out);

/* ==== device-resident batch API (hot path) =============================== */

/* Symbol layout of a batch of objects in device memory: shard s of object o
 * starts at base + o*obj_stride + s*shard_stride (uint32 elements). */
typedef struct slime_rs_layout {
  uint64_t obj_stride;
  uint64_t shard_stride;
} slime_rs_layout_t;

typedef struct slime_rs_plan *slime_rs_plan_t;

/* Encode: inputs = src shards 0..need-1, outputs = parity rows need..total-1
 * written to dst shards 0..total-need-1. */
int slime_rs_plan_encode(int device, int need, int total, slime_rs_plan_t *plan);
/* Reconstruct: inputs = src shards have[0..need-1] (code-row indices of the
 * survivors, any order, distinct), outputs = code rows want[0..nwant-1]
 * (data rows < need, or parity rows) written to dst shards 0..nwant-1.
 * Bit-identical to RecoverData (+CreateParity for parity targets). */
int slime_rs_plan_reconstruct(int device, int need, int total, const int *have, const int *want, int nwant,
                              slime_rs_plan_t *plan);
/* Arbitrary rows x k coefficient matrix (host, row-major) applied to src
 * shards in_shards[0..k-1], written to dst shards 0..rows-1. */
int slime_rs_plan_matrix(int device, const uint32_t *coeff, int rows, int k, const int *in_shards,
                         slime_rs_plan_t *plan);
/* Launch the plan over nobj objects of L symbols per shard.  src and dst are
 * device pointers on the plan's device; stream is a hipStream_t (NULL = the
 * null stream).  Asynchronous; capturable into a hipGraph. */
int slime_rs_plan_execute(slime_rs_plan_t plan, const uint32_t *src, slime_rs_layout_t src_layout, uint32_t *dst,
                          slime_rs_layout_t dst_layout, uint64_t L, uint64_t nobj, void *stream);
/* Write output row i to dst shard out_shards[i] instead of shard i (e.g. a
 * repair that writes rebuilt shards back into their erased slots of the
 * source layout, which is also the faster placement on MI355X: DESIGN.md).
 * Only before the plan's first launch (SLIME_RS_ERR_INVALID_ARG after it:
 * launches in flight read the table). */
int slime_rs_plan_set_outputs(slime_rs_plan_t plan, const int *out_shards);
/* Verify: are the stored shards consistent with the plan?  For every object o
 * and every output row i, verify reports how many columns would change if the
 * plan were executed into the compared buffer, and the lowest such column.
 * cmp is read at the plan's output shard indices (slime_rs_plan_set_outputs)
 * and may alias src: the common call is one full-slot layout for both and an
 * encode plan whose outputs are need..total-1.  A column mismatches iff the
 * word the plan would write (the canonical residue) is not bit-identical to
 * the stored word, so a stored non-canonical p+3 where 3 is computed counts;
 * inputs may be any uint32.
 * Results: two device arrays of nobj x rows uint64, row-major [o][i]:
 * mismatches[o][i] the exact count, first[o][i] the lowest mismatching column
 * or UINT64_MAX.  The call initialises both on the stream whenever nobj > 0
 * (also for L == 0), so the caller never clears them and a captured graph
 * re-initialises them on every replay (a linear chain: one initialising kernel
 * node, then one kernel node per 64 plan rows).  Asynchronous; nothing is copied to the host; the call marks
 * the plan as launched.  Reads src and cmp once and uses no scratch memory.
 * Codes of up to 16 inputs take the 4-columns-per-lane kernels; wide codes
 * (k > 16) take the one-column-per-lane form (no matrix-core verify). */
int slime_rs_plan_verify(slime_rs_plan_t plan, const uint32_t *src, slime_rs_layout_t src_layout,
                         const uint32_t *cmp, slime_rs_layout_t cmp_layout, uint64_t L, uint64_t nobj,
                         uint64_t *mismatches, uint64_t *first, void *stream);
/* Shape of a plan: rows written and inputs read per column. */
int slime_rs_plan_shape(slime_rs_plan_t plan, int *rows, int *k);
/* Host copy of the plan's coefficient rows (rows x k, row-major). */
int slime_rs_plan_coefficients(slime_rs_plan_t plan, uint32_t *out);
int slime_rs_plan_destroy(slime_rs_plan_t plan);

/* ---- ragged batches: one launch over objects of different lengths ----------
 * A span places one object: its shard s is read at src + src_off +
 * s*src_shard_stride and written at dst + dst_off + s*dst_shard_stride (all in
 * uint32 elements, shard indices as the plan gives them), L symbols per shard.
 * L == 0 is allowed (the object is skipped). */
typedef struct slime_rs_span {
  uint64_t src_off;          /* uint32 elements from the launch's src to this object's shard 0 */
  uint64_t src_shard_stride; /* elements between its shards in src */
  uint64_t dst_off;          /* the same two for dst */
  uint64_t dst_shard_stride;
  uint64_t L;                /* symbols per shard */
} slime_rs_span_t;

typedef struct slime_rs_batch *slime_rs_batch_t;

/* Host array of nobj spans -> a device-resident work table for plans with k
 * inputs on `device`.  Synchronous.  A batch is bound to (device, k), not to a
 * plan: one batch serves the encode plan and every reconstruct plan of a code.
 * Refused with SLIME_RS_ERR_INVALID_ARG: null arguments, k <= 0, any L of 2^30
 * or more (shards of a ragged batch stay under 4 GiB; slime_rs_plan_execute
 * remains for larger ones), nobj or a work-unit count of 2^32 or more.  nobj
 * == 0, or every L == 0, gives a valid empty batch.  The tables take 64 bytes
 * per object, 8 per unit of up to 1536 (k > 4) or 3072 (k <= 4) columns and 8
 * per column of L % 4. */
int slime_rs_batch_create(int device, int k, const slime_rs_span_t *spans, uint64_t nobj, slime_rs_batch_t *batch);
/* Objects, columns (the sum of L) and work units of a batch; any output may be NULL. */
int slime_rs_batch_info(slime_rs_batch_t batch, uint64_t *nobj, uint64_t *columns, uint64_t *units);
/* Frees the tables with hipFree, which waits for the device (as
 * slime_rs_plan_destroy does): launches in flight finish first.  Not inside a
 * graph capture; a graph that captured a launch of the batch must be destroyed
 * before it. */
int slime_rs_batch_destroy(slime_rs_batch_t batch);
/* out[o][out_idx[i]][b] = sum_j coeff[i][j] * in[o][in_idx[j]][b] for every
 * span o of the batch and b < L_o, in ONE launch; bit-identical to
 * slime_rs_plan_execute run object by object.  Asynchronous.  The launch reads
 * device memory only (the batch's and the plan's tables, src, dst), so it is
 * capturable under exactly the rules of slime_rs_plan_execute
 * (slime_rs_kernel_schedule); it marks the plan as launched.  The plan's k and
 * device must be the batch's (SLIME_RS_ERR_INVALID_ARG).  An empty batch
 * launches nothing and returns 0.  dst may be src with the outputs in each
 * object's own slots; outputs of different objects that overlap each other or
 * another object's inputs are undefined, like overlapping layouts.
 * Forms: plans of up to 16 inputs over 4-byte aligned src and dst run the
 * 4-columns-per-lane kernel (dynamic schedule, or static where
 * slime_rs_plan_execute would take it); wider plans, and bases that are not
 * 4-byte aligned, run one column per lane (correct, not fast: there is no
 * matrix-core or k-template ragged kernel).  Stored chunk bytes take the
 * byte launches below (slime_rs_decode_objects_batch, and the ragged byte
 * encode, slime_rs_encode_objects_batch); what remains out of scope there is
 * matrix-core forms.  A batch made by
 * slime_rs_batch_create_planned is accepted too: its plan indices are ignored
 * here, and its SLIME_RS_NO_PLAN objects are skipped. */
int slime_rs_plan_execute_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint32_t *src, uint32_t *dst,
                                void *stream);

/* ---- plan sets: objects with different erasures repaired in one launch --------
 * A plan set is a device-resident table of several plans with the same k.  A
 * planned batch names one plan of a set per object, and ONE launch applies to
 * every object its own plan: that plan's input shards, coefficient rows and
 * output shards.  The plans of a set may have different row counts.  The use
 * is a repair sweep: after a store dies every affected object misses a
 * different shard, some more than one -- one reconstruct plan per distinct
 * erasure pattern, one set, one launch. */
typedef struct slime_rs_planset *slime_rs_planset_t;

/* plan_of[o] for an intact object: no work, exactly like L == 0. */
#define SLIME_RS_NO_PLAN UINT32_MAX
/* Plans a set may hold (and the bound on a planned batch's nplans). */
#define SLIME_RS_PLANSET_MAX_PLANS (1u << 20)

/* A snapshot of nplans plans in one device table: each plan's rows, k, input
 * indices, coefficient rows and its output indices as slime_rs_plan_set_outputs
 * had set them at this moment.  Synchronous.  The member plans may be
 * destroyed afterwards, and a later slime_rs_plan_set_outputs on one of them
 * does not reach the set; creating a set does not mark them launched.  All
 * plans must be on one device and share k.  SLIME_RS_ERR_INVALID_ARG: null
 * arguments (or a null member), nplans == 0 or above
 * SLIME_RS_PLANSET_MAX_PLANS, mixed k or device, a table of 16 GiB or more.
 * The table takes 64 bytes per plan plus, per plan, its indices padded to 64
 * bytes each and 64 * ceil(k / 16) bytes per row. */
int slime_rs_planset_create(const slime_rs_plan_t *plans, uint32_t nplans, slime_rs_planset_t *set);
/* Plans, k, the most rows of any plan and the highest input / output shard
 * index over the set; any output may be NULL. */
int slime_rs_planset_info(slime_rs_planset_t set, uint32_t *nplans, int *k, uint32_t *max_rows, uint32_t *in_max,
                          uint32_t *out_max);
/* As slime_rs_batch_destroy: hipFree waits for launches in flight; not inside
 * a capture, and after the graphs that captured a launch of the set. */
int slime_rs_planset_destroy(slime_rs_planset_t set);
/* slime_rs_batch_create with a plan index per object: plan_of[o] < nplans (else
 * SLIME_RS_ERR_INVALID_ARG, checked here on the host) is stored in object o's
 * descriptor; plan_of[o] == SLIME_RS_NO_PLAN marks an intact object, which gets
 * no work units and is neither read nor written, exactly like L == 0 (it does
 * not count in slime_rs_batch_info's columns).  nplans is the plan count of the
 * sets the batch will run with, 1..SLIME_RS_PLANSET_MAX_PLANS.  The batch stays
 * usable with slime_rs_plan_execute_batch (see there). */
int slime_rs_batch_create_planned(int device, int k, const slime_rs_span_t *spans, const uint32_t *plan_of,
                                  uint32_t nplans, uint64_t nobj, slime_rs_batch_t *batch);
/* For every span o of the batch with a plan, plan p = plan_of[o] of the set:
 * out[o][out_idx_p[i]][b] = sum_j coeff_p[i][j] * in[o][in_idx_p[j]][b], b <
 * L_o, in ONE launch; bit-identical to slime_rs_plan_execute run object by
 * object with that object's plan.  Asynchronous, and capturable under exactly
 * the rules of slime_rs_plan_execute_batch (static schedule inside captures at
 * slime_rs_kernel_schedule 1, dynamic with a graph-held counter set at 2).
 * The batch must be planned, and its nplans, k and device must equal the
 * set's (SLIME_RS_ERR_INVALID_ARG).  dst == src with every plan's outputs set
 * to its erased shards is the common call: each object is repaired in its own
 * slots.  Forms as slime_rs_plan_execute_batch: k <= 16 over 4-byte aligned
 * bases runs four columns a lane, anything else one column a lane.
 * The byte-slot twin is slime_rs_planset_decode_objects_batch; the ragged byte
 * encode (slime_rs_encode_objects_batch) takes one plan, not a set.  Out of
 * scope: matrix-core forms (matrix-core or k-template planned kernels for wide
 * codes, symbols or bytes), and sets mixing different k. */
int slime_rs_planset_execute_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint32_t *src, uint32_t *dst,
                                   void *stream);

/* ---- ragged verify: scrub objects of different lengths in one launch ----------
 * slime_rs_plan_verify asked of every span of a batch, in ONE launch: inputs
 * are read at src + src_off + in_idx[j]*src_shard_stride, stored rows at cmp +
 * dst_off + out_idx[i]*dst_shard_stride (cmp may be src), L_o columns each.  A
 * column mismatches iff the canonical residue is not bit-identical to the
 * stored word (a stored p+3 where 3 is computed counts); inputs may be any
 * uint32.
 * Results: two device arrays of nobj x rows uint64, row-major [o][i] -- for the
 * set form nobj x max_rows, max_rows as slime_rs_planset_info reports it.
 * first[o][i] is a column inside object o, 0 .. L_o-1, or UINT64_MAX.  The call
 * initialises both arrays on the stream whenever nobj > 0 (one kernel node,
 * as slime_rs_plan_verify); entries of objects with L == 0, of
 * SLIME_RS_NO_PLAN objects and, in the set form, of rows at or past an object's
 * own plan's row count keep the initial values (0, UINT64_MAX).  An empty
 * batch launches nothing but the initialisation.
 * Nothing but the two result arrays is written and no scratch is used.
 * Asynchronous, and capturable under exactly the rules of
 * slime_rs_plan_execute_batch; plans or sets of more than 64 rows run in row
 * blocks of 64, one launch (and one counter set) each.  The single-plan form
 * marks the plan as launched and accepts a planned batch (plan indices
 * ignored, SLIME_RS_NO_PLAN objects skipped); the set form marks nothing.
 * SLIME_RS_ERR_INVALID_ARG: null arguments, a plan or set whose k or device is
 * not the batch's, and for the set form an unplanned batch or one whose nplans
 * differs from the set's.
 * Forms: k <= 16 over 4-byte aligned src and cmp runs four columns a lane,
 * anything else one column a lane (correct, not fast).  The ragged and planned
 * forms of slime_rs_verify_objects are slime_rs_verify_objects_batch and
 * slime_rs_planset_verify_objects_batch below, and what they scrub is written
 * by the ragged byte encode (slime_rs_encode_objects_batch).  Verify tells
 * which rows disagree; which SHARD is wrong is slime_rs_plan_locate_batch
 * below, which takes these mismatch counts as its filter.  Out of scope:
 * matrix-core forms (matrix-core or k-template ragged verify for wide codes). */
int slime_rs_plan_verify_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint32_t *src,
                               const uint32_t *cmp, uint64_t *mismatches, uint64_t *first, void *stream);
int slime_rs_planset_verify_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint32_t *src,
                                  const uint32_t *cmp, uint64_t *mismatches, uint64_t *first, void *stream);

/* ---- ragged byte objects: repair and scrub stored chunks in one launch --------
 * The four ragged launches above over what a store holds: chunk BYTES, every
 * 4-byte word big-endian and XOR-ed with its object's mapping value
 * (MapFromGF; meta.File.MappingValue), as the byte-slot pipeline below reads
 * and writes them.  A batch made by slime_rs_batch_create or
 * slime_rs_batch_create_planned is used as it is: in these launches a span's
 * offsets and strides count 4-byte words of chunk bytes, so chunk c of object
 * o starts at src + 4*(src_off + c*src_shard_stride) bytes and holds 4*L_o
 * bytes (dst and cmp likewise with dst_off, dst_shard_stride).  One batch
 * serves the symbol launches and the byte launches alike.
 * mapping: a device array of the batch's nobj words; mapping[o] may be any
 * uint32 (0, 1<<31 or a random fallback value).  Entries of objects with
 * L == 0 or SLIME_RS_NO_PLAN are not read for their value.
 * Decode: for every object o with work, row i of its plan and b < L_o, with
 * m = mapping[o]: out[o][out_idx[i]] word b = BE(((sum_j coeff[i][j] *
 * (BE(in[o][in_idx[j]] word b) ^ m)) mod p) ^ m) -- bit-identical to
 * slime_rs_decode_objects_chunked run on that object alone with its plan.
 * Input words at or above p after the XOR (corrupt chunks) are accepted and
 * reduced exactly as the uniform byte decode reduces them.  dst may be src
 * with the outputs in each object's own chunk slots: dst == src and every
 * plan's outputs set to its erased chunks is the common call.  The set form
 * takes the plan named by each object's descriptor, as
 * slime_rs_planset_execute_batch does.
 * Verify: slime_rs_verify_objects's rule per span -- a column mismatches iff
 * BE(stored word) != computed ^ m (a stored BE((computed + p) ^ m) counts).
 * The result arrays follow slime_rs_plan_verify_batch and
 * slime_rs_planset_verify_batch in every respect: nobj x rows (set: nobj x
 * max_rows) uint64, first a column inside the object or UINT64_MAX, both
 * initialised by the call whenever nobj > 0, entries of objects without work
 * and of rows past an object's plan keep (0, UINT64_MAX), nothing else
 * written, no scratch, more than 64 rows in row blocks of 64.
 * Asynchronous, and capturable under exactly the rules of
 * slime_rs_plan_execute_batch (static walk inside captures at
 * slime_rs_kernel_schedule 1, dynamic with a graph-held counter set at 2).
 * The single-plan forms mark the plan as launched and accept a planned batch;
 * the set forms mark nothing.  An empty batch launches nothing (verify: only
 * the initialisation).  SLIME_RS_ERR_INVALID_ARG: null arguments -- decode's
 * buffers and every mapping only when the batch has work, verify's buffers
 * and result arrays always, as the symbol twins --, a plan or set whose k or
 * device is not the batch's, and for the set forms an unplanned batch or one
 * whose nplans differs from the set's.
 * Forms: k <= 16 over 4-byte aligned src and dst (cmp) runs four columns a
 * lane on the walks of the symbol launches, with the byte swap and the XOR
 * applied where a tile's registers are consumed; anything else one column a
 * lane (correct, not fast).  Writing such chunks is the ragged byte encode
 * below (slime_rs_encode_objects_batch).  Out of scope: matrix-core forms or
 * k-template ragged byte kernels for wide codes, the host entry points and
 * digests. */
int slime_rs_decode_objects_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint8_t *src, uint8_t *dst,
                                  const uint32_t *mapping, void *stream);
int slime_rs_planset_decode_objects_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint8_t *src,
                                          uint8_t *dst, const uint32_t *mapping, void *stream);
int slime_rs_verify_objects_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint8_t *src,
                                  const uint8_t *cmp, const uint32_t *mapping, uint64_t *mismatches, uint64_t *first,
                                  void *stream);
int slime_rs_planset_verify_objects_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint8_t *src,
                                          const uint8_t *cmp, const uint32_t *mapping, uint64_t *mismatches,
                                          uint64_t *first, void *stream);

/* ---- ragged locate: name the corrupt shards of scrubbed objects ----------------
 * The step between scrub and repair.  Verify reports which parity ROWS of an
 * object disagree; a repair (slime_rs_planset_execute_batch) needs to know
 * which SHARD to rebuild.  With rows >= 2 the code answers that itself: one
 * wrong shard in a column is identified by that column's syndrome.
 * The rule, per column b of object o, for a plan with k inputs and rows output
 * rows c[i][j]: computed_i is the canonical residue of row i over the stored
 * inputs, d_i is set iff the stored word of row i is not bit-identical to
 * computed_i (verify's rule: a stored p+3 where 3 is computed counts), and
 * s_i = (stored_i mod p - computed_i) mod p.  The column is
 *   clean         no d_i set;
 *   output row i  exactly one d_i set: slot k + i;
 *   input j       J = { j : s_0 != 0 and s_i*c[0][j] == s_0*c[i][j] (mod p) for
 *                 all i } has exactly one member: slot j;
 *   unlocated     anything else: slot k + rows.
 * For the plans this library builds (encode and reconstruct plans of the MDS
 * code) a single wrong shard in a column is always named.  TWO OR MORE wrong
 * shards in ONE column are beyond what `rows` syndromes can decide: such a
 * column is reported as unlocated, or, with probability about k/p per such
 * column, blamed on a third shard.  Wrong shards in DIFFERENT columns of one
 * object are each named.  For slime_rs_plan_matrix plans the rule is applied as
 * written, whatever the matrix.
 * Addressing is exactly slime_rs_plan_verify_batch's (and, for the byte form,
 * slime_rs_verify_objects_batch's: symbol = BE(word) ^ mapping[o]): inputs
 * through the span's src side, stored rows through its dst side at the plan's
 * output shards; cmp may be src.  A planned batch is accepted; objects with
 * SLIME_RS_NO_PLAN or L == 0 are skipped.
 * Results: two device arrays of nobj x (k + rows + 1) uint64, row-major:
 * counts[o][slot] is the number of columns blamed on slot, first[o][slot] the
 * lowest such column inside the object or UINT64_MAX.  Slots 0..k-1 are the
 * plan's inputs in its own order, k..k+rows-1 its output rows, k+rows is
 * `unlocated`.  The call initialises both arrays on the stream whenever
 * nobj > 0 (one kernel node, as verify: replays of a captured graph start
 * clean), writes nothing else and uses no scratch.
 * filter: NULL, or the `mismatches` array of a preceding verify of the same
 * plan and batch on the same stream (nobj x rows).  An object whose `rows`
 * entries are all zero is passed over without reading its data and keeps the
 * initial values; NULL scans every object.  The filter is read on the device:
 * verify followed by locate is one capturable chain with no host round trip.
 * Asynchronous, and capturable under the rules of slime_rs_plan_verify_batch
 * (the walk is static in every schedule mode: no counter set is taken).  Marks
 * the plan as launched.  SLIME_RS_ERR_INVALID_ARG: null arguments (filter may
 * be NULL), a plan whose k or device is not the batch's, rows < 2 (one parity
 * row cannot tell which shard is wrong), k + rows > 63 (a wave's running tally
 * keeps one slot per lane).
 * Forms: k <= 16 over 4-byte aligned src and cmp runs four columns a lane,
 * anything else one column a lane (correct, not fast).  Out of scope:
 * uniform-layout entry points (a uniform batch is a packed batch of equal
 * lengths), matrix-core forms and k + rows > 63, correcting more than one
 * wrong shard per column, device digests.  Plan-set locate is below. */
int slime_rs_plan_locate_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint32_t *src,
                               const uint32_t *cmp, const uint64_t *filter, uint64_t *counts, uint64_t *first,
                               void *stream);
int slime_rs_locate_objects_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint8_t *src,
                                  const uint8_t *cmp, const uint32_t *mapping, const uint64_t *filter,
                                  uint64_t *counts, uint64_t *first, void *stream);

/* ---- plan-set locate: name the corrupt shards of degraded objects ---------------
 * The two calls above with a set in place of the plan, as
 * slime_rs_planset_verify_batch is to slime_rs_plan_verify_batch: object o of
 * a PLANNED batch is classified with its own plan of the set -- its own k input
 * shard indices, its own rows_o coefficient rows and its own output shard
 * indices.  A degraded object (a chunk missing, a disk out) cannot be checked
 * against the encode plan, whose slots include the absent shard; its own plan
 * reads k present shards and checks the other present ones, so scrub
 * (slime_rs_planset_verify_batch), locate and repair stay on the device.
 * SLIME_RS_NO_PLAN objects and L == 0 objects keep the initial values.
 * Results: two device arrays of nobj x (k + max_rows + 1) uint64, max_rows the
 * set's (slime_rs_planset_info), initialised by the call as above.  For object
 * o, slot j < k is its plan's input j, slot k + i for i < rows_o its output row
 * i; slots k + rows_o .. k + max_rows - 1 keep (0, UINT64_MAX); `unlocated` is
 * ALWAYS slot k + max_rows, so one column of the result means the same thing
 * for every object.
 * The rule is the one above with the object's own plan, and one addition: an
 * object whose plan has rows_o < 2 reports every mismatching column as
 * unlocated (one row cannot tell an input from its output).  A set may hold
 * such plans next to better ones, so this is an answer per object, not a
 * refusal.
 * filter: NULL, or the `mismatches` array of a preceding
 * slime_rs_planset_verify_batch / _verify_objects_batch of the same set and
 * batch on the stream (nobj x max_rows; rows past an object's own are zero by
 * that call's contract).  An object whose max_rows entries are all zero is
 * passed over before any load of its data.
 * Asynchronous, no scratch, a static walk in every schedule and pipeline mode,
 * no counter set, capturable.  A set carries no launched mark.
 * SLIME_RS_ERR_INVALID_ARG, checked in this order: a null set or batch, a batch
 * that is not planned or was planned for another plan count, k or device;
 * max_rows < 2 (no object of the set could be located); k + max_rows > 63; null
 * result arrays; null buffers; for the byte form a null mapping.
 * Forms as above (k <= 16 over 4-byte aligned bases: four columns a lane; else
 * one column a lane).  Out of scope: matrix-core forms, k + max_rows > 63, more
 * than one wrong shard per column, a register-resident rare path, device
 * digests. */
int slime_rs_planset_locate_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint32_t *src,
                                  const uint32_t *cmp, const uint64_t *filter, uint64_t *counts,
                                  uint64_t *first, void *stream);
int slime_rs_planset_locate_objects_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint8_t *src,
                                          const uint8_t *cmp, const uint32_t *mapping, const uint64_t *filter,
                                          uint64_t *counts, uint64_t *first, void *stream);

/* ---- pair locate: name TWO wrong shards per column ------------------------------
 * The four locate calls above with a pair rule behind their rule, for plans of
 * rows >= 4 (8/12, 10/14, 16/20, scrub plans of four rows or more): four
 * syndromes decide two errors as two decide one.  Two whole chunks of an object
 * wrong -- truncated, zeroed, stale -- makes every column of the object
 * unlocated for the calls above; these name both shards on the device.
 * With h_a the column of slot a -- (c[0][a], ..., c[rows-1][a]) for an input
 * a < k, the unit vector e_i for output row slot k + i -- a column is classified
 * in this order:
 *   1. the rule above names a slot or says clean: that is the answer;
 *   2. rows < 4: unlocated, as above;
 *   3. exactly two d_i set: those two output rows (bit-wise, as d_i is);
 *   4. P = the unordered pairs {a, b} of slots with h_a, h_b independent and
 *      s = alpha*h_a + beta*h_b for some alpha != 0, beta != 0.  |P| == 1: both
 *      slots are named.  Anything else: unlocated.
 * For the plans this library builds (the MDS code restricted to the shards a
 * plan touches: distance rows + 1 >= 5) one or two wrong shards in a column are
 * always named.  Three or more in one column are unlocated, or blamed on a
 * wrong pair with probability about (k + rows)^2 / (2 p^(rows - 2)) per such
 * column.  For slime_rs_plan_matrix plans the rule is applied as written,
 * whatever the matrix.
 * Results have the shape, initialisation and meaning of the calls above.  A
 * column decided as a pair adds 1 to counts of BOTH slots and takes part in
 * first of both; `unlocated` stays the last slot.  Arguments, addressing, the
 * filter and the forms are those of each call's twin above.  Sets: an object
 * whose own plan has rows_o >= 4 gets the pair rule, 2 <= rows_o < 4 the rule
 * above, rows_o < 2 reports every mismatching column as unlocated.
 * Asynchronous, no scratch (a block keeps the flagged columns' syndromes in
 * rows x 256 words of LDS, at most 60 KiB), a static walk, no counter set,
 * capturable; the plan is marked launched.  SLIME_RS_ERR_INVALID_ARG, in this
 * order: the twin's handle and batch checks; rows < 4 (a set: max_rows < 4);
 * k + rows > 63; null result arrays; null buffers; for the byte forms a null
 * mapping.  Out of scope: three or more wrong shards per column, matrix-core
 * forms, k + rows > 63, device digests.  Correcting in place: the correct calls
 * below. */
int slime_rs_plan_locate_pairs_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint32_t *src,
                                     const uint32_t *cmp, const uint64_t *filter, uint64_t *counts, uint64_t *first,
                                     void *stream);
int slime_rs_locate_pairs_objects_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, const uint8_t *src,
                                        const uint8_t *cmp, const uint32_t *mapping, const uint64_t *filter,
                                        uint64_t *counts, uint64_t *first, void *stream);
int slime_rs_planset_locate_pairs_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint32_t *src,
                                        const uint32_t *cmp, const uint64_t *filter, uint64_t *counts,
                                        uint64_t *first, void *stream);
int slime_rs_planset_locate_pairs_objects_batch(slime_rs_planset_t set, slime_rs_batch_t batch, const uint8_t *src,
                                                const uint8_t *cmp, const uint32_t *mapping, const uint64_t *filter,
                                                uint64_t *counts, uint64_t *first, void *stream);

/* ---- correct: fix the words locate names, in place ------------------------------
 * The locate calls above that also REPAIR what they name: every column the rule
 * names is rewritten where it is stored, so a following verify finds the column
 * clean.  One flipped word costs a rewrite of that word, not a host round trip
 * and a rewrite of its shard; verify -> correct is one capturable chain; and
 * damage spread over more shards than the code has parity rows is repaired as
 * long as each column has no more wrong shards than the rule handles (five
 * shards of an 8/12 object wrong in five different columns: five erasures
 * exceed four rows, column by column it is corrected).
 * max_wrong: 1 is the one-shard rule (slime_rs_plan_locate_batch's), 2 the pair
 * rule behind it (slime_rs_plan_locate_pairs_batch's, rows >= 4).  Arguments,
 * addressing, the filter, the result arrays with their shape and
 * initialisation, skipped objects (SLIME_RS_NO_PLAN, L == 0, cleared by the
 * filter), the forms, the capture rules and the launched mark are each call's
 * locate twin's; src and cmp are written.
 * Per column, with s_i = stored_i - computed_i (mod p) and h_a the column of
 * slot a as above:
 *   clean or unlocated   nothing is written;
 *   output row k + i     the stored word of row i becomes computed_i (two named
 *                        rows: both);
 *   input j alone        with r the first row of c[r][j] != 0 (row 0 for this
 *                        library's plans), the word becomes
 *                        x_j + s_r / c[r][j] (mod p);
 *   a pair {a, b}        s = alpha*h_a + beta*h_b is solved from the non-zero
 *                        minor the pair rule takes; an input a becomes
 *                        x_a + alpha, an output row becomes the row over the
 *                        corrected inputs (which is stored - beta).
 * A named input whose coefficient column is all zero cannot be solved (only a
 * slime_rs_plan_matrix plan can have one): nothing is written and the column is
 * counted under `unlocated`.  For this library's MDS plans every coefficient is
 * non-zero and counts / first equal the locate twin's exactly.
 * The symbol forms write canonical residues: a wrong word whose original was
 * the alias p + t comes back as t.  The byte forms write BE(sym ^ mapping[o]);
 * stored symbols are below p by MapToGF's contract, so chunks come back bit for
 * bit.  Only named words are written.
 * Results: counts[o][slot] and first[o][slot] as locate's, now "columns
 * corrected in this shard"; `unlocated` is what is left for erasure repair.
 * The caller's contract, not checked (as slime_rs_plan_execute_batch's
 * outputs): the shards a plan touches, and the objects of a batch, do not
 * overlap in memory.  cmp may be src.
 * Misattribution is locate's: more wrong shards in a column than the rule
 * handles are unlocated, or "corrected" towards a wrong codeword, with
 * probability about k / p per such column for max_wrong = 1 and about
 * (k + rows)^2 / (2 p^(rows - 2)) for max_wrong = 2.
 * Asynchronous, no scratch (max_wrong = 2: the twin's LDS strip), a static
 * walk, no counter set, capturable.  SLIME_RS_ERR_INVALID_ARG, in this order:
 * max_wrong neither 1 nor 2; then the locate twin's refusals in its order.
 * Out of scope: three or more wrong shards per column, matrix-core forms,
 * k + rows > 63, host-memory entry points, the Go shim. */
int slime_rs_plan_correct_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, uint32_t *src, uint32_t *cmp,
                                const uint64_t *filter, int max_wrong, uint64_t *counts, uint64_t *first,
                                void *stream);
int slime_rs_correct_objects_batch(slime_rs_plan_t plan, slime_rs_batch_t batch, uint8_t *src, uint8_t *cmp,
                                   const uint32_t *mapping, const uint64_t *filter, int max_wrong, uint64_t *counts,
                                   uint64_t *first, void *stream);
int slime_rs_planset_correct_batch(slime_rs_planset_t set, slime_rs_batch_t batch, uint32_t *src, uint32_t *cmp,
                                   const uint64_t *filter, int max_wrong, uint64_t *counts, uint64_t *first,
                                   void *stream);
int slime_rs_planset_correct_objects_batch(slime_rs_planset_t set, slime_rs_batch_t batch, uint8_t *src,
                                           uint8_t *cmp, const uint32_t *mapping, const uint64_t *filter,
                                           int max_wrong, uint64_t *counts, uint64_t *first, void *stream);

/* ---- ragged byte encode: ingest objects of different sizes in one launch -------
 * slime_rs_encode_objects over the spans of a batch, each object with its own
 * size: the write side of the four launches above.  The batch
 * (slime_rs_batch_create or _create_planned) is used as it is, under the byte
 * launches' layout rule: data chunk j of object o is the 4*L_o bytes at
 * src + 4*(src_off + j*src_shard_stride), parity row i goes to
 * dst + 4*(dst_off + out_idx[i]*dst_shard_stride).  dst may be src: in-place
 * slots with the plan's outputs set to need..total-1 is the common call.  The
 * plan must read inputs 0..k-1 in that order (slime_rs_plan_encode gives such a
 * plan), because padding depends on a chunk's position in the object; anything
 * else is SLIME_RS_ERR_INVALID_ARG.  A planned batch is accepted: its plan
 * indices are ignored and its SLIME_RS_NO_PLAN objects are skipped.
 * sizes: a device array of nobj uint64, object o's byte length S with
 * slime_rs_chunk_size(S, k) == 4*L_o.  The kernels clamp the object's word
 * count to k*L_o, so a wrong size never makes a launch touch a byte outside
 * the object's own chunks; what such an object encodes to is unspecified.
 * Entries of objects without work are not read.
 * Arithmetic, per object, exactly slime_rs_encode_objects's (map.go:15-67,
 * multi_store.go:271-296, :526-554): word w < nw = ceil(S/4) is BE(bytes), a
 * partial last word masked to its valid high bytes; words nw..kL-1 are symbol
 * 0 and are not XOR-ed; parity word = BE(row ^ m); the data-chunk tail is
 * REWRITTEN IN src: BE(packed) for the partial word, BE(m) for every padding
 * word.  Bytes past S inside the object's data chunks may be garbage on entry:
 * they neither raise a flag nor survive.
 * mapping, status: device arrays of nobj words, both initialised by the call
 * for every object, on the stream.  mapping[o] receives MapToGF's choice;
 * status[o] = 1 marks an object that needs the random fallback (its parity is
 * not final until slime_rs_resolve_fallbacks_batch).  After either call
 * returns its work to the stream a caller sees only 0 or 1 in status.
 * slime_rs_encode_objects_batch is asynchronous, reads and writes device
 * memory only and takes no scratch.  It is several kernel nodes in a linear
 * chain (initialisation, the speculative pass with m = 0, the choice of
 * mapping, the re-encode of the objects whose mapping is not 0, a clean-up),
 * capturable under exactly the rules of slime_rs_plan_execute_batch (static
 * walk at slime_rs_kernel_schedule 1, dynamic with graph-held counter sets at
 * 2; each dynamic pass takes its own set).  It marks the plan launched.  An
 * empty batch launches only the initialisation.  SLIME_RS_ERR_INVALID_ARG:
 * null handles, a plan whose k or device is not the batch's, null mapping or
 * status, and -- when the batch has work -- null buffers or sizes.
 * slime_rs_encode_objects_batch_phased records phase_event (a hipEvent_t, or
 * NULL) on the stream after the speculative pass, for measurements.
 * slime_rs_resolve_fallbacks_batch is synchronous, like
 * slime_rs_resolve_fallbacks: it reads status, finds a mapping for every object
 * with status 1 (64 candidates a device pass from the stream slime_gf_seed
 * steers; the first non-zero fit wins), writes mapping[o], re-encodes only
 * those objects -- one launch for all of them -- and clears their status;
 * *resolved (optional) = objects fixed.  SLIME_RS_ERR_MAPPING_FALLBACK as the
 * uniform call; nothing has been written then.
 * Forms: k <= 16 over 4-byte aligned src and dst runs four columns a lane on
 * the walks of slime_rs_decode_objects_batch over each object's interior (no
 * partial word or padding), and one column a lane over its at most k + 3 edge
 * columns; anything else one column a lane (correct, not fast).  Out of scope:
 * the mid-object switch, redo lists and top-bit correction for ragged objects
 * (a switched object is re-encoded whole), a matrix-core or k-template ragged
 * encode, a plan-set encode, host entry points and digests. */
int slime_rs_encode_objects_batch(slime_rs_plan_t encode_plan, slime_rs_batch_t batch, uint8_t *src, uint8_t *dst,
                                  const uint64_t *sizes, uint32_t *mapping, uint32_t *status, void *stream);
int slime_rs_encode_objects_batch_phased(slime_rs_plan_t encode_plan, slime_rs_batch_t batch, uint8_t *src,
                                         uint8_t *dst, const uint64_t *sizes, uint32_t *mapping, uint32_t *status,
                                         void *stream, void *phase_event);
int slime_rs_resolve_fallbacks_batch(slime_rs_plan_t encode_plan, slime_rs_batch_t batch, uint8_t *src, uint8_t *dst,
                                     const uint64_t *sizes, uint32_t *mapping, uint32_t *status, void *stream,
                                     int *resolved);

/* ==== fused byte-domain object pipeline (writeChunks / reconstruct on device) ====
 * Object slots: object o's slot starts at slots + o*slot_stride bytes and holds
 * its `total` chunks of 4L bytes (chunk c at slot + c*4L, L = ceil(ceil(S/4)/need),
 * multi_store.go:272).  The object's S bytes are the first S bytes of its slot,
 * so the data chunks are in place: after encoding, chunk c of the slot is
 * exactly MapFromGF(mapping, part c) (multi_store.go:526-554).  Any need (k > 16
 * runs the 16-chunk byte kernels). */

/* Encode nobj objects of S bytes: mapping[o] receives gf.MapToGF's choice
 * (map.go:35-62) and status[o] = 1 marks an object that needs MapToGF's random
 * fallback (map.go:64-66; its chunks are not final until
 * slime_rs_resolve_fallbacks).  mapping/status are device arrays of nobj
 * words.  Speculative single pass (mapping 0) plus a re-encode pass only for
 * objects whose mapping is 1<<31.  Asynchronous. */
int slime_rs_encode_objects(slime_rs_plan_t encode_plan, uint8_t *slots, uint64_t slot_stride, uint64_t object_size,
                            uint64_t nobj, uint32_t *mapping, uint32_t *status, void *stream);
/* Synchronous: for each object with status 1, draw random mapping candidates
 * (64 per device pass) until one fits, store it in mapping[o], clear status[o]
 * and re-encode the object.  *resolved (optional) = objects fixed. */
int slime_rs_resolve_fallbacks(slime_rs_plan_t encode_plan, uint8_t *slots, uint64_t slot_stride,
                               uint64_t object_size, uint64_t nobj, uint32_t *mapping, uint32_t *status, void *stream,
                               int *resolved);
/* Rebuild chunks from `need` surviving chunks of each slot: a reconstruct plan
 * whose inputs are the survivors' chunk indices and whose outputs
 * (slime_rs_plan_set_outputs) are the chunk slots to write.  mapping[o] is the
 * object's mapping value (meta.File.MappingValue).  Asynchronous. */
int slime_rs_decode_objects(slime_rs_plan_t reconstruct_plan, uint8_t *slots, uint64_t slot_stride, uint64_t L,
                            uint64_t nobj, const uint32_t *mapping, void *stream);
/* The same three over a slot layout whose chunks are chunk_stride bytes apart
 * (chunk c at slot + c*chunk_stride; chunk_stride >= 4L, a multiple of 4; 0
 * selects 4L, the forms above).  Object byte i then lives in chunk i / 4L at
 * offset i % 4L: the device-resident layout the caller fills chunk by chunk
 * (e.g. 256 B-aligned chunk_stride, every chunk on a line boundary). */
int slime_rs_encode_objects_chunked(slime_rs_plan_t encode_plan, uint8_t *slots, uint64_t slot_stride,
                                    uint64_t chunk_stride, uint64_t object_size, uint64_t nobj, uint32_t *mapping,
                                    uint32_t *status, void *stream);
int slime_rs_resolve_fallbacks_chunked(slime_rs_plan_t encode_plan, uint8_t *slots, uint64_t slot_stride,
                                       uint64_t chunk_stride, uint64_t object_size, uint64_t nobj, uint32_t *mapping,
                                       uint32_t *status, void *stream, int *resolved);
int slime_rs_decode_objects_chunked(slime_rs_plan_t reconstruct_plan, uint8_t *slots, uint64_t slot_stride,
                                    uint64_t chunk_stride, uint64_t L, uint64_t nobj, const uint32_t *mapping,
                                    void *stream);
/* slime_rs_plan_verify over object slots: for every object o and every output
 * row i, how many 4-byte columns of chunk out[i] would change if
 * slime_rs_decode_objects_chunked ran the plan on the slot, and the lowest
 * such column (BE(stored) != computed ^ mapping[o]).  The plan's inputs and
 * outputs are chunk indices of the slot: an encode-shaped plan (survivors
 * 0..need-1, outputs need..total-1) checks a slot's parity.  Layout
 * preconditions are those of slime_rs_decode_objects_chunked (chunk_stride 0
 * selects 4L); bytes between 4L and chunk_stride are never read.  Results as
 * for slime_rs_plan_verify: nobj x rows uint64 each, initialised by the call,
 * UINT64_MAX in first for none; wide codes take the one-column-per-lane form;
 * no scratch is used.  Asynchronous. */
int slime_rs_verify_objects(slime_rs_plan_t plan, const uint8_t *slots, uint64_t slot_stride, uint64_t chunk_stride,
                            uint64_t L, uint64_t nobj, const uint32_t *mapping, uint64_t *mismatches,
                            uint64_t *first, void *stream);
/* encode_objects_chunked that also records the hipEvent_t `phase_event` (may be
 * null) on `stream` between its two passes: after the speculative pass and the
 * mapping selection, before the re-encode of the objects mapped with 1<<31 --
 * so a caller can time the re-encode's share of the call.  A call with nothing
 * to encode (nobj or the object size 0) records nothing. */
int slime_rs_encode_objects_phased(slime_rs_plan_t encode_plan, uint8_t *slots, uint64_t slot_stride,
                                   uint64_t chunk_stride, uint64_t object_size, uint64_t nobj, uint32_t *mapping,
                                   uint32_t *status, void *stream, void *phase_event);

/* ---- Object entry points over host memory (the callers' data paths) ----
 *
 * Byte length of every chunk of a `size`-byte object split `need` ways:
 * 4 * ceil(ceil(size/4) / need)  (splitVector, multi_store.go:271-278). */
uint64_t slime_rs_chunk_size(uint64_t size, int need);

/* The data path of Multi.writeChunks (multi_store.go:526-531 and :554):
 *   mapping, all := gf.MapToGF(data); parts := splitVector(all, need);
 *   parity i := rs.CreateParity(parts, need+i, nil); chunk i := gf.MapFromGF(mapping, part i)
 * in one device pass (fused byte kernels) with pinned, overlapped transfers.
 * chunks[0..total-1] each receive slime_rs_chunk_size(size, need) bytes;
 * *mapping receives MappingValue.  The random-mapping fallback draws from the
 * library's stream (slime_gf_seed).  need >= 1 and total >= need (total ==
 * need: a store without parity, multi_config.go:36); size 0 gives mapping 0
 * and empty chunks.  Zero-copy data chunks: chunks[j] (j < need) may be
 * data + j*chunk_size when that chunk lies wholly inside the object; its bytes
 * are then already final and are not copied.  Any other overlap between a
 * chunk buffer and data is refused (SLIME_RS_ERR_INVALID_ARG).  Synchronous;
 * thread-safe. */
int slime_rs_write_chunks(const uint8_t *data, uint64_t size, int need, int total, uint8_t *const *chunks,
                          uint32_t *mapping);

/* The slow path of Multi.reconstruct (multi_store.go:215-241): the first
 * `need` available chunks (chunk_bytes each; a length that is not a multiple
 * of 4 is zero-padded to whole words as MapToGFWith does) with their
 * chunk indices, and the file's MappingValue -> the object's `size` bytes in
 * out:  chunk := MapToGFWith(data, mapping); RecoverData(chunks, indices);
 * MapFromGF each data row; data[:size].  Same panics as RecoverData for bad
 * indices.  Bytes past need*chunk_bytes are zero, as
 * in the reference's data[:Size] of a zeroed buffer.  Synchronous. */
int slime_rs_reconstruct(const uint8_t *const *chunks, const int *indices, int need, uint64_t chunk_bytes,
                         uint32_t mapping, uint64_t size, uint8_t *out);

/* Device codec (internal/rs/gf/map.go) over device buffers, asynchronous on
 * `stream`.  pack: words[i] = BE(bytes[4i..4i+3]) ^ mapping (zero low bytes
 * in a partial last word); if flags != NULL it is OR-ed with bit0 = some
 * unmapped word >= p, bit1 = some (word ^ 1<<31) >= p  (MapToGF's choice).
 * unpack: bytes = BE(words[i] ^ mapping). */
int slime_gf_pack_device(int device, const uint8_t *bytes, uint64_t len, uint32_t mapping, uint32_t *words,
                         uint32_t *flags, void *stream);
int slime_gf_unpack_device(int device, const uint32_t *words, uint64_t count, uint32_t mapping, uint8_t *bytes,
                           void *stream);

/* Device batch buffers (MI355X; no reference counterpart: the Go path works in
 * host memory).  A hipMalloc'd batch of tens of GiB lands, allocation by
 * allocation, in one of two physical placements, and the apply kernels stream
 * about 13% slower from the bad one (DESIGN.md "Placement modes").  This allocator
 * builds the buffer from physical chunks (HIP virtual memory: hipMemCreate,
 * mapped in order into one reserved virtual range): 2 MiB-chunk buffers landed
 * in the slow placement in 1 of 58 trials, hipMalloc'd ones in 36 of 98
 * (DESIGN.md "the allocator changes the odds").  `bytes` is
 * rounded up to the chunk size (env SLIME_RS_VMM_CHUNK_MIB, default 2 MiB);
 * *ptr receives a base usable by every device entry point.  Synchronous.
 * Returns 0, SLIME_RS_ERR_INVALID_ARG, SLIME_RS_ERR_NO_DEVICE or
 * SLIME_RS_ERR_HIP (out of memory). */
int slime_rs_device_alloc(int device, uint64_t bytes, void **ptr);
/* How a slime_rs_device_alloc buffer was placed.  Buffers of at least
 * SLIME_RS_PLACEMENT_PROBE_GIB GiB (default 16; 0 disables) are probed when
 * created: the apply kernel's C3-shaped read/write walk over the whole buffer
 * (GB/s of algorithmic traffic).  Below SLIME_RS_PLACEMENT_MIN_GBS (default
 * 6350, the top of the rates seen, so in practice always) the allocator tries
 * up to two other placements (1 GiB chunks, then one hipMalloc), holding the
 * first meanwhile, and keeps the fastest (DESIGN.md "Placement"). */
typedef struct slime_rs_alloc_info {
  int kind;                /* kept placement: 0 = physical chunks mapped into one range, 1 = hipMalloc */
  int probes;              /* placements probed (0: buffer too small, not probed) */
  int chosen;              /* index into probe_* of the kept placement */
  uint64_t chunk_bytes;    /* kept placement's chunk size (0 for hipMalloc) */
  double probe_gbs[4];     /* each probed placement's rate */
  uint64_t probe_chunk[4]; /* each probed placement's chunk size (0: hipMalloc) */
} slime_rs_alloc_info_t;
int slime_rs_device_alloc_info(const void *ptr, slime_rs_alloc_info_t *info);
/* The same placement probe over a caller's own device range [ptr, ptr+bytes)
 * on `device` (e.g. a hipMalloc'd or torch batch buffer): *gbs = GB/s of
 * algorithmic traffic of the C3-shaped read/write walk, 0 when the range is
 * too small to measure (under ~400 MB).  The physical placement of a large
 * buffer fixes, for its whole life, whether the kernels stream in the fast
 * mode (~6.0-6.4 TB/s at C3) or the slow one (~5.3-5.7): a buffer that
 * probes in the slow mode is worth re-allocating, or allocating with
 * slime_rs_device_alloc, which probes and re-places by itself.
 * OVERWRITES the range: probe a buffer before filling it.  The range must lie
 * inside one device allocation on `device` (else SLIME_RS_ERR_INVALID_ARG).
 * Synchronous. */
int slime_rs_probe_placement(void *ptr, uint64_t bytes, int device, double *gbs);
/* The allocator's re-placement threshold, GB/s (env SLIME_RS_PLACEMENT_MIN_GBS,
 * default 6350: a first placement below it is re-placed, keeping the fastest
 * of up to three; 6350 is about the C3 apply kernel at 8.2 ms). */
double slime_rs_placement_threshold(void);
/* Frees a buffer from slime_rs_device_alloc (its base).  Waits for the device
 * first (hipDeviceSynchronize), so work still queued on it cannot fault.
 * Returns SLIME_RS_ERR_INVALID_ARG for other pointers. */
int slime_rs_device_free(void *ptr);

/* Deterministic synthetic symbols (benchmarks/tests): word g of the buffer is
 * a pure function of (seed, g), uniform over [0, p). Asynchronous. */
int slime_rs_fill_symbols(int device, uint32_t *dst, uint64_t count, uint64_t seed, void *stream);

/* ==== *_ex forms: the entry points above with a per-call context ==========
 * Same arguments and results as the plain forms; `call` gives the device and
 * receives this call's failure detail (see slime_rs_call_t).  These are what
 * the cgo shim binds. */
int slime_rs_create_parity_ex(const slime_rs_call_t *call, const uint32_t *const *data, const uint64_t *lens,
                              int ndata, int index, uint32_t *out);                       /* vector.go:18 */
int slime_rs_create_parities_ex(const slime_rs_call_t *call, const uint32_t *const *data, const uint64_t *lens,
                                int ndata, int total, uint32_t *const *out);              /* multi_store.go:528-531 */
int slime_rs_recover_data_ex(const slime_rs_call_t *call, const uint32_t *const *chunks, const uint64_t *lens,
                             int nchunks, const int *indices, int nindices, uint32_t *const *out); /* vector.go:50 */
int slime_rs_write_chunks_ex(const slime_rs_call_t *call, const uint8_t *data, uint64_t size, int need, int total,
                             uint8_t *const *chunks, uint32_t *mapping);                  /* multi_store.go:526-554 */
int slime_rs_reconstruct_ex(const slime_rs_call_t *call, const uint8_t *const *chunks, const int *indices, int need,
                            uint64_t chunk_bytes, uint32_t mapping, uint64_t size, uint8_t *out); /* :215-241 */
int slime_gf_map_to_gf_ex(const slime_rs_call_t *call, const uint8_t *in, uint64_t len, uint32_t *mapping,
                          uint32_t *out);                                                 /* map.go:15 */
int slime_gf_map_to_gf_with_ex(const slime_rs_call_t *call, const uint8_t *in, uint64_t len, uint32_t n,
                               uint32_t *out);                                            /* map.go:74 */
int slime_gf_map_from_gf_ex(const slime_rs_call_t *call, uint32_t n, const uint32_t *in, uint64_t count,
                            uint8_t *out);                                                /* map.go:103 */
int slime_rs_parity_matrix_ex(const slime_rs_call_t *call, int d, int p, uint32_t *out);  /* matrix.go:27 */
int slime_rs_vandermonde_matrix_ex(const slime_rs_call_t *call, int d, int p, uint32_t *out); /* matrix.go:8 */
int slime_rs_solve_sub_identity_ex(const slime_rs_call_t *call, uint32_t *m, int rows, int cols); /* matrix.go:35 */
int slime_rs_invert_matrix_ex(const slime_rs_call_t *call, const uint32_t *m, int d, uint32_t *inv); /* matrix.go:112 */

/* ==== plan cache and device pool (host entry points) =====================
 * Host entry points keep their device plans (coefficient tables; recovery
 * plans keyed by survivor set, reference: vector.go:69-77) in one bounded LRU
 * per process (default 256 plans, env SLIME_RS_PLAN_CACHE).  An evicted plan
 * releases its device table once no call in flight still uses it. */
typedef struct slime_rs_cache_stats {
  uint64_t live;          /* plans cached now (<= capacity) */
  uint64_t capacity;
  uint64_t hits, misses, evictions;
  uint64_t device_tables; /* plan tables allocated on devices and not yet freed (all plans, cached or not) */
} slime_rs_cache_stats_t;
int slime_rs_plan_cache_stats(slime_rs_cache_stats_t *stats);
/* Set the cache capacity (>= 1); shrinking evicts at once. */
int slime_rs_plan_cache_capacity(uint64_t capacity);
/* Where the host entry points' windowed pipeline spends its wall time (all
 * threads, since the start or the last reset; microseconds): copy_in = host
 * copies into pinned staging, enqueue = DMA/kernel launches, wait = waiting
 * for a stage's transfers and kernels (device and link side), copy_out = host
 * copies out of pinned staging.  reset != 0 zeroes the counters after reading. */
typedef struct slime_rs_host_stats {
  uint64_t calls, windows;
  uint64_t copy_in_us, enqueue_us, wait_us, copy_out_us, total_us;
} slime_rs_host_stats_t;
int slime_rs_host_stats(slime_rs_host_stats_t *stats, int reset);
/* Host calls the device pool has routed to `device` so far and calls in flight there. */
int slime_rs_pool_calls(int device, uint64_t *calls, int *inflight);
/* Host calls (the data entry points over host memory) that run at once in
 * this process: half its usable CPUs (affinity mask capped by the cgroup CPU
 * quota), at least 4.  Further callers wait, asleep, for a slot -- more calls
 * than CPUs only time-slice, and a process over its CPU quota is throttled
 * as a whole. */
int slime_rs_host_call_slots(void);
/* Ticket-counter sets of the dynamic-schedule kernels on `device`: *sets
 * allocated so far, *held by launches not yet known to have finished plus
 * those owned by captured graphs.  A set is reused by any stream once its
 * launch has finished (each launch leaves its set zero; DESIGN.md "Dynamic
 * schedule"). */
int slime_rs_ticket_sets(int device, uint64_t *sets, uint64_t *held);
/* Launches on `device` since start that ran the dynamic schedule on a counter
 * set, and that asked for one and were sent to the static kernels instead
 * (no set to be had) -- diagnostics and tests.  Launches the mode itself
 * keeps on the static kernels (mode 0, captures under mode 1) count in
 * neither. */
int slime_rs_schedule_counts(int device, uint64_t *dynamic, uint64_t *fallback);

/* ==== chunk and object digests ======================
 * Host computations on the library's digest threads (DESIGN.md "Chunk
 * digests"): SHA-256 and FNV-1a are sequential per message, so one x86 core
 * with the SHA extensions outruns a GPU lane ~100x; what the library adds is
 * hashing writeChunks' chunks while its device pipeline still runs. */

/* SHA-256 of len bytes (sha256.Sum256 as store.DataV uses it,
 * internal/store/store.go:104-110, and reconstruct's verify, multi_store.go:244). */
int slime_rs_sha256(const uint8_t *data, uint64_t len, uint8_t *out /* 32 bytes */);

/* For each of n chunks (lens[i] bytes): sha[32i..] = SHA-256 of the chunk
 * (store.DataV per chunk, multi_store.go:554-556) and, if hdr != NULL,
 * hdr[8i..] = the chunk file's header hash: FNV-1a-64 over SHA-256 ‖ chunk,
 * big-endian as hash.Sum appends it (storedir/directory.go:25-28,548-553).
 * Chunks are hashed in parallel, one per digest thread. */
int slime_rs_chunk_digests(const uint8_t *const *chunks, const uint64_t *lens, uint32_t n, uint8_t *sha,
                           uint8_t *hdr);

/* slime_rs_write_chunks plus every chunk's digests as slime_rs_chunk_digests
 * gives them (sha: total x 32 bytes; hdr optional, total x 8), computed while
 * the device pipeline runs: data chunks are hashed from `data` at once and
 * finished when the mapping is known, parity chunks as their windows land in
 * the caller's buffers.  Replaces writeChunks' per-chunk goroutines'
 * MapFromGF + store.DataV (multi_store.go:552-557). */
int slime_rs_write_chunks_digest(const uint8_t *data, uint64_t size, int need, int total, uint8_t *const *chunks,
                                 uint32_t *mapping, uint8_t *sha, uint8_t *hdr);

/* slime_rs_reconstruct, then the object's SHA-256 against want_sha (the
 * file's SHA256, multi_store.go:244-249): SLIME_RS_ERR_BAD_HASH on mismatch
 * (out holds the rebuilt bytes either way). */
int slime_rs_reconstruct_verify(const uint8_t *const *chunks, const int *indices, int need, uint64_t chunk_bytes,
                                uint32_t mapping, uint64_t size, uint8_t *out, const uint8_t *want_sha);

/* Whether SHA-256 runs on the CPU's SHA extensions, and the digest threads
 * besides the caller (env SLIME_RS_DIGEST_THREADS). */
int slime_rs_digest_info(int *sha_extensions, int *threads);

int slime_rs_write_chunks_digest_ex(const slime_rs_call_t *call, const uint8_t *data, uint64_t size, int need,
                                    int total, uint8_t *const *chunks, uint32_t *mapping, uint8_t *sha,
                                    uint8_t *hdr);
int slime_rs_reconstruct_verify_ex(const slime_rs_call_t *call, const uint8_t *const *chunks, const int *indices,
                                   int need, uint64_t chunk_bytes, uint32_t mapping, uint64_t size, uint8_t *out,
                                   const uint8_t *want_sha);

#ifdef __cplusplus
}
#endif
#endif /* SLIME_RS_H */
