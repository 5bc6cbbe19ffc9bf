/*
 * speck_c_api.h -- C-ABI boundary of the MI355X-native SpGEMM backend
 * (libspeck_amd.so).  Plain pointers and sizes only; every pointer inside a
 * speck_dcsr is a DEVICE pointer (HIP), exactly as in the reference's dCSR<T>.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to the upstream GPUPeople/spECK tree).
 */
#ifndef SPECK_C_API_H
#define SPECK_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference printf()s and returns; include/common.h:19-33,
 *      source/GPU/Multiply.cu:57-97 -- a C ABI reports instead) ---- */
enum {
    SPECK_OK = 0,
    SPECK_ERR_INVALID = 1,        /* null pointers / inconsistent sizes */
    SPECK_ERR_DIM_LIMIT = 2,      /* rows(A) or cols(B) > 2^27, source/GPU/Multiply.cu:57-66 */
    SPECK_ERR_HIP = 3,            /* a HIP runtime call failed */
    SPECK_ERR_OOM = 4,            /* device allocation failed, source/GPU/Multiply.cu:594-599 */
    SPECK_ERR_NNZ_OVERFLOW = 5,   /* nnz(C) does not fit the u32 row_offsets of dCSR */
    SPECK_ERR_NO_DEVICE = 6,
    SPECK_ERR_IO = 7,
    SPECK_ERR_UNSORTED = 8,       /* a row of B is not strictly ascending / column >= cols: the reference's
                                   * undocumented precondition (its loader sorts, source/CSR.cpp:173-212) */
    SPECK_ERR_COMM = 9            /* RCCL / shared-memory transport failure (row-sharded multi-GPU exchange) */
};

/* ---- device CSR: field-for-field the reference's dCSR<T> / dCSRNoDealloc<T>
 *      (include/dCSR.h:9-35): rows, cols, nnz, data, row_offsets, col_ids.
 *      row_offsets has rows+1 entries; they may be ABSOLUTE offsets into
 *      col_ids/data of a larger matrix (a row-range view used for sharding).
 *      Such a view may reach a last offset of 0xFFFFFFFF in every call that says
 *      it takes one, except as A of speck_multiply_* (and of speck_analysis,
 *      speck_symbolic, speck_partition_rows): row_offsets[0] + nnz > 2^32 - 2^16
 *      is SPECK_ERR_INVALID there before any kernel starts, nothing written (the
 *      walks over a row of A count in 32 bits and step by up to 2^11 entries;
 *      DESIGN.md 4.18.1). ---- */
typedef struct speck_dcsr {
    uint64_t rows, cols, nnz;
    void *data;             /* double* or float*  (device) */
    uint32_t *row_offsets;  /* device */
    uint32_t *col_ids;      /* device */
} speck_dcsr;

/* ---- per-stage timings: the reference's Timings (include/Timings.h:4-18),
 *      milliseconds, same field names/order ---- */
typedef struct speck_timings {
    int32_t measureAll;
    int32_t measureCompleteTime;
    float init, countProducts, loadBalanceCounting, globalMapsCounting, spGEMMCounting, allocC,
        loadBalanceNumeric, globalMapsNumeric, spGEMMNumeric, sorting, cleanup, complete;
} speck_timings;

/* ---- what the last multiply did (drives bench.py's roofline object) ---- */
#define SPECK_NUM_SYM_BINS 16
#define SPECK_NUM_NUM_BINS 16
typedef struct speck_stats {
    uint64_t sum_products;                       /* P, u64 (reference: u32, Multiply.cu:237) */
    uint64_t nnz_c;
    uint32_t max_row_ops;                        /* maxComputationsPerRow, Multiply.cu:252 */
    uint32_t max_row_nnz_c;                      /* maxElementsPerRow, Multiply.cu:615 */
    uint32_t sym_bin_rows[SPECK_NUM_SYM_BINS];   /* rows per symbolic kernel class */
    uint32_t num_bin_rows[SPECK_NUM_NUM_BINS];   /* rows per numeric kernel class */
    uint64_t num_bin_bytes[SPECK_NUM_NUM_BINS];  /* algorithmic bytes per numeric class */
    uint64_t sym_bin_bytes[SPECK_NUM_SYM_BINS];
    float num_bin_ms[SPECK_NUM_NUM_BINS];        /* HIP-event ms of each numeric kernel launch */
    float sym_bin_ms[SPECK_NUM_SYM_BINS];
    float analysis_ms, scan_ms;
    float sym_light_ms, num_light_ms;            /* merged launch of the 256-thread classes (big-LDS part) */
    float sym_tiny_ms, num_tiny_ms;              /* ... and of the small classes, launched right behind it */
    int32_t kernel_events_valid;                 /* 1 if *_ms were recorded for the last call */
    int32_t numeric_reruns;                      /* replayed sequences rejected by the device-side checks */
    int32_t graph_replays;                       /* multiplies served by a reuse sequence (cumulative; the field names are
                                                  *    those of rounds 2-4 -- no executable graph is involved any more) */
    int32_t graph_captures;                      /* reuse sequences planned (cumulative) */
    float sym_phase_ms, num_phase_ms;            /* fork-to-join span of the symbolic / numeric launches (pipeline stream) */
    int32_t replayed;                            /* 1: the last multiply was served by a reuse sequence */
    int32_t nf_direct;                           /* 1: that sequence wrote the numeric-first rows straight to C at the row
                                                  *    offsets of the previous identical call (verified) */
    int32_t pool_fallbacks;                      /* scratch-pool classes switched off because the pool did not fit */
    int32_t esc_fused;                           /* 1: that sequence finished the rows of the register classes (<= 64
                                                  *    products) in its symbolic phase, at those offsets */
    uint64_t scratch_pool_bytes;                 /* numeric-first / global-key-set pool currently allocated */
    int32_t pred_stages;                         /* that sequence's integer stages verified the previous identical call's
                                                  *    decisions instead of folding them again: bit 0 the row-offset scan +
                                                  *    numeric binning (one kernel), bit 1 the symbolic binning (inside the
                                                  *    analysis kernel), bit 2 the analysis itself (a verifier on its own
                                                  *    stream beside the sequence), bit 3 no scan kernel at all (every row's
                                                  *    nnz compared where it is produced), bit 4 no symbolic pass for the hash
                                                  *    / dense rows either (their numeric bodies verify the nnz themselves:
                                                  *    option num_verify) -- DESIGN.md 4.3 */
    int32_t eager_speculated;                    /* an EAGER call that ran analysis .. scan as one batch sized from the previous
                                                  * eager call on the config (one read-back instead of two; option
                                                  * eager_speculate): 1 = its device-side checks held, -1 = they did not and
                                                  * the two-read-back sequence re-ran, 0 = not attempted */
    int32_t one_walk;                            /* 1: the last multiply was a ONE-WALK complete call (walk.hip): the
                                                  * rows of the register classes were finished inside the kernel that places the
                                                  * rows -- no symbolic pass for them, no scan kernel; scan_ms is that kernel */
    int32_t walk_misses;                         /* one-walk calls the device-side checks declared void (cumulative; the
                                                  * two-phase call re-ran) */
    int32_t eager_through;                       /* 1: the last multiply was a complete two-phase call enqueued as ONE batch --
                                                  * the numeric launches queued behind the scan, into the buffers matOut already
                                                  * had, everything the host checks between the phases checked by the scan
                                                  * (option eager_through; eager_speculated is 1 as well); -1: attempted, the
                                                  * device-side checks did not hold, nothing of C was written, the call re-ran */
} speck_stats;

typedef struct speck_config speck_config; /* opaque; reference: spECKConfig, include/spECKConfig.h:8-53 */

/* spECKConfig::initialize(device) -- include/spECKConfig.h:15-32: queries the
 * device (CU count, LDS limits), creates 6 streams and 4 events, and (new) a
 * grow-only scratch arena reused across calls. */
int speck_config_create(int device, speck_config **out);
/* spECKConfig::cleanup() -- include/spECKConfig.h:34-43 */
int speck_config_destroy(speck_config *cfg);
/* spECKConfig::{sm,maxStaticSharedMemoryPerBlock,maxDynamicSharedMemoryPerBlock} */
int speck_config_info(const speck_config *cfg, int *sm, int *max_static_lds, int *max_dynamic_lds);
/* spECKConfig::{streams, completeStart, completeEnd, individualStart, individualEnd} (include/spECKConfig.h:12-13):
 * the 6 hipStream_t and 4 hipEvent_t the config created, as void*; they stay owned by the config. */
int speck_config_handles(const speck_config *cfg, void *streams6[6], void *events4[4]);
/* Run the pipeline on a caller-owned stream (e.g. torch's current stream); NULL restores streams[0]. */
int speck_config_set_stream(speck_config *cfg, void *hip_stream);
/* Tunables (thresholds the reference hard-codes in Multiply.cu:128-131,321-324); name -> value. */
int speck_config_set_option(speck_config *cfg, const char *name, int64_t value);
/* Record HIP events around every kernel of the next calls (fills speck_stats.*_ms); enable = 2: around the
 * phases only (analysis_ms, scan_ms, sym_phase_ms, num_phase_ms -- no event between the launches of a phase). */
int speck_config_profile_kernels(speck_config *cfg, int enable);
int speck_last_stats(const speck_config *cfg, speck_stats *out);

/* spECK::MultiplyspECK<double,...>(A, B, matOut, config, timings) --
 * include/Multiply.h:15-16, source/GPU/Multiply.cu:51-1128.
 * Ownership as in the reference: A,B caller-owned, read-only; C is
 * allocated by the callee and freed by the caller (speck_dcsr_free); if
 * C->rows == A->rows and C->row_offsets != NULL that buffer is reused; data/col_ids are
 * re-allocated only when C->nnz != nnz(C).  On error the C STRUCT and its allocations are left untouched
 * (no field rewritten, nothing freed or allocated).  The CONTENTS of the buffers are untouched too, with one
 * exception: a repeated call on the same buffers that runs the replayed launch sequence places finished rows
 * straight into C->col_ids / C->data (options nf_direct / esc_fused, both on by default) before the device-side
 * checks of that sequence can reject it; if the eager re-run that follows then fails as well (inputs changed in
 * place into something invalid, out of memory for a grown C), the call returns the error with the contents of
 * col_ids / data unspecified.  The same holds for a ONE-WALK complete call (option one_walk, OFF by default: a complete
 * call on a matOut that is already allocated finishes short rows straight into C->col_ids / C->data before the input
 * check of B and its own device-side checks have spoken; a miss re-runs the two-phase call, an invalid input returns its
 * error with the contents unspecified).  A complete call enqueued as one batch (option eager_through, on by default) keeps
 * the rule: its scan looks at the verdict of the input check and at its own checks before any numeric kernel starts, and a
 * voided batch writes nothing.  row_offsets is rewritten only by a call that completes. */
int speck_multiply_f64(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B, speck_dcsr *C,
                       speck_timings *timings);
/* the <float,...> instantiation, source/GPU/Multiply.cu:1130 */
int speck_multiply_f32(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B, speck_dcsr *C,
                       speck_timings *timings);

/* ---- staged entry points (each a prefix of the pipeline; used by the parity
 *      tests and by the row-shard partitioner) ---- */
/* readOperations -- include/common.cuh:321-459, launch source/GPU/Multiply.cu:239-252.
 * d_* are device arrays of A->rows u32 (any may be NULL); h_* are host scalars. */
int speck_analysis(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B, uint32_t *d_row_ops,
                   uint32_t *d_row_max_ops, uint32_t *d_row_col_min, uint32_t *d_row_col_max,
                   uint64_t *h_sum_products, uint32_t *h_max_row_ops);
/* analysis + binning + symbolic + scan (source/GPU/Multiply.cu:239-575):
 * d_row_offsets (A->rows+1 u32, device) receives C's row offsets; *h_nnz_c = nnz(C). */
int speck_symbolic(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B,
                   uint32_t *d_row_offsets, uint64_t *h_nnz_c);
/* Row-shard boundaries with equal sum of per-row products:
 * h_bounds[parts+1], h_bounds[0]=0, h_bounds[parts]=A->rows. */
int speck_partition_rows(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B, int parts,
                         uint64_t *h_bounds);

/* ---- dCSR memory helpers: dCSR<T>::alloc / reset / convert(),
 *      include/dCSR.h:19-47, source/dCSR.cpp:25-115 ---- */
int speck_dcsr_alloc(speck_dcsr *m, uint64_t rows, uint64_t cols, uint64_t nnz, int alloc_offsets,
                     size_t value_size);
int speck_dcsr_free(speck_dcsr *m);
int speck_dcsr_upload(speck_dcsr *dst, uint64_t rows, uint64_t cols, uint64_t nnz,
                      const uint32_t *h_row_offsets, const uint32_t *h_col_ids, const void *h_data,
                      size_t value_size);
/* convert(CSR&, const dCSR&) -- source/dCSR.cpp:67-76; any of the host arrays may be NULL.  `src` may be a row-range
 * view with absolute offsets (first offset not 0, last offset = first + nnz): the host receives exactly what a
 * download of its speck_dcsr_copy gives -- the nnz entries from the first offset on, offsets rebased to start at 0.
 * Every other matrix (an owner: first offset 0; offsets that do not span nnz entries) is downloaded as it lies in
 * memory: offsets unchanged, the first nnz entries of col_ids / data. */
int speck_dcsr_download(const speck_dcsr *src, uint32_t *h_row_offsets, uint32_t *h_col_ids,
                        void *h_data, size_t value_size);
/* convert(dCSR&, const CSR&, padding) -- source/dCSR.cpp:51-66: buffers for rows + padding rows and nnz + 8 * padding
 * entries, rows / nnz of the source, the padding zero-filled.  speck_dcsr_upload = padding 0. */
int speck_dcsr_upload_padded(speck_dcsr *dst, uint64_t rows, uint64_t cols, uint64_t nnz,
                             const uint32_t *h_row_offsets, const uint32_t *h_col_ids, const void *h_data,
                             size_t value_size, uint32_t padding);
/* convert(dCSR&, const dCSR&, padding) -- source/dCSR.cpp:81-89: device-to-device, no host round trip.  `src` may be
 * a row-range view with absolute offsets: the copy is rebased to start at 0.  dst must not share any buffer with src
 * (SPECK_ERR_INVALID: the allocation of dst frees what it held).  Like every speck_dcsr_* call it works on the NULL
 * stream and returns when the copy is complete; a caller that produced src on its own non-blocking stream synchronises
 * that stream first. */
int speck_dcsr_copy(speck_dcsr *dst, const speck_dcsr *src, size_t value_size, uint32_t padding);
/* overwrite the contents of an existing device matrix in place (same rows / nnz, same device
 * pointers); any of the host arrays may be NULL */
int speck_dcsr_update(speck_dcsr *dst, const uint32_t *h_row_offsets, const uint32_t *h_col_ids,
                      const void *h_data, size_t value_size);
/* spECK::Compare(ref, cmp, compare_data) -- include/Compare.h:5-6, source/GPU/Compare.cu:11-82;
 * stricter: offsets + col ids bit-exact; values |x-y| <= rel_tol*max(|x|,|y|) when compare_data.
 * Special values (here and in speck_compare_bounded_f64): x and y match iff both are NaN, or x == y,
 * or both are finite and within the bound -- equal infinities match, an infinity never matches a
 * finite value or the opposite infinity, NaN matches NaN only (the reference passes NaN against any
 * value, source/GPU/Compare.cu:50).
 * *h_mismatches = number of differing rows (0 = equal); a row that differs in its pattern AND in a value is one row. */
int speck_compare_f64(speck_config *cfg, const speck_dcsr *ref, const speck_dcsr *cmp,
                      int compare_data, double rel_tol, uint64_t *h_mismatches);
/* ... and its float instantiation (source/GPU/Compare.cu:84) */
int speck_compare_f32(speck_config *cfg, const speck_dcsr *ref, const speck_dcsr *cmp,
                      int compare_data, double rel_tol, uint64_t *h_mismatches);
/* The value check a SpGEMM result admits whatever its summation order: |ref - cmp| <= tol * S per
 * entry, S = sum |a*b| of the entry, handed over as `abs_products` = |A|*|B| (same pattern as ref).
 * Role of the reference's compare against cuSPARSE (source/Executor.cpp:29-40), made to FAIL on
 * values: *h_structure_rows / *h_value_rows = rows that differ in pattern / rows of equal pattern with a value beyond
 * the bound (no row is in both counts). */
int speck_compare_bounded_f64(speck_config *cfg, const speck_dcsr *ref, const speck_dcsr *cmp,
                              const speck_dcsr *abs_products, double tol, uint64_t *h_structure_rows,
                              uint64_t *h_value_rows);
/* Order-preserving transpose (source/GPU/Transpose.cu:10-117; DataLoader.cpp:65-69 for rows!=cols).
 * nnz > 2^32 - 64: SPECK_ERR_NNZ_OVERFLOW before anything is allocated (the kernel that expands the rows counts a row's
 * entries in 32 bits, a wave of 64 at a time: a row that ends within one step of 2^32 would send the counter round). */
int speck_transpose_f64(speck_config *cfg, const speck_dcsr *A, speck_dcsr *At);
/* ... and its float instantiation (source/GPU/Transpose.cu:116) */
int speck_transpose_f32(speck_config *cfg, const speck_dcsr *A, speck_dcsr *At);

/* ---- rows of a device CSR sorted in place (new: the reference sorts on the host while it loads, source/CSR.cpp:173-212;
 *      a matrix that is already on the device -- the output of a library SpGEMM, a CSR assembled from element
 *      contributions, columns relabelled in place -- has no loader in the way).  Makes `M` acceptable as an input of
 *      speck_multiply_*: every row ascending by column id, optionally with equal columns merged into one entry.
 *  IN PLACE: the three device pointers of M are the same after the call, nothing of M is allocated or freed.  Temporaries
 *      (class lists, the long-row class, the compaction) are grow-only buffers of the config, released with it; cfg == NULL
 *      is allowed as for speck_transpose_*, with temporaries of the call's own on the NULL stream.
 *  SPECK_SORT_KEEP_DUPLICATES: every row becomes the STABLE sort of itself by column id -- entries of equal column keep
 *      their input order.  row_offsets and nnz are not written.  Works on a row-range view with absolute offsets: only the
 *      entries of the view's rows are touched.
 *  SPECK_SORT_SUM_DUPLICATES: as above, then every run of equal columns becomes ONE entry whose value is the sum of the
 *      run, accumulated in double for both precisions and rounded once; the order of the sum is unspecified.  An entry is
 *      kept even if its sum is zero.  Rows are compacted to the front of col_ids / data, row_offsets is rewritten, M->nnz and
 *      info->nnz_out are the new count; the tail of the buffers is unspecified.  A view with row_offsets[0] != 0 that has
 *      duplicates is refused with SPECK_ERR_INVALID and left as it was (without duplicates the flag changes nothing and a
 *      view is fine).
 *  A matrix that is already canonical costs one streaming read of row_offsets and col_ids and writes nothing.  The same
 *      pass is the input check: row_offsets descending or leaving [row_offsets[0], row_offsets[0] + nnz], or a column id
 *      >= cols, returns SPECK_ERR_INVALID with NO BYTE of M written; no kernel leaves the buffers on such input (the pass
 *      clamps, the sorting kernels start after its verdict).  Limits as for the multiply: rows, cols <= 2^27
 *      (SPECK_ERR_DIM_LIMIT), nnz < 2^32.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns with M complete.  With the debug option
 *      guard_bytes the canary zones of M's buffers and of the temporaries are checked after the call.
 *  Rows are handled by length: <= SPECK_SORT_REG_MAX entries in registers (when the row's column range is below 2^24 - 1),
 *      <= SPECK_SORT_LDS_MAX in LDS, longer ones by a radix sort through global memory; options sort_reg_max / sort_lds_max
 *      lower the two limits (values are clamped to the constants). ---- */
enum { SPECK_SORT_KEEP_DUPLICATES = 0, SPECK_SORT_SUM_DUPLICATES = 1 };
#define SPECK_SORT_REG_MAX 256
#define SPECK_SORT_LDS_MAX 4096
typedef struct speck_sort_info {
    uint64_t rows_in_order;      /* rows that were strictly ascending already: not touched */
    uint64_t rows_sorted[3];     /* rows handled by the register / LDS / global-memory class */
    uint64_t duplicates;         /* entries whose column equals that of an earlier entry of their row (found, and
                                    with SUM_DUPLICATES removed) */
    uint64_t nnz_out;            /* nnz after the call */
} speck_sort_info;
int speck_sort_rows_f64(speck_config *cfg, speck_dcsr *M, int flags, speck_sort_info *info /* may be NULL */);
int speck_sort_rows_f32(speck_config *cfg, speck_dcsr *M, int flags, speck_sort_info *info);

/* ---- masked SpGEMM (new: the reference has no counterpart): C = M o (A B), the product kept only where the mask M has an
 *      entry -- triangle counting L o (L L), a Galerkin product kept on the pattern of A, the gradient of a sparse product
 *      with respect to a sparse operand.  The table a row accumulates in is its mask row: nothing beyond nnz(M) entries is
 *      counted, allocated, sorted or stored.
 *  M is rows(A) x cols(B); only its pattern is read, M->data may be NULL.  A row of M that is not strictly ascending or holds
 *      an id >= cols(B): SPECK_ERR_UNSORTED (as for B in the multiply; the remedy is speck_sort_rows_*).  A and B under the
 *      multiply's preconditions with the multiply's statuses (a row of B not strictly ascending or an id >= cols(B):
 *      SPECK_ERR_UNSORTED; an id of A >= rows(B): SPECK_ERR_INVALID), checked with every call.  Offsets of A / M descending or
 *      leaving [row_offsets[0], row_offsets[0] + nnz], inconsistent shapes, NULL buffers with nnz > 0, unknown flags, C sharing
 *      a buffer with A, B or M: SPECK_ERR_INVALID.  rows, cols <= 2^27 and fewer than 2^32 products in any one row
 *      (SPECK_ERR_DIM_LIMIT), nnz < 2^32.  A and M may both be row-range views with absolute offsets (sharding: rank p
 *      passes its rows of both).
 *  SPECK_MASK_STRUCTURE: C(i,j) exists iff (i,j) is in M AND some k has (i,k) in A and (k,j) in B -- structural, as in the
 *      multiply: an entry whose products cancel to 0.0 stays.  Offsets and column ids are bit for bit what speck_multiply_*
 *      followed by "keep (i,j) in M" gives; the values are the sums of a*b in unspecified order, each product rounded to the
 *      value type, the sum kept in double and rounded once (the multiply's bound).  Rows ascending: the mask row's order is
 *      the output order.
 *  SPECK_MASK_FULL_PATTERN: C has exactly M's pattern (offsets rebased to 0), +0.0 where no product falls -- the sampled
 *      product; no count, scan or compaction.
 *  Ownership of C as speck_multiply_* documents it: row_offsets reused when C->rows == A->rows, data / col_ids re-allocated
 *      only when C->nnz differs from the result's.  On any error the struct, its allocations AND the contents of C are
 *      untouched: there is no speculative path here.  No kernel uses a column id of A to index B->row_offsets, or an offset
 *      to index col_ids, before it has been checked, and nothing of C is written before the verdict on all three inputs
 *      is in.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns with C complete.  Temporaries are grow-only
 *      buffers of the config's own (not the multiply's arena: a masked call between two identical multiplies does not disturb
 *      the second one's reuse sequence), released with it; cfg == NULL is allowed as for speck_sort_rows_*.  With the debug
 *      option guard_bytes the canary zones of the temporaries and of C are checked after the call.
 *  Rows are handled by the length of their mask row: <= SPECK_MASK_GROUP_MAX entries by 8 / 16 / 32 / 64 lanes, several rows
 *      per workgroup; <= SPECK_MASK_LDS_MAX by a workgroup with a table in LDS; longer ones through global memory.  Options
 *      mask_group_max / mask_lds_max lower the two limits (values are clamped to the constants). ---- */
enum { SPECK_MASK_STRUCTURE = 0, SPECK_MASK_FULL_PATTERN = 1 };
#define SPECK_MASK_GROUP_MAX 256
#define SPECK_MASK_LDS_MAX 4096
typedef struct speck_masked_info {
    uint64_t rows_idle;          /* rows with an empty mask row or an empty row of A: no product is formed for them */
    uint64_t rows_class[3];      /* rows with work, by mask-row length: group / LDS / global-memory class */
    uint64_t products;           /* products a(i,k)*b(k,j) of the rows with work */
    uint64_t hits;               /* ... of which (i,j) is in the mask */
    uint64_t nnz_out;            /* nnz(C) */
} speck_masked_info;
int speck_multiply_masked_f64(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B, const speck_dcsr *M,
                              speck_dcsr *C, int flags, speck_masked_info *info /* may be NULL */);
int speck_multiply_masked_f32(speck_config *cfg, const speck_dcsr *A, const speck_dcsr *B, const speck_dcsr *M,
                              speck_dcsr *C, int flags, speck_masked_info *info);

/* ---- filter (new: the reference has no counterpart): C = the entries of A that every selected predicate keeps -- the
 *      strict lower triangle of a matrix that is already on the device (triangle counting: L o (L L)), "keep (i,j) in M"
 *      behind a full product and its complement (frontiers, new edges only), the explicit zeros a product leaves where its
 *      terms cancel, everything below a tolerance.  Every row of C is the row of A without the dropped entries, IN INPUT ORDER;
 *      column ids and values are copied bit for bit (-0.0, NaN payloads and subnormals survive).  Rows of A need NOT be
 *      sorted or free of duplicates.
 *  flags selects the predicates; an entry is kept iff EVERY selected one holds; SPECK_SELECT_NOT_x negates predicate x.
 *      flags == 0 keeps everything (speck_dcsr_copy with the offsets rebased).  A NOT_x bit without x, or an unknown bit:
 *      SPECK_ERR_INVALID.
 *  SPECK_SELECT_BAND: band_lo <= (int64)col - (int64)(row_base + i) <= band_hi, i the row inside A.  band_lo = INT64_MIN /
 *      band_hi = INT64_MAX leave that side open: tril(k) is hi = k, triu(k) is lo = k, the diagonal lo = hi = 0, off the
 *      diagonal the same with NOT_BAND.  band_lo > band_hi, or row_base > 2^62: SPECK_ERR_INVALID.  row_base is the global
 *      index of A's first row where A is a row-range view of a larger matrix, else 0; the other predicates ignore it.
 *  SPECK_SELECT_ABS: !(|v| <= abs_threshold), compared in double for both value types (a float is widened; the threshold
 *      is never rounded).  Written that way a NaN VALUE IS KEPT: a filter must not hide one.  With NOT_ABS the test is
 *      |v| <= abs_threshold, and a NaN is dropped.  abs_threshold = 0 drops exactly +0.0 and -0.0.  The threshold is >= 0 and
 *      may be +inf; NaN or negative: SPECK_ERR_INVALID.
 *  SPECK_SELECT_PATTERN: (i,j) is an entry of *pattern, a matrix of rows(A) x cols(A) of which only the pattern is read
 *      (data may be NULL).  A row of it that is not strictly ascending or holds an id >= cols: SPECK_ERR_UNSORTED (the
 *      remedy is speck_sort_rows_*, as for the mask of the masked product).  A and pattern may both be row-range views
 *      with absolute offsets.
 *  Offsets of A / pattern descending or leaving [row_offsets[0], row_offsets[0] + nnz], a last offset of A that is not
 *      row_offsets[0] + nnz (as for speck_reduce_*: the declared nnz is what the rows hold), a column id of A >= cols, NULL
 *      buffers with nnz > 0, a NULL pattern or one of another shape, C sharing a buffer with A or pattern:
 *      SPECK_ERR_INVALID.  rows, cols <= 2^27 (SPECK_ERR_DIM_LIMIT), nnz < 2^32.
 *  Ownership of C as speck_multiply_* and speck_multiply_masked_* document it: row_offsets reused when C->rows == A->rows,
 *      data / col_ids re-allocated only when C->nnz differs from the result's (a result of 0 entries owns buffers of one
 *      entry).  On any error the struct, its allocations AND the contents of C are untouched.  One pass checks the inputs and
 *      marks the entries; it clamps and never follows an offset or id it has not checked, and every kernel that writes C
 *      starts after the host has read its verdict.
 *  There is NO in-place mode: rows moving left inside one buffer in parallel race (a workgroup overwrites entries another
 *      has not read yet), and the way round it that the row sort takes -- compact into a temporary, copy back -- costs the
 *      memory of the second matrix anyway.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns with C complete.  Temporaries are grow-only
 *      buffers of the config's own (not the multiply's arena: a select between two identical multiplies does not disturb
 *      the second one's reuse sequence), released with it; cfg == NULL is allowed as for speck_sort_rows_*.  With the debug
 *      option guard_bytes the canary zones of the temporaries and of C are checked after the call.
 *  The marking pass walks tiles of SPECK_SELECT_TILE_ROWS_LONG rows where a row of A (and of pattern) holds
 *      SPECK_SELECT_LONG_ROW_AVG entries or more on average, of SPECK_SELECT_TILE_ROWS_SHORT rows elsewhere. ---- */
enum { SPECK_SELECT_BAND = 1, SPECK_SELECT_ABS = 2, SPECK_SELECT_PATTERN = 4,
       SPECK_SELECT_NOT_BAND = 16, SPECK_SELECT_NOT_ABS = 32, SPECK_SELECT_NOT_PATTERN = 64 };
#define SPECK_SELECT_TILE_ROWS_LONG 256
#define SPECK_SELECT_TILE_ROWS_SHORT 1024
#define SPECK_SELECT_LONG_ROW_AVG 32
typedef struct speck_select_params {
    uint32_t flags;              /* SPECK_SELECT_* */
    int64_t band_lo, band_hi;    /* BAND */
    uint64_t row_base;           /* BAND: global index of A's first row */
    double abs_threshold;        /* ABS */
    const speck_dcsr *pattern;   /* PATTERN */
} speck_select_params;
typedef struct speck_select_info {
    uint64_t kept;               /* entries of A that went to C */
    uint64_t dropped;            /* ... and that did not */
    uint64_t rows_unchanged;     /* rows that kept every entry (empty rows among them) */
    uint64_t nnz_out;            /* nnz(C) = kept */
} speck_select_info;
int speck_select_f64(speck_config *cfg, const speck_dcsr *A, const speck_select_params *p, speck_dcsr *C,
                     speck_select_info *info /* may be NULL */);
int speck_select_f32(speck_config *cfg, const speck_dcsr *A, const speck_select_params *p, speck_dcsr *C,
                     speck_select_info *info);

/* ---- addition (new: the reference has no counterpart): C = alpha A + beta B on two matrices that are already on the
 *      device -- S + S^T (a graph symmetrised before tril and the triangle count), C + A B accumulated over several
 *      products (Galerkin terms, the shards of a column-split product), the difference A - B of two results, alpha A alone.
 *  SPECK_ADD_UNION is the only mode; any other flags value: SPECK_ERR_INVALID.  C(i,j) exists iff (i,j) is in A or in B --
 *      structural, as in the multiply: an entry that cancels to 0.0 stays, and alpha == 0 or beta == 0 removes nothing and
 *      shields nothing (0 * inf is NaN).  Rows of C strictly ascending, offsets from 0: C is a valid input of every
 *      speck_multiply_*.
 *  Values are computed in double for both value types T (alpha and beta are never rounded): an entry of A alone is
 *      T(alpha a), one of B alone T(beta b), one of both T(alpha a + beta b) -- each product rounded to double, the sum
 *      rounded to double, then once to T; no fused multiply-add.  Bit for bit alpha * a.astype(f64) + beta * b.astype(f64)
 *      of numpy, cast to T.  Deterministic from run to run: every entry of C is written once by one thread, there are no
 *      atomics on values.  Subnormal results are kept.
 *  A and B under the multiply's rules for its B, checked with every call: a row of either that is not strictly ascending
 *      or holds an id >= cols: SPECK_ERR_UNSORTED (the remedy is speck_sort_rows_*).  Offsets descending or leaving
 *      [row_offsets[0], row_offsets[0] + nnz], a last offset that is not row_offsets[0] + nnz, rows(A) != rows(B) or cols(A) != cols(B), NULL buffers with nnz > 0, C sharing
 *      a buffer with A or B: SPECK_ERR_INVALID.  rows, cols <= 2^27 (SPECK_ERR_DIM_LIMIT).  nnz(A) + nnz(B) >= 2^32:
 *      SPECK_ERR_NNZ_OVERFLOW before anything runs -- conservative, an overlap might have fitted, but it is known without a
 *      device and keeps every count in 32 bits.  A and B may be the SAME matrix, and they may be row-range views with
 *      absolute offsets, each with its own base.
 *  Ownership of C as speck_select_* documents it: row_offsets reused when C->rows == A->rows, data / col_ids re-allocated
 *      only when C->nnz differs from the result's (a result of 0 entries owns buffers of one entry).  On any error the
 *      struct, its allocations AND the contents of C are untouched.  One pass checks both inputs and marks the entries
 *      that lie in both; it clamps and never follows an offset or id it has not checked, and every kernel that writes C
 *      starts after the host has read its verdict (one read-back per call).  There is NO in-place A += B, for the reason
 *      speck_select_* gives.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns with C complete.  Temporaries are grow-only
 *      buffers of the config's own (not the multiply's arena: an add between two identical multiplies does not disturb the
 *      second one's reuse sequence), released with it; cfg == NULL is allowed as for speck_sort_rows_*.  With the debug
 *      option guard_bytes the canary zones of the temporaries and of C are checked after the call.
 *  The marking pass walks tiles of SPECK_ADD_TILE_ROWS_LONG rows where a row of A and of B together hold
 *      SPECK_ADD_LONG_ROW_AVG entries or more on average, of SPECK_ADD_TILE_ROWS_SHORT rows elsewhere; the pass that writes C
 *      walks each operand in tiles of SPECK_ADD_TILE_ENTRIES entries. ---- */
enum { SPECK_ADD_UNION = 0 };
#define SPECK_ADD_TILE_ROWS_LONG 256
#define SPECK_ADD_TILE_ROWS_SHORT 1024
#define SPECK_ADD_LONG_ROW_AVG 32
#define SPECK_ADD_TILE_ENTRIES 4096
typedef struct speck_add_info {
    uint64_t only_a, only_b, both;   /* entries of C that come from A alone / B alone / from both */
    uint64_t nnz_out;                /* nnz(C) = only_a + only_b + both */
} speck_add_info;
int speck_add_f64(speck_config *cfg, double alpha, const speck_dcsr *A, double beta, const speck_dcsr *B, speck_dcsr *C,
                  int flags, speck_add_info *info /* may be NULL */);
int speck_add_f32(speck_config *cfg, double alpha, const speck_dcsr *A, double beta, const speck_dcsr *B, speck_dcsr *C,
                  int flags, speck_add_info *info);

/* ---- reduction (new: the reference has no counterpart): per row and over all entries of a matrix that is already on the
 *      device, a sum or an extremum -- the triangle count and the per-vertex counts behind symmetrize -> tril ->
 *      multiply_masked, the max-abs or Frobenius norm of a residual A - B, the row sums, row norms and largest entries
 *      that a row normalisation or a pruning threshold asks of a product.  The one map matrix -> vector / scalar.
 *  d_row_out[i] (a DEVICE array of A->rows doubles, may be NULL) is the reduction of row i, *h_total (HOST, may be NULL)
 *      that of all entries; both NULL: SPECK_ERR_INVALID.  Results are double for both value types: a float is widened
 *      exactly and never rounded back.
 *  SUM adds v, ABS_SUM |v|, SQ_SUM v v (each square rounded to double before it is added, no fused multiply-add: every code
 *      path adds the same terms); MAX / MIN / ABS_MAX take the largest v, the smallest v, the largest |v|.  A row without
 *      an entry (and the total of a matrix without one) is +0.0 for the three sums and ABS_MAX, -inf for MAX, +inf for MIN.
 *      A NaN entry makes its row's result and the total NaN for EVERY op -- the extrema do not drop it as fmax does: a NaN
 *      is not hidden -- and touches no other row.  Infinities follow IEEE (inf + -inf is NaN).  The sign of a zero result
 *      is unspecified.
 *  No floating-point atomic anywhere.  Every result comes from a combination tree that depends only on the ABSOLUTE
 *      positions of the entries in data (counted from the buffer's start, not from row_offsets[0]): the same call gives
 *      the same bits from run to run, and a row-range view gives bit for bit the rows r0..r1 of the whole matrix's result
 *      -- a row-sharded reduction equals the unsharded one.  The total is reproducible from run to run; its tree is
 *      otherwise unspecified.  Against the exact sum |got - exact| <= g_n sum|term|, g_n = n 2^-53 / (1 - n 2^-53), n the
 *      number of terms of the row (of the matrix, for the total): the bound of any summation order.  The extrema are exact.
 *  Only row_offsets and data are read: col_ids is never dereferenced and may be NULL or garbage, and rows need not be
 *      sorted or free of duplicates.  Offsets descending, leaving [row_offsets[0], row_offsets[0] + nnz], or a last offset
 *      that is not row_offsets[0] + nnz: SPECK_ERR_INVALID.  NULL A, NULL row_offsets, data == NULL with nnz > 0, an unknown
 *      op, d_row_out equal to one of A's three pointers: SPECK_ERR_INVALID.  rows > 2^27: SPECK_ERR_DIM_LIMIT.  nnz >= 2^32:
 *      SPECK_ERR_NNZ_OVERFLOW.  A may be a row-range view with absolute offsets; rows == 0 or nnz == 0 is valid (identities).
 *  On any error d_row_out and *h_total are untouched (*info is zero once the arguments have passed).  No offset is used as
 *      an address before it was checked, and there is NO read-back in the middle of the call: a checking pass raises the
 *      verdict in a status block, the kernels that read data and write results are queued behind it and do nothing where it
 *      is raised, and the host reads the status once, at the end -- the verdict, the counters, the total.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns with the results complete.  Temporaries
 *      are grow-only buffers of the config's own (not the multiply's arena: a reduce between two identical multiplies does
 *      not disturb the second one's reuse sequence), released with it; cfg == NULL is allowed as for speck_sort_rows_*.
 *      With the debug option guard_bytes the canary zones of the temporaries are checked after the call.
 *  The entries are walked in tiles of SPECK_REDUCE_TILE_ENTRIES, aligned to absolute positions; a thread holds
 *      SPECK_REDUCE_THREAD_ENTRIES consecutive ones, a wave SPECK_REDUCE_WAVE_ENTRIES.  One path for every row length.
 *  Not built: column reductions (transpose, then reduce); counts (a row's is the difference of two offsets); means;
 *      user-defined monoids; a reduce fused into the product that made A. ---- */
enum { SPECK_REDUCE_SUM = 0, SPECK_REDUCE_ABS_SUM = 1, SPECK_REDUCE_SQ_SUM = 2,
       SPECK_REDUCE_MAX = 3, SPECK_REDUCE_MIN = 4, SPECK_REDUCE_ABS_MAX = 5 };
#define SPECK_REDUCE_TILE_ENTRIES 4096
#define SPECK_REDUCE_THREAD_ENTRIES 16
#define SPECK_REDUCE_WAVE_ENTRIES 1024
typedef struct speck_reduce_info {
    uint64_t rows_empty;   /* rows without an entry: they receive the identity */
    uint64_t rows_split;   /* rows whose entries lie in more than one tile */
    uint64_t tiles;        /* tiles walked */
    uint64_t entries;      /* entries reduced = nnz */
} speck_reduce_info;
int speck_reduce_f64(speck_config *cfg, const speck_dcsr *A, int op, double *d_row_out, double *h_total,
                     speck_reduce_info *info /* may be NULL */);
int speck_reduce_f32(speck_config *cfg, const speck_dcsr *A, int op, double *d_row_out, double *h_total,
                     speck_reduce_info *info);

/* ---- scaling (new: the reference has no counterpart): C(i,j) = ((alpha g(A(i,j))) (.) l[i]) (.) r[j] on the pattern of a
 *      matrix that is already on the device -- the one map from a device vector back into a matrix, as speck_reduce_* is
 *      the one out of it: the row normalisation of a product by its row sums (Markov matrices, the inflation v v and the
 *      normalisation of an MCL step), D^-1/2 (S + S^T) D^-1/2 with one vector on both sides, D^-1 A of a Jacobi-smoothed
 *      prolongator, the indicator matrix of a weighted graph before a triangle count.  g is p->map: IDENTITY, ABS |v|,
 *      SQUARE v v, ONE (1.0 whatever the entry holds, a NaN included).  The vectors are optional; each multiplies
 *      (SPECK_SCALE_MUL) or divides (SPECK_SCALE_DIV).  C == NULL works IN PLACE -- the structure does not change, so
 *      this is the one side operation that can.
 *  Values: every step in double for both value types, in this order: x = (double)a; x = g(x); x = alpha * x (always);
 *      x = x * l[i] or x / l[i] where row_mode is set; x = x * r[j] or x / r[j] where col_mode is set; ONE rounding to T.
 *      Each step is rounded to double on its own, the division is the correctly rounded IEEE division, nothing is fused:
 *      every result that is not a NaN is bit for bit numpy's (((alpha * g(a.astype(f64))) (.) l[row]) (.) r[col]).astype(T),
 *      signed zeros and subnormals included, and a NaN stands exactly where numpy has one.  Nothing is hidden: 0 * inf,
 *      x / 0, a NaN in a vector land in the entry; info->nonfinite counts the results that are inf or NaN AFTER the
 *      rounding to T, and they do not make the call fail.  Every entry is written once by one thread: the same bits from
 *      run to run.  Structural: no entry is dropped, a result of 0.0 stays (as in speck_add_*).
 *  d_row (DEVICE, A->rows doubles) is indexed by the row INSIDE A -- for a row-range view the caller offsets the pointer,
 *      not the library; d_col (DEVICE, A->cols doubles) by the column id.  The two may be the same array.  A mode set with
 *      a NULL vector, a vector given with mode NONE, a vector equal to one of A's or C's three pointers, an unknown map
 *      or mode, alpha NaN: SPECK_ERR_INVALID.
 *  In place (C == NULL): only A->data[row_offsets[0] .. row_offsets[0] + nnz) is written; row_offsets, col_ids, nnz and
 *      the three pointers stay as they were.  On a row-range view with absolute offsets only the view's entries are
 *      touched: the owner's entries in front of and behind them keep their bytes.
 *  Out of place: C receives A's pattern -- the offsets rebased to 0, col_ids copied bit for bit -- under the ownership
 *      rule of speck_select_*: rows(C) == rows(A) keeps C->row_offsets, nnz(C) == nnz(A) keeps data / col_ids, anything
 *      else is freed and re-allocated; C sharing a buffer with A: SPECK_ERR_INVALID.
 *  Rows need not be sorted or free of duplicates.  col_ids is read only where col_mode != NONE or C != NULL: in place
 *      without a column vector it may be NULL or garbage.  Offsets descending, leaving [row_offsets[0], row_offsets[0] +
 *      nnz], or a last offset that is not row_offsets[0] + nnz; a column id >= cols where col_ids is read; NULL A or p,
 *      NULL row_offsets, data == NULL with nnz > 0: SPECK_ERR_INVALID.  rows or cols > 2^27: SPECK_ERR_DIM_LIMIT.
 *      nnz >= 2^32: SPECK_ERR_NNZ_OVERFLOW.  rows == 0 or nnz == 0 is valid.
 *  On any error NOTHING is written: not A->data, not C's buffers, not C's struct (*info is zero once the arguments have
 *      passed).  As in speck_reduce_*: no offset or column id is used as an address before it was checked; a checking pass
 *      raises its verdict in a status block, the kernels that write are queued behind it and do nothing where it is raised,
 *      and the host reads the status ONCE, at the end -- the verdict, nonfinite.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns complete.  Temporaries are two grow-only
 *      buffers of the config's own (not the multiply's arena: a scale between two identical multiplies does not disturb
 *      the second one's reuse sequence), released with it; cfg == NULL is allowed as for speck_sort_rows_*.  With the debug
 *      option guard_bytes the canary zones of the temporaries and of C (in place: of A's buffers) are checked after the call.
 *  Without a row vector the call is a plain stream over the entries, 16 bytes per lane and step, and knows nothing of rows
 *      beyond the check of the offsets (info->tiles is 0).  With one the entries are walked in tiles of
 *      SPECK_SCALE_TILE_ENTRIES, aligned to absolute positions as the reduction's; one path for every row length; l[i]
 *      is loaded once per row segment.  The 16-byte form needs data (and col_ids where read) on 16-byte boundaries and,
 *      out of place, row_offsets[0] a multiple of 4; elsewhere the entries go one by one, with the same results.
 *  Not built: pow and other libm maps (not bit-reproducible against numpy; the row softmax, exp included, is
 *      speck_softmax_*); sqrt modes (the vector is the caller's: a torch rsqrt_ on it is plumbing); per-row thresholds in speck_select_*; a scale fused into the product that made A;
 *      vectors in float. ---- */
enum { SPECK_MAP_IDENTITY = 0, SPECK_MAP_ABS = 1, SPECK_MAP_SQUARE = 2, SPECK_MAP_ONE = 3 };
enum { SPECK_SCALE_NONE = 0, SPECK_SCALE_MUL = 1, SPECK_SCALE_DIV = 2 };
#define SPECK_SCALE_TILE_ENTRIES 4096
typedef struct speck_scale_params {
    uint32_t map;                 /* SPECK_MAP_*   */
    uint32_t row_mode, col_mode;  /* SPECK_SCALE_* */
    double alpha;
    const double *d_row;          /* DEVICE, A->rows doubles, indexed by the row INSIDE A (a view offsets the pointer) */
    const double *d_col;          /* DEVICE, A->cols doubles */
} speck_scale_params;
typedef struct speck_scale_info {
    uint64_t entries;             /* entries written = nnz */
    uint64_t nonfinite;           /* ... of which the result, after rounding to T, is inf or NaN */
    uint64_t tiles;               /* entry tiles walked (0 for a call without a row vector: it has no tiles) */
} speck_scale_info;
int speck_scale_f64(speck_config *cfg, const speck_dcsr *A, const speck_scale_params *p, speck_dcsr *C /* NULL: in place */,
                    speck_scale_info *info /* may be NULL */);
int speck_scale_f32(speck_config *cfg, const speck_dcsr *A, const speck_scale_params *p, speck_dcsr *C,
                    speck_scale_info *info);

/* ---- matrix-vector product (new: the reference has no counterpart): y = alpha A x + beta y on a matrix that is already
 *      on the device -- the one map (matrix, vector) -> vector beside speck_reduce_* (matrix -> vector) and speck_scale_*
 *      (vector -> matrix): a PageRank or power iteration on the row-normalised matrix, the residual b - A x or a Jacobi
 *      sweep beside the Galerkin product, the check || A x - P (Q x) || of a product that never downloads it.
 *  d_x is a DEVICE array of A->cols doubles, indexed by the column id; d_y a DEVICE array of A->rows doubles, indexed by
 *      the row INSIDE A -- for a row-range view the caller offsets the pointer, as for speck_scale_*.  The vectors are
 *      double for both value types.
 *  Values: every step in double, each rounded on its own, nothing fused.  The term of an entry is t = (double)a * x[j],
 *      rounded once; s_i is the combination of the row's terms in the SAME TREE speck_reduce_* uses for SPECK_REDUCE_SUM,
 *      a function of the absolute positions of the entries in data alone; a row without entries has s_i = +0.0.  Then
 *      y_i = alpha * s_i + beta * y_i: two products, each rounded, and one sum.  beta == 0.0 means y is NOT READ:
 *      y_i = alpha * s_i, and a NaN or garbage in y does not survive (the BLAS convention -- unlike speck_add_*, where a
 *      zero coefficient shields nothing and 0 * NaN stays NaN).  alpha is always applied (alpha == 0 with an infinite s_i
 *      is NaN).  Nothing else is hidden: 0 * inf, a NaN in x or in A land in exactly the rows that reference them and in
 *      no other row.  The sign of a zero s_i is unspecified, as in the reduction.
 *  What follows: the same bits from run to run; a row-range view gives bit for bit the rows of the whole matrix's result
 *      -- a row-sharded product equals the unsharded one; for fp64 with alpha = 1, beta = 0, y equals bit for bit the row
 *      results of speck_reduce_f64(SUM) on speck_scale_f64(A, col = x, MUL), NaN where that has a NaN; and
 *      |s_i - exact| <= g_n sum|t| with the reduction's g_n.  No floating-point atomic anywhere.
 *  Rows need not be sorted or free of duplicates: duplicates simply add.  Offsets descending, leaving [row_offsets[0],
 *      row_offsets[0] + nnz], or a last offset that is not row_offsets[0] + nnz; a column id >= cols; NULL A, NULL
 *      row_offsets or NULL d_y with rows > 0; NULL d_x, data or col_ids with nnz > 0; alpha or beta NaN; d_x or d_y equal
 *      to one of A's three pointers; the ranges [d_x, d_x + cols) and [d_y, d_y + rows) overlapping: SPECK_ERR_INVALID.
 *      rows or cols > 2^27: SPECK_ERR_DIM_LIMIT.  nnz >= 2^32: SPECK_ERR_NNZ_OVERFLOW.  rows == 0 is valid and writes
 *      nothing; nnz == 0 is valid and gives y_i = alpha * (+0.0) + beta * y_i.
 *  On any error NOTHING of y is written (*info is zero once the arguments have passed).  No offset or column id is used as
 *      an address before it was checked: the kernels that read the entries are queued behind the verdict on the offsets,
 *      an id >= cols raises the verdict and is not followed, and the row sums wait in a temporary of rows doubles until the
 *      kernel queued last has seen the verdict of EVERY tile -- only it writes y, each row once by one thread.  There is NO
 *      read-back in the middle of the call: the host reads the status block once, at the end.
 *  Runs on the config's stream (speck_config_set_stream is honoured) and returns complete.  Temporaries are grow-only
 *      buffers of the config's own (not the multiply's arena: a spmv between two identical multiplies does not disturb the
 *      second one's reuse sequence), released with it; cfg == NULL is allowed as for speck_reduce_*.  With the debug
 *      option guard_bytes their canary zones are checked after the call.
 *  The entries are walked in tiles of SPECK_SPMV_TILE_ENTRIES, the reduction's, aligned to absolute positions; one path for
 *      every row length.  The 16-byte loads need data and col_ids on 16-byte boundaries; elsewhere the entries are loaded
 *      one by one, with the same results.
 *  Not built (A^T x: speck_spmm_t_* below with k = 1; (min, +) and kin: speck_spmv_sr_* below): vectors in float; a spmv
 *      fused into the product that made A.  (Several right-hand sides: speck_spmm_* below.) ---- */
#define SPECK_SPMV_TILE_ENTRIES 4096
typedef struct speck_spmv_info {
    uint64_t rows_empty;   /* rows without an entry: s_i = +0.0 */
    uint64_t rows_split;   /* rows whose entries lie in more than one tile */
    uint64_t tiles;        /* tiles walked */
    uint64_t entries;      /* entries multiplied = nnz */
} speck_spmv_info;
int speck_spmv_f64(speck_config *cfg, double alpha, const speck_dcsr *A, const double *d_x, double beta, double *d_y,
                   speck_spmv_info *info /* may be NULL */);
int speck_spmv_f32(speck_config *cfg, double alpha, const speck_dcsr *A, const double *d_x, double beta, double *d_y,
                   speck_spmv_info *info);

/* ---- product with several right-hand sides (new: the reference has no counterpart): Y = alpha A X + beta Y, the block of
 *      k vectors a block power or LOBPCG iteration, personalised PageRank for many seeds, a smoother applied to several
 *      near-null-space vectors, the feature aggregation A X of a graph layer or a check with several probes holds.  A is
 *      read ONCE for all k columns; the offsets and the ids are checked once and there is one read-back, where k calls of
 *      speck_spmv_* read data and col_ids k times, queue 4 k launches and wait for k read-backs.
 *  X is cols x k and Y is rows x k, both ROW-MAJOR DEVICE arrays of doubles for both value types: X(j,c) = d_X[j ldx + c],
 *      Y(i,c) = d_Y[i ldy + c] with ldx >= k, ldy >= k -- a contiguous torch tensor or a column slice of one.  (Row-major
 *      makes the gather of an entry's k values one contiguous read.)  The padding [k, ldx) of every row of X is never
 *      read; the padding [k, ldy) of every row of Y is never read or written.  Y is indexed by the row INSIDE A: for a
 *      row-range view the caller offsets the pointer by r0 ldy.  All index arithmetic i ld + c is 64-bit.
 *  The defining property: for every c < k, column c of Y is BIT FOR BIT what speck_spmv_*(alpha, A, X(:,c), beta, Y(:,c))
 *      writes on contiguous copies of the two columns.  So everything said there holds per column: the term
 *      (double)a * X(j,c) rounded once, nothing fused; the tree of speck_reduce_*(SUM) over the absolute positions of the
 *      entries; the same bits from run to run; a row-range view gives the rows of the whole result; beta == 0.0 does NOT
 *      READ Y; alpha is always applied; a NaN or 0 * inf of X(j,c) lands in column c of exactly the rows that reference
 *      j and nowhere else; duplicates add, rows need not be sorted.  k == 1 with ldx == ldy == 1 is speck_spmv_*.  No
 *      floating-point atomic anywhere.
 *  Refused before anything runs: all that speck_spmv_* refuses, with the vectors' ranges replaced by the SPANS
 *      [d_X, d_X + (cols - 1) ldx + k) and [d_Y, d_Y + (rows - 1) ldy + k) -- padding between the rows included, so two
 *      column slices of ONE tensor interleave and are refused (SPECK_ERR_INVALID) although they share no element; spans
 *      that touch are served.  ldx < k or ldy < k: SPECK_ERR_INVALID.  k > SPECK_SPMM_MAX_RHS, ldx or ldy > 2^32, rows or
 *      cols > 2^27: SPECK_ERR_DIM_LIMIT.  k == 0 or rows == 0: SPECK_OK, nothing written, *info zero.  nnz == 0 is valid
 *      and gives Y = alpha * (+0.0) + beta * Y.
 *  On any error NOTHING of Y is written (*info is zero once the arguments have passed).  No offset or column id is used as
 *      an address before it was checked; an id >= cols raises the verdict, is clamped and never followed; the row sums
 *      wait in a temporary of rows k doubles until the kernel queued last has seen the verdict of EVERY tile -- only it
 *      writes Y, each element once by one thread.  One read-back, at the end.
 *  Config stream, cfg == NULL and the guard_bytes canary zones as for speck_spmv_*; the temporaries are grow-only buffers
 *      of the config's own, neither the multiply's arena nor those of speck_spmv_*.
 *  The tiles are speck_spmv_*'s, each walked once: a thread keeps its 16 values and checked ids and takes the k columns in
 *      blocks of SPECK_SPMM_COLUMN_BLOCK whose gathers are in flight together -- one 16-byte load per entry and pair of
 *      columns where d_X lies on a 16-byte boundary and ldx is even, 8-byte loads elsewhere, with the same results.
 *  info: rows_empty, rows_split, tiles and entries as speck_spmv_info -- they describe A, not k.
 *  Not built (A^T X: speck_spmm_t_* below; float blocks: speck_spmm_*_b32 below; (min, +) and kin: speck_spmm_sr_* below):
 *      column-major vectors. ---- */
#define SPECK_SPMM_MAX_RHS 1024
#define SPECK_SPMM_COLUMN_BLOCK 4
typedef struct speck_spmm_info {
    uint64_t rows_empty;   /* rows without an entry: s(i,c) = +0.0 */
    uint64_t rows_split;   /* rows whose entries lie in more than one tile */
    uint64_t tiles;        /* tiles walked (each once, for all columns) */
    uint64_t entries;      /* entries read = nnz */
    uint64_t terms;        /* products formed = entries * k */
} speck_spmm_info;
int speck_spmm_f64(speck_config *cfg, double alpha, const speck_dcsr *A, const double *d_X, uint64_t ldx, uint32_t k,
                   double beta, double *d_Y, uint64_t ldy, speck_spmm_info *info /* may be NULL */);
int speck_spmm_f32(speck_config *cfg, double alpha, const speck_dcsr *A, const double *d_X, uint64_t ldx, uint32_t k,
                   double beta, double *d_Y, uint64_t ldy, speck_spmm_info *info);

/* ---- products over a (min | max, + | x | second) semiring (new: the reference has no counterpart): what shortest paths and
 *      hop counts ((min, +)), label propagation for connected components ((min, second)), widest or most reliable paths
 *      ((max, x) on probabilities) and "best neighbour" queries need on a matrix that is already on the device.
 *      s_i = (+)_{(i,j) in A} (a_ij (x) x_j), where (+) is min or max and (x) is
 *          PLUS   (double)a_ij + x[j]          TIMES   (double)a_ij * x[j]          SECOND   x[j] alone,
 *      then y_i = s_i where d_z == NULL and y_i = z_i (+) s_i otherwise.  A row without entries has s_i = the identity:
 *      +inf for min, -inf for max.  With SECOND A->data is NEVER dereferenced: it may be NULL or garbage, and a NaN there
 *      does not show.  Vectors and blocks are doubles for both value types as for speck_spmv_* / speck_spmm_*: x / X
 *      indexed by the column id, y / Y / z / Z by the row INSIDE A; blocks row-major, X(j,c) = d_X[j ldx + c], with
 *      ld >= k and k <= SPECK_SPMM_MAX_RHS; the padding of a row of a block is neither read nor written.
 *  Values: one rounding per term, nothing fused.  min and max PROPAGATE a NaN (fmin would drop it): a NaN in x, an
 *      inf + -inf, a 0 * inf, a NaN in A (PLUS / TIMES) or a NaN in z lands in exactly the rows -- and for blocks the
 *      column -- that reference it, and in no other.  The sign of a zero result is unspecified.  min and max are EXACT,
 *      so every combination order gives the same value and the following hold with no tolerance: the same values from
 *      run to run; a row-range view gives the rows of the whole; float A equals the call on the widened matrix; column c
 *      of speck_spmm_sr_* equals speck_spmv_sr_* on contiguous copies of column c.
 *  info->changed counts the elements with y_new != z_old compared as doubles (a NaN equals a NaN, +0.0 equals -0.0); 0
 *      where d_z == NULL.  It is counted by the kernel that writes y, in integers, and comes back in the call's one
 *      read-back: it ends a relaxation loop without a download of y.
 *  Aliasing: x and z are only read; z may overlap x in any way or BE x (y = x (+) A (x) x: a Bellman-Ford step between
 *      two ping-pong buffers, no copy).  z may be exactly y -- the same pointer and, for blocks, the same ld: in place,
 *      every element is read and then written by the one thread that owns it.  Refused with SPECK_ERR_INVALID before
 *      anything runs: the range (for blocks the SPAN, padding included, as for speck_spmm_*) of y overlapping that of x;
 *      y overlapping z in any other way than being identical; any of the three pointers equal to one of A's; an unknown
 *      semiring; ld < k; and the NULL pointers speck_spmm_* refuses (d_z and, with SECOND, A->data may be NULL).
 *      Dimension and nnz limits, rows == 0, k == 0 as speck_spmm_*; nnz == 0 gives the identity, or z.
 *  Safety as for speck_spmv_* / speck_spmm_*: the offsets are checked before an entry is read; an id >= cols raises the
 *      verdict, is clamped and never followed; only the kernel queued last writes y, after it has seen the verdict of every
 *      tile; on any error NOTHING of y is written and *info is zero.  All index arithmetic i ld + c is 64-bit.  No
 *      floating-point atomic; one read-back, at the end.  Config stream, cfg == NULL and guard_bytes as there; the
 *      temporaries are grow-only buffers of the config's own, neither those of speck_spmv_* nor those of speck_spmm_*.
 *  The tiles and the walk are speck_spmv_*'s and speck_spmm_*'s (blocks of SPECK_SPMM_COLUMN_BLOCK columns, 16-byte
 *      gathers where d_X lies on a 16-byte boundary and ldx is even).
 *  Not built: argmin / parent pointers; a frontier mask; vectors in float; (or, and) on bit vectors; a semiring SpGEMM;
 *      A^T through the transpose plan (transpose A once instead). ---- */
enum { SPECK_SR_MIN_PLUS = 0, SPECK_SR_MAX_PLUS = 1, SPECK_SR_MIN_TIMES = 2, SPECK_SR_MAX_TIMES = 3,
       SPECK_SR_MIN_SECOND = 4, SPECK_SR_MAX_SECOND = 5 };
typedef struct speck_semiring_info {
    uint64_t rows_empty;   /* rows without an entry: s_i = the identity */
    uint64_t rows_split;   /* rows whose entries lie in more than one tile */
    uint64_t tiles;        /* tiles walked (each once, for all columns) */
    uint64_t entries;      /* entries read = nnz */
    uint64_t terms;        /* terms formed = entries * k (k = 1 for a vector) */
    uint64_t changed;      /* elements of y that differ from z (0 where z == NULL) */
} speck_semiring_info;
int speck_spmv_sr_f64(speck_config *cfg, int semiring, const speck_dcsr *A, const double *d_x,
                      const double *d_z /* may be NULL */, double *d_y, speck_semiring_info *info /* may be NULL */);
int speck_spmv_sr_f32(speck_config *cfg, int semiring, const speck_dcsr *A, const double *d_x,
                      const double *d_z, double *d_y, speck_semiring_info *info);
int speck_spmm_sr_f64(speck_config *cfg, int semiring, const speck_dcsr *A, const double *d_X, uint64_t ldx, uint32_t k,
                      const double *d_Z /* may be NULL */, uint64_t ldz, double *d_Y, uint64_t ldy,
                      speck_semiring_info *info /* may be NULL */);
int speck_spmm_sr_f32(speck_config *cfg, int semiring, const speck_dcsr *A, const double *d_X, uint64_t ldx, uint32_t k,
                      const double *d_Z, uint64_t ldz, double *d_Y, uint64_t ldy, speck_semiring_info *info);

/* ---- sampled dense-dense product (new: the reference has no counterpart): C = alpha (U V^T) on A's pattern + beta A, the
 *      one map (block, block) -> matrix beside speck_spmm_* ((matrix, block) -> block): d(i,j) = sum_c U(i,c) V(j,c) is
 *      computed ONLY where A holds an entry.  The gradient of speck_spmm_* with respect to A's values (dA = dY X^T on A's
 *      pattern), the edge scores of an attention layer, cosine or Gram similarities on the edges of a graph (U == V), the
 *      residual R - U V^T of a factorisation on the observed entries (alpha = -1, beta = 1).  The structure does not
 *      change, so C == NULL works IN PLACE, as speck_scale_*; k == 1 is speck_scale_* with a row and a column vector.
 *  U is rows x k and V is cols x k, both ROW-MAJOR DEVICE arrays of doubles for both value types: U(i,c) = d_U[i ldu + c],
 *      V(j,c) = d_V[j ldv + c] with ldu >= k, ldv >= k -- a contiguous torch tensor or a column slice of one.  U is
 *      indexed by the row INSIDE A (for a row-range view the caller offsets d_U by r0 ldu), V by the column id.  The
 *      padding [k, ld) of a row of U or V is never read.  All index arithmetic i ld + c is 64-bit.  U and V are only read:
 *      they may overlap each other in any way, or be one block.
 *  Values: every step in double for both value types, each rounded on its own, nothing fused.  t_c = U(i,c) * V(j,c),
 *      rounded once.  d(i,j) is the sum of the t_c in a tree that is a function of k ALONE: a group of L(k) lanes (a
 *      power of two <= 64) serves one entry; the columns are taken in pairs q = c >> 1; lane l owns the pairs q = l (mod L) and adds their terms one
 *      after the other in ascending c, starting from its first term (no zero seed); a lane that owns no column holds +0.0;
 *      the L partial sums are combined by the butterfly p = p + p[l ^ s] for s = L/2, ..., 1 (IEEE addition commutes: every
 *      lane ends with the same bits).  Then
 *        SPECK_SDDMM_AXPBY     x = alpha * d; where beta != 0.0 only: x = x + beta * (double)a, the product rounded, then
 *                              the sum.  beta == 0.0 means A->data is NOT READ: a NaN there does not survive, and out of
 *                              place A->data may be NULL (the BLAS convention, as speck_spmv_*).
 *        SPECK_SDDMM_HADAMARD  x = alpha * d; x = x * (double)a.  beta must be 0.0 (SPECK_ERR_INVALID otherwise).
 *      alpha is always applied.  ONE rounding to T.  info->nonfinite counts the results that are inf or NaN AFTER that
 *      rounding; they do not make the call fail.  k == 0 is valid: d = +0.0, and d_U, d_V may be NULL.  The sign of a
 *      zero d is unspecified, as for the reduction's s_i.
 *  L(k) = min(8, max(1, pow2ceil(ceil(k / 4)))): 1 for k <= 4, 2 for k <= 8, 4 for k <= 16, 8 beyond -- two pairs of
 *      columns per lane up to k = 32, ceil(k / 16) of them beyond.  Set from measurement (one lane per pair of columns,
 *      L up to 64, was 1.3 to 2.4 times slower from k = 8 on: DESIGN.md 4.19) and fixed: it is part of the numeric
 *      contract; info->lanes reports it.
 *  What follows: the same bits from run to run.  The bits of an entry do not depend on where the entry lies in data, on
 *      ldu or ldv, on the alignment of d_U / d_V (16-byte loads where the pointer lies on 16 bytes and ld is even, 8-byte
 *      loads elsewhere, with the same results), or on whether the call is in place.  A row-range view gives bit for bit
 *      the entries of the whole matrix's result.  For k = 1, alpha = 1, beta = 0, fp64 the result is bit for bit
 *      speck_scale_f64(A, map ONE, row = U(:,0), col = V(:,0)).  |d - exact| <= g_k sum_c |U(i,c) V(j,c)|.  A NaN or
 *      0 * inf of U(i,c) lands in exactly the entries of row i, one of V(j,c) in exactly the entries with column id j.
 *      No floating-point atomic anywhere.
 *  Structure: rows need not be sorted; duplicates each get the same value.  No entry is dropped, a result of 0.0 stays.
 *      In place (C == NULL) only A->data[row_offsets[0] .. row_offsets[0] + nnz) is written: on a row-range view the
 *      owner's entries in front of and behind the view's keep their bytes.  Out of place C receives A's pattern -- the
 *      offsets rebased to 0, col_ids copied bit for bit -- under the ownership rule of speck_scale_* / speck_select_*.
 *  Refused before anything runs, SPECK_ERR_INVALID: NULL A or p; NULL row_offsets with rows > 0; NULL d_U or d_V with
 *      nnz > 0 and k > 0; NULL col_ids with nnz > 0 and (k > 0 or C != NULL); NULL data with nnz > 0 unless the call is
 *      out of place, AXPBY and beta == 0; an unknown mode; alpha or beta NaN; ldu < k or ldv < k; nnz > 0 with rows == 0
 *      or cols == 0; the span [d_U, d_U + (rows - 1) ldu + k) or [d_V, d_V + (cols - 1) ldv + k), padding inside
 *      included, containing one of A's or C's three pointers (a span that ENDS at such a pointer is served); C sharing a
 *      buffer with A.  SPECK_ERR_DIM_LIMIT: k > SPECK_SDDMM_MAX_K; ldu or ldv > 2^32; rows or cols > 2^27.
 *      SPECK_ERR_NNZ_OVERFLOW: nnz >= 2^32.  rows == 0 or nnz == 0 is valid.
 *  Refused on the device, SPECK_ERR_INVALID: offsets descending, leaving [row_offsets[0], row_offsets[0] + nnz], or a last
 *      offset that is not row_offsets[0] + nnz; a column id >= cols.
 *  On any error NOTHING is written: not A->data, not C's buffers, not C's struct (*info is zero once the arguments have
 *      passed).  No offset or id is used as an address before it was checked: in-place output cannot wait in a temporary,
 *      so a checking pass over the offsets and ALL the ids raises its verdict in a status block, the kernels that write are
 *      queued behind it and do nothing where it is raised, and the host reads the status ONCE, at the end.
 *  Config stream, cfg == NULL, grow-only temporaries of the config's own (not the multiply's arena) and the guard_bytes
 *      canary zones: all as speck_scale_*.
 *  The entries are walked in tiles of SPECK_SDDMM_TILE_ENTRIES, aligned to absolute positions as the reduction's; one path
 *      for every row length.  The ids are loaded 16 bytes at a time where col_ids (and C's) lie on 16-byte boundaries,
 *      one by one elsewhere, with the same results.
 *  Not built (float blocks: speck_sddmm_*_b32 below): U^T / column-major blocks; a map fused behind the dot (the row
 *      softmax of the scores is the next call, speck_softmax_*, in place on the same matrix); the product fused into
 *      speck_multiply_masked_*. ---- */
#define SPECK_SDDMM_MAX_K 1024            /* = SPECK_SPMM_MAX_RHS */
#define SPECK_SDDMM_TILE_ENTRIES 4096
enum { SPECK_SDDMM_AXPBY = 0, SPECK_SDDMM_HADAMARD = 1 };
typedef struct speck_sddmm_params {
    uint32_t mode;                /* SPECK_SDDMM_* */
    uint32_t k;
    double alpha, beta;
    const double *d_U;            /* DEVICE, rows x k row-major, indexed by the row INSIDE A (a view offsets the pointer) */
    uint64_t ldu;
    const double *d_V;            /* DEVICE, cols x k row-major, indexed by the column id */
    uint64_t ldv;
} speck_sddmm_params;
typedef struct speck_sddmm_info {
    uint64_t entries;             /* entries written = nnz */
    uint64_t terms;               /* products formed = entries * k */
    uint64_t nonfinite;           /* results that, after rounding to T, are inf or NaN */
    uint64_t tiles;               /* entry tiles walked */
    uint64_t lanes;               /* L(k) */
} speck_sddmm_info;
int speck_sddmm_f64(speck_config *cfg, const speck_dcsr *A, const speck_sddmm_params *p, speck_dcsr *C /* NULL: in place */,
                    speck_sddmm_info *info /* may be NULL */);
int speck_sddmm_f32(speck_config *cfg, const speck_dcsr *A, const speck_sddmm_params *p, speck_dcsr *C,
                    speck_sddmm_info *info);

/* ---- row softmax (new: the reference has no counterpart): the softmax of every row over the entries the row holds, on a
 *      matrix that is already on the device, and its backward -- the step between speck_sddmm_* (the edge scores) and
 *      speck_spmm_* (the aggregation) of an attention layer on a graph (GAT, graph transformers, sparse attention with a
 *      fixed pattern): sddmm -> softmax -> spmm runs on one device CSR, in place, and with SPECK_SOFTMAX_BACKWARD (sddmm
 *      and spmm being each other's gradients) the layer can be trained.  The structure does not change, so C == NULL works
 *      IN PLACE, as speck_scale_*.
 *  Values: every step in double for both value types, each rounded on its own, nothing fused; ONE rounding to T at the end.
 *      Forward, for an entry a of row i:  x = alpha * (double)a (first: any finite alpha of either sign is served);
 *      m_i = the largest x of the row, as speck_reduce_*(MAX) combines (a NaN comes out; exact, so no tree matters);
 *      e = exp(x - m_i), the device's double exp;  s_i = the sum of the row's e IN THE TREE OF speck_reduce_*(SUM) -- over
 *      the absolute positions of the entries;  SPECK_SOFTMAX_NORMALIZED: p = e / s_i, the IEEE division;
 *      SPECK_SOFTMAX_EXP: the result is e.  d_row_max[i] = m_i and d_row_sum[i] = s_i are written where the pointers are
 *      given; a row without entries has m_i = -inf and s_i = +0.0, the reduction's identities.
 *      SPECK_SOFTMAX_BACKWARD: A holds P, g = (double)d_G[q] for the entry at ABSOLUTE position q of A->data -- d_G is
 *      indexed exactly as A->data, so for a row-range view the caller passes the owner's sibling array, not an offset one;
 *      w = p * g;  r_i = the sum of the row's w in the same tree;  x = g - r_i;  x = p * x;  x = alpha * x.
 *      d_row_sum[i] = r_i where given; d_row_max must be NULL.
 *  What follows: the same bits from run to run, in place and out of place; a row-range view gives bit for bit the entries
 *      and vector elements of the whole matrix's result; _f32 on A32 equals _f64 on the widened matrix, rounded to float;
 *      the bits of an entry do not depend on whether the 16-byte or the entry-by-entry path served it.  For fp64:
 *      d_row_max is bit for bit speck_reduce_f64(MAX) of speck_scale_f64(A, alpha); with E the EXP result, d_row_sum is
 *      bit for bit speck_reduce_f64(E, SUM), and the NORMALIZED result is bit for bit speck_scale_f64(E, row = that, DIV):
 *      only exp itself is left to a tolerance.  The backward is bit for bit numpy's (alpha * (p * (g - r[row]))).astype(T)
 *      with r from speck_reduce_f64(SUM) of the matrix of the products p g in double.
 *  Nothing is hidden, as torch.softmax: a -inf entry (a mask) gives e = 0, p = 0; a row of only -inf becomes NaN
 *      (-inf - -inf); a +inf entry makes its whole row NaN; a NaN entry makes its row NaN and touches no other row;
 *      alpha * a overflowing to +inf makes that row NaN.  info->nonfinite counts the results that are inf or NaN AFTER
 *      the rounding to T; they do not make the call fail.  Structural: no entry is dropped, a result of 0.0 stays.  Rows
 *      need not be sorted; duplicates are separate terms.  No floating-point atomic anywhere.
 *  The vectors (DEVICE, A->rows doubles, double for both value types) are indexed by the row INSIDE A -- for a row-range
 *      view the caller offsets the pointer, as for speck_scale_*.
 *  In place (C == NULL): only A->data[row_offsets[0] .. row_offsets[0] + nnz) is written; row_offsets, col_ids, nnz and
 *      the three pointers stay as they were; col_ids is not read and may be NULL or garbage.  On a row-range view only
 *      the view's entries are touched: the owner's entries in front of and behind them keep their bytes.
 *  Out of place: C receives A's pattern -- the offsets rebased to 0, col_ids copied bit for bit -- under the ownership
 *      rule of speck_select_*: rows(C) == rows(A) keeps C->row_offsets, nnz(C) == nnz(A) keeps data / col_ids, anything
 *      else is freed and re-allocated.
 *  Refused before anything runs, SPECK_ERR_INVALID: NULL A or p; an unknown mode; reserved != 0; alpha NaN or infinite
 *      (speck_scale_* refuses the NaN only); d_G NULL in BACKWARD with nnz > 0, or given in a forward mode; d_row_max
 *      given in BACKWARD; any of d_G, d_row_max, d_row_sum equal to one of A's or C's three pointers, or to each other;
 *      the ranges [d_row_max, + rows) and [d_row_sum, + rows) overlapping; C sharing a buffer with A; NULL row_offsets with
 *      rows > 0; NULL data with nnz > 0; out of place, NULL col_ids with nnz > 0.  SPECK_ERR_DIM_LIMIT: rows or cols >
 *      2^27.  SPECK_ERR_NNZ_OVERFLOW: nnz >= 2^32.  rows == 0 or nnz == 0 is valid.
 *  Refused on the device, SPECK_ERR_INVALID: offsets descending, leaving [row_offsets[0], row_offsets[0] + nnz], or a last
 *      offset that is not row_offsets[0] + nnz; out of place, a column id >= cols.
 *  On any error NOTHING is written: not A->data, not C's buffers, not C's struct, not the two vectors (*info is zero once
 *      the arguments have passed).  No offset is used as an address before it was checked: a checking pass (two kernels
 *      out of place) raises its verdict in a status block, every kernel that writes -- the vectors included -- is queued
 *      behind it and does nothing where it is raised, and the host reads the status ONCE, at the end.
 *  Runs on the config's stream and returns complete.  Temporaries are three grow-only buffers of the config's own (not
 *      the multiply's arena, not another operation's), released with it; cfg == NULL is allowed.  With the debug option
 *      guard_bytes the canary zones of the temporaries and of C (in place: of A's buffers) are checked after the call.
 *  The entries are walked in tiles of SPECK_SOFTMAX_TILE_ENTRIES, aligned to absolute positions as the reduction's.  A row
 *      that lies whole inside one tile -- on everything but pathological inputs nearly every row -- is finished in the one
 *      visit of its tile: data is read once and written once.  A row that leaves its tile (info->rows_split) gets its m_i
 *      and s_i from the tile records in kernels of their own and its entries in a last visit of the tiles that hold a part
 *      of such a row; no kernel waits on another workgroup.  The 16-byte form needs data (d_G; out of place col_ids) on
 *      16-byte boundaries and, out of place, row_offsets[0] a multiple of 4.
 *  Not built: log_softmax and the log-sum-exp vector; a column softmax (transpose, then softmax); the softmax fused into
 *      speck_sddmm_* or speck_spmm_*; vectors in float; a per-row temperature; a pattern check of G inside the call (the
 *      Python wrapper offers speck_compare_* first). ---- */
enum { SPECK_SOFTMAX_NORMALIZED = 0, SPECK_SOFTMAX_EXP = 1, SPECK_SOFTMAX_BACKWARD = 2 };
#define SPECK_SOFTMAX_TILE_ENTRIES 4096
typedef struct speck_softmax_params {
    uint32_t mode;                /* SPECK_SOFTMAX_* */
    uint32_t reserved;            /* 0; anything else: SPECK_ERR_INVALID */
    double alpha;                 /* the temperature: the softmax of alpha * A */
    const void *d_G;              /* BACKWARD only: DEVICE, values of type T laid out as A->data; NULL otherwise */
    double *d_row_max;            /* optional DEVICE out, A->rows doubles (the forward modes) */
    double *d_row_sum;            /* optional DEVICE out, A->rows doubles (all modes; BACKWARD: r_i) */
} speck_softmax_params;
typedef struct speck_softmax_info {
    uint64_t entries;             /* entries written = nnz */
    uint64_t nonfinite;           /* ... of which the result, after rounding to T, is inf or NaN */
    uint64_t rows_empty;          /* rows without an entry */
    uint64_t rows_split;          /* rows whose entries lie in more than one tile */
    uint64_t tiles;               /* entry tiles walked */
} speck_softmax_info;
int speck_softmax_f64(speck_config *cfg, const speck_dcsr *A, const speck_softmax_params *p, speck_dcsr *C /* NULL: in place */,
                      speck_softmax_info *info /* may be NULL */);
int speck_softmax_f32(speck_config *cfg, const speck_dcsr *A, const speck_softmax_params *p, speck_dcsr *C,
                      speck_softmax_info *info);

/* ---- transposed product through a plan (new: the reference has no counterpart): Y = alpha A^T X + beta Y, the gradient of
 *      speck_spmm_* with respect to X (dX = A^T dY) and of speck_sddmm_* with respect to V (dV = (dC)^T U) -- what the
 *      backward pass of the attention layer above needs beside speck_softmax_*(BACKWARD).  In a training step the values
 *      change every iteration and the pattern never does, so the work that depends on the pattern alone -- the stable sort
 *      of the entries by column, speck_transpose_*'s -- is done ONCE, as a speck_tplan, and every call gathers the current
 *      values through it.  No floating-point atomic: the entries of a column are added in the tree of speck_reduce_*(SUM).
 *  THE PLAN holds four device arrays: t_ro[cols + 1], the offsets of A^T from 0; t_row[nnz], the row INSIDE A of the e-th
 *      entry in column order; t_pos[nnz], that entry's position in A relative to row_offsets[0]; ro0[rows + 1], A's offsets
 *      from 0.  Column order is speck_transpose_*'s: inside a column ascending position in A, duplicates of one (i,j) in
 *      their input order.  A->data is not read and may be NULL: a plan belongs to a PATTERN and fits every matrix that has
 *      it wherever its entries lie in their buffers -- a row-range view, its speck_dcsr_copy, the out-of-place result of
 *      speck_scale_*, speck_sddmm_* or speck_softmax_* on it -- and both value types.
 *  Unlike speck_transpose_* the creation CHECKS its input before it sorts or follows anything: offsets that descend or leave
 *      [row_offsets[0], row_offsets[0] + nnz], a last offset that is not row_offsets[0] + nnz, a column id >= cols, NULL
 *      buffers with nnz > 0: SPECK_ERR_INVALID, *out untouched, nothing left allocated.  Rows need not be sorted.  rows or
 *      cols > 2^27: SPECK_ERR_DIM_LIMIT; nnz > 2^32 - 64 (as speck_transpose_*): SPECK_ERR_NNZ_OVERFLOW; a failed allocation: SPECK_ERR_OOM, nothing
 *      leaked.  nnz == 0 and rows == 0 give valid plans.  Like speck_transpose_* the creation works on the NULL stream and
 *      returns complete; cfg may be NULL.  After the creation a plan is only ever read: several calls, streams and configs
 *      may use one.  speck_tplan_destroy(NULL) is SPECK_OK.
 *  THE PRODUCT: X is rows x k, indexed by the row INSIDE A (for a row-range view the caller offsets the pointer by
 *      r0 ldx), Y is cols x k, both row-major device arrays of doubles as for speck_spmm_* (ld >= k, padding never read
 *      or written, 64-bit index arithmetic).  A ROW-RANGE VIEW GIVES THE PARTIAL SUM OF ITS ROWS, not rows of the whole
 *      result: a row-sharded A^T X needs an all-reduce of the shards' Y, which is not built.
 *  The defining property: for every c < k, column c of Y is BIT FOR BIT what speck_spmm_*(alpha, At, X, beta, Y) writes with
 *      At = speck_transpose_*(A) -- the transpose keeps the order, the tree depends on the absolute positions in At->data
 *      alone, and those start at 0 as the plan's do.  So per column: the term (double)a * X(i,c) rounded once, nothing
 *      fused; the tree of speck_reduce_*(SUM); the same bits from run to run; beta == 0.0 does NOT READ Y; alpha is always
 *      applied; a NaN or 0 * inf of X(i,c) lands in column c of exactly the rows j of Y with (i,j) in A; duplicates add.
 *  THE PLAN IS VERIFIED, EXACTLY, IN EVERY CALL (a plan applied to another pattern would give plausible wrong numbers).
 *      Before anything runs: plan == NULL, or rows, cols or nnz of A differing from the plan's: SPECK_ERR_INVALID.  On the
 *      device the kernel queued first compares row_offsets[i] - row_offsets[0] with ro0[i] for all i, and the tile kernel
 *      compares col_ids[base + t_pos[e]] with the column entry e lies in according to t_ro; t_pos is a bijection, so the
 *      two together prove the patterns equal.  Any difference: SPECK_ERR_INVALID with NOTHING of Y written -- the column
 *      sums wait in a temporary of cols k doubles, and only the kernel queued last, which has seen the verdict of every
 *      tile, writes Y, each element once by one thread.  The call never follows an index of the caller's: t_pos < nnz and
 *      t_row < rows are the library's, A's ids are only compared, and base is used only behind the offsets check.
 *  Refused before anything runs beside that: alpha or beta NaN, ld < k, d_X or d_Y one of A's three arrays, the spans
 *      [d_X, d_X + (rows - 1) ldx + k) and [d_Y, d_Y + (cols - 1) ldy + k) overlapping (spans that touch are served), NULL
 *      where something would be read or written: SPECK_ERR_INVALID.  k > SPECK_SPMM_MAX_RHS, ld > 2^32: SPECK_ERR_DIM_LIMIT.
 *      k == 0 or cols == 0: SPECK_OK, nothing written.  nnz == 0 gives Y = alpha * (+0.0) + beta * Y.
 *  Config stream, ONE read-back at the end, cfg == NULL and the guard_bytes canary zones as for speck_spmm_*; the
 *      temporaries are grow-only buffers of the config's own, not those of speck_spmm_*.
 *  One workgroup per tile of SPECK_SPMV_TILE_ENTRIES plan entries, from 0; a thread loads 16 t_pos and 16 t_row with
 *      16-byte loads, gathers its 16 values and ids through t_pos and takes the k columns in speck_spmm_*'s blocks.
 *  info: cols_empty and cols_split describe A^T as rows_empty and rows_split of speck_spmm_info describe A.
 *  Not built: a switch that trusts the plan and skips the verification; a transpose that only gathers values through a
 *      plan; a column-side reduce or softmax; a torch.autograd.Function; the sharded all-reduce. ---- */
typedef struct speck_tplan speck_tplan;          /* opaque; owns its device buffers */
typedef struct speck_tplan_info {
    uint64_t rows, cols, nnz;     /* of the matrix the plan was made from */
    uint64_t cols_empty;          /* columns without an entry */
    uint64_t max_col_entries;     /* the longest column */
    uint64_t bytes;               /* device memory the plan holds */
} speck_tplan_info;
int speck_tplan_create(speck_config *cfg, const speck_dcsr *A, speck_tplan **out, speck_tplan_info *info /* may be NULL */);
int speck_tplan_destroy(speck_tplan *plan);      /* NULL is SPECK_OK */
typedef struct speck_spmm_t_info {
    uint64_t cols_empty;   /* columns of A without an entry: s(j,c) = +0.0 */
    uint64_t cols_split;   /* columns whose entries lie in more than one tile of the plan */
    uint64_t tiles;        /* tiles of the plan walked (each once, for all k) */
    uint64_t entries;      /* = nnz */
    uint64_t terms;        /* = entries * k */
} speck_spmm_t_info;
int speck_spmm_t_f64(speck_config *cfg, const speck_tplan *plan, double alpha, const speck_dcsr *A, const double *d_X,
                     uint64_t ldx, uint32_t k, double beta, double *d_Y, uint64_t ldy, speck_spmm_t_info *info /* may be NULL */);
int speck_spmm_t_f32(speck_config *cfg, const speck_tplan *plan, double alpha, const speck_dcsr *A, const double *d_X,
                     uint64_t ldx, uint32_t k, double beta, double *d_Y, uint64_t ldy, speck_spmm_t_info *info);

/* ---- float blocks for the three calls that take dense blocks (new: the reference has no counterpart): speck_spmm_*_b32,
 *      speck_spmm_t_*_b32 and speck_sddmm_*_b32 take X, Y, U and V as ROW-MAJOR DEVICE arrays of FLOATS -- the features and
 *      activations of a torch model as they are, without a widened copy, two conversion kernels and twice the gathered
 *      bytes per call.  The first suffix is A's value type, as everywhere; _b32 says the blocks are float.  Everything not
 *      said here is the double-block call's (speck_spmm_*, speck_spmm_t_*, speck_sddmm_* above): the arguments, alpha and
 *      beta in double, the info structs, the refusals, the plan, the config, the temporaries (sums stays rows k DOUBLES).
 *  What differs.  ld* count elements of 4 bytes; the spans are [d_X, d_X + 4 ((n - 1) ld + k)) bytes.  A block element is
 *      widened to double where it is loaded (exact, subnormals included); from there every step is the double call's:
 *      the term (double)a * (double)x rounded once, nothing fused, the same tree.
 *        spmm_b32, spmm_t_b32:  Y(i,c) = (float)(alpha s + beta (double)Y(i,c)) -- ONE rounding to float, at the end;
 *            beta == 0.0 does not read Y.  The defining property: the result is BIT FOR BIT
 *            float(speck_spmm_*(alpha, A, double(X), beta, double(Y))) (speck_spmm_t_* with the same plan).  A result
 *            beyond float's range becomes inf in its element, as a conversion makes it; it is neither refused nor counted.
 *        sddmm_b32:  C is BIT FOR BIT what speck_sddmm_* writes for double(U), double(V) -- in place and into a new C,
 *            both modes, info->nonfinite and info->lanes included.  L(k) and the tree are unchanged.
 *      So what the double calls promise per column or per entry carries over: the same bits from run to run, views, where
 *      a NaN lands, duplicates, the plan verified in every call, nothing written on any error, one read-back.
 *  Alignment: the gathers of spmm / spmm_t take SPECK_SPMM_COLUMN_BLOCK_B32 columns per block, one 16-byte load per entry
 *      and four columns where the block lies on 16 bytes and ld % 4 == 0, 8-byte loads where it lies on 8 and ld is even,
 *      4-byte loads elsewhere; sddmm loads a lane's pair of columns with 8 bytes where the block lies on 8 and ld is
 *      even, 4-byte loads elsewhere.  Every form gives the same bits; the padding [k, ld) is never touched.
 *  Not built: half / bf16 blocks; accumulation in float; X in float with Y in double (or the reverse); float vectors for
 *      speck_spmv_*, speck_scale_*, speck_reduce_* and speck_softmax_*. ---- */
#define SPECK_SPMM_COLUMN_BLOCK_B32 4
typedef struct speck_sddmm_params_b32 {           /* speck_sddmm_params field for field, the blocks in float */
    uint32_t mode;                /* SPECK_SDDMM_* */
    uint32_t k;
    double alpha, beta;
    const float *d_U;             /* DEVICE, rows x k row-major, indexed by the row INSIDE A */
    uint64_t ldu;                 /* in floats */
    const float *d_V;             /* DEVICE, cols x k row-major, indexed by the column id */
    uint64_t ldv;
} speck_sddmm_params_b32;
int speck_spmm_f64_b32(speck_config *cfg, double alpha, const speck_dcsr *A, const float *d_X, uint64_t ldx, uint32_t k,
                       double beta, float *d_Y, uint64_t ldy, speck_spmm_info *info /* may be NULL */);
int speck_spmm_f32_b32(speck_config *cfg, double alpha, const speck_dcsr *A, const float *d_X, uint64_t ldx, uint32_t k,
                       double beta, float *d_Y, uint64_t ldy, speck_spmm_info *info);
int speck_spmm_t_f64_b32(speck_config *cfg, const speck_tplan *plan, double alpha, const speck_dcsr *A, const float *d_X,
                         uint64_t ldx, uint32_t k, double beta, float *d_Y, uint64_t ldy, speck_spmm_t_info *info /* may be NULL */);
int speck_spmm_t_f32_b32(speck_config *cfg, const speck_tplan *plan, double alpha, const speck_dcsr *A, const float *d_X,
                         uint64_t ldx, uint32_t k, double beta, float *d_Y, uint64_t ldy, speck_spmm_t_info *info);
int speck_sddmm_f64_b32(speck_config *cfg, const speck_dcsr *A, const speck_sddmm_params_b32 *p, speck_dcsr *C /* NULL: in place */,
                        speck_sddmm_info *info /* may be NULL */);
int speck_sddmm_f32_b32(speck_config *cfg, const speck_dcsr *A, const speck_sddmm_params_b32 *p, speck_dcsr *C,
                        speck_sddmm_info *info);

/* ---- device COO triplets to a device CSR and back (the reference converts on the host only: convert(CSR&, const COO&),
 *      source/CSR.cpp:173-212).  The caller of a graph layer owns an edge list on the device -- a 2 x E int64 edge_index in
 *      no particular order and perhaps E weights --, not a CSR: speck_from_coo_* is the way in without a trip through the
 *      host, speck_to_coo the way out (the row index per entry that a CSR does not have).
 *  speck_from_coo_*: row i of C holds exactly the triplets with row id i, IN INPUT ORDER (stable): with p the stable
 *      argsort of the row ids, C.col_ids = col[p] and C.data = val[p] bit for bit (NaN payloads, -0.0 and subnormals are
 *      kept), and row_offsets is the running sum of the ids' histogram from 0.  Rows are NOT sorted by column and duplicates
 *      are kept: that is speck_sort_rows_*, one call away, and there is no flag for it here -- a second stage that can fail
 *      after C was written would break the rule below.  data == NULL: every value is 1.0 (an unweighted edge list).
 *  index_bytes 4: uint32_t ids; 8: int64_t ids (torch.long).  An 8-byte id is compared as an unsigned 64-bit number, so a
 *      negative one and one whose upper word is not zero (2^32 + 3 does not pass as 3) are above every limit.
 *  SPECK_ERR_INVALID with NOTHING written -- not C's struct, not its allocations, not the contents of buffers it would
 *      reuse: a row id >= rows or a column id >= cols; index_bytes not 4 or 8; NULL id arrays with nnz > 0; nnz > 0 with
 *      no row or no column; one of C's three buffers (as far as C declares them) overlapping an input array.  rows, cols
 *      <= 2^27 (SPECK_ERR_DIM_LIMIT), nnz < 2^32 (SPECK_ERR_NNZ_OVERFLOW).  nnz == 0 is valid: every offset is 0.
 *  One pass in tiles of SPECK_COO_TILE_ENTRIES checks every id (16-byte loads where both id arrays start on 16 bytes),
 *      writes the u32 row keys -- clamped: no id is used as an address or a key before it was compared -- and decides
 *      whether the row ids are already non-descending.  The host reads that verdict before anything of C is allocated.
 *      Row ids in order (speck_to_coo's output, a row-sorted edge_index, anything exported from a CSR): NO sort; columns
 *      and values are copied straight over, narrowed where 8 bytes wide.  Else: the stable radix sort of
 *      speck_transpose_* on (row key, position), ceil(log2(rows) / 8) passes of 8 bits, and one gather through the
 *      positions.  The offsets are the lower bounds of the rows in the sorted keys.  No atomic decides the order of two
 *      entries and no floating-point atomic exists: the same bytes from run to run.
 *  Ownership of C as speck_select_* documents it: row_offsets reused when C->rows == rows, data / col_ids re-allocated
 *      only when C->nnz differs.  Runs on the config's stream (speck_config_set_stream is honoured: ids produced on that
 *      stream need no synchronisation in front of the call) and returns with C complete.  Temporaries are grow-only
 *      buffers of the config's own (not the multiply's arena), 16 bytes per entry and 1 MiB; cfg == NULL is allowed as
 *      for speck_sort_rows_*.  With the debug option guard_bytes the canary zones of the temporaries and of C are checked
 *      after the call.  Two read-backs: the verdict with the sorted flag, and the counters of info.
 *  speck_to_coo: for entry e of row i INSIDE A, d_row_out[e - row_offsets[0]] = row_base + i; where d_col_out is given it
 *      receives the column id widened to index_bytes.  Values are not touched -- the caller reads A->data from entry
 *      row_offsets[0] on --, so this is ONE function for both value types.  A may be a row-range view with absolute
 *      offsets; row_base is the global index of its first row.  Both outputs hold nnz indices of index_bytes each.
 *  Refused with nothing written: offsets that descend or leave [row_offsets[0], row_offsets[0] + nnz] or whose last one
 *      does not span nnz (as everywhere); where d_col_out is given, a column id >= cols; an output inside one of A's
 *      buffers or the two outputs overlapping; row_base + rows exceeding 2^32 (index_bytes 4) or 2^63 (8); index_bytes
 *      not 4 or 8; NULL d_row_out: SPECK_ERR_INVALID.  The limits are speck_from_coo_*'s.  rows == 0: SPECK_OK.
 *      "Inside A->data": this one function does not know A's value type, so it refuses an output that touches the bytes
 *      from 4 row_offsets[0] to 8 (row_offsets[0] + nnz) behind A->data, the entries as floats and as doubles.  With FLOAT
 *      values that span reaches 4 (row_offsets[0] + nnz) bytes behind the last value -- up to 16 GiB for a view that ends
 *      near 2^32 -- and an output that lies there is refused although it touches nothing of A: keep the outputs clear of
 *      it (tests/test_gpu_high_offsets_side.py does).  Telling the two apart needs the value type in the call.
 *  The checking kernel takes a thread per row and, for the ids, one streaming pass over the entries; the writing kernel
 *      is queued behind it and does nothing where the verdict is raised: a wave takes 64 rows at a time, a lane each, a
 *      row longer than 16 entries takes the whole wave, lanes striding its entries; the columns are widened in a streaming
 *      pass.  ONE read-back, at the end.  Stream, cfg == NULL and guard_bytes as above.
 *  Not built: a fused sort by column or sum of duplicates; COO with negative int32 sentinels; float16 values; CSC input
 *      (speck_transpose_* afterwards); blocked or batched graphs. ---- */
#define SPECK_COO_TILE_ENTRIES 2048
typedef struct speck_dcoo {          /* field names of the reference's COO<T>, include/COO.h */
    uint64_t rows, cols, nnz;
    const void *data;                /* DEVICE, nnz values of T; NULL: every value is 1.0 */
    const void *row_ids, *col_ids;   /* DEVICE, nnz indices each */
    uint32_t index_bytes;            /* 4: uint32_t; 8: int64_t */
} speck_dcoo;
typedef struct speck_from_coo_info {
    uint64_t entries;            /* = nnz */
    uint64_t rows_empty;         /* rows of C without an entry */
    uint64_t max_row_entries;    /* the longest row of C */
    uint64_t sorted_input;       /* 1: the row ids were already non-descending -- nothing was sorted */
    uint64_t sort_passes;        /* radix passes of 8 bits that ran: 0, or ceil(log2(rows) / 8) */
} speck_from_coo_info;
int speck_from_coo_f64(speck_config *cfg, const speck_dcoo *coo, speck_dcsr *C, speck_from_coo_info *info /* may be NULL */);
int speck_from_coo_f32(speck_config *cfg, const speck_dcoo *coo, speck_dcsr *C, speck_from_coo_info *info);
int speck_to_coo(speck_config *cfg, const speck_dcsr *A, uint32_t index_bytes, uint64_t row_base, void *d_row_out,
                 void *d_col_out /* may be NULL */);

/* ---- sub-matrix by index (new: the reference has no counterpart): C = A(p, q) -- the rows of A a device index list
 *      names, in the list's order, with every column id sent through a device map that renumbers or drops it.  A
 *      mini-batch's induced subgraph A[nodes][:, nodes] with the vertices renumbered 0 .. m-1, a permutation P A P^T before
 *      a triangle count or a Galerkin product, the four blocks of a coarse / fine splitting, the unsmoothed aggregation
 *      A P with a piecewise constant P (a map that is not injective, then speck_sort_rows_* with SUM_DUPLICATES), a shard by
 *      an arbitrary row set: one call each, nothing leaves the device.
 *  d_row_index: n_rows indices into the rows INSIDE A (A may be a row-range view with absolute offsets), in any order,
 *      REPEATS ALLOWED (sampling with replacement, hub duplication).  NULL: the rows 0 .. A->rows - 1 in order; then n_rows
 *      must be A->rows.
 *  d_col_map: A->cols entries; map[j] is the new id of column j, or "dropped".  It need be neither injective nor monotone.
 *      NULL: identity; then out_cols must be A->cols.
 *  index_bytes: the width of BOTH arrays, as for speck_from_coo_*.  8: int64_t (torch.long goes in as it is) -- any negative
 *      map value means "dropped", a negative row index is refused.  4: uint32_t -- a map value of 0xFFFFFFFF means "dropped".
 *  Row i of C is row p[i] of A without the dropped entries, IN INPUT ORDER, each column id replaced by map[id], each value
 *      copied bit for bit (NaN payloads, -0.0 and subnormals survive); C->cols = out_cols; offsets start at 0.  Nothing is
 *      sorted and duplicates stay -- rows of A need not be sorted or free of duplicates either.  The rows of C ascend where
 *      those of A do and the map is monotone on what it keeps; otherwise speck_sort_rows_* is one call away (there is no flag
 *      for it here: a second stage that can fail after C was written would break the rule below).  With
 *          glen = ro[p+1] - ro[p];  G = [0, cumsum(glen)];  src = repeat(ro[p] - G[:-1], glen) + arange(G[-1])
 *          m = map[col[src]];  keep = m is not "dropped"
 *      C holds m[keep] and the bits of val[src][keep], and row i of it the kept entries among G[i] .. G[i+1] - 1.
 *  SPECK_ERR_INVALID with NOTHING written -- not C's struct, not its allocations, not the contents of buffers it would reuse:
 *      offsets of A that descend, leave [row_offsets[0], row_offsets[0] + nnz] or whose last one does not span nnz (all rows
 *      are checked, as everywhere); a row index >= A->rows (8 bytes wide: compared as an unsigned 64-bit number, so a
 *      negative one and 2^32 + 3 are above every limit); a map value that is neither "dropped" nor < out_cols (all A->cols
 *      entries are checked, referenced or not); a column id >= A->cols in a GATHERED row, found before it indexes the map,
 *      and without a map too (C must be a sound matrix) -- the ids of rows that are not gathered are NEVER READ, so a
 *      matrix with a bad id in a row nobody asks for is served; index_bytes not 4 or 8; NULL buffers with a count > 0; a
 *      NULL index with n_rows != A->rows; a NULL map with out_cols != A->cols; d_row_index or d_col_map overlapping one of
 *      A's or C's buffers (spans, as for speck_to_coo); C sharing a buffer with A.  A->rows, A->cols, n_rows or out_cols >
 *      2^27: SPECK_ERR_DIM_LIMIT.  The gathered rows holding 2^32 entries or more BEFORE the drop (repeats make that
 *      possible), or A->nnz >= 2^32: SPECK_ERR_NNZ_OVERFLOW -- decided from a 64-bit sum before any 32-bit offset is used.
 *      n_rows == 0 gives an empty C of out_cols columns; no gathered entry, or every one dropped, gives n_rows empty rows
 *      (C owns buffers of one entry).  *info is zero once the arguments have passed, and again on an error.
 *  Three passes, a read-back of the status block behind the first two.  CHECK: the rows of A, the indices and the map, a
 *      thread each; the length of every gathered row -- 0 where its index or its own two offsets are unsound: clamped, never
 *      followed -- and their 64-bit sum; the shared scan of the lengths gives the gross offsets G.  MARK: one workgroup per
 *      tile of SPECK_EXTRACT_TILE_ENTRIES gathered ("gross") entries, four consecutive ones per thread, whatever the row
 *      lengths -- a hub row repeated 1000 times is just many tiles; the tile's first row by one search in G, the following
 *      ones from LDS; every id compared with A->cols before it indexes the map; a keep byte per entry and the kept entries
 *      per row.  Without a map the pass checks the ids and writes nothing.  PLACE, after C's buffers were prepared: gross
 *      order is output order, so an entry's place is the number of kept entries in front of it (the shared scan over the
 *      keep bytes); every entry of C is written once by one thread.  Atomics run on integer counts only: the same bytes
 *      from run to run.
 *  Ownership of C as speck_select_* documents it: row_offsets reused when C->rows == n_rows, data / col_ids re-allocated
 *      only when C->nnz differs.  There is no in-place mode.  Runs on the config's stream (speck_config_set_stream is
 *      honoured: indices produced on that stream need no synchronisation in front of the call) and returns with C complete.
 *      Temporaries are grow-only buffers of the config's own (not the multiply's arena): 16 bytes per output row, 1 byte per
 *      gathered entry and 4 per tile; cfg == NULL is allowed as for speck_sort_rows_*.  With the debug option guard_bytes the
 *      canary zones of the temporaries and of C are checked after the call.
 *  Not built: the inverse map from a node list inside the C call (one scatter in the caller's framework: the Python
 *      wrappers do it); a fused sort or sum of duplicates; in-place extraction; A(p, q) = B (scatter into a matrix);
 *      hstack / vstack; per-row top-k; a plan that is reused across calls on one pattern. ---- */
#define SPECK_EXTRACT_TILE_ENTRIES 4096
typedef struct speck_extract_params {
    uint64_t n_rows, out_cols;               /* rows and columns of C */
    const void *d_row_index, *d_col_map;     /* DEVICE: n_rows indices / A->cols map values; either may be NULL */
    uint32_t index_bytes;                    /* 4: uint32_t; 8: int64_t */
} speck_extract_params;
typedef struct speck_extract_info {
    uint64_t rows_out;           /* rows of C = n_rows */
    uint64_t rows_empty;         /* rows of C without an entry */
    uint64_t gross;              /* entries of the gathered rows before the drop */
    uint64_t nnz_out;            /* entries of C */
    uint64_t dropped;            /* gross - nnz_out */
    uint64_t cols_kept;          /* map entries that are not "dropped"; A->cols without a map */
    uint64_t max_row_entries;    /* the longest row of C */
} speck_extract_info;
int speck_extract_f64(speck_config *cfg, const speck_dcsr *A, const speck_extract_params *p, speck_dcsr *C,
                      speck_extract_info *info /* may be NULL */);
int speck_extract_f32(speck_config *cfg, const speck_dcsr *A, const speck_extract_params *p, speck_dcsr *C,
                      speck_extract_info *info);

/* ---- per-row top-k (new: the reference has no counterpart; the "per-row top-k" the block above names): C = the k best
 *      entries of every row of a matrix that is already on the device.  speck_select_* cuts by a threshold, a predicate on
 *      one entry; "the k largest of my row" is a predicate on the row.  The pruning of an MCL iteration (multiply -> topk ->
 *      scale(map = square) -> normalize_rows), a kNN or similarity graph from speck_sddmm_* scores, top-k sparse attention
 *      in front of speck_softmax_*, the strength-of-connection cut of an AMG setup, "at most k neighbours per vertex" in
 *      front of a sampled mini-batch: one call, nothing leaves the device.
 *  The KEY of an entry with the value v, widened to double: v (SPECK_TOPK_LARGEST), -v (SPECK_TOPK_SMALLEST), |v|
 *      (SPECK_TOPK_LARGEST_ABS).  A NaN ranks ABOVE every number in every mode: the call never drops one silently in favour
 *      of a number (speck_select_* keeps a NaN too; torch.topk ranks it the same way).  -0.0 and +0.0 are equal keys.
 *      Entry e of a row BEATS entry e' of the same row if its key is larger, or if the keys are equal and e comes first in
 *      the row.  An entry is KEPT iff fewer than k entries of its row beat it.  So a row of at most k entries is kept whole,
 *      a row of more than k keeps exactly k; k == 0 gives A->rows empty rows; a k of 2^32 or more keeps every row whole.
 *  Kept entries stay IN INPUT ORDER -- ascending rows stay ascending: a canonical A gives a C that speck_multiply_* accepts
 *      --, column ids and values are copied bit for bit (NaN payloads, -0.0 and subnormals survive); C->cols = A->cols; the
 *      offsets of C start at 0.  Rows need not be sorted or free of duplicates; nothing is merged.  As numpy, per row:
 *          order = np.lexsort((pos, -key, ~isnan));  kept = np.sort(order[:k])
 *      (tests/test_topk_host.py states it as numpy_topk and compares it with a count of beaters).
 *  A may be a row-range view with absolute offsets: the rows of the view's result are the rows of the whole matrix's
 *      result, bit for bit.  _f32 gives the structure of the _f64 call on the widened matrix and the float bits (widening is
 *      monotone and one-to-one: the kernels rank 32-bit keys).  Keys are order-preserving unsigned integers; atomics run on
 *      integer counts only, there is no floating-point atomic and no floating-point arithmetic at all: the same bytes from
 *      run to run.
 *  *info: rows_cut = the rows longer than k; dropped = entries_in - nnz_out; ties_cut = the rows in which a dropped entry has
 *      the key of a kept one (the tie rule decided there); nan_kept = the NaN entries of C; max_row_entries = the longest row
 *      of C.  *info is zero once the arguments have passed, and again on an error.
 *  SPECK_ERR_INVALID with NOTHING written -- not C's struct, not its allocations, not the contents of buffers it would reuse:
 *      offsets that descend, leave [row_offsets[0], row_offsets[0] + nnz] or whose last one does not span nnz; a column id >=
 *      A->cols ANYWHERE in A (C must be a sound matrix); mode not one of the three; reserved != 0; NULL A, p or C; NULL
 *      buffers with a count > 0; C sharing a buffer with A.  A->rows or A->cols > 2^27: SPECK_ERR_DIM_LIMIT.  A->nnz > 2^32 -
 *      1024: SPECK_ERR_NNZ_OVERFLOW (the copy of the rows kept whole numbers a tile's entries in 32 bits, 1024 a step).  No offset is used as an address before it has been checked.
 *  CHECK AND CLASSIFY: one pass over row_offsets and col_ids; min(len, k) per row, which the shared scan turns into C's
 *      offsets -- they depend on the lengths alone: there is no marking pass and no keep byte; the rows longer than k go to
 *      lists by length.  ONE read-back (the verdict, nnz(C), the lists) before C is allocated; every kernel that writes C
 *      starts after it.  Rows of at most k entries: a streaming copy that knows nothing of keys -- on a matrix without a
 *      longer row the call is that copy.  Rows of up to SPECK_TOPK_GROUP_MAX entries: a group of 8 / 16 / 32 / 64 lanes (up
 *      to GROUP_MAX / 8, / 4, / 2, GROUP_MAX entries) counts for every entry the entries that beat it.  Rows of up to
 *      SPECK_TOPK_LDS_MAX entries: one workgroup, the keys in LDS, a radix select from the most significant byte (a histogram
 *      of 256 bins per pass; it stops where the narrowed set is exactly what is still needed) for the threshold key and the
 *      number of its equals to keep, then one ordered walk.  Longer rows: the same select and walk with the values read
 *      again from global memory in every pass -- nothing is moved, there is no temporary.  At most one more read-back at the
 *      end, for ties_cut and nan_kept (none with info == NULL).
 *  Ownership of C, the stream, cfg == NULL, guard_bytes and the grow-only scratch of the config's own (20 bytes per row) as
 *      speck_select_* / speck_extract_* document them.  There is no in-place mode.  The debug options topk_group_max and
 *      topk_lds_max (clamped to the two defines) lower the class limits: every class gives the same bytes.
 *  Not built: a per-row k from a device array; a threshold or cumulative-mass cut fused in; the row's threshold key returned
 *      as a vector; top-k per column (speck_transpose_* first); in-place; a hub row split over several workgroups; top-k
 *      fused behind speck_sddmm_* or the product. ---- */
enum { SPECK_TOPK_LARGEST = 0, SPECK_TOPK_SMALLEST = 1, SPECK_TOPK_LARGEST_ABS = 2 };
#define SPECK_TOPK_GROUP_MAX 256    /* rows up to this many entries are ranked by a group of lanes */
#define SPECK_TOPK_LDS_MAX 4096     /* rows up to this many entries are selected with their keys in LDS */
typedef struct speck_topk_params {
    uint64_t k;                  /* entries a row keeps at most */
    uint32_t mode;               /* SPECK_TOPK_* */
    uint32_t reserved;           /* must be 0 */
} speck_topk_params;
typedef struct speck_topk_info {
    uint64_t rows;               /* rows of C = A->rows */
    uint64_t rows_cut;           /* rows of A longer than k */
    uint64_t entries_in;         /* entries of A */
    uint64_t nnz_out;            /* entries of C */
    uint64_t dropped;            /* entries_in - nnz_out */
    uint64_t max_row_entries;    /* the longest row of C */
    uint64_t ties_cut;           /* rows in which a dropped entry has the key of a kept one */
    uint64_t nan_kept;           /* NaN entries of C */
} speck_topk_info;
int speck_topk_f64(speck_config *cfg, const speck_dcsr *A, const speck_topk_params *p, speck_dcsr *C,
                   speck_topk_info *info /* may be NULL */);
int speck_topk_f32(speck_config *cfg, const speck_dcsr *A, const speck_topk_params *p, speck_dcsr *C,
                   speck_topk_info *info);

/* ---- fan-out neighbour sampling (new: the reference has no counterpart): row i of C = at most k entries of row p[i] of A,
 *      chosen uniformly at random -- the step in front of a sampled mini-batch (DGL's sample_neighbors, PyG's NeighborLoader):
 *      sample_neighbors -> induced_subgraph -> sddmm -> softmax -> spmm.  speck_topk_* keeps the k LARGEST and takes no row
 *      list; speck_extract_* gathers the rows and keeps every entry of a hub.  This call does both in one, and the random key
 *      of an entry is a PURE FUNCTION of (seed, global row, place in the row): the sample is reproducible bit for bit in
 *      numpy, the same from run to run, and needs no random-number state and no floating point.
 *  d_row_index / n_rows / index_bytes as for speck_extract_*: n_rows indices into the rows INSIDE A, any order, REPEATS
 *      ALLOWED; NULL: the rows 0 .. A->rows - 1, then n_rows must be A->rows.  row_base: the global index of A's first row
 *      where A is a row-range view, else 0.  C has n_rows rows and A->cols columns; its offsets start at 0.
 *  KEYS.  All arithmetic modulo 2^64, GOLDEN = 0x9E3779B97F4A7C15:
 *          mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *          row_key(seed, g) = mix(seed + GOLDEN * (g + 1))       g = row_base + p[i], the GLOBAL index of the source row
 *          key(seed, g, t)  = mix(row_key(seed, g) + GOLDEN * (t + 1))        t = 0, 1, 2, ...
 *      key(., ., t) is output number t of the SplitMix64 generator started at row_key.
 *  SPECK_SAMPLE_WITHOUT_REPLACEMENT: the entry at place t of its row (0-based, in input order) carries key(seed, g, t); it is
 *      KEPT iff fewer than k entries of the row have a lexicographically smaller (key, t).  A row of at most k entries is
 *      kept whole, a longer one keeps exactly k; k == 0 gives empty rows, a k of 2^32 or more keeps everything.  Kept entries
 *      stay IN INPUT ORDER, ids and values bit for bit (NaN payloads, -0.0 and subnormals survive): a canonical A gives a C
 *      that speck_multiply_* accepts.  As numpy, per row:  kept = np.sort(np.lexsort((t, key))[:k]).
 *  SPECK_SAMPLE_WITH_REPLACEMENT: a source row of len >= 1 entries gives exactly k entries, an empty one gives none.  Entry u
 *      of the output row, in draw order u = 0 .. k - 1, is the source entry at place (key(seed, g, u) * len) >> 64 (the high
 *      word of the 128-bit product).  The bias of that map is below len / 2^64.  Repeats stay and nothing is sorted:
 *      speck_sort_rows_* is one call away.
 *  (tests/test_sample_host.py states both as numpy_sample, compares it with a count of smaller (key, t) and tests the
 *      uniformity of the places it takes.)
 *  So the sample does not depend on values, column ids, the value type, the absolute offsets of a view or the class a row
 *      falls in: _f32 and _f64 give the same structure; a view with the right row_base gives the rows of the whole matrix's
 *      sample; the same row named twice gives the same sample twice -- the caller varies seed per hop or epoch.  Integer
 *      arithmetic and integer atomics only: the same bytes from run to run.
 *  *info: rows_out = n_rows; rows_empty = rows of C without an entry; rows_cut = gathered rows longer than k; gross = the
 *      entries of the gathered rows; max_row_entries = the longest row of C.  *info is zero once the arguments have passed,
 *      and again on an error.
 *  SPECK_ERR_INVALID with NOTHING written -- not C's struct, not its allocations, not the contents of buffers it would reuse:
 *      offsets of A that descend, leave [row_offsets[0], row_offsets[0] + nnz] or whose last one does not span nnz (all rows
 *      are checked); a row index >= A->rows (8 bytes wide: compared unsigned, so -1 and 2^32 + 3 are refused); a column id >=
 *      A->cols anywhere in a GATHERED row, whichever entries the sample would have taken -- the verdict does not depend on the
 *      seed; the ids of rows nobody gathers are NEVER READ, so a matrix with a bad id in a row nobody asks for is served; an
 *      unknown mode; index_bytes not 4 or 8; a NULL index with n_rows != A->rows; row_base > 2^62; the index overlapping a
 *      buffer of A or C; C sharing a buffer with A; NULL A, p or C; NULL buffers with a count > 0.  A->rows, A->cols or
 *      n_rows > 2^27: SPECK_ERR_DIM_LIMIT.  A->nnz > 2^32 - 1024, an output of 2^32 entries or more (mode 1 reaches that easily:
 *      k times the non-empty gathered rows) or gathered rows of more than 2^32 - 1024 entries (the copy of the rows kept
 *      whole numbers a tile's entries in 32 bits, 1024 a step):
 *      SPECK_ERR_NNZ_OVERFLOW, decided from 64-bit sums in the first pass before any 32-bit offset exists.
 *  CHECK: a thread per row of A and per index -- the offsets, the indices, the gathered length (0 where unsound: clamped,
 *      never followed), the output length min(len, k) or (len ? k : 0), the 64-bit sums of both and, for mode 0, the rows
 *      longer than k sent to lists by length.  The shared scan gives C's offsets -- they depend on the lengths alone: no
 *      marking pass, no keep byte -- and the gross offsets.  ID CHECK: tiles of SPECK_SAMPLE_TILE_ENTRIES gross entries over
 *      the gathered rows, every id compared with A->cols.  ONE read-back (the verdict, nnz(C), the lists) before C is
 *      allocated; every kernel that writes C starts after it.  Mode 0: rows of at most k entries are a streaming copy; rows
 *      of up to SPECK_SAMPLE_GROUP_MAX entries: a group of 8 / 16 / 32 / 64 lanes counts, per entry, the entries with a smaller
 *      (key, t); rows of up to SPECK_SAMPLE_LDS_MAX: one workgroup, the keys computed once into LDS, a radix select from the
 *      most significant byte for the threshold key and the number of its equals to keep, then one ordered walk; longer rows:
 *      the same select with the keys RECOMPUTED in every pass -- no global read before the walk.  Mode 1: one stream over the
 *      output entries, the row by a search in C's offsets per tile; every entry is independent.  A key costs two 64-bit
 *      multiplies; the work on a cut row is O(len), not O(k).
 *  Ownership of C, the stream, cfg == NULL, guard_bytes and the grow-only scratch of the config's own (32 bytes per output
 *      row) as speck_select_* / speck_extract_* document them.  The debug options sample_group_max and sample_lds_max
 *      (clamped to the two defines) lower the class limits: every class gives the same bytes.
 *  Not built: weighted sampling (needs log / pow: not bit-reproducible); a per-row k; several hops in one call; sampling
 *      by column (speck_transpose_* first); an O(k) draw for hub rows (Floyd's algorithm: the work here is O(len) per cut
 *      row); the positions of the kept entries returned by the C call (the Python wrapper gets them from a second call on
 *      values that are positions). ---- */
enum { SPECK_SAMPLE_WITHOUT_REPLACEMENT = 0, SPECK_SAMPLE_WITH_REPLACEMENT = 1 };
#define SPECK_SAMPLE_GROUP_MAX 256    /* cut rows up to this many entries are ranked by a group of lanes */
#define SPECK_SAMPLE_LDS_MAX 4096     /* cut rows up to this many entries are selected with their keys in LDS */
#define SPECK_SAMPLE_TILE_ENTRIES 4096
typedef struct speck_sample_params {
    uint64_t k;                  /* fan-out: entries a row of C holds at most (mode 0) / exactly, if its source row is not empty (mode 1) */
    uint64_t seed;
    uint64_t row_base;           /* global index of A's first row (A a row-range view), else 0; > 2^62: INVALID */
    uint64_t n_rows;             /* rows of C */
    const void *d_row_index;     /* DEVICE, n_rows indices into the rows INSIDE A, any order, repeats allowed; NULL: rows 0..A->rows-1, n_rows == A->rows */
    uint32_t index_bytes;        /* 4: uint32_t, 8: int64_t -- as speck_extract_* */
    uint32_t mode;               /* SPECK_SAMPLE_* */
} speck_sample_params;
typedef struct speck_sample_info {
    uint64_t rows_out;           /* rows of C = n_rows */
    uint64_t rows_empty;         /* rows of C without an entry */
    uint64_t rows_cut;           /* gathered rows longer than k */
    uint64_t gross;              /* entries of the gathered rows */
    uint64_t nnz_out;            /* entries of C */
    uint64_t max_row_entries;    /* the longest row of C */
} speck_sample_info;
int speck_sample_f64(speck_config *cfg, const speck_dcsr *A, const speck_sample_params *p, speck_dcsr *C,
                     speck_sample_info *info /* may be NULL */);
int speck_sample_f32(speck_config *cfg, const speck_dcsr *A, const speck_sample_params *p, speck_dcsr *C,
                     speck_sample_info *info);

/* ---- assembly from blocks (new: the reference has no counterpart; the "hstack / vstack" and the "blocked or batched
 *      graphs" two blocks above name): C = bmat(grid) -- a grid of block_rows x block_cols cells that hold matrices already
 *      on the device, an absent cell a zero block.  block_diag(G_1 .. G_n) makes one matrix of n small graphs, so that sddmm ->
 *      softmax -> spmm, or one speck_multiply_* (block_diag(A_i) block_diag(B_i) = block_diag(A_i B_i)), runs once instead
 *      of n times; [[H, A^T], [A, 0]] is a saddle-point system; vstack puts row shards back, hstack the column slices of a
 *      column-split product: one call each, nothing leaves the device.
 *  Block row g has the height h_g = row_sizes[g] where row_sizes is given, else the common `rows` of the blocks of block row
 *      g; block column q the width w_q likewise.  R0 and C0 are their running sums (the ORIGINS).  Row R0_g + i of C is the
 *      concatenation, in ascending q, of row i of every block present in block row g, each column id with C0_q added, each
 *      value copied bit for bit (NaN payloads, -0.0 and subnormals survive).  Nothing is sorted, summed or dropped: rows of
 *      the blocks need not be sorted or free of duplicates; where every block has strictly ascending rows C has them too and is
 *      a valid input of speck_multiply_*.  With the cells of block row g in ascending q numbered 0 .. nb_g - 1, a PIECE is
 *      (output row, block present in that row's block row): piece P0_g + i nb_g + q is row i of block q of block row g, the
 *      pieces in this order are the entries of C in order, G = [0, cumsum(piece lengths)], and C.row_offsets[r] = G[first
 *      piece of r].
 *  blocks: HOST, n_blocks cells in ANY order (a sparse list: a block_diag of 1000 graphs is 1000 descriptors, not a million
 *      pointers).  A block may be a row-range view with absolute offsets, each with its own base; one matrix may stand in
 *      several cells; all blocks hold the call's value type.  A block with 0 rows or 0 columns, n_blocks == 0 with both size
 *      arrays given, and a result with no entry (C then owns buffers of one entry) are all valid.
 *  speck_bmat_layout is exactly the host computation the device call starts with, on its own: no device, no config.  It
 *      returns the shape, nnz = the sum of the blocks' nnz, the pieces and, where the arrays are given, the origins -- where
 *      graph i's vertices land in the batch.  It refuses what the device call refuses on the host, with the same status,
 *      and then writes nothing.
 *  SPECK_ERR_INVALID with NOTHING written -- not C's struct, not its allocations, not the contents of buffers it would reuse:
 *      NULL p, C or M; n_blocks > 0 with NULL blocks; a cell outside the grid; a cell named twice; a line of the grid with
 *      neither a block nor a size; a block that disagrees with its line; a block with nnz > 0 and a NULL buffer, no row or no
 *      column; C sharing a buffer with any block; in any block offsets that descend, leave [ro[0], ro[0] + nnz] or whose last
 *      one does not span nnz (every row of every block is checked; an unsound offset is clamped, never followed); a column id
 *      >= cols OF ITS OWN BLOCK -- such an id may be smaller than cols(C), so only a per-block check finds it, and without
 *      it the entry would land in a neighbour block's columns.  SPECK_ERR_DIM_LIMIT, decided on the host: n_blocks >
 *      SPECK_BMAT_MAX_BLOCKS; rows or cols of C or of any block above 2^27; 2^32 pieces or more (a 64-bit count); 8 bytes per
 *      piece that the config's scratch cannot hold.  SPECK_ERR_NNZ_OVERFLOW: the blocks' nnz sum to 2^32 or more (a 64-bit
 *      sum on the host, before anything runs).  *info is zero once the arguments have passed, and again on an error.
 *  The sum of the blocks' nnz is known before anything runs, so C's buffers are prepared first and the call has ONE read-back,
 *      at the end.  CHECK: a thread per piece against the table of blocks uploaded once per call (three pointers, rows, cols,
 *      nnz, C0); its block row by a search in P0, i and q by a division; the row's two offsets; the piece's length, 0 where
 *      they are unsound; the shared scan gives G.  IDS: the tile kernel below in a mode that writes nothing compares every id
 *      with its own block's cols.  PLACE: one workgroup per tile of SPECK_BMAT_TILE_ENTRIES output entries, four consecutive
 *      ones per thread, whatever the row and block sizes; the tile's pieces by two searches in G, per piece its end, its
 *      source offset and its block in LDS (up to 4096 pieces; a tile that more touch reads them from global memory).  A tile
 *      that touches only block rows of a single block (vstack, block_diag) takes the blocks themselves for its units: a
 *      shift per block from origins the host made, neither G nor a row offset is read.  Every kernel that writes into C's
 *      buffers, the row offsets included, is queued behind the checks and does nothing where the verdict is raised; the host
 *      reads the status once (verdict, empty rows, longest row) and only then publishes C.  Values move as integers; no
 *      floating-point instruction and no atomic on anything but the two counters of the statistics: the same bytes from run
 *      to run.  16-byte loads and stores only where the address allows; every form gives the same bytes.
 *  Ownership of C as speck_select_* documents it: row_offsets reused when C->rows == rows(C), data / col_ids re-allocated
 *      only when C->nnz differs.  There is no in-place mode.  Runs on the config's stream (speck_config_set_stream is
 *      honoured: blocks produced on that stream need no synchronisation in front of the call) and returns with C complete.
 *      Temporaries are grow-only buffers of the config's own (not the multiply's arena): 48 bytes per block, 4 per output
 *      row, 8 per piece; cfg == NULL is allowed as for speck_sort_rows_*.  With the debug option guard_bytes the canary
 *      zones of the temporaries and of C are checked after the call.
 *  Not built: blocks of mixed value type, or pattern-only blocks; overlapping placements that add (assembly by speck_add_*);
 *      a fused sort; a Kronecker product; the batch vector itself (torch's repeat_interleave on the returned origins); a plan
 *      reused across calls; writing into a region of an existing C. ---- */
#define SPECK_BMAT_MAX_BLOCKS 65536
#define SPECK_BMAT_TILE_ENTRIES 4096
typedef struct speck_bmat_block {
    uint32_t block_row, block_col;           /* the cell */
    const speck_dcsr *M;                     /* what stands there (the struct on the HOST, its buffers on the device) */
} speck_bmat_block;
typedef struct speck_bmat_params {
    uint32_t block_rows, block_cols, n_blocks;
    const speck_bmat_block *blocks;          /* HOST, n_blocks cells in ANY order; a cell named twice is refused */
    const uint64_t *row_sizes, *col_sizes;   /* HOST, block_rows / block_cols entries; either may be NULL */
} speck_bmat_params;
typedef struct speck_bmat_info {
    uint64_t blocks;             /* cells that hold a block = n_blocks */
    uint64_t rows_out;           /* rows of C */
    uint64_t cols_out;           /* columns of C */
    uint64_t nnz_out;            /* entries of C = the sum of the blocks' nnz */
    uint64_t pieces;             /* (output row, block of its block row) pairs */
    uint64_t rows_empty;         /* rows of C without an entry */
    uint64_t max_row_entries;    /* the longest row of C */
} speck_bmat_info;
typedef struct speck_bmat_layout_out {       /* all HOST; the arrays may be NULL */
    uint64_t rows, cols, nnz, pieces;
    uint64_t *row_origins, *col_origins;     /* block_rows + 1 / block_cols + 1 entries */
} speck_bmat_layout_out;
int speck_bmat_layout(const speck_bmat_params *p, speck_bmat_layout_out *out);   /* host only: no device, no config */
int speck_bmat_f64(speck_config *cfg, const speck_bmat_params *p, speck_dcsr *C, speck_bmat_info *info /* may be NULL */);
int speck_bmat_f32(speck_config *cfg, const speck_bmat_params *p, speck_dcsr *C, speck_bmat_info *info);

/* ---- row-sharded multi-GPU (new: the reference is single-GPU, source/Executor.cpp:25).  One process per GPU;
 *      rank p multiplies the row range [b_p, b_{p+1}) of A (a view with absolute offsets, boundaries from
 *      speck_partition_rows) with a replicated B, then ONE exchange concatenates the shards on a root rank:
 *      ncclAllGather of the shard sizes + a gatherv built from grouped ncclSend / ncclRecv over xGMI (RCCL has no
 *      gatherv) + a rebase of the received row offsets.  librccl is resolved with dlopen at the first call. ---- */
enum {
    SPECK_TRANSPORT_RCCL = 0,     /* device-to-device over xGMI */
    SPECK_TRANSPORT_HOSTMEM = 1   /* staged through POSIX shared memory: ranks that cannot form an RCCL
                                   * communicator (several ranks on one GPU -- plumbing checks) */
};
typedef struct speck_comm speck_comm;
typedef struct speck_gather_plan speck_gather_plan;
/* ncclGetUniqueId: 128 bytes made by ONE rank and handed to the others by the launcher (file, pipe, MPI, ...) */
int speck_comm_unique_id(int transport, void *id128);
/* ncclCommInitRank on `device`; collective over all ranks of the job */
int speck_comm_init(int device, int nranks, int rank, int transport, const void *id128, speck_comm **out);
int speck_comm_destroy(speck_comm *comm);
int speck_comm_info(const speck_comm *comm, int *nranks, int *rank, int *transport);
/* One-shot gatherv (collective): every rank passes its shard of C (local row offsets, as speck_multiply returns
 * it for a row-range view of A); on `root`, *full receives the concatenated matrix (callee allocates, caller
 * frees with speck_dcsr_free); other ranks may pass NULL. */
int speck_gatherv_csr(speck_comm *comm, int root, const speck_dcsr *shard, uint64_t cols, size_t value_size,
                      speck_dcsr *full);
/* Repeated exchange of shards whose sizes do not change (the benchmark loop): sizes are exchanged and the
 * root's buffers allocated ONCE (collective; create plans in the same order on every rank), start() posts the
 * transfers of a slot on the communicator's own stream and returns -- they overlap the next multiply -- and
 * wait() blocks on the slot's event.  A slot's shard must stay untouched between start() and wait() (alternate
 * two output matrices).  On the root, wait() fills *full_view with a VIEW of the slot's buffers (owned by the
 * plan, valid until the slot is started again). */
int speck_gather_plan_create(speck_comm *comm, int root, uint64_t rows_local, uint64_t cols, uint64_t nnz_local,
                             size_t value_size, int slots, speck_gather_plan **out);
int speck_gather_start(speck_gather_plan *plan, int slot, const speck_dcsr *shard);
int speck_gather_wait(speck_gather_plan *plan, int slot, speck_dcsr *full_view);
/* displacements of every rank's rows / entries in the concatenation (nranks + 1 entries each; either may be NULL) */
int speck_gather_plan_layout(const speck_gather_plan *plan, uint64_t *row_displs, uint64_t *nnz_displs);
int speck_gather_plan_destroy(speck_gather_plan *plan);

/* ---- host-side synthetic inputs and on-disk formats ---- */
typedef struct speck_host_csr speck_host_csr; /* opaque host CSR<double>, include/CSR.h */
/* kind: "uniform" (config #1), "scircuit", "webbase", "mac_econ", "cant", "nlpkkt";
 * scale multiplies the row count (1.0 = the SuiteSparse dimensions). */
int speck_gen_matrix(const char *kind, double scale, uint64_t seed, int signed_values,
                     speck_host_csr **out);
/* loadMTX + convert(COO->CSR) -- source/COO.cpp:53-164, source/CSR.cpp:173-212 */
int speck_load_mtx(const char *path, speck_host_csr **out);
/* MatrixMarket writer (no reference counterpart): coordinate real, general or -- symmetric_lower != 0 -- the
 * lower triangle as `symmetric` (the caller vouches for the symmetry) */
int speck_store_mtx(const speck_host_csr *m, const char *path, int symmetric_lower);
/* loadCSR / storeCSR (.hicsr) -- source/CSR.cpp:88-137 */
int speck_load_hicsr(const char *path, speck_host_csr **out);
int speck_store_hicsr(const speck_host_csr *m, const char *path);
/* DataLoader: "<path>d_.hicsr" cache, else .mtx then write cache -- source/DataLoader.cpp:24-58 */
int speck_load_matrix(const char *path, int write_cache, speck_host_csr **out);
int speck_host_csr_dims(const speck_host_csr *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz);
int speck_host_csr_copy(const speck_host_csr *m, uint32_t *row_offsets, uint32_t *col_ids, double *data);
int speck_host_csr_from_arrays(uint64_t rows, uint64_t cols, uint64_t nnz, const uint32_t *row_offsets,
                               const uint32_t *col_ids, const double *data, speck_host_csr **out);
int speck_host_csr_free(speck_host_csr *m);

const char *speck_status_string(int status);
const char *speck_version(void);

#ifdef __cplusplus
}
#endif
#endif
