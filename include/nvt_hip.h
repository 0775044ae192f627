/*
 * nvt_hip.h -- C ABI of the MI355X (gfx950) kernels behind the NVTabular hot path.
 *
 * This is the drop-in boundary: every O(rows) step that NVTabular's operators
 * hand to a dataframe backend (pandas on CPU, libcudf on GPU) for the
 * Categorify / FillMissing / Normalize / HashBucket / JoinGroupby /
 * TargetEncoding path has one entry point here.  Signatures use plain device
 * pointers and sizes only (no torch / Arrow types).  Conventions:
 *
 *   - every function returns 0 on success, a negative NVT_E* code on failure;
 *     nvt_last_error() returns a thread-local message for the last failure;
 *   - all data pointers are DEVICE pointers (HBM); the caller owns every buffer
 *     (nvt_gb_table objects own their slot arrays);
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous;
 *   - `valid` is an Arrow validity bitmap (LSB-first, 1 = valid, bit i = row i)
 *     or NULL when the column has no nulls.  Float columns additionally treat
 *     NaN as null (pandas isna() semantics);
 *   - re-entrant: no global mutable state.
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   nvtabular/ops/categorify.py:955-1051   _top_level_groupby   -> nvt_count_*          (size-only)
 *   nvtabular/ops/categorify.py:1054-1137  _mid/_bottom_level   -> nvt_count_merge_*, nvt_gb_merge
 *   nvtabular/ops/categorify.py:1149-1337  _write_uniques sorts -> nvt_count_compact_*, nvt_vocab_sort_*
 *   nvtabular/ops/categorify.py:1558-1807  _encode              -> nvt_encode_build_*, nvt_encode_*
 *   nvtabular/ops/categorify.py:1837-1852  _hash_bucket         -> nvt_hash_bucket_* / nvt_encode_* (num_buckets)
 *   nvtabular/ops/hash_bucket.py:86-100    HashBucket.transform -> nvt_hash_bucket_*
 *   nvtabular/ops/moments.py:64-77         _chunkwise_moments   -> nvt_moments
 *   nvtabular/ops/fill.py:49-57            FillMissing          -> nvt_fill_normalize (do_norm = 0)
 *   nvtabular/ops/normalize.py:71-90       Normalize.transform  -> nvt_fill_normalize
 *   nvtabular/ops/normalize.py:150-186     NormalizeMinMax      -> nvt_minmax, nvt_fill_normalize
 *   nvtabular/ops/join_groupby.py:175-217  JoinGroupby.transform-> nvt_gb_lookup + nvt_gather_f64
 *   nvtabular/ops/target_encoding.py:301-384 _op_group_logic    -> nvt_gb_lookup + nvt_te_apply
 *   nvtabular/ops/groupby.py:236-263       Groupby.transform    -> nvt_order_rows + nvt_seg_aggregate, nvt_seg_nunique
 *   nvtabular/ops/data_stats.py:52-92      DataStats.fit        -> nvt_col_profile_many (+ nvt_dense_count_many)
 *   nvtabular/ops/reduce_dtype_size.py:40-56 ReduceDtypeSize    -> nvt_col_profile_many, nvt_cast_many
 *   cpp/nvtabular/inference/categorify.cc:145-252, fill.cc:91-102 (serving-time
 *   encode / fill loops) have the same element semantics as nvt_encode_* /
 *   nvt_fill_normalize.
 */
#ifndef NVT_HIP_H
#define NVT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVT_OK 0
#define NVT_EINVAL (-1)   /* bad argument */
#define NVT_EHIP (-2)     /* a HIP runtime call failed */
#define NVT_ENOMEM (-3)
#define NVT_EUNSUPPORTED (-4) /* valid input this library does not handle (the caller falls back) */

/* element types of continuous columns */
#define NVT_F32 0
#define NVT_F64 1
#define NVT_I32 2
#define NVT_I64 3
#define NVT_U8 4
/* narrow integers: outputs of nvt_cast_many and sources of nvt_pq_widen_i32_many only */
#define NVT_I8 5
#define NVT_I16 6

/* sentinel keys marking an empty hash slot; rows holding this key value are
 * counted in state[NVT_ST_SENTINEL] instead of the table */
#define NVT_EMPTY_I32 INT32_MIN
#define NVT_EMPTY_I64 INT64_MIN

/* layout of the uint64_t state[NVT_STATE_WORDS] block every count/groupby table carries */
#define NVT_ST_NULLS 0     /* rows whose key was null                        */
#define NVT_ST_SENTINEL 1  /* rows whose key equalled the empty sentinel     */
#define NVT_ST_OCCUPIED 2  /* distinct keys currently in the table           */
#define NVT_ST_OVERFLOW 3  /* != 0: table too full, result invalid -> regrow */
/* range path, diagnostic bits beside overflow bit0: WHY the column has to be rerun */
#define NVT_OVF_REGION 16ull  /* a (bucket, workgroup) region of the partition pass filled up  */
#define NVT_OVF_PROBE 32ull   /* a probe chain left the bucket table (keys cluster in a range) */
#define NVT_OVF_FULL 64ull    /* a bucket holds more than 3/4 * 16384 distinct keys            */
#define NVT_ST_ROWS 4      /* rows consumed (nulls included)                 */
/* words 5..7: scratch cursors of nvt_dense_count_*                                  */
#define NVT_ST_MAXCOUNT 8  /* nvt_dense_count_*: largest count in the output list; the sentinel
                              key's rows are not in the list of the hash paths and not in this
                              word either.  The ordering passes would do with an upper bound
                              (nvt_vocab_sort_*), but the value is EXACT on every path: the
                              tree merge hands it on as the max_count of every merged list, and
                              a bound that is only "at least" would grow from level to level
                              and buy the vocabulary sort radix passes it does not need     */
#define NVT_ST_BIG 9       /* range path: entries whose count is >= 255            */
#define NVT_ST_NEED 10     /* range path, overflow bit1: entries the output list needs */
#define NVT_STATE_WORDS 16

int nvt_version(void);
const char *nvt_last_error(void);

/* ---- Categorify.fit: groupby-size tables (open addressing, linear probe) ----
 * i32 table slot = {int32 key, uint32 count} (8 B); i64 slot = {int64 key,
 * uint64 count} (16 B).  capacity must be a power of two. */
int nvt_count_table_bytes(int key_bytes, uint64_t capacity, uint64_t *bytes);
int nvt_count_clear(void *table, int key_bytes, uint64_t capacity, uint64_t *state, void *stream);
int nvt_count_i32(const int32_t *keys, const uint8_t *valid, uint64_t n, void *table,
                  uint64_t capacity, uint64_t *state, void *stream);
int nvt_count_i64(const int64_t *keys, const uint8_t *valid, uint64_t n, void *table,
                  uint64_t capacity, uint64_t *state, void *stream);
/* weighted insert of an (key,count) list -- the tree-merge step (_mid_level_groupby)
 * and the owner-side merge after the multi-GPU exchange.  The list has no validity bitmap.
 * An i32 slot keeps a uint32 count: sums that may pass 2^32 need an i64 table (the driver's
 * weighted last resort widens int32 keys for that reason). */
int nvt_count_merge_i32(const int32_t *keys, const int64_t *counts, uint64_t n, void *table,
                        uint64_t capacity, uint64_t *state, void *stream);
int nvt_count_merge_i64(const int64_t *keys, const int64_t *counts, uint64_t n, void *table,
                        uint64_t capacity, uint64_t *state, void *stream);
/* table -> dense (key,count) arrays, arbitrary order; *out_n (device) = rows written.
 * out arrays must hold state[NVT_ST_OCCUPIED] entries (capacity is always enough) */
int nvt_count_compact_i32(const void *table, uint64_t capacity, int32_t *out_keys,
                          int64_t *out_counts, uint64_t *out_n, void *stream);
int nvt_count_compact_i64(const void *table, uint64_t capacity, int64_t *out_keys,
                          int64_t *out_counts, uint64_t *out_n, void *stream);

/* ---- Categorify.fit, atomic-free: key column -> dense (key,count) list ----
 * Replaces categorify.py:1018 (the groupby-size of _top_level_groupby) and, with weights,
 * the concat + re-groupby of categorify.py:1059-1063.  `path` selects the kernel family:
 *   0  LDS tables, two launches: 256 workgroups count their row slab into a private LDS
 *      table and flush it grouped by home range; 256 workgroups merge one range each
 *      (<= ~11000 distinct int32 keys, ~5000 for int64 keys / weighted input);
 *   6  path 0 for <= 64 distinct keys: hot keys replicated per 8-lane group (same-address
 *      LDS atomics serialise);
 *   7  path 0 with 2 key classes per row slab: each LDS table keeps the keys of one class,
 *      the column is read twice (<= ~21000 distinct keys; 350 us against 420 us on path 1);
 *   1 / 2 / 3  hash-partition the rows into 256 / 64 x 64 / 64 x 256 buckets (exact
 *      per-tile histograms + scan, no cursor atomics), then one LDS table per bucket; a
 *      bucket inflated by a hot key is cut into a primary chunk plus small excess chunks
 *      (dispatched last) whose partial lists are merged per bucket.
 *   path | NVT_PATH_HOT (paths 1 / 2 / 3, int32 keys, no weights): a hot-key filter in front
 *      of the partition -- the histogram pass also counts the rows of a few thousand frequent
 *      keys (picked from a sample of the column) in LDS and switches them off for the
 *      scatter / count stages, which then handle only the remaining rows (60-95 % fewer on
 *      power-law columns).  Exact for any hot set.
 *   NVT_PATH_RANGE | (log2(buckets) << 8)  (int32 keys, no weights, 64 .. 1024 buckets of
 *      <= ~6000 distinct keys each): ONE pass partitions the rows that the hot-key filter does
 *      not absorb by KEY RANGE through per-workgroup write-combining bins in LDS (64-byte lines
 *      into a private region per (bucket, workgroup): no histogram pre-pass, no cursors); one
 *      workgroup per bucket then counts its rows in an LDS table addressed by a monotone
 *      function of the key and emits it in key order.  The output list is SORTED BY KEY
 *      (sentinel key first), and hot_image[NVT_RANGE_AUX_HIST + c] receives the number of
 *      entries with min(count, 255) == c -- what nvt_vocab_finalize_many needs to order the
 *      vocabulary by (count desc, key asc) in ONE stable counting pass (nvt_vocab_col.src_keys).
 *      hot_image must then be the column's own int32[NVT_RANGE_AUX_WORDS].  Ranges are derived
 *      from the sampled min / max: keys that are not spread over their range overflow a region
 *      or a table (overflow bit0) and the column is rerun on a hash path.
 * weights (optional, int64 per row) turns the count into a weighted sum -- the tree-merge
 * of (key,count) lists (_mid_level_groupby).  ws: device scratch of
 * nvt_dense_count_ws_bytes().  state (device uint64[NVT_STATE_WORDS], written):
 * [NVT_ST_NULLS] null rows (weighted), [NVT_ST_SENTINEL] rows whose key is the empty
 * sentinel (NOT in the list), [NVT_ST_OCCUPIED] entries written, [NVT_ST_MAXCOUNT] the
 * largest count, [NVT_ST_OVERFLOW] bit0: an LDS table filled up (rerun on a larger path),
 * bit1: out_capacity too small.  The output list is in no particular order. */
#define NVT_PATH_HOT 16
#define NVT_HOT_IMAGE_WORDS 8192
#define NVT_PATH_RANGE 9
#define NVT_PATH_PIECES 0x10000     /* with NVT_PATH_RANGE: let the sample decide on a piecewise map
                                       (sampled quantile splitters) -- for keys that are not spread
                                       over their range; asked for after the linear map overflowed */
#define NVT_PATH_SORT 10            /* int32 keys, no weights, any number of distinct keys: radix sort of
                                       the rows + run lengths; key-sorted output like the range path;
                                       hot_image = uint32[256] receiving the histogram of min(count, 255) */
#define NVT_RANGE_WGS 256           /* partition workgroups = runs per bucket                 */
#define NVT_RANGE_AUX_LO 8192       /* aux words behind the hot image: range origin (biased),
                                       span, multiplier, 0, pre-shift of the monotone map (nvt_range.hpp) */
#define NVT_RANGE_AUX_HIST 8208     /*   uint32[256] histogram of min(count, 255)             */
#define NVT_RANGE_AUX_HOTSTART 8464 /*   uint32[1025]: hot image slots by bucket (CSR offsets) */
#define NVT_RANGE_AUX_HOTORDER 9504 /*   uint16[8192]: the image slots in bucket order         */
#define NVT_RANGE_AUX_PW 13600      /*   piecewise map (keys not spread over their range): u32
                                       splitters[65], mul[64], shift flags[2]; word LO + 7 = fine
                                       slots per piece (0: the linear map)                      */
#define NVT_RANGE_AUX_WORDS (13600 + 256)
int nvt_dense_count_ws_bytes(int key_bytes, uint64_t n, int path, int weighted, uint64_t *bytes);
int nvt_dense_count_i32(const int32_t *keys, const uint8_t *valid, const int64_t *weights,
                        uint64_t n, int path, void *ws, int32_t *out_keys, int64_t *out_counts,
                        uint64_t out_capacity, uint64_t *state, void *stream);
int nvt_dense_count_i64(const int64_t *keys, const uint8_t *valid, const int64_t *weights,
                        uint64_t n, int path, void *ws, int64_t *out_keys, int64_t *out_counts,
                        uint64_t out_capacity, uint64_t *state, void *stream);

/* ---- vocabulary order (_write_uniques): count descending, key ascending ----
 * LSD radix sort of n (key,count) pairs; tmp must hold nvt_vocab_sort_tmp_bytes(). */
int nvt_vocab_sort_tmp_bytes(int key_bytes, uint64_t n, uint64_t *bytes);
/* max_count: an upper bound on counts[] (e.g. state[NVT_ST_MAXCOUNT]) lets the sort pick
 * its count passes without reading anything back; <= 0 = unknown (the sort then builds
 * per-pass histograms and synchronises the stream once). */
int nvt_vocab_sort_i32(int32_t *keys, int64_t *counts, uint64_t n, int64_t max_count, void *tmp,
                       void *stream);
int nvt_vocab_sort_i64(int64_t *keys, int64_t *counts, uint64_t n, int64_t max_count, void *tmp,
                       void *stream);

/* ---- Categorify.transform (_encode) ----
 * encode table slot: i32 = {int32 key, int32 label}; i64 = {int64 key, int64 label}.
 * Build assigns label first_label + i to vocab_keys[i]. */
int nvt_encode_table_bytes(int key_bytes, uint64_t capacity, uint64_t *bytes);
/* Diagnostic of the cache-mode encode (int32 keys whose vocabulary exceeds the LDS head): with
 * NVT_ENC_STATS=1 in the environment the kernels count out2[0] = rows that went on to the table in
 * HBM and out2[1] = rows looked up, since the last reset (synchronises the stream). */
int nvt_encode_stats(uint64_t *out2, int reset, void *stream);
/* unique_keys != 0 promises vocab_keys holds no duplicates (true for fitted vocabularies):
 * int32 slots are then claimed and filled with one 64-bit CAS.  With duplicates (user
 * vocabs) the lowest label wins. */
int nvt_encode_build_i32(const int32_t *vocab_keys, uint64_t n_vocab, int64_t first_label,
                         void *table, uint64_t capacity, int64_t *sentinel_label, int unique_keys,
                         void *stream);
int nvt_encode_build_i64(const int64_t *vocab_keys, uint64_t n_vocab, int64_t first_label,
                         void *table, uint64_t capacity, int64_t *sentinel_label, int unique_keys,
                         void *stream);
/* out[i] = null_label            if key i is null
 *        = table[key]            if present
 *        = oov_label             if absent and num_buckets <= 1
 *        = oov_label + h32(key) % num_buckets   otherwise      (out_bytes: 4 or 8)
 * vocab_keys / n_vocab / first_label (optional: pass NULL, 0, 0): the ordered, duplicate-free
 * vocabulary the table was built from.  Its head -- the most frequent keys -- is then
 * staged in LDS by every workgroup and only rows that miss it probe the table in HBM.
 * A vocabulary of at most NVT_ENCODE_RESIDENT_I32 (8192) int32 / NVT_ENCODE_RESIDENT_I64
 * (6144) int64 keys is staged in full: table and sentinel_label may then be NULL and
 * nvt_encode_build_* need not be called at all. */
#define NVT_ENCODE_RESIDENT_I32 8192
#define NVT_ENCODE_RESIDENT_I64 6144
int nvt_encode_i32(const int32_t *keys, const uint8_t *valid, uint64_t n, const void *table,
                   uint64_t capacity, const int64_t *sentinel_label, int64_t null_label,
                   int64_t oov_label, uint32_t num_buckets, void *out, int out_bytes,
                   const int32_t *vocab_keys, uint64_t n_vocab, int64_t first_label, void *stream);
int nvt_encode_i64(const int64_t *keys, const uint8_t *valid, uint64_t n, const void *table,
                   uint64_t capacity, const int64_t *sentinel_label, int64_t null_label,
                   int64_t oov_label, uint32_t num_buckets, void *out, int out_bytes,
                   const int64_t *vocab_keys, uint64_t n_vocab, int64_t first_label, void *stream);

/* ---- HashBucket / hashed OOV buckets: out[i] = h32(key) % num_buckets (int32);
 * a null row (valid bit clear) hashes as key 0 whatever bytes its slot holds (Arrow leaves the
 * values under a null undefined; the pandas path hashes fillna(0)).
 * xor_in (optional, uint64 per row) is XORed into the 64-bit hash first and
 * xor_out (optional) receives the 64-bit hash -- the "combo" XOR chain of
 * categorify.py:1846-1851 */
int nvt_hash_bucket_i32(const int32_t *keys, const uint8_t *valid, uint64_t n, uint32_t num_buckets,
                        int32_t *out, const uint64_t *xor_in, uint64_t *xor_out, void *stream);
int nvt_hash_bucket_i64(const int64_t *keys, const uint8_t *valid, uint64_t n, uint32_t num_buckets,
                        int32_t *out, const uint64_t *xor_in, uint64_t *xor_out, void *stream);

/* ---- Normalize.fit (_chunkwise_moments): out[3] (double, device) += {count, sum, sum of
 * squares} over non-null rows; with has_fill, nulls count as fill_val (FillMissing
 * upstream of Normalize).  partials: device scratch of nvt_moments_scratch_bytes(). */
uint64_t nvt_moments_scratch_bytes(void);
int nvt_moments(const void *x, int dtype, const uint8_t *valid, uint64_t n, int has_fill,
                double fill_val, double *out3, void *partials, void *stream);
/* NormalizeMinMax.fit: out2 = {min, max} over non-null rows (NaN if none), merged with
 * the values already in out2 when accumulate != 0 */
int nvt_minmax(const void *x, int dtype, const uint8_t *valid, uint64_t n, int accumulate,
               double *out2, void *partials, void *stream);

/* ---- FillMissing + Normalize.transform, fused:
 *   v      = isnull(x[i]) ? (has_fill ? fill_val : NaN) : x[i]
 *   out[i] = do_norm ? (scale > 0 ? (v - shift) / scale : v - shift) : v
 * out dtype NVT_F32 / NVT_F64 (or the input dtype when do_norm == 0 and ints are
 * filled); filled (optional, uint8 0/1 per row) receives isnull(x[i]) -- the
 * `<col>_filled` column of FillMissing(add_binary_cols=True). */
int nvt_fill_normalize(const void *x, int dtype, const uint8_t *valid, uint64_t n, int has_fill,
                       double fill_val, int do_norm, double shift, double scale, void *out,
                       int out_dtype, uint8_t *filled, void *stream);

/* ---- Clip + LogOp (the reference benchmark's default continuous branch,
 * bench/examples/dask-nvtabular-criteo-benchmark.py:201-204; clip.py:49-55, logop.py:43-53),
 * fused with a pending FillMissing constant:
 *   v = isnull(x) ? (has_fill ? fill_val : null) : x;  v = clamp(v, vmin, vmax);
 *   out = do_log ? logf((float)v + 1) : v          (nulls stay null; NaN for float outputs)
 * out_dtype: NVT_F32 / NVT_F64, or the input dtype for integer clipping without log.  Integer
 * clipping clamps in the integer type (a value inside the bounds is returned bit for bit);
 * fill_val / vmin / vmax must then be integers of that type with |v| <= 2^53, else NVT_EINVAL.
 * The same holds for fill_val of nvt_fill_normalize with an integer out_dtype. */
int nvt_clip_log(const void *x, int dtype, const uint8_t *valid, uint64_t n, int has_fill,
                 double fill_val, int has_min, double vmin, int has_max, double vmax, int do_log,
                 void *out, int out_dtype, void *stream);

/* ---- Bucketize (bucketize.py:76-94): out[i] = np.digitize(x[i], boundaries, right=False),
 * i.e. the number of (ascending, float64, device) boundaries <= x[i]; null / NaN rows get
 * n_boundaries (numpy's answer for NaN).  n_boundaries <= 8192. */
int nvt_bucketize(const void *x, int dtype, const uint8_t *valid, uint64_t n,
                  const double *boundaries, int n_boundaries, int32_t *out, void *stream);

/* ---- JoinGroupby / TargetEncoding / combo-Categorify: multi-key groupby tables ----
 * A table over nkeys (1..3) key columns (each int64 after widening; null components
 * allowed and form their own groups, pandas dropna=False) and nvals (0..8) value
 * columns.  Accumulators per group: size (all rows), count (rows whose FIRST key
 * component is non-null -- categorify.py:995-999), and per value column
 * sum / sum of squares / min / max over its non-null entries. */
typedef struct nvt_gb_table nvt_gb_table;
#define NVT_GB_SUMSQ 1   /* keep sum of squares (std / var requested)  */
#define NVT_GB_MINMAX 2  /* keep min / max                             */
/* The table object owns its device arrays (hipMalloc'ed on the current device). */
int nvt_gb_create(int nkeys, int nvals, int flags, uint64_t capacity, nvt_gb_table **out);
void nvt_gb_destroy(nvt_gb_table *t);
/* The same table in CALLER-provided device memory (nvt_gb_table_bytes() bytes): hipMalloc and
 * hipFree synchronise the device, which a fit that builds a table per partition cannot
 * afford.  nvt_gb_destroy then only frees the handle. */
int nvt_gb_table_bytes(int nkeys, int nvals, int flags, uint64_t capacity, uint64_t *bytes);
int nvt_gb_create_in(int nkeys, int nvals, int flags, uint64_t capacity, void *memory,
                     uint64_t bytes, nvt_gb_table **out);
/* device address of the table's uint64[NVT_STATE_WORDS] state block (read it back with
 * nvt_mailbox_post instead of the blocking nvt_gb_state) */
uint64_t *nvt_gb_state_ptr(nvt_gb_table *t);
/* nvt_gb_update orders the rows by group (assign slot -> radix sort -> segmented reduce; no
 * per-row accumulator atomics) and needs nvt_gb_update_ws_bytes(n) bytes of scratch: owned and
 * grown by the table unless the caller hands one over with nvt_gb_set_workspace. */
int nvt_gb_update_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_gb_set_workspace(nvt_gb_table *t, void *ws, uint64_t bytes);
int nvt_gb_clear(nvt_gb_table *t, void *stream);
/* keys[k]: int64 device column, key_valid[k]: bitmap or NULL; vals[j]: column of vdtype[j].
 * Values of every dtype are reduced as float64 (here and in nvt_seg_aggregate), so int64 values
 * are exact up to +-2^53 and round beyond. */
int nvt_gb_update(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *const *key_valid,
                  const void *const *vals, const int *vdtypes, const uint8_t *const *val_valid,
                  uint64_t n, void *stream);
/* merge another table's groups into t (tree reduce / multi-GPU owner merge) given its
 * compacted columns */
int nvt_gb_merge(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *key_null_mask,
                 const int64_t *size, const int64_t *count, const double *const *sum,
                 const double *const *sumsq, const double *const *vmin,
                 const double *const *vmax, uint64_t n, void *stream);
/* host-visible occupancy / overflow: state[NVT_STATE_WORDS] copied to host memory */
int nvt_gb_state(nvt_gb_table *t, uint64_t *host_state, void *stream);
/* compact groups: out_keys[k][g], out_null_mask[g] (bit k = component k is null),
 * out_size/out_count[g], out_sum/sumsq/min/max[j][g]; any out pointer may be NULL.
 * *out_n (device) = number of groups.
 * min / max of a group without a non-null value are NaN.  The table keeps no per-column value
 * count: "no value seen" is the initial +inf in min (-inf in max) itself, so a group whose
 * non-null values are ALL +inf reports min NaN, and one whose values are all -inf max NaN
 * (nvt_seg_aggregate returns a count per column and leaves that decision to its caller). */
int nvt_gb_compact(nvt_gb_table *t, int64_t *const *out_keys, uint8_t *out_null_mask,
                   int64_t *out_size, int64_t *out_count, double *const *out_sum,
                   double *const *out_sumsq, double *const *out_min, double *const *out_max,
                   uint64_t *out_n, void *stream);
/* transform side: build a lookup table over compacted group keys, then map rows to
 * group ids (row i -> index into the compacted arrays, -1 when unseen) */
int nvt_gb_index_build(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *key_null_mask,
                       uint64_t n_groups, void *stream);
int nvt_gb_lookup(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *const *key_valid,
                  uint64_t n, int64_t *out_group, void *stream);
/* ---- Groupby operator (groupby.py:236-263): row order by (group, sort columns) + aggregates.
 * nvt_sort_key_u64: order-preserving 64-bit image of a column (nulls / NaN last in either
 * direction, pandas na_position="last"; -0.0 and +0.0 share one image).  The largest image
 * is reserved for nulls, so the value that would map to it takes the image next to it: the two
 * values at that end of the order -- INT64_MAX and INT64_MAX - 1 ascending, INT64_MIN and
 * INT64_MIN + 1 descending -- tie and keep their row order.  Only int64 columns reach it:
 * int32 / uint8 are widened first, and the float images of that end are NaN bit patterns
 * (-inf and -DBL_MAX order exactly).  nvt_order_rows: stable refinement of a row order by
 * such a key (two 32-bit radix passes) or by group id (-1 = null key, sorted last); perm
 * entries are 64-bit words whose LOW 32 bits are the row index (after a gid refinement the high
 * half is the group id: exactly the `words` nvt_seg_aggregate takes).  nvt_seg_aggregate:
 * out_size uint64[ngroups] rows per group, out_count uint64[nvals][ngroups] non-null values per
 * column, out_sum / out_sumsq / out_min / out_max double[nvals][ngroups] (any of the last
 * three pairs may be NULL) in one wave-level segmented reduction; outputs pre-initialised by
 * the caller (0 / 0 / 0 / 0 / +inf / -inf). */
int nvt_sort_key_u64(const void *x, int dtype, const uint8_t *valid, uint64_t n, int ascending,
                     uint64_t *out, void *stream);
int nvt_order_rows_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_order_rows(const uint64_t *key64, const int64_t *gid, uint64_t ngroups,
                   const uint64_t *perm_in, uint64_t n, uint64_t *perm_out, void *ws, void *stream);
int nvt_seg_aggregate(const uint64_t *words, uint64_t n, uint64_t ngroups, const void *const *vals,
                      const int *vdtypes, const uint8_t *const *val_valid, int nvals,
                      uint64_t *out_size, uint64_t *out_count, double *out_sum, double *out_sumsq,
                      double *out_min, double *out_max, void *stream);
/* Groupby nunique (groupby.py:190-198): out[c][g] = number of distinct values of column c among
 * the rows of group g, pandas groupby(...).nunique() with dropna=True.  `words`: the n words
 * nvt_seg_aggregate takes (group << 32 | row, ordered by group, rows of a group in any order;
 * words of a group >= ngroups -- the rows of null keys -- are ignored).  vals[c]: device column
 * of vdtypes[c] (NVT_F32 / F64 / I32 / I64 / U8), indexed by row; val_valid: NULL, or per column
 * a bitmap or NULL.  An entry counts when it is valid and not NaN; two entries are one value when
 * == says so on the column's own type: -0.0 and +0.0 are one value, +-inf are ordinary values,
 * and every int64 value is its own (INT64_MAX and INT64_MAX - 1 included: the image the rows
 * are ordered by is injective, unlike nvt_sort_key_u64's, because nulls leave through the group
 * id and need no image).  out: uint64[ncols][ngroups], zeroed by the caller; a group without a
 * counting entry keeps 0.  ncols 0..8.  n == 0 or ngroups == 0 returns NVT_OK without a launch;
 * otherwise null pointers, ncols outside 0..8 and an unknown dtype are NVT_EINVAL before any
 * launch.  ws: nvt_seg_nunique_ws_bytes(n) bytes.  Per column: the rows are refined by value
 * inside their groups (stable radix sorts of 32-bit key chunks, then of the group id) and the
 * value changes are summed per group by a wave-level segmented reduction -- the cost of a sort,
 * whatever the group sizes; work on `stream` only, no read-back. */
int nvt_seg_nunique_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_seg_nunique(const uint64_t *words, uint64_t n, uint64_t ngroups, const void *const *vals,
                    const int *vdtypes, const uint8_t *const *val_valid, int ncols, uint64_t *out,
                    void *ws, void *stream);
/* out[i] = group[i] >= 0 ? src[group[i]] : miss   (stat columns joined back onto rows) */
int nvt_gather_f64(const double *src, const int64_t *group, uint64_t n, double miss, void *out,
                   int out_dtype, void *stream);
/* TargetEncoding (target_encoding.py:341-363): with g = group_all[i], f = group_fold[i]
 *   out[i] = (g < 0 || f < 0) ? y_mean     (the reference's unmatched left merges)
 *          : (sum_all[g] - sum_fold[f] + p*y_mean) / (cnt_all[g] - cnt_fold[f] + p)
 * -> float32/float64.  group_fold == NULL means kfold <= 1: no fold terms, only g decides. */
int nvt_te_apply(const int64_t *group_all, const int64_t *group_fold, const double *sum_all,
                 const int64_t *cnt_all, const double *sum_fold, const int64_t *cnt_fold,
                 uint64_t n, double p_smooth, double y_mean, void *out, int out_dtype,
                 void *stream);

/* the same with the DENSE fold statistics of nvt_sgb_reduce: f = g * kfold + fold[i], a pair
 * with cnt_fold[f] == 0 has no rows (unmatched merge: y_mean). */
int nvt_te_apply_folds(const int64_t *group_all, const uint8_t *fold, int kfold,
                       const double *sum_all, const int64_t *cnt_all, const double *sum_fold,
                       const int64_t *cnt_fold, uint64_t n, double p_smooth, double y_mean,
                       void *out, int out_dtype, void *stream);

/* ---- ONE int32 key column without nulls: groupby-aggregate by sorting ------------------
 * (categorify.py:955-1137 _top_level_groupby .. _bottom_level_groupby for JoinGroupby /
 * TargetEncoding, join_groupby.py:150-173, target_encoding.py:254-299.)  The rows are radix-
 * sorted by (key, fold), the groups come out DENSE and ordered by key:
 *   out_keys / out_keys32 [cap]            the group keys, ascending
 *   out_size  uint64[cap * kfold]          rows of (group g, fold f) at g * kfold + f
 *   out_sum / out_sumsq / out_min / out_max  double[nvals][cap * kfold] (NaN / null values
 *                                          skipped; min / max of an empty entry stay +-inf;
 *                                          the last three per flags NVT_GB_SUMSQ / _MINMAX)
 *   tot_size uint64[cap], tot_sum double[nvals][cap]   (kfold > 1 only) sums over the folds
 *   te_records double[nvals][cap][2 * (kfold + 1)] or NULL (kfold > 1 only): per group
 *                                          {sum, count, (sum_f, count_f) for every fold}, the
 *                                          layout nvt_flat_lookup_te reads with one probe
 * Keys: an int32 column (key_bias = INT32_MIN) or an int64 column whose keys span less than
 * 2^32 (key_bias = the smallest key; nvt_key_minmax writes {min, max} to device memory); the
 * 32-bit key image is key - key_bias.  out_keys hold the keys themselves, out_keys32 =
 * key - key_bias - 2^31 (what the flat index stores: pass key_offset = key_bias + 2^31 to the
 * nvt_flat_lookup* functions; 0 for int32 columns).
 * nvt_sgb_sort: words (key image << 32 | fold << row_bits | row) sorted on bits [row_bits, 64);
 * fold: uint8[n] ids < kfold, NULL with kfold == 1; n <= 2^(32 - bits(kfold - 1)), n < 2^30.
 * *sorted_out = device pointer INSIDE ws (nvt_sgb_sort_ws_bytes(n) bytes; keep ws alive),
 * *row_bits_out = 32 - bits(kfold - 1).  The sorted words serve every aggregate on the same key
 * column of the same rows (JoinGroupby after TargetEncoding ignores the fold bits: kfold = 1).
 * nvt_sgb_regroup: run heads of the sorted words -> group ids (out_keys / out_keys32 [cap]) and
 * the words rewritten as ((g * kfold + fold) << 32 | row) into regrouped[n] (not aliasing
 * sorted); cap * kfold < 2^32 - 1.  state[NVT_ST_OCCUPIED] = groups found; more than cap:
 * only the first cap groups are kept (their rows carry slot 0xFFFFFFFF) and
 * state[NVT_ST_NEED] = the capacity a second call needs.  ws: nvt_sgb_regroup_ws_bytes(n).
 * nvt_sgb_reduce: the statistics of the regrouped words (the arrays above; they are
 * initialised here).  kfold = words_kfold: per-(group, fold) entries + totals (+ te_records);
 * kfold = 1 with words_kfold > 1: per-group entries from words regrouped for ANOTHER
 * aggregate's folds (JoinGroupby after TargetEncoding on the same column: one sort, one
 * regroup).  state: the block nvt_sgb_regroup filled (device, read by the kernels only).
 * sorted_out[j] (array may be NULL, entries may be NULL): value column j in the order of the
 * words, in its own dtype [n] -- written while the column is gathered by row; sorted_in[j]: such
 * an array from an earlier aggregate on the same words, read streaming INSTEAD of the gather by
 * row (columns without validity bitmap, not int64).  No host synchronisation anywhere. */
int nvt_sgb_sort_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_key_minmax(const void *keys, int key_dtype, uint64_t n, int64_t *out2, void *stream);
int nvt_sgb_sort(const void *keys, int key_dtype, int64_t key_bias, const uint8_t *fold, int kfold,
                 uint64_t n, void *ws, uint64_t **sorted_out, int *row_bits_out, void *stream);
int nvt_sgb_regroup_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_sgb_regroup(const uint64_t *sorted, int row_bits, int kfold, int64_t key_bias, uint64_t n,
                    uint64_t cap, int64_t *out_keys, int32_t *out_keys32, uint64_t *regrouped,
                    uint64_t *state, void *ws, void *stream);
int nvt_sgb_reduce(const uint64_t *regrouped, int words_kfold, int kfold, const void *const *vals,
                   const int *vdtypes, const uint8_t *const *val_valid, int nvals, int flags,
                   uint64_t n, uint64_t cap, uint64_t *out_size, double *out_sum, double *out_sumsq,
                   double *out_min, double *out_max, uint64_t *tot_size, double *tot_sum,
                   double *te_records, const uint64_t *state, const void *const *sorted_in,
                   void *const *sorted_out, void *stream);
/* Owner-side merge of the (key, count) rows of the multi-GPU exchange by sorting
 * (categorify.py:1054-1070 _mid_level_groupby, done on the owner rank): rows = n words
 * (count << 32 | int32 key), 0 <= count < 2^31, in nseg segments [seg_off[s], seg_off[s + 1])
 * (device uint64[nseg + 1]; source-major, column-minor: segment s holds column s % ncol).
 * Output: the (column, key) groups ordered by column, then key: out_keys int32[n], out_col
 * int64[n], out_sum double[n] (summed counts: exact below 2^53); state[NVT_ST_OCCUPIED] =
 * groups.  n < 2^26, ncol <= 64.  ws: nvt_count_merge_sorted_ws_bytes(n).  No host sync. */
int nvt_count_merge_sorted_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_count_merge_sorted(const int64_t *rows, uint64_t n, const uint64_t *seg_off, int nseg,
                           int ncol, int32_t *out_keys, int64_t *out_col, double *out_sum,
                           uint64_t *state, void *ws, void *stream);
/* Seeded TargetEncoding folds (target_encoding.py:427-439: numpy.random.RandomState(seed)
 * .choice(arange(kfold), n)) on the device: MT19937 seeded by init_genrand(seed), 32-bit draws
 * masked to the next 2^k - 1 and rejected while >= kfold -- out[i] (uint8) = the i-th accepted
 * value, bit for bit numpy's sequence.  One workgroup walks the generator (it is sequential);
 * kfold <= 128. */
int nvt_fold_mt19937(uint32_t seed, int kfold, uint64_t n, uint8_t *out, void *stream);
/* The same values from chunks of 2^18 draws generated in parallel (jump-ahead polynomials of the
 * generator's characteristic polynomial, tools/mt_jump_polys.py): ws = nvt_fold_mt19937_par_ws_bytes
 * bytes of device scratch; *total_out (device word) receives the accepted values the chunks held --
 * the caller checks total >= n (the chunk count carries an 8-sigma margin) and falls back to
 * nvt_fold_mt19937 otherwise. */
int nvt_fold_mt19937_par_ws_bytes(uint64_t n, int kfold, uint64_t *bytes);
int nvt_fold_mt19937_par(uint32_t seed, int kfold, uint64_t n, uint8_t *out, void *ws, uint64_t ws_bytes,
                         uint64_t *total_out, void *stream);
/* Distinct keys of the first n rows of every column, ESTIMATED (HyperLogLog, 4096 registers: 1.6 %
 * standard error, small counts by linear counting), and the valid rows among them: what steers
 * the first counting path of a fit that has no cardinality hints (the role of the reference's
 * `cat_cache` / `tree_width` heuristics around categorify.py:1423-1478: sizing, never results).
 * out uint64[ncols][2] = {estimate, valid rows} (device).  One launch for all columns. */
typedef struct nvt_prefix_col {
  const void *keys;       /* int32 (key_bytes 4) or int64 (8) */
  const uint8_t *valid;   /* Arrow validity bitmap or NULL */
  uint64_t n;             /* rows to look at */
  int key_bytes;
} nvt_prefix_col;
int nvt_prefix_distinct(const nvt_prefix_col *cols, int ncols, uint64_t *out, void *stream);
/* ---- tree merge of KEY-SORTED partial results (multi-partition fit) ------------------------
 * Replaces the concat + re-groupby of _mid_level_groupby (categorify.py:1054-1070) inside the
 * tree of categorify.py:1423-1478 -- and the same tree under join_groupby.py:140-173 /
 * target_encoding.py:171-214 -- for partial results that are already ORDERED BY KEY (range path,
 * sort path, sort-path groupby): out = the union of the ascending, duplicate-free int32 key
 * lists A and B in key order; the counts of a key that occurs in both are summed.  out_keys /
 * out_counts hold na + nb entries, *out_n (device) receives the merged length.  counts are
 * optional (both NULL: keys only).  src_a / src_b (optional, int32[na + nb], on every column of
 * a call or on none): position in A / in B every output entry came from, -1 = none -- the map
 * nvt_merge_payload combines further payload arrays with.  na + nb < 2^31.  One merge-path
 * search launch + one tile launch for ALL columns of the call; ws:
 * nvt_merge_sorted_ws_bytes(cols, ncols) bytes, 16-byte aligned.  No host synchronisation. */
typedef struct nvt_merge_col {
  const int32_t *a_keys;
  const int64_t *a_counts;
  uint64_t na;
  const int32_t *b_keys;
  const int64_t *b_counts;
  uint64_t nb;
  int32_t *out_keys;
  int64_t *out_counts;
  int32_t *src_a;
  int32_t *src_b;
  uint64_t *out_n;
} nvt_merge_col;
int nvt_merge_sorted_ws_bytes(const nvt_merge_col *cols, int ncols, uint64_t *bytes);
int nvt_merge_sorted_many(const nvt_merge_col *cols, int ncols, void *ws, uint64_t ws_bytes,
                          void *stream);
/* out[i * width + j] = op(a[src_a[i] * width + j], b[src_b[i] * width + j]), a side whose index
 * is -1 contributes nothing.  dtype NVT_I64 / NVT_F64; op 0 add, 1 min, 2 max (NaN = no value). */
int nvt_merge_payload(const int32_t *src_a, const int32_t *src_b, uint64_t n, int width, int dtype,
                      int op, const void *a, const void *b, void *out, void *stream);
/* ---- multi-GPU vocabulary exchange: the device work around the collectives (the
 * reference's tree reduce of per-partition frames, categorify.py:1423-1529).  One launch per step
 * for ALL columns of a fit (<= 64 columns of int32 keys + int64 counts, ranks x columns <= 4096):
 *   nvt_exchange_ranges   rng int64[ncol][3] = {-min key, max key, sum of counts}; a column
 *                         without entries: {-INT64_MAX, -INT64_MAX, 0} (one MAX all-reduce follows)
 *   nvt_exchange_hist     send_mat uint64[G][ncol] = rows of column j owned by rank g, with
 *                         owner(key) = min((key - lo[j]) / width[j], G - 1) (key ranges)
 *   nvt_exchange_scatter  rows_out = (count << 32 | key) words grouped by (owner, column);
 *                         cursors uint64[G][ncol] (device) = the start of every group, advanced by
 *                         the call; the order inside a group is unspecified (counts < 2^31)
 *   nvt_exchange_pack_ordered  the same send buffer for KEY-SORTED lists: a group is a contiguous
 *                         slice of its column, row r of the column goes to start[cell] + (r -
 *                         first_row[cell]) -- every group arrives in key order and the owner merges
 *                         sorted runs (nvt_merge_sorted_many) instead of sorting; first_row / start:
 *                         device uint64[G][ncol]
 *   nvt_exchange_unpack   n gathered words in nseg segments [seg_off[s], seg_off[s + 1]) ->
 *                         keys_out / counts_out at dst_off[s] + (position in the segment)
 * lo / width: HOST arrays; seg_off / dst_off: device arrays.  No host synchronisation.
 * A column whose counts sum to 0 is reported by nvt_exchange_ranges like a column without entries.
 * A count of 2^31 or more does not fit the word: its low 32 bits travel and nvt_exchange_unpack
 * returns them sign-extended, so callers keep every count below 2^31. */
typedef struct nvt_xcol {
  const int32_t *keys;
  const int64_t *counts;
  uint64_t n;
} nvt_xcol;
int nvt_exchange_ranges(const nvt_xcol *cols, int ncol, int64_t *rng, void *stream);
/* the same for KEY-SORTED lists: {-first key, last key, 0} (no pass over the lists; the caller
 * supplies its own bound of the rows counted) */
int nvt_exchange_ranges_sorted(const nvt_xcol *cols, int ncol, int64_t *rng, void *stream);
int nvt_exchange_hist(const nvt_xcol *cols, int ncol, const int64_t *lo, const uint64_t *width, int G,
                      uint64_t *send_mat, void *stream);
int nvt_exchange_scatter(const nvt_xcol *cols, int ncol, const int64_t *lo, const uint64_t *width, int G,
                         uint64_t *cursors, int64_t *rows_out, void *stream);
int nvt_exchange_pack_ordered(const nvt_xcol *cols, int ncol, const int64_t *lo, const uint64_t *width,
                              int G, const uint64_t *first_row, const uint64_t *start, int64_t *rows_out,
                              void *stream);
int nvt_exchange_unpack(const int64_t *words, uint64_t n, const uint64_t *seg_off, const uint64_t *dst_off,
                        int nseg, int32_t *keys_out, int64_t *counts_out, void *stream);
/* nvt_exchange_unpack with one int32 of payload per word (extra[i] travels with words[i]: the
 * labels of the distributed vocabulary ordering, nvt_vocab_label_shard) */
int nvt_exchange_unpack2(const int64_t *words, const int32_t *extra, uint64_t n, const uint64_t *seg_off,
                         const uint64_t *dst_off, int nseg, int32_t *keys_out, int64_t *counts_out,
                         int32_t *extra_out, void *stream);
/* key -> position in an ascending int32 key list (the group ids of nvt_sgb_regroup) through
 * a flat range table laid out from the list in one pass (no inserts): replaces
 * nvt_gb_index_build + nvt_gb_lookup for such groups (join_groupby.py:198-203,
 * target_encoding.py:350-371).  aux: int32[NVT_FLAT_AUX_WORDS]; table: capacity 8-byte slots,
 * capacity >= slots + n + 64 (slots: home slots, any count from 64 to 2^32 - 1); tmp:
 * nvt_flat_index_tmp_bytes(n).
 * aux[NVT_FLAT_AUX_MAXDISP] = longest displacement (keys clustered in their range make long
 * probe runs: the caller may prefer a hashed index).  nvt_flat_lookup: out[i] = position of
 * keys[i] - key_offset (int32 / int64 column, optional validity bitmap) or -1. */
int nvt_flat_index_tmp_bytes(uint64_t n, uint64_t *bytes);
int nvt_flat_index_build(const int32_t *keys, uint64_t n, uint64_t slots, int32_t *aux, void *table,
                         uint64_t capacity, void *tmp, void *stream);
int nvt_flat_lookup(const void *keys, int dtype, const uint8_t *valid, uint64_t n, const int32_t *aux,
                    const void *table, uint64_t capacity, int64_t key_offset, int64_t *out,
                    void *stream);
/* JoinGroupby.transform in one pass (join_groupby.py:198-217): outs[c][i] = records[g][c] with
 * g = the group of keys[i], miss[c] when the key has no group; records double[groups][ncols]
 * (ncols <= 16), out_dtypes f32 / f64 / i32 / i64 (value-converting stores).  *unseen (device
 * word, may be NULL) is OR-ed with 1 when any row had no group -- the reference's
 * astype(int32) of a count column raises then (join_groupby.py:214). */
int nvt_flat_lookup_gather(const void *keys, int dtype, const uint8_t *valid, uint64_t n,
                           const int32_t *aux, const void *table, uint64_t capacity,
                           int64_t key_offset, const double *records, int ncols, void *const *outs,
                           const int *out_dtypes, const double *miss, uint64_t *unseen, void *stream);
/* TargetEncoding.transform in one pass (target_encoding.py:341-371): probe + nvt_te_apply(_folds)
 * on records double[groups][2 * (kfold + 1)] = {sum, count, (sum_f, count_f) ...} (te_records
 * of nvt_sgb_reduce); fold == NULL (kfold 1): records double[groups][2] = {sum, count}. */
int nvt_flat_lookup_te(const void *keys, int dtype, const uint8_t *valid, uint64_t n, const int32_t *aux,
                       const void *table, uint64_t capacity, int64_t key_offset, const uint8_t *fold,
                       int kfold, const double *records, double p_smooth, double y_mean, void *out,
                       int out_dtype, void *stream);

/* Lookup images: ONE probe and ONE packed record per row for every operator on a key column
 * (JoinGroupby.transform join_groupby.py:198-217 + TargetEncoding.transform
 * target_encoding.py:341-371 on the same key are two left merges on that key in the reference).
 * image = bytes[groups][stride_bytes] (stride a multiple of 8): every operator owns a byte range
 * of the record and stores there what a row receives, already in the OUTPUT dtype.
 * nvt_flat_lookup_image: g = gid_in[i] when gid_in != NULL, else the flat-index probe of keys[i];
 * gid_out (may be NULL) receives g as int32 (-1: no group).  Output c copies `sizes[c]` (4 / 8)
 * bytes from image[g][offs[c] + (folds[c] ? (1 + folds[c][i]) * sizes[c] : 0)] to outs[c][i];
 * rows without group receive miss_bits[c].  *unseen (may be NULL) is OR-ed with 1 when any row had
 * no group.  ncols <= 24.
 * nvt_image_pack: image[g][offs[c]] = (dst dtype) src[c][g], src float64 / int64 arrays [groups].
 * nvt_te_image: (kfold + 1) values per group at image[g][off + slot * size]: slot 0 =
 * (sum + p*mean) / (count + p), slot 1 + f = the out-of-fold value of fold f (mean when the
 * (group, fold) pair has no rows), from the totals tot_count / tot_sum [groups] and the dense fold
 * statistics fold_count / fold_sum [groups * kfold] of nvt_sgb_reduce (kfold = 0: totals only)
 * -- the expression nvt_te_apply_folds evaluates per row, evaluated once per (group, fold):
 * identical bits. */
int nvt_flat_lookup_image(const void *keys, int dtype, const uint8_t *valid, uint64_t n,
                          const int32_t *aux, const void *table, uint64_t capacity, int64_t key_offset,
                          const int32_t *gid_in, int32_t *gid_out, const void *image,
                          uint32_t stride_bytes, int ncols, void *const *outs,
                          const uint8_t *const *folds, const uint32_t *offs, const uint32_t *sizes,
                          const uint64_t *miss_bits, uint64_t *unseen, void *stream);
int nvt_image_pack(const void *const *src, const int *src_dtypes, const int *dst_dtypes,
                   const uint32_t *offs, int ncols, uint64_t groups, void *image,
                   uint32_t stride_bytes, void *stream);
/* JoinGroupby's values from the fit's accumulators (count int64 [groups]; sum / sumsq / mn / mx:
 * arrays of nvals float64 [groups] pointers, NULL arrays / entries when no requested statistic
 * needs them): output c = statistic kinds[c] (0 count, 1 sum, 2 mean, 3 min, 4 max, 5 var, 6 std;
 * categorify.py:1087-1131) of value column vals[c], stored as dst_dtypes[c] at image[g][offs[c]]. */
int nvt_jg_image(const int64_t *count, const double *const *sum, const double *const *sumsq,
                 const double *const *mn, const double *const *mx, int nvals, const int *kinds,
                 const int *vals, const int *dst_dtypes, const uint32_t *offs, int ncols, uint64_t groups,
                 void *image, uint32_t stride_bytes, void *stream);
int nvt_te_image(const int64_t *tot_count, const double *tot_sum, const int64_t *fold_count,
                 const double *fold_sum, int kfold, uint64_t groups, double p_smooth, double y_mean,
                 int out_dtype, void *image, uint32_t stride_bytes, uint32_t off, void *stream);

/* ---- key directory: the key -> group step in ONE 16-byte read -----------------------------------
 * (the same left merges, join_groupby.py:198-217 / target_encoding.py:341-371.)  The flat-index
 * probe above walks {key, group} slots across 64-byte lines: ~2.4 L2 misses per row with the
 * record, and the kernel runs at the rate the fabric takes misses (tools/pmc_lookup.sh).  Here the
 * groups' keys are ascending (group g = position g of keys32) and
 *   dir[b] = uint32[4] {first, k0, k1, k2}, b = 0 .. dir_slots : first = index of the first key
 *            that maps to a bucket >= b under the monotone range map over [keys32[0],
 *            keys32[nkeys - 1]] (dir[dir_slots].first = nkeys); k0..k2 = the bucket's first three
 *            keys (a shorter bucket repeats its last key, an empty one holds the list's next key,
 *            or the last key when there is none behind it);
 * a row whose key is k0 / k1 / k2 has its group from that read, a key above k2 walks keys32 from
 * first + 3 (bisection inside the bucket when the keys cluster).  No parameter block, no failure
 * mode to read back.
 * nvt_keydir_build: dir (uint32[4 * (dir_slots + 1)], 16-byte aligned) from the ascending
 * duplicate-free key list.
 * nvt_keydir_lookup_image: nvt_flat_lookup_image's image / outputs / folds / offs / sizes /
 * miss_bits / unseen; keys int32 / int64 (list key = column key - key_offset), rows with a null
 * key take record `null_group` (-1: they miss).
 * nvt_image_build: records [records][stride_bytes] (stride <= 192) written WHOLE in one pass: up
 * to 4 operators' byte ranges, each evaluated exactly as nvt_jg_image / nvt_te_image evaluate it
 * (kind NVT_IMAGE_PART_JG: count / sum / sumsq / mn / mx / nvals / kinds / vals / dst_dtypes /
 * offs / ncols as in nvt_jg_image; NVT_IMAGE_PART_TE: tot_* / fold_* / kfold / p_smooth / y_mean
 * / out_dtype / offset as in nvt_te_image); a part fills its first `groups` records, every other
 * byte of the image is zero. */
#define NVT_IMAGE_PART_JG 0
#define NVT_IMAGE_PART_TE 1
typedef struct nvt_image_part {
  int32_t kind;
  int32_t nvals;               /* JG */
  int32_t ncols;               /* JG */
  int32_t kfold;               /* TE */
  int32_t out_dtype;           /* TE: NVT_F32 / NVT_F64 */
  uint32_t offset;             /* TE: byte offset of slot 0 inside the record */
  uint64_t groups;
  const int64_t *count;        /* JG */
  const double *const *sum;    /* JG: nvals pointers each (or NULL) */
  const double *const *sumsq;
  const double *const *mn;
  const double *const *mx;
  const int32_t *kinds;        /* JG: ncols entries each */
  const int32_t *vals;
  const int32_t *dst_dtypes;
  const uint32_t *offs;
  const int64_t *tot_count;    /* TE */
  const double *tot_sum;
  const int64_t *fold_count;
  const double *fold_sum;
  double p_smooth;
  double y_mean;
  const double *moments;       /* TE: NULL, or {count, sum} of the target on the device: the kernel
                                  takes y_mean = sum / count from there (the fit's mean need not
                                  have reached the host when the image is enqueued) */
} nvt_image_part;
int nvt_keydir_build(const int32_t *keys32, uint64_t n, uint64_t dir_slots, uint32_t *dir, void *stream);
int nvt_keydir_lookup_image(const void *keys, int dtype, const uint8_t *valid, uint64_t n,
                            const uint32_t *dir, uint64_t dir_slots, const int32_t *keys32, uint64_t nkeys,
                            int64_t key_offset, int64_t null_group, const void *image,
                            uint32_t stride_bytes, int ncols, void *const *outs, const uint8_t *const *folds, const uint32_t *offs,
                            const uint32_t *sizes, const uint64_t *miss_bits, uint64_t *unseen,
                            void *stream);
int nvt_image_build(const nvt_image_part *parts, int nparts, uint64_t records, void *image,
                    uint32_t stride_bytes, void *stream);

/* ---- parquet in: PLAIN / uncompressed column chunks of flat numeric columns -------------
 * (merlin.io.Dataset(engine="parquet") under Workflow.fit / transform:
 * tests/unit/workflow/test_cpu_workflow.py:67-81, bench/examples/dask-nvtabular-criteo-benchmark.py
 * :216-237; the reference's dataframe backend decodes the pages.)
 * nvt_pq_decode_chunk (HOST function, no GPU, thread-safe): chunk = the bytes of one column chunk
 * from its first data page on (DataPage v1 / v2, PLAIN values, definition levels in the RLE /
 * bit-packed hybrid, max_def_level 0 = REQUIRED or 1 = OPTIONAL).  Writes the rows' Arrow validity
 * bitmap (LSB first, row i = bit valid_bit_offset + i: consecutive row groups of a partition go
 * into ONE bitmap, by one thread; valid_out needs ceil((offset + rows) / 8) + 8 bytes) and the
 * pages' values -- non-null ones only -- behind each other into values_out.  *rows_out must come
 * out as expect_rows; *values_count = non-null rows.  NVT_EUNSUPPORTED: dictionary / compressed /
 * other encodings / nested columns (the caller reads the file another way).
 * nvt_expand_valid: out[i] = bit i of bitmap ? packed[valid rows in front of i] : 0 for n rows
 * of 4- or 8-byte values (bitmap 8-byte aligned, ceil(n / 64) * 8 bytes readable); ws:
 * nvt_expand_valid_ws_bytes(n). */
int nvt_pq_decode_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int type_size, int max_def_level,
                        uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                        uint8_t *values_out, uint64_t values_cap_bytes, uint64_t *rows_out,
                        uint64_t *values_count);
/* nvt_pq_decode_chunk_codec (round 6): the same for what real files hold -- chunk = the bytes of the
 * column chunk from its FIRST page on (the dictionary page when there is one), codec = the chunk's
 * parquet CompressionCodec (0 UNCOMPRESSED, 1 SNAPPY: every page is one raw snappy block; v2 pages
 * keep their levels uncompressed), values PLAIN or dictionary indices (PLAIN_DICTIONARY /
 * RLE_DICTIONARY: RLE / bit-packed hybrid at width <= 32 behind a PLAIN dictionary page).  The
 * decoder writes packed PLAIN values exactly like nvt_pq_decode_chunk.  scratch (host memory the
 * decoder owns during the call: the uncompressed dictionary + one uncompressed page):
 * 2 * total_uncompressed_size of the chunk + 64 bytes always suffice; may be null for codec 0.
 * NVT_EUNSUPPORTED: other codecs (gzip, zstd, lz4, brotli) / encodings (DELTA_*, BYTE_STREAM_SPLIT). */
int nvt_pq_decode_chunk_codec(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int type_size,
                              int max_def_level, uint64_t expect_rows, uint8_t *valid_out,
                              uint64_t valid_bit_offset, uint8_t *values_out, uint64_t values_cap_bytes,
                              uint8_t *scratch, uint64_t scratch_bytes, uint64_t *rows_out,
                              uint64_t *values_count);
/* nvt_pq_decode_list_chunk (HOST function, thread-safe): one column chunk of a standard three-level
 * list column (max repetition level 1; max definition level max_def_level = O + 1 + E with O / E = 1
 * for an optional outer group / leaf, leaf_level = O + 1), pages and codecs as above.  The levels of
 * the chunk's expect_slots slots (the chunk's num_values) are APPENDED to the partition's staging
 * streams at slot `slot_offset`: repetition levels 1 bit per slot in rep_out, definition levels W bits
 * per slot in def_out (W = 1 for max_def_level 1, else 2), LSB first and continuous over pages, chunks
 * and row groups (one thread per column: chunks may share a word).  Both buffers hold
 * ceil(slot_cap * W' / 64) * 8 bytes (W' = 1 / W) and slot_offset + expect_slots <= slot_cap.  The
 * non-null leaves go packed behind each other into values_out, PLAIN or through the dictionary.
 * counts[4] = {slots, row starts (rep 0), leaf slots (def >= leaf_level), non-null leaves
 * (def == max_def_level)} of the chunk.  NVT_EINVAL: the first slot is no row start, slots !=
 * expect_slots, row starts != expect_rows, a level above its maximum, level runs or values that do
 * not fit their page.  NVT_EUNSUPPORTED: BIT_PACKED level streams, other codecs / value encodings. */
int nvt_pq_decode_list_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int type_size,
                             int leaf_level, int max_def_level, uint64_t expect_slots, uint64_t expect_rows,
                             uint8_t *rep_out, uint8_t *def_out, uint64_t slot_offset, uint64_t slot_cap,
                             uint8_t *values_out, uint64_t values_cap_bytes, uint8_t *scratch,
                             uint64_t scratch_bytes, uint64_t *counts);
/* ---- parquet in: string columns (flat BYTE_ARRAY annotated UTF8 / STRING) ----
 * A string column is not expanded on the host.  Per partition and column the decoder fills a STAGE:
 *   entries  an Arrow string table in the layout nvt_str_hash takes: offsets[entries_cap + 1] (int64,
 *            offsets[0] = 0) and chars[chars_cap] (chars_cap a multiple of 4; the bytes up to the
 *            4-byte boundary behind the last char are zeroed).  The values of a dictionary page are
 *            appended as they are, every value of a PLAIN data page as a fresh entry; nothing is
 *            deduplicated.
 *   runs     the run table: runs_cap records of 4 uint32 {start, kind | width << 8, a, b}, in value
 *            order, `start` the position of the run's first value among the column's non-null values
 *            of the partition.  A run ends where the next record starts; no run is empty; the record
 *            behind the last run is the closing one {total, NVT_PQ_RUN_END, 0, 0}.
 *              NVT_PQ_RUN_REPEAT    every value is entry a (an RLE run; bit width 0)
 *              NVT_PQ_RUN_PACKED    value k is entry a + (the width-bit number at bit k * width,
 *                                   LSB first, of the bytes from packed[4 * b] on); width 1 .. 32,
 *                                   a = the chunk's first dictionary entry
 *              NVT_PQ_RUN_SEQUENCE  value k is entry a + k (the values of PLAIN pages)
 *            A repeat run whose index lies outside its dictionary has a = 0xFFFFFFFF.
 *   packed   packed_cap bytes: the bytes of the bit-packed runs as the file holds them, each run's on
 *            a 4-byte boundary and clipped to the values its page still owes, 8 zero bytes behind
 *            the last.
 * entries / nchars / nruns (without the closing record) / npacked / nvalues say how far the stage is
 * filled; zero them for a new partition.
 *
 * nvt_pq_decode_str_chunk (HOST function, no GPU call, thread-safe; one thread per stage): appends
 * one column chunk (pages, codecs and definition levels as nvt_pq_decode_chunk_codec; values PLAIN
 * or dictionary indices, also mixed in one chunk) to `stage` and writes the rows' validity bits at
 * valid_bit_offset.  scratch: the largest page uncompressed (total_uncompressed_size of the chunk
 * suffices); may be null for codec 0.  The stage advances on NVT_OK only.  NVT_PQ_STR_GROW: a
 * staging buffer is too small -- need[4] = {entries, chars, runs, packed} holds, for that buffer,
 * a capacity that reaches further (0 for the others); the caller enlarges it, keeps the filled part
 * and calls again with the same chunk.  NVT_EINVAL: a length prefix or run past its page, a
 * dictionary count that does not fit its page, a bit width above 32, row counts that do not add up.
 * NVT_EUNSUPPORTED: other codecs / encodings / page kinds, 2^31 - 1 or more entries or values.
 *
 * nvt_pq_expand_runs (device): out[q] = the entry id of non-null value q for q < nvalues, from the
 * run table (device memory, 16-byte aligned, nruns records + the closing one) and the packed bytes
 * (device memory, 4-byte aligned, packed_bytes readable, 8 of them behind the last run).  An id
 * outside [0, entries) is written as -1 and counted: *bad += their number (a device word the caller
 * zeroes; one atomic per wave).  Every read is bounded by nruns / packed_bytes whatever the table
 * says.  closing: the closing record in HOST memory; NVT_EINVAL before any launch when it does not
 * say nvalues, or on a null pointer.  nvalues == 0: NVT_OK without a launch.  nvalues < 2^32 - 2048.
 * No read-back; works on `stream` only. */
#define NVT_PQ_RUN_REPEAT 0u
#define NVT_PQ_RUN_PACKED 1u
#define NVT_PQ_RUN_SEQUENCE 2u
#define NVT_PQ_RUN_END 3u
#define NVT_PQ_STR_GROW 1
typedef struct nvt_pq_str_stage {
  int64_t *offsets;
  uint8_t *chars;
  uint32_t *runs;
  uint8_t *packed;
  uint64_t entries_cap, chars_cap, runs_cap, packed_cap;
  uint64_t entries, nchars, nruns, npacked, nvalues;
} nvt_pq_str_stage;
int nvt_pq_decode_str_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int max_def_level,
                            uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                            nvt_pq_str_stage *stage, uint8_t *scratch, uint64_t scratch_bytes, uint64_t *need);
int nvt_pq_expand_runs(const uint32_t *runs, uint64_t nruns, const uint32_t *closing, const uint8_t *packed,
                       uint64_t packed_bytes, uint64_t entries, uint64_t nvalues, int32_t *out, uint32_t *bad,
                       void *stream);
int nvt_expand_valid_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_expand_valid(const void *packed, int type_size, const uint8_t *bitmap, uint64_t n, void *out,
                     void *ws, void *stream);

/* ---- parquet, flat int8 / int16 / bool columns ("Narrow and bool columns in the parquet
 * path"; the reference's label idiom (col > 3).astype("int8"), ops/reduce_dtype_size.py) ----
 * In the file an int8 / int16 column is an INT32 column (annotated INTEGER{8 | 16, signed}) of
 * sign-extended values and a BOOLEAN page holds its non-null values one per bit, LSB first.
 *
 * nvt_pq_decode_bool_chunk (HOST function, no GPU, thread-safe): one column chunk of a flat BOOLEAN
 * column -- DataPage v1 / v2, codec 0 / 1, definition levels as nvt_pq_decode_chunk_codec, values
 * PLAIN (bit-packed) or RLE (u32 length | RLE / bit-packed hybrid at bit width 1).  Writes the rows'
 * validity bits at valid_bit_offset like its neighbours and the non-null values ONE BYTE EACH (0 / 1)
 * into values_out (values_cap bytes).  scratch: the largest page uncompressed; may be null for codec
 * 0.  NVT_EINVAL: any length that does not fit what remains of its page or chunk, a run that claims
 * more values than its page still owes, row counts that do not add up; nothing outside
 * [chunk, chunk + chunk_bytes) is read.  NVT_EUNSUPPORTED: other codecs / encodings / page kinds.
 *
 * nvt_expand_narrow (device): out[i] = bit i of bitmap ? (dst type) packed[valid rows in front of i]
 * : 0 for n < 2^32 rows; src_size -> dst_size is 4 -> 1, 4 -> 2 (int32 staging values to int8 /
 * int16: a value outside the target range keeps its low bits) or 1 -> 1 (bool bytes).  bitmap NULL:
 * the pure narrowing copy out[i] = (dst type) packed[i] (ws may be NULL).  bitmap 8-byte aligned,
 * ceil(n / 64) * 8 bytes readable; ws: nvt_expand_valid_ws_bytes(n).
 *
 * nvt_pq_widen_i32_many (device): dst[i] = (int32) src[i] for every descriptor, one launch per 32
 * of them.  src (NVT_I8 / NVT_I16) is aligned to its element size only, dst to 4 bytes; nothing
 * outside [src, src + n) is read; n == 0 launches nothing.
 *
 * nvt_pq_bool_pack (device): the non-null values `vals` of a chunk (one byte each, != 0 is true) cut
 * into pages at page_start[npages + 1] (device, int64, value positions): page p's values become bits,
 * LSB first, from out + byte_at[p] (device, int64[npages + 1]; byte_at[p + 1] - byte_at[p] >=
 * ceil(values of p / 8)); exactly ceil(values / 8) bytes per page are written, the tail bits of the
 * last one 0.  npages == 0 launches nothing.  No read-back; works on `stream` only. */
typedef struct nvt_pq_widen_col {
  const void *src;
  int32_t *dst;
  uint64_t n;
  int32_t src_dtype; /* NVT_I8 / NVT_I16 */
  int32_t reserved;
} nvt_pq_widen_col;
int nvt_pq_decode_bool_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int max_def_level,
                             uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                             uint8_t *values_out, uint64_t values_cap, uint8_t *scratch, uint64_t scratch_bytes,
                             uint64_t *rows_out, uint64_t *values_count);
int nvt_expand_narrow(const void *packed, int src_size, int dst_size, const uint8_t *bitmap, uint64_t n, void *out,
                      void *ws, void *stream);
int nvt_pq_widen_i32_many(const nvt_pq_widen_col *cols, int ncols, void *stream);
int nvt_pq_bool_pack(const uint8_t *vals, const int64_t *page_start, const int64_t *byte_at, uint64_t npages,
                     uint8_t *out, void *stream);

/* ---- batched entry points: ONE call per operator per partition -----------------------
 * The reference hands a whole dataframe to the backend per operator call
 * (`df[cols].fillna(...)`, `for col in columns: _encode(...)` -- categorify.py:477-537,
 * normalize.py:71-90, moments.py:64-77); the per-column functions above cost one host
 * round trip (ctypes + launch) per column per step, which made the 45 M-row Criteo step
 * host-bound on slow hosts.  These take an array of per-column descriptors (HOST memory,
 * plain pointers and sizes) and enqueue every launch from C++; where the columns are
 * independent streaming passes they run as ONE kernel launch (blockIdx.y = column).
 * Results are bit-identical to calling the per-column function on each descriptor. */
typedef struct nvt_moments_col {
  const void *x;            /* device column                                    */
  const uint8_t *valid;     /* bitmap or NULL                                   */
  uint64_t n;
  int32_t dtype, has_fill;
  double fill_val;
  double *out3;             /* device double[3], accumulated into               */
} nvt_moments_col;
/* partials: device scratch of ncols * nvt_moments_scratch_bytes() */
int nvt_moments_many(const nvt_moments_col *cols, int ncols, void *partials, void *stream);

typedef struct nvt_fillnorm_col {
  const void *x;
  const uint8_t *valid;
  uint64_t n;
  int32_t dtype, has_fill;
  double fill_val;
  int32_t do_norm, out_dtype;
  double shift, scale;
  void *out;
  uint8_t *filled;          /* optional                                         */
  const double *moments;    /* NULL, or the column's {count, sum, sum of squares} on the device
                               (nvt_moments_many's out3): shift = mean and scale = std (0 when it
                               is not > 0) are then finished by the kernel exactly as the host
                               finishes them (moments.py:89-116) -- a fit whose moments have not
                               reached the host yet does not hold the transform back */
} nvt_fillnorm_col;
int nvt_fill_normalize_many(const nvt_fillnorm_col *cols, int ncols, void *stream);

/* one column of Categorify.fit's groupby-size; fields as the arguments of nvt_dense_count_* */
typedef struct nvt_count_col {
  const void *keys;
  const uint8_t *valid;
  const int64_t *weights;
  uint64_t n;
  int32_t key_bytes, path;
  void *ws;                 /* nvt_dense_count_ws_bytes().  Columns of a call that SHARE a workspace
                               run in order; columns given different workspaces (at most 3
                               distinct pointers per call) run concurrently on internal streams
                               forked from / joined into `stream`                          */
  void *out_keys;
  int64_t *out_counts;
  uint64_t out_capacity;
  uint64_t *state;          /* device uint64[NVT_STATE_WORDS]                   */
  int32_t *hot_image;       /* path | NVT_PATH_HOT: device int32[NVT_HOT_IMAGE_WORDS] of this column's
                               own (workspaces may be shared): the hot-key samples of all columns
                               are then taken by ONE launch ahead of the pipelines.  NULL: sampled
                               inside the column's pipeline, image kept in ws                 */
  void *range_table;        /* NVT_PATH_RANGE, optional: nvt_range_table_bytes(buckets) bytes.  The
                               per-bucket count tables are written out as they are: an encode table
                               addressed by the same monotone map, slot = {key, position in the
                               key-ordered output list}.  nvt_vocab_finalize_many turns the positions
                               into labels (nvt_vocab_col.range_table), nvt_encode_many probes it
                               (nvt_encode_col.range_aux).                                        */
  uint32_t *out_slots;      /* optional, read only together with range_table: uint32[out_capacity].
                               out_slots[i] = the slot of range_table that holds entry i of the
                               output list (0xFFFFFFFF for the smallest int32, which owns none).
                               Passed on as nvt_vocab_col.src_slots, it lets the ordering write the
                               labels straight into the table instead of streaming over all of it.
                               Unspecified after an overflow (state[NVT_ST_OVERFLOW] != 0).        */
} nvt_count_col;
/* bytes of the range table of a column counted with 2^nb_log2 buckets */
int nvt_range_table_bytes(int nb_log2, uint64_t *bytes);
int nvt_dense_count_many(const nvt_count_col *cols, int ncols, void *stream);

/* one vocabulary of Categorify.fit_end: sort (count desc, key asc) in place, then build its
 * encode table (skipped when table == NULL: LDS-resident vocabularies).  Independent
 * vocabularies are spread over a few internal HIP streams forked from / joined into
 * `stream` (the one-workgroup kernels of small vocabularies run beside the radix passes of
 * large ones); all small vocabularies of a call are sorted by ONE launch. */
typedef struct nvt_vocab_col {
  void *keys;               /* device int32/int64[n], sorted in place            */
  int64_t *counts;          /* device int64[n], permuted with the keys           */
  uint64_t n;
  int64_t max_count;        /* upper bound on counts (<= 0: unknown)             */
  int32_t key_bytes, unique_keys;
  void *sort_tmp;           /* nvt_vocab_sort_tmp_bytes(); per column.  Optional for int32 keys with
                             * 2 <= n <= 16384 and 0 < max_count < 2^32 (8 n bytes are used when it
                             * is there: above 2048 entries the list is then sorted by many
                             * workgroups instead of one)                                  */
  int64_t first_label;
  void *table;              /* encode table to build, or NULL                    */
  uint64_t capacity;
  int64_t *sentinel_label;
  void *ready_event;        /* optional nvt_event: recorded behind this vocabulary's last
                             * kernel INSTEAD of joining its stream into `stream`; whoever
                             * reads the vocabulary / table next waits on it
                             * (nvt_encode_col.wait_event, nvt_stream_wait_event)        */
  /* KEY-SORTED source list (range path of nvt_dense_count_many; int32 keys): when src_keys is
   * set, (keys, counts) are OUTPUT arrays of n entries -- the list is ordered out of place by
   * ONE stable counting pass on min(count, 255), the n_big entries with count >= 255 are sorted
   * on their own, and the encode table is filled by the same pass.  sort_tmp then needs
   * nvt_vocab_order_tmp_bytes(n, n_big) bytes. */
  const void *src_keys;
  const int64_t *src_counts;
  const uint32_t *cls_hist;  /* device uint32[256]: entries per min(count, 255)           */
  uint64_t n_big;            /* entries with count >= 255 (state[NVT_ST_BIG])             */
  /* with a key-sorted source: `table` is the RANGE TABLE the counting pass dumped
   * (nvt_count_col.range_table; slots {key, position in the source list}): its positions are
   * replaced by labels in one streaming pass -- no clear, no random inserts.  range_aux = the
   * column's aux block (nvt_count_col.hot_image) that holds the map parameters. */
  const int32_t *range_aux;
  int32_t range_nb_log2;
  /* flat_slots > 0 (with a key-sorted source, int32 keys): `table` is BUILT here as a flat
   * range table of flat_slots home slots (any count from 64 to 2^32 - 1; + n + 64 tail slots:
   * capacity = the sum) straight
   * from the sorted keys by a prefix maximum -- no random inserts; range_aux = a device
   * int32[NVT_FLAT_AUX_WORDS] block that RECEIVES the map parameters (pass it to nvt_encode_col)
   * and, in word NVT_FLAT_AUX_MAXDISP, the longest displacement of an entry from its home slot
   * (large: the keys cluster in their range, build an ordinary table with nvt_encode_build_*) */
  uint64_t flat_slots;
  /* with a key-sorted source: the 0-based position of every source entry in the vocabulary order
   * (int32[n]; multi-GPU fits label their shards on the owners, nvt_vocab_label_shard).  cls_hist
   * / n_big are then ignored: (keys, counts) are filled by one scatter and the table (flat, or
   * hashed when flat_slots == 0) is built from the labels -- no ordering pass.  sort_tmp:
   * nvt_vocab_order_tmp_bytes(n, 0) bytes. */
  const int32_t *src_labels;
  /* optional (int32 keys, n > NVT_ENCODE_RESIDENT_I32, unique keys): NVT_ENCODE_HEAD_BYTES bytes that
   * receive the LDS head of the cache-mode encode -- the first keys of the ORDERED vocabulary laid
   * out as the launch's workgroups hold them -- built once here, on the stream that orders the
   * vocabulary, instead of by every workgroup of every encode launch (nvt_encode_col.head_image). */
  void *head_image;
  /* optional, with a dumped range table (flat_slots == 0) and no src_labels: uint32[n], the slot of
   * `table` that holds each source entry (nvt_count_col.out_slots of the same counting pass;
   * 0xFFFFFFFF: none).  The ordering pass then stores every label into its slot and the streaming
   * pass over the whole table is not run.  NULL (a list that was merged or otherwise no longer
   * matches the dump entry for entry): the streaming pass. */
  const uint32_t *src_slots;
} nvt_vocab_col;
#define NVT_ENCODE_HEAD_BYTES (12288 * 12 + 64)
#define NVT_FLAT_AUX_WORDS (NVT_RANGE_AUX_LO + 16)
#define NVT_FLAT_AUX_MAXDISP (NVT_RANGE_AUX_LO + 8)
#define NVT_FLAT_AUX_NULLGROUP (NVT_RANGE_AUX_LO + 10)  /* nvt_flat_lookup*: 1 + the group of rows whose
                                                          key is null (0: none, such rows miss); set
                                                          by the caller after nvt_flat_index_build */
int nvt_vocab_order_tmp_bytes(uint64_t n, uint64_t n_big, uint64_t *bytes);
/* One rank's SHARD (a key range) of a key-sorted (key, count) list that is ordered "count
 * descending, key ascending" as a whole (categorify.py:1300,1316): label_of[i] = the 0-based
 * position of entry i in the order of the UNION for entries with count < 255, -1 for the others,
 * which are written out compacted in key order (big_keys / big_counts / big_src = their positions
 * in the shard; the caller gathers all ranks' and sorts them exactly).  class_base_diff
 * uint32[256], indexed by class c = min(count, 255): with base(c) = (entries of the union in
 * classes 255 .. c + 1) + (entries of class c on the ranks in front of this one), the value at c is
 * base(c - 1) - base(c) modulo 2^32 for 2 <= c <= 254, base(254) at 255, anything at 1 (the kernel's
 * exclusive prefix over the classes 255, 254, ... reproduces the bases).  tmp:
 * nvt_vocab_order_tmp_bytes(n, 0) bytes; big_* hold as many entries as the shard has with count >=
 * 255. */
int nvt_vocab_label_shard(const int32_t *keys, const int64_t *counts, uint64_t n, const uint32_t *class_base_diff,
                          void *tmp, int32_t *label_of, int32_t *big_keys, int64_t *big_counts,
                          int32_t *big_src, void *stream);
/* hist[c] = entries with min(counts[i], 255) == c, for a key-sorted list that did not come from
 * the range path (multi-GPU: gathered owner shards); hist[255] = n_big */
int nvt_class_hist(const int64_t *counts, uint64_t n, uint32_t *hist, void *stream);
int nvt_vocab_finalize_many(const nvt_vocab_col *cols, int ncols, void *stream);

/* one column of Categorify.transform; fields as the arguments of nvt_encode_* */
typedef struct nvt_encode_col {
  const void *keys;
  const uint8_t *valid;
  uint64_t n;
  const void *table;
  uint64_t capacity;
  const int64_t *sentinel_label;
  int64_t null_label, oov_label;
  uint32_t num_buckets;
  int32_t key_bytes, out_bytes;
  void *out;
  const void *vocab_keys;
  uint64_t n_vocab;
  int64_t first_label;
  void *wait_event;         /* optional nvt_event the launch waits for (stream-side)     */
  const int32_t *range_aux; /* `table` is a range table (nvt_count_col.range_table): probed by
                               the monotone map whose parameters sit in this aux block      */
  const void *head_image;   /* optional: the head image nvt_vocab_finalize_many built for this
                               vocabulary (valid once wait_event has fired)                 */
} nvt_encode_col;
/* The columns are independent (own output, own table): they are spread round-robin over
 * NVT_ENCODE_STREAMS (environment, default 3, 1 = none; read at every call) internal streams forked
 * from / joined into `stream` -- everything the call enqueues is ordered behind what `stream` held
 * and in front of what the caller enqueues next. */
int nvt_encode_many(const nvt_encode_col *cols, int ncols, void *stream);

/* Stream-ordered hand-off between nvt_vocab_finalize_many (which orders the large
 * vocabularies on internal streams) and the calls that consume a vocabulary: with a
 * ready_event per vocabulary the caller's stream is NOT blocked until every sort and table
 * build has finished -- FillMissing + Normalize.transform and the encodes of the small
 * vocabularies run underneath the radix passes of the large ones.  An nvt_event is an
 * opaque handle (a hipEvent_t without timing). */
int nvt_event_create(void **event);
void nvt_event_destroy(void *event);
int nvt_stream_wait_event(void *stream, void *event);

/* ---- device -> host read-back of a few words without a blocking runtime wait ----------
 * The fit needs two tiny read-backs per partition (the counting kernels' state words, the
 * moments).  A hipMemcpy + stream synchronise blocks the host thread in an interrupt-driven
 * wait; on some hosts that wake-up was observed to cost ~10 ms per wait (a 20 ms step became
 * 39 ms with identical kernel times).  A mailbox is coherent, device-mapped pinned host
 * memory: nvt_mailbox_post enqueues ONE small kernel that copies `bytes` (multiple of 8) from
 * device memory into the mailbox and then stores a sequence number with system scope;
 * nvt_mailbox_wait spins on that word on the host (no interrupt, no runtime call) and returns
 * NVT_OK when it reaches `seq` (NVT_EHIP after timeout_s seconds).  nvt_mailbox_data is the
 * host pointer of the payload. */
typedef struct nvt_mailbox nvt_mailbox;
int nvt_mailbox_create(uint64_t bytes, nvt_mailbox **out);
void nvt_mailbox_destroy(nvt_mailbox *mb);
void *nvt_mailbox_data(nvt_mailbox *mb);
uint64_t nvt_mailbox_capacity(nvt_mailbox *mb);
int nvt_mailbox_post(nvt_mailbox *mb, const void *src_device, uint64_t bytes, void *stream,
                     uint64_t *seq_out);
int nvt_mailbox_wait(nvt_mailbox *mb, uint64_t seq, double timeout_s);

/* ---- instrumentation ------------------------------------------------------------------
 * HIP-event timing of every kernel family, recorded on the stream the kernels are launched
 * on.  nvt_prof_begin() arms it; nvt_prof_report() synchronises the device, disarms it and
 * writes a JSON object {"kernels": {name: [total_ms, launches, algorithmic_bytes]},
 * "busy_ms": union of the recorded intervals, "span_ms": first start .. last stop} into buf
 * (*needed = bytes required).  Off = zero cost.  Every scope is also a roctx range, and
 * nvt_range_push/pop let the host layer open ranges named after the reference's @annotate
 * strings (categorify.py:345,477,955,1054,1073,1149). */
int nvt_prof_begin(void);
int nvt_prof_report(char *buf, uint64_t cap, uint64_t *needed);
void nvt_range_push(const char *name);
void nvt_range_pop(void);

/* ---- string categoricals: Arrow string buffers -> 64-bit surrogate keys ----
 * A string column is keyed by pandas.util.hash_array(v, categorize=False) viewed as int64, the
 * surrogate the host path (nvtabular_amd/strings.py) computes; these entries compute the same
 * bits from the column's Arrow buffers.  Restated from pandas 2.3.3:
 *   pandas/core/util/hashing.py:44        _default_hash_key "0123456789123456"  -> nvt_str_hash
 *   pandas/core/util/hashing.py:326       hash_object_array (pandas/_libs/hashing.pyx):
 *                                         SipHash-2-4 of the UTF-8 bytes        -> nvt_str_hash
 *   pandas/core/util/hashing.py:333-338   _hash_ndarray's final mixing step     -> nvt_str_hash
 *   pandas/core/util/hashing.py:318-323   factorize + hash of the categories    -> nvt_str_dedup,
 *                                         (the {surrogate -> string} table)        nvt_str_gather
 * `offsets` holds n + 1 int32 (Arrow string) or int64 (large_string) entries, offset_bytes = 4
 * or 8; offsets[0] may be non-zero (a sliced array): `chars` points at the byte offsets[0]
 * names, must be 4-byte aligned and readable up to the 4-byte boundary after the last byte.
 * Null rows (valid bit 0) get the key 0.
 *
 * nvt_str_hash: out[i] = surrogate of string i (one lane per string, aligned 4-byte loads).
 * nvt_str_take_keys: dictionary-encoded columns: out[i] = dict_keys[indices[i]] (0 for a null
 *   row, or an index outside [0, n_dict)); index_bytes = 4 or 8.
 * nvt_str_dedup: the first row of every distinct key among the valid rows, in row order:
 *   out_keys[j] = its key, out_strs[j] = its string (index[row] when `index` is given -- the
 *   dictionary entry of a dictionary-encoded row --, else the row itself); out_counts[0] =
 *   distinct keys, out_counts[1] = valid rows whose bytes differ from those of the first row
 *   of their key (64-bit collisions).  Strings come from offsets / chars (n_strings entries).
 *   out_keys / out_strs hold n entries.  ws: nvt_str_dedup_ws_bytes(n), 256-byte aligned (an
 *   open-addressing table claimed by 64-bit CAS; the key INT64_MIN has a slot of its own).
 * nvt_str_gather: strings strs[0 .. m) -> out_offsets[m + 1] (int64, from 0) + out_chars
 *   (out_capacity bytes, < 4 GiB; a string that would end past it is not copied, and
 *   out_offsets[m] then exceeds out_capacity).  ws: nvt_str_gather_ws_bytes(m), 256-byte
 *   aligned. */
int nvt_str_hash(const void *offsets, int offset_bytes, const uint8_t *chars, const uint8_t *valid,
                 uint64_t n, int64_t *out, void *stream);
int nvt_str_take_keys(const int64_t *dict_keys, uint64_t n_dict, const void *indices, int index_bytes,
                      const uint8_t *valid, uint64_t n, int64_t *out, void *stream);
int nvt_str_dedup_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_str_dedup(const int64_t *keys, const uint8_t *valid, uint64_t n, const void *index, int index_bytes,
                  const void *offsets, int offset_bytes, const uint8_t *chars, uint64_t n_strings, void *ws,
                  uint64_t ws_bytes, int64_t *out_keys, int64_t *out_strs, uint64_t *out_counts,
                  void *stream);
int nvt_str_gather_ws_bytes(uint64_t m, uint64_t *bytes);
int nvt_str_gather(const int64_t *strs, uint64_t m, const void *offsets, int offset_bytes,
                   const uint8_t *chars, uint64_t n_strings, void *ws, uint64_t ws_bytes,
                   int64_t *out_offsets, uint8_t *out_chars, uint64_t out_capacity, void *stream);

/* ---- row compaction: ops.Filter / ops.Dropna ----
 * Dropping rows is three steps over a PLAN, a workspace of nvt_compact_ws_bytes(n) bytes, 256-byte
 * aligned, that covers n rows in tiles of 2048 (n < 2^32 - 2048):
 *   1. a keep mask: a bitmap over the tiles plus a uint32 count of kept rows per tile, written in
 *      one launch by nvt_compact_keep_mask (row i is kept iff mask[i] != 0; bool / uint8, n bytes),
 *      nvt_compact_keep_dropna (row i is kept iff every descriptor column is valid there: bitmap
 *      bit 1, and not NaN for NVT_F32 / NVT_F64; ONE launch per 64 descriptors, ANDed together)
 *      or nvt_compact_list_keep (the leaves of a list column: a leaf is kept iff its row is kept
 *      in row_plan; offsets are the n + 1 int64 row offsets, offsets[0] possibly non-zero);
 *   2. nvt_compact_plan: the exclusive scan of the tile counts (nvt_scan.hpp, no inter-workgroup
 *      waits); *out_m (device uint64, optional) = m, the kept rows;
 *   3. nvt_compact_many: ONE launch per 64 descriptors (blockIdx.y = column) moves the kept rows
 *      of every column, in row order, to [0, m) of its output: `width` = 1, 4 or 8 bytes per
 *      value (bool, uint8, int32, int64, float32, float64), each descriptor with its own plan and
 *      n (the leaves of a list column go with their leaf plan).  src_valid / dst_valid (both or
 *      neither): the validity bitmap compacted bit-exactly; the call zeroes dst_valid first, over
 *      ceil(m / 64) * 8 bytes (the padding of every bitmap here), so bits past m are 0.
 * nvt_compact_list_offsets: the m + 1 new offsets (from 0) of a list column whose leaves were
 *   compacted with leaf_plan (n_leaves = 0: every list is empty and leaf_plan may be NULL).
 * Every entry is stream-ordered and does not synchronise; n = 0 is a no-op.  Nothing is read back:
 * the caller sizes the outputs from *out_m.
 *
 * nvt_compact_keep_terms (Dataset(filters=...)) is a keep-mask producer like the two of step 1, in
 * ONE launch and without global atomics: it writes the plan's mask words (bits past n zero) and the
 * tile counts from a predicate in disjunctive normal form.  `terms` are 1 to NVT_FILTER_MAX_TERMS
 * comparisons sorted by `conj` (non-decreasing, from 0); a row is kept iff in some conjunction
 * every term holds.  A term names one of the 1 to NVT_FILTER_MAX_COLS columns (`col`), whose
 * dtype is NVT_F32 .. NVT_I16 (a bool column is NVT_U8): a float column is widened to double and
 * compared with value.f, an integer column to int64 and compared with value.i (string surrogates
 * and datetime counts are int64 columns).  NVT_FILTER_IN / NVT_FILTER_NOT_IN bisect the run
 * sets[set_off, set_off + set_len) of 8-byte words (int64, or double bit patterns for a float
 * column), ascending and distinct, -0.0 stored as 0.0; set_len = 0 is legal (`in` keeps nothing).
 * A null (bitmap bit 0) fails every term but NVT_FILTER_NOT_IN, which it passes; a NaN fails
 * every comparison but NVT_FILTER_NE and is in no set; -0.0 == 0.0.  Adjacent terms on one column
 * share the load of its value.  Refused with NVT_EINVAL before the launch: null descriptors, ncols /
 * nterms out of range, a dtype, op or col out of range, an x that is null or not aligned to its
 * dtype, terms not sorted by conj, a set run past set_words, n >= 2^32 - 2048, a null, misaligned
 * or short workspace. */
#define NVT_COMPACT_MAX_COLS 64
#define NVT_FILTER_MAX_COLS 16
#define NVT_FILTER_MAX_TERMS 64
#define NVT_FILTER_EQ 0
#define NVT_FILTER_NE 1
#define NVT_FILTER_LT 2
#define NVT_FILTER_LE 3
#define NVT_FILTER_GT 4
#define NVT_FILTER_GE 5
#define NVT_FILTER_IN 6
#define NVT_FILTER_NOT_IN 7
typedef struct nvt_filter_col {
  const void *x;            /* n values, aligned to their width                 */
  const uint8_t *valid;     /* bitmap or NULL                                   */
  int32_t dtype;            /* NVT_F32 .. NVT_I16                               */
  int32_t reserved;
} nvt_filter_col;
typedef struct nvt_filter_term {
  int32_t col;              /* index into the column descriptors                */
  int32_t op;               /* NVT_FILTER_EQ .. NVT_FILTER_NOT_IN               */
  int32_t conj;             /* the conjunction this term belongs to             */
  int32_t set_len;          /* IN / NOT_IN: words of the run                    */
  uint64_t set_off;         /* IN / NOT_IN: first word of the run in `sets`     */
  union {
    int64_t i;              /* the constant of an integer column                */
    double f;               /* the constant of a float column                   */
  } value;
} nvt_filter_term;
typedef struct nvt_dropna_col {
  const void *x;            /* values (read for NVT_F32 / NVT_F64 only)         */
  const uint8_t *valid;     /* bitmap or NULL                                   */
  int32_t dtype;            /* NVT_F32 .. NVT_U8                                */
  int32_t reserved;
} nvt_dropna_col;
typedef struct nvt_compact_col {
  const void *src;          /* n values                                         */
  void *dst;                /* m values                                         */
  const uint8_t *src_valid; /* bitmap or NULL                                   */
  uint8_t *dst_valid;       /* bitmap of ceil(m / 64) * 8 bytes, 4-byte aligned, or NULL */
  const void *plan;         /* the plan of these n rows                          */
  uint64_t n;
  int32_t width;            /* bytes per value: 1, 4 or 8                       */
  int32_t reserved;
} nvt_compact_col;
int nvt_compact_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_compact_keep_mask(const uint8_t *mask, uint64_t n, void *ws, uint64_t ws_bytes, void *stream);
int nvt_compact_keep_dropna(const nvt_dropna_col *cols, int ncols, uint64_t n, void *ws, uint64_t ws_bytes,
                            void *stream);
int nvt_compact_keep_terms(const nvt_filter_col *cols, int ncols, const nvt_filter_term *terms, int nterms,
                           const void *sets, uint64_t set_words, uint64_t n, void *ws, uint64_t ws_bytes,
                           void *stream);
int nvt_compact_list_keep(const int64_t *offsets, uint64_t n, const void *row_plan, uint64_t n_leaves,
                          void *leaf_ws, uint64_t leaf_ws_bytes, void *stream);
int nvt_compact_plan(uint64_t n, void *ws, uint64_t ws_bytes, uint64_t *out_m, void *stream);
int nvt_compact_many(const nvt_compact_col *cols, int ncols, void *stream);
int nvt_compact_list_offsets(const int64_t *offsets, uint64_t n, const void *row_plan, const void *leaf_plan,
                             uint64_t n_leaves, int64_t *out_offsets, void *stream);

/* ---- hash join against an external table: ops.JoinExternal ----
 * Keys: 1 to NVT_JOIN_MAX_KEYS components, each read in its native dtype (NVT_F32 .. NVT_U8) and
 * reduced to a canonical 64-bit word plus a null bit: NVT_JOIN_INT compares by value (integers of
 * any width, string surrogates), NVT_JOIN_FLOAT by double value (-0.0 == 0.0, integers converted
 * to double; a float column needs it).  A null component is a validity bit 0 or a NaN; nulls
 * match nulls, as in pandas' merge.
 * Build (once per external table):
 *   nvt_join_hash: per external row its tag (one component: the word; more: a fingerprint of the
 *     words and null bits), the null bits (bit k = component k) and, for 2+ components, the
 *     words [nkeys][n] that verify a fingerprint hit;
 *   the caller groups the rows by (tag, null bits) with a stable sort, permutes its payload
 *     columns into that order and picks `empty`, a tag no external key has;
 *   nvt_join_insert: the distinct tags into an open-addressing table of nvt_join_table_bytes
 *     (16-byte slots {tag, first, count}, load <= 0.5) with a 64-bit CAS; the caller fills the
 *     slots with {empty, 0, 0} first.  One component: the null group is not inserted, it is
 *     described by null_first / null_count of the index.
 * Probe (per partition, n left rows, no read-back):
 *   nvt_join_probe_gather: left join on unique keys; per left row the matched external row's
 *     value of every payload column, 0 and a cleared validity bit on a miss (dst_valid required:
 *     ceil(n / 64) * 8 bytes, 8-byte aligned, bits past n are 0); *unmatched (device, optional)
 *     += the rows without a match;
 *   nvt_join_probe: out_first[i] = grouped position of the first matching external row or -1,
 *     out_count[i] = k (inner) or max(1, k) (left), out_keep[i] = match, *out_total (device)
 *     += sum of out_count; every output but out_first is optional;
 *   nvt_join_offsets: exclusive scan of counts[0 .. n] in place (counts[n] = 0 on entry, the
 *     total below 2^32), with a workspace of nvt_join_scan_ws_bytes(n) bytes;
 *   nvt_join_expand: per output row j < m its left row (the last i with offsets[i] <= j) and its
 *     external position (first[i] + j - offsets[i], or -1 where first[i] < 0);
 *   nvt_join_gather: dst[j] = src[idx[j]] for every column (0 and a cleared validity bit where
 *     idx[j] < 0); dst_valid optional.
 * At most NVT_JOIN_MAX_COLS columns per launch; every entry is stream-ordered and n = 0 is a no-op. */
#define NVT_JOIN_MAX_KEYS 4
#define NVT_JOIN_MAX_COLS 16
#define NVT_JOIN_INT 0
#define NVT_JOIN_FLOAT 1
typedef struct nvt_join_key {
  const void *x;            /* n values                                         */
  const uint8_t *valid;     /* bitmap or NULL                                   */
  int32_t dtype;            /* NVT_F32 .. NVT_U8                                */
  int32_t mode;             /* NVT_JOIN_INT / NVT_JOIN_FLOAT                    */
} nvt_join_key;
typedef struct nvt_join_index {
  const void *slots;        /* capacity 16-byte slots, 16-byte aligned          */
  uint64_t capacity;        /* a power of two                                   */
  uint64_t empty;           /* tag of an empty slot                             */
  const uint64_t *words;    /* [nkeys][n_ext] grouped words (nkeys >= 2)        */
  const uint8_t *nulls;     /* [n_ext] grouped null bits (nkeys >= 2)           */
  uint64_t n_ext;
  uint64_t null_first;      /* one component: the null group's rows             */
  uint64_t null_count;
  int32_t nkeys;
  int32_t reserved;
} nvt_join_index;
typedef struct nvt_join_col {
  const void *src;          /* external (or left) values                        */
  const uint8_t *src_valid; /* bitmap or NULL                                   */
  void *dst;                /* one value per output row                         */
  uint8_t *dst_valid;       /* bitmap of ceil(rows / 64) * 8 bytes, or NULL     */
  int32_t width;            /* bytes per value: 1, 4 or 8                       */
  int32_t reserved;
} nvt_join_col;
int nvt_join_table_bytes(uint64_t n_groups, uint64_t *capacity, uint64_t *bytes);
int nvt_join_hash(const nvt_join_key *keys, int nkeys, uint64_t n, uint64_t *out_tag, uint64_t *out_words,
                  uint8_t *out_nulls, void *stream);
int nvt_join_insert(void *slots, uint64_t capacity, uint64_t empty, const uint64_t *tags, const uint32_t *first,
                    const uint32_t *count, uint64_t n_groups, void *stream);
int nvt_join_probe(const nvt_join_index *ix, const nvt_join_key *keys, int nkeys, uint64_t n, int inner,
                   int64_t *out_first, uint32_t *out_count, uint8_t *out_keep, uint64_t *out_total, void *stream);
int nvt_join_probe_gather(const nvt_join_index *ix, const nvt_join_key *keys, int nkeys, uint64_t n,
                          const nvt_join_col *cols, int ncols, uint64_t *unmatched, void *stream);
int nvt_join_scan_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_join_offsets(uint32_t *counts, uint64_t n, void *ws, uint64_t ws_bytes, void *stream);
int nvt_join_expand(const uint32_t *offsets, const int64_t *first, uint64_t n, uint64_t m, int64_t *out_left,
                    int64_t *out_ext, void *stream);
int nvt_join_gather(const int64_t *idx, uint64_t m, const nvt_join_col *cols, int ncols, void *stream);

/* ---- session features: ops.ListSlice / ops.ValueCount / ops.DifferenceLag ----
 * A list column is its leaves plus n + 1 int64 row offsets (offsets[0] possibly non-zero: leaf 0
 * of the values is the leaf offsets[0] names).  Everything here is 64 bits wide: a column may hold
 * more than 2^32 leaves.
 * ListSlice: output row i = row[start:end] of input row i as Python slices it (negative indices
 *   count from the row's end, both clamped to the row; `end` = INT64_MAX is "to the end").
 *   nvt_list_slice_offsets: the n + 1 new offsets (from 0) into out_offsets; out_offsets[n] is the
 *     number of output leaves (the caller reads it back to size the outputs).  ws:
 *     nvt_list_slice_ws_bytes(n) bytes, 8-byte aligned.  n > 0.
 *   nvt_list_slice_many: ONE launch per NVT_LIST_MAX_COLS descriptors moves the leaves of every
 *     column that shares `offsets`; the work is spread over the `total` OUTPUT leaves.  Ragged:
 *     out_offsets from nvt_list_slice_offsets, total = out_offsets[n], pad_width = 0.  Padded:
 *     out_offsets = NULL, every output row is pad_width leaves (total = n * pad_width, nothing is
 *     read back): the sliced row, then pad_bits (the low `width` bytes) in leaves that are valid.
 *     src_valid / dst_valid: the leaf bitmap carried bit-exactly, ceil(total / 64) * 8 bytes
 *     written in whole 64-bit words (bits past `total` are 0); a padded column may pass dst_valid
 *     without src_valid.  total = 0 is a no-op.
 * ValueCount: nvt_list_len_minmax folds min / max of offsets[i + 1] - offsets[i] over the n rows
 *   of every descriptor into acc[0] / acc[1] (device int64, the caller starts them at INT64_MAX /
 *   INT64_MIN and may accumulate several partitions); n = 0 adds nothing.
 * DifferenceLag: nvt_difference_lag_many writes, for every descriptor, out[i] = x[i] - x[j] with
 *   j = i - shift where 0 <= j < n, every partition column (0 to NVT_LAG_MAX_KEYS) is non-null and
 *   equal at i and j (floats by value, NaN is null) and x is valid at both; NaN elsewhere.  NVT_I32
 *   / NVT_I64 / NVT_U8 values are converted to double before the subtraction and the difference is
 *   rounded to float; NVT_F64 subtracts in double, NVT_F32 in float (what pandas computes).  ONE
 *   launch per NVT_LIST_MAX_COLS descriptors.
 * Every entry is stream-ordered and does not synchronise. */
#define NVT_LIST_MAX_COLS 32
#define NVT_LAG_MAX_KEYS 4
typedef struct nvt_list_col {
  const void *src;          /* input leaves                                     */
  void *dst;                /* `total` output leaves                            */
  const uint8_t *src_valid; /* leaf bitmap or NULL                              */
  uint8_t *dst_valid;       /* ceil(total / 64) * 8 bytes, 8-byte aligned, or NULL */
  uint64_t pad_bits;        /* the pad value's bits (padded mode)               */
  int32_t width;            /* bytes per leaf: 1, 4 or 8                        */
  int32_t reserved;
} nvt_list_col;
typedef struct nvt_list_len_col {
  const int64_t *offsets;   /* n + 1 row offsets                                */
  uint64_t n;
  int64_t *acc;             /* device {min, max}                                */
} nvt_list_len_col;
typedef struct nvt_lag_key {
  const void *x;            /* n values of a partition column                   */
  const uint8_t *valid;     /* bitmap or NULL                                   */
  int32_t dtype;            /* NVT_F32 .. NVT_U8                                */
  int32_t reserved;
} nvt_lag_key;
typedef struct nvt_lag_col {
  const void *x;            /* n values                                         */
  const uint8_t *valid;     /* bitmap or NULL                                   */
  float *out;               /* n differences                                    */
  int64_t shift;
  int32_t dtype;            /* NVT_F32 .. NVT_U8                                */
  int32_t reserved;
} nvt_lag_col;
int nvt_list_slice_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_list_slice_offsets(const int64_t *offsets, uint64_t n, int64_t start, int64_t end, int64_t *out_offsets,
                           void *ws, uint64_t ws_bytes, void *stream);
int nvt_list_slice_many(const nvt_list_col *cols, int ncols, const int64_t *offsets, uint64_t n, int64_t start,
                        int64_t end, const int64_t *out_offsets, uint64_t total, uint64_t pad_width,
                        void *stream);
int nvt_list_len_minmax(const nvt_list_len_col *cols, int ncols, void *stream);
int nvt_difference_lag_many(const nvt_lag_key *keys, int nkeys, const nvt_lag_col *cols, int ncols, uint64_t n,
                            void *stream);

/* ---- parquet list columns: repetition / definition level streams (Dataset.to_parquet) ----
 * A list column is written as the standard three-level list (max repetition level 1, max
 * definition level 3).  There are no null lists, so a row of L leaves occupies max(L, 1) SLOTS: an
 * empty row is one slot (rep 0, def 1), leaf i of a row has rep 0 (first leaf of its row) or 1 and
 * def 3 (valid) or 2 (null).  `offsets` points at the n + 1 offsets of the rows to write (any row
 * range of a column); n > 0.
 * nvt_pqlist_plan: slot_start[r] (n + 1 words) = the exclusive prefix sum of max(len_r, 1), and
 *   the page table.  Nominal page p starts at the first row r with slot_start[r] >= p * page_slots;
 *   a page that gets no row is dropped, so a page is never cut inside a row and may exceed
 *   page_slots by less than one row.  table: NVT_PQLIST_HEADER_WORDS + max_pages *
 *   NVT_PQLIST_PAGE_WORDS uint64:
 *     header {pages, slots, rep bytes, def bytes, pack tiles, offsets[0] - origin[0],
 *             offsets[n] - origin[0], overflow}    (origin: the column's first offset; the two
 *             differences are the range of the rows' leaves in the column's value buffer)
 *     page   {first row, rows, first slot, slots, rep offset, def offset, first pack tile, leaves}
 *   A page's repetition levels are ceil(slots / 8) bytes at `rep offset` of the rep buffer (regions
 *   are padded to 8 bytes), its definition levels 2 * ceil(slots / 8) bytes at `def offset` of a
 *   def buffer (padded to 16): the payload of ONE bit-packed run of the RLE / bit-packing hybrid at
 *   bit width 1 / 2, LSB first, the bits behind the last slot 0.  `overflow` is 1 -- and the pack
 *   writes nothing -- when there are more than max_pages pages or more than rep_cap / def_cap
 *   bytes.  ws: nvt_pqlist_ws_bytes(n) bytes, 8-byte aligned.
 * nvt_pqlist_pack_many: ONE launch per NVT_PQLIST_MAX_COLS descriptors writes rep_out (once) and
 *   every descriptor's def_out, and counts its non-null leaves per page into nonnull[max_pages]
 *   (zeroed here; integer atomics).  A descriptor is one definition stream: a leaf bitmap, or NULL
 *   for every column without one.  Leaf L (a value of `offsets`) is bit bit0 + (L - origin[0]) of
 *   leaf_valid; a bit at or past nbits is null.  max_slots bounds the slot total (it sizes the
 *   grid).  Buffers 8-byte aligned.
 * Every entry is stream-ordered and does not synchronise. */
#define NVT_PQLIST_MAX_COLS 16
#define NVT_PQLIST_HEADER_WORDS 8
#define NVT_PQLIST_PAGE_WORDS 8
typedef struct nvt_pqlist_col {
  const uint8_t *leaf_valid; /* leaf bitmap or NULL                              */
  uint64_t bit0;             /* bit of the leaf that origin[0] names             */
  uint64_t nbits;            /* bits of leaf_valid that may be read              */
  uint8_t *def_out;          /* def_cap bytes                                    */
  uint64_t *nonnull;         /* max_pages counters                               */
} nvt_pqlist_col;
int nvt_pqlist_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_pqlist_plan(const int64_t *offsets, const int64_t *origin, uint64_t n, uint64_t page_slots, uint64_t max_pages, uint64_t rep_cap,
                    uint64_t def_cap, uint64_t *slot_start, uint64_t *table, void *ws, uint64_t ws_bytes,
                    void *stream);
int nvt_pqlist_pack_many(const nvt_pqlist_col *cols, int ncols, const int64_t *offsets, const int64_t *origin,
                         uint64_t n, const uint64_t *slot_start, const uint64_t *table, uint64_t max_pages,
                         uint64_t max_slots, uint8_t *rep_out, void *stream);
/* The way back (the parquet reader): the staged level streams of nvt_pq_decode_list_chunk -- rep 1
 * bit per slot, def `def_width` (1 or 2) bits per slot, n_slots < 2^32 slots, both 8-byte aligned and
 * ceil(n_slots * width / 64) words long -- become offsets[rows + 1] (offsets[r] = leaf slots in front
 * of the r-th slot with rep 0, offsets[rows] = leaves; a null or empty list is one slot that is no
 * leaf, i.e. an empty row) and, when leaf_valid is not NULL, the Arrow validity bitmap of the leaves
 * (ceil(leaves / 64) words, bit = def == max_def, bits past the last leaf 0).  rows and leaves are the
 * host decoder's counts: a stream that disagrees with them gives wrong numbers, never a store outside
 * offsets / leaf_valid.  ws: nvt_pqlist_unpack_ws_bytes(n_slots) bytes, 8-byte aligned.
 * Stream-ordered, no read-back. */
int nvt_pqlist_unpack_ws_bytes(uint64_t n_slots, uint64_t *bytes);
int nvt_pqlist_unpack(const uint8_t *rep, const uint8_t *def, int def_width, uint64_t n_slots, int leaf_level,
                      int max_def, uint64_t rows, uint64_t leaves, int64_t *offsets, uint8_t *leaf_valid,
                      void *ws, uint64_t ws_bytes, void *stream);

/* ---- parquet dictionary pages: Dataset.to_parquet(use_dictionary=...) ----
 * One column chunk's n NON-NULL values (NVT_I32 / NVT_I64; every bit pattern is a value) become a
 * dictionary -- their distinct values in ascending signed order -- and RLE_DICTIONARY index pages.
 * nvt_pq_dict_build: dict receives the d distinct values (room for min(n, max_entries) entries),
 *   state[NVT_PQ_DICT_STATE_WORDS] = {d, overflow, internal, 0}.  More than max_entries distinct
 *   values set overflow (bit 0): d and dict mean nothing then, dict holds no more than max_entries
 *   entries, and the work that grows with d stops.  1 <= max_entries <= NVT_PQ_DICT_MAX_ENTRIES.
 *   The value -> rank table stays in ws for the pack: an open-addressing table of
 *   2 * next_pow2(min(n, max_entries)) slots (at least 16), the home slot of a value v is the top
 *   log2(slots) bits of (v ^ sign bit, zero-extended to 64 bits) * 0x9E3779B97F4A7C15, probing is
 *   linear.  n = 0 clears state and does nothing else.
 * nvt_pq_dict_pack: the same values and n / max_entries, and page_start[npages + 1] on the device:
 *   page p holds values [page_start[p], page_start[p + 1]).  W = max(1, bit_length(d - 1)) is
 *   derived from state on the device.  Page p's indices are ONE bit-packed run's payload --
 *   W * ceil(nv_p / 8) bytes, LSB first, pad bits 0 -- at byte 16 * sum_{q<p} ceil(W *
 *   ceil(nv_q / 8) / 16) of out; the bytes up to the next 16-byte boundary are written as 0.
 *   Nothing is written when overflow is set; a page_start that is negative, descending or past n,
 *   or an out_cap smaller than the total, sets overflow bit 1 and writes nothing either.
 *   out 16-byte aligned.
 * ws: nvt_pq_dict_ws_bytes(n, max_entries, npages) bytes, 16-byte aligned, the same buffer for both
 * calls (build alone: npages = 0).  Stream-ordered, no allocation, no synchronisation. */
#define NVT_PQ_DICT_MAX_ENTRIES (1u << 20)
#define NVT_PQ_DICT_STATE_WORDS 4
int nvt_pq_dict_ws_bytes(uint64_t n, uint64_t max_entries, uint64_t npages, uint64_t *bytes);
int nvt_pq_dict_build(const void *values, int dtype, uint64_t n, uint64_t max_entries, void *dict,
                      uint64_t *state, void *ws, uint64_t ws_bytes, void *stream);
int nvt_pq_dict_pack(const void *values, int dtype, uint64_t n, uint64_t max_entries,
                     const int64_t *page_start, uint64_t npages, uint64_t *state, uint8_t *out,
                     uint64_t out_cap, void *ws, uint64_t ws_bytes, void *stream);

/* ---- parquet out: string columns (PLAIN BYTE_ARRAY pages) ----
 * A string column is int64 surrogates and a host dict {surrogate -> string}.  The dict travels to
 * the device once as an ENTRY TABLE: keys[n_entries] ascending, and the entries in key order as Arrow
 * string buffers -- offsets int64[n_entries + 1], chars 4-byte aligned and readable up to the 4-byte
 * boundary behind the last byte (what nvt_str_hash reads).  n_entries < 2^31.
 * nvt_pq_str_entry_ids: out_ids[j] = the position of surrogates[j] in keys (binary search) for the m
 *   NON-NULL values of a chunk; a surrogate that is no key gives id 0 and adds 1 to *bad (uint64 on
 *   the device, zeroed by the caller).
 * nvt_pq_byte_array_plan: the value at position j takes 4 + len(entry ids[j]) bytes (an id outside
 *   the table counts as the empty entry).  pos[m + 1] receives the 64-bit exclusive scan of those
 *   sizes, pos[m] the total; page_at[p] = pos[page_start[p]] for p in [0, pages] (page_start
 *   int64[pages + 1] on the device, in value positions, clamped to [0, m]): a page without values
 *   has page_at[p] == page_at[p + 1].  ws: nvt_pq_byte_array_ws_bytes(m) bytes, 8-byte aligned.
 * nvt_pq_byte_array_fill: every value's length as 4 bytes little endian, then its bytes, at
 *   out + pos[j] -- parquet's PLAIN encoding of BYTE_ARRAY.  out 4-byte aligned; the chars are read
 *   with aligned 4-byte loads, and no word is loaded that holds no byte of the entry.  A value that
 *   would end past out_bytes, or whose pos[j + 1] - pos[j] is not 4 + its length, is not written;
 *   nothing is ever written outside [out, out + out_bytes).
 * m = 0: nothing is done (no output is touched).  Stream-ordered, no allocation, no synchronisation. */
int nvt_pq_str_entry_ids(const int64_t *keys, uint64_t n_entries, const int64_t *surrogates, uint64_t m,
                         int32_t *out_ids, uint64_t *bad, void *stream);
int nvt_pq_byte_array_ws_bytes(uint64_t m, uint64_t *bytes);
int nvt_pq_byte_array_plan(const int32_t *ids, uint64_t m, const int64_t *offsets, uint64_t n_entries,
                           const int64_t *page_start, uint64_t pages, uint64_t *pos, uint64_t *page_at, void *ws,
                           uint64_t ws_bytes, void *stream);
int nvt_pq_byte_array_fill(const int32_t *ids, uint64_t m, const int64_t *offsets, const uint8_t *chars,
                           uint64_t n_entries, const uint64_t *pos, uint8_t *out, uint64_t out_bytes,
                           void *stream);

/* ---- parquet out: snappy pages, Dataset.to_parquet(device_compression="snappy") ----
 * The values regions of the column chunks of a row group become snappy ELEMENT streams (literals and
 * copies with 2-byte offsets; the varint in front of a page body is the host's).  A region is cut at
 * its page starts and then into fragments of at most NVT_SNAPPY_FRAG bytes; a fragment is parsed on
 * its own (no copy reaches in front of it), so the streams of a page's fragments, one behind the
 * other, are the page's elements.  All columns of a row group go through three calls that take the
 * same descriptors and the same batch; each launches once per NVT_SNAPPY_MAX_COLS descriptors.
 * Descriptor: src (nbytes readable bytes, any alignment; only words that hold a byte of src are
 *   loaded), page_start[npages + 1] on the device in units of `unit` bytes (a value is clamped to
 *   [0, nbytes], a descending pair is an empty page), elem (4 or 8: the parse also looks one element
 *   back), frag_base / max_frags (the column's records in the batch: frag_base of column 0 is 0,
 *   every next one follows; max_frags >= ceil(nbytes / FRAG) + npages), dense (dense_cap bytes,
 *   4-byte aligned) and out[npages + NVT_SNAPPY_OUT_WORDS] (8-byte aligned): out[p] = compressed
 *   bytes of page p, then {total, error, fragments, 0}.  error: NVT_SNAPPY_ERR_PLAN (the page table
 *   needs more than max_frags records) or NVT_SNAPPY_ERR_SLOT (a fragment's stream did not fit
 *   slot_cap; it reports 0 bytes): the column's output means nothing then.
 * Batch: frag_table (total_frags records of NVT_SNAPPY_FRAG_WORDS uint64 {source byte offset,
 *   bytes, page, column}; bytes = 0: unused), frag_size / frag_pos (total_frags + 1 uint64: the
 *   bytes of every fragment's stream and their exclusive scan over the batch), slots (total_frags
 *   * slot_cap bytes, 4-byte aligned; fragment e writes slots + e * slot_cap and never more than
 *   slot_cap bytes; NVT_SNAPPY_SLOT_BYTES holds any stream: DESIGN.md), ws (nvt_snappy_ws_bytes).
 * nvt_snappy_plan_many fills the table and clears every out; nvt_snappy_compress_many parses (one
 *   wave per fragment; the same input gives the same bytes); nvt_snappy_gather_many scans the sizes
 *   and moves the streams of column c, page after page, to dense: page p's elements start at the
 *   sum of out[q < p].  A column whose total passes dense_cap is not moved (its sizes stand).
 * Argument errors (null pointers, ncols <= 0, an element size other than 4 / 8, ranges that do not
 * tile [0, total_frags)) return NVT_EINVAL before anything is launched.  Stream-ordered, no
 * allocation, no synchronisation. */
#define NVT_SNAPPY_FRAG 32768u
#define NVT_SNAPPY_SLOT_BYTES (NVT_SNAPPY_FRAG + NVT_SNAPPY_FRAG / 32 + 16)
#define NVT_SNAPPY_MAX_COLS 16
#define NVT_SNAPPY_FRAG_WORDS 4
#define NVT_SNAPPY_OUT_WORDS 4
#define NVT_SNAPPY_OUT_TOTAL 0
#define NVT_SNAPPY_OUT_ERROR 1
#define NVT_SNAPPY_OUT_FRAGS 2
#define NVT_SNAPPY_ERR_PLAN 1
#define NVT_SNAPPY_ERR_SLOT 2
typedef struct nvt_snappy_col {
  const uint8_t *src;
  const int64_t *page_start;
  uint64_t npages;
  uint64_t nbytes;
  uint32_t unit;
  uint32_t elem;
  uint64_t frag_base;
  uint64_t max_frags;
  uint8_t *dense;
  uint64_t dense_cap;
  uint64_t *out;
} nvt_snappy_col;
typedef struct nvt_snappy_batch {
  uint64_t *frag_table;
  uint64_t *frag_size;
  uint64_t *frag_pos;
  uint8_t *slots;
  uint64_t total_frags;
  uint64_t slot_cap;
  void *ws;
  uint64_t ws_bytes;
} nvt_snappy_batch;
int nvt_snappy_slot_bytes(uint64_t *bytes);
int nvt_snappy_ws_bytes(uint64_t total_frags, uint64_t *bytes);
int nvt_snappy_plan_many(const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch, void *stream);
int nvt_snappy_compress_many(const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch, void *stream);
int nvt_snappy_gather_many(const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch, void *stream);

/* ---- exact column medians: ops.FillMedian (MSD radix select) ----
 * A value maps to an order-preserving unsigned key of its own width: floats flip all bits of a
 * negative value and the sign bit of the others, integers flip the sign bit.  The two middle
 * ranks k_lo = (m - 1) / 2 and k_hi = m / 2 of the m participating rows are selected digit by
 * digit, 11 bits at a time from the top: 3 passes for NVT_F32 / NVT_I32, 6 for NVT_F64 / NVT_I64.
 * A row takes part when its validity bit is set (or valid is NULL) and its value is not NaN; with
 * has_fill the other rows take part with fill_val, cast to the column type (the (x, valid, fill)
 * convention of nvt_moments_many).
 *
 * state: ncols blocks of NVT_SELECT_STATE_WORDS uint64 words on the device, 8-byte aligned.  The
 *   caller zeroes a block and sets NVT_SELECT_ST_BITS (32 / 64) and NVT_SELECT_ST_ALLOW_CAND
 *   before pass 0.  The launch sequence does not depend on the data and nothing is read back
 *   between the launches:
 *     for pass in 0 .. passes - 1:
 *       select_hist_many once per chunk (partition) of the columns   -- histograms add up
 *       [ranks of a job: sum the NVT_SELECT_ST_HIST words of every block over the ranks]
 *       select_step
 *       pass == 1: select_finish
 *   select_hist_many: one launch per NVT_SELECT_MAX_COLS descriptors; descriptor i belongs to
 *     state block i.  Adds, per column, the digit of pass `pass` of every participating row
 *     whose higher digits equal the prefix of a rank to that rank's NVT_SELECT_BINS-bin histogram
 *     (per-workgroup LDS histograms, one global atomic per non-empty bin; a row is binned once
 *     while both ranks share a prefix).  Returns at once for a column that is done or has no
 *     digit `pass`.
 *   select_step: one workgroup per column.  Pass 0: m = the rows counted, and the ranks.  Every
 *     pass: the bin that holds each rank is appended to the rank's prefix, the rank becomes
 *     relative to the bin, the histograms are zeroed.  NVT_SELECT_ST_DONE is set behind the last
 *     digit, or at once when m == 0.
 *   candidate path: when, behind pass 0, the bins of the two ranks hold at most
 *     NVT_SELECT_CAND_CAP rows (and NVT_SELECT_ST_ALLOW_CAND is set), the pass-1 launch copies
 *     the keys of those rows to the block's candidate buffer instead of counting them, and
 *     select_finish (one workgroup per column) resolves the remaining digits there and sets
 *     NVT_SELECT_ST_DONE.  Ranks of a job each hold only their own candidates: they leave
 *     NVT_SELECT_ST_ALLOW_CAND 0.
 *   result: NVT_SELECT_ST_M, and the keys of the two ranks in NVT_SELECT_ST_KEY_LO / _KEY_HI.
 * Every entry is stream-ordered and does not synchronise. */
#define NVT_SELECT_MAX_COLS 32
#define NVT_SELECT_MAX_PASSES 6
#define NVT_SELECT_BINS 2048
#define NVT_SELECT_CAND_CAP 65536
#define NVT_SELECT_ST_M 0           /* participating rows                                   */
#define NVT_SELECT_ST_RANK_LO 1     /* the ranks, relative to the rows that share the prefix */
#define NVT_SELECT_ST_RANK_HI 2
#define NVT_SELECT_ST_KEY_LO 3      /* the digits selected so far (the bits below are 0)     */
#define NVT_SELECT_ST_KEY_HI 4
#define NVT_SELECT_ST_DONE 5
#define NVT_SELECT_ST_NCAND 6       /* keys in the candidate buffer                          */
#define NVT_SELECT_ST_USE_CAND 7
#define NVT_SELECT_ST_PATH 8        /* NVT_SELECT_PATH_*: which way the column went (0: m == 0) */
#define NVT_SELECT_ST_BITS 9        /* caller: key width, 32 or 64                           */
#define NVT_SELECT_ST_ALLOW_CAND 10 /* caller: != 0 allows the candidate path                */
#define NVT_SELECT_ST_HIST 16       /* 2 * NVT_SELECT_BINS counts: low rank, high rank       */
#define NVT_SELECT_ST_CAND (16 + 2 * NVT_SELECT_BINS)
#define NVT_SELECT_STATE_WORDS (NVT_SELECT_ST_CAND + NVT_SELECT_CAND_CAP)
#define NVT_SELECT_PATH_CAND 1
#define NVT_SELECT_PATH_FULL 2
typedef struct nvt_select_col {
  const void *x;            /* n values of one chunk, 16-byte aligned            */
  const uint8_t *valid;     /* bitmap or NULL                                    */
  uint64_t n;
  int32_t dtype;            /* NVT_F32 / NVT_F64 / NVT_I32 / NVT_I64             */
  int32_t has_fill;
  double fill_val;
} nvt_select_col;
int nvt_select_hist_many(const nvt_select_col *cols, int ncols, int pass, void *state, void *stream);
int nvt_select_step(void *state, int ncols, int pass, void *stream);
int nvt_select_finish(void *state, int ncols, void *stream);

/* ---- column profile and narrowing casts: ops.DataStats / ops.ReduceDtypeSize ----
 * nvt_col_profile_many: every statistic of every column of a partition in ONE read of the column
 *   (one launch per NVT_PROFILE_MAX_COLS descriptors plus one small final launch; no atomics, so a
 *   result does not depend on scheduling).  A row counts when its validity bit is set (or valid is
 *   NULL) and its value is not NaN.  The accumulators are device memory the caller initialises and
 *   may fold several calls (partitions) into:
 *     counts[2]   int64 {rows seen, rows that count}, added; start at 0.
 *     extrema[2]  {min, max} of the rows that count.  NVT_I32 / NVT_I64: int64, exact (the value
 *                 never passes through a double); start at INT64_MAX / INT64_MIN.  NVT_F32 /
 *                 NVT_F64: double, NaN = nothing folded in yet (as nvt_minmax); -0.0 orders below
 *                 +0.0, so the zero that comes out does not depend on where the zeros sit.
 *     sums[2]     double {sum, sum of squares} of the rows that count, each converted to double
 *                 first, added (nvt_moments with has_fill = 0); start at 0.
 *   x need only be aligned to its element size (a slice of a larger buffer); nothing outside
 *   [x, x + n) is read.  A descriptor with n == 0 launches nothing and leaves its accumulators
 *   untouched.  partials: NVT_PROFILE_SCRATCH_BYTES of device scratch, 8-byte aligned, shared by
 *   the batches of one call (they run in stream order).  A null descriptor array, ncols <= 0, a
 *   null accumulator or an unknown dtype is NVT_EINVAL before the first launch.
 * nvt_cast_many: dst[i] = (dst type) src[i], one launch per NVT_PROFILE_MAX_COLS descriptors.
 *   NVT_I32 -> NVT_I8 / NVT_I16 and NVT_I64 -> NVT_I8 / NVT_I16 / NVT_I32 keep the low bits (two's
 *   complement wrap, numpy's astype); NVT_F64 -> NVT_F32 rounds to nearest, ties to even, NaN stays
 *   NaN and overflow goes to +-inf.  Any other pair (widening, int <-> float, same type) is
 *   NVT_EINVAL before the first launch.  src / dst need only be aligned to their element size; a
 *   lane writes whole 16-byte stores when dst is 16-byte aligned.  Validity bitmaps are not
 *   touched: the output column shares the input's.
 * Both entries are stream-ordered and do not synchronise. */
#define NVT_PROFILE_MAX_COLS 32
#define NVT_PROFILE_SCRATCH_BYTES (32 * 5 * 1024 * 8)
typedef struct nvt_profile_col {
  const void *x;            /* n values                                          */
  const uint8_t *valid;     /* bitmap or NULL                                    */
  uint64_t n;
  int32_t dtype;            /* NVT_F32 / NVT_F64 / NVT_I32 / NVT_I64             */
  int32_t reserved;
  int64_t *counts;          /* device int64[2]                                   */
  void *extrema;            /* device int64[2] (integer dtype) or double[2]      */
  double *sums;             /* device double[2]                                  */
} nvt_profile_col;
typedef struct nvt_cast_col {
  const void *src;          /* n values of src_dtype                             */
  void *dst;                /* n values of dst_dtype                             */
  uint64_t n;
  int32_t src_dtype, dst_dtype;
} nvt_cast_col;
int nvt_col_profile_many(const nvt_profile_col *cols, int ncols, void *partials, void *stream);
int nvt_cast_many(const nvt_cast_col *cols, int ncols, void *stream);

/* ---- hash partitioning of rows by key: Dataset.shuffle_by_keys ----
 * nvt_partition_ids: pid[i] = (uint32)(((mix(tags[i]) >> 32) * P) >> 32) with tags from
 *   nvt_join_hash (equal key tuples, nulls included, have equal tags) and the fixed finaliser
 *     mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *             z ^= z >> 31                                    (64-bit arithmetic, wrapping)
 *   The partition comes from the high half of mix(tag): the raw tag's low bits, which address the
 *   join tables, do not decide the balance.
 * nvt_partition_plan: a STABLE counting sort of the row indices by pid (every pid < P): perm lists
 *   the rows of partition 0 in ascending row order, then those of partition 1, ...; counts[p] = rows
 *   of partition p.  1 <= P <= NVT_PARTITION_MAX, n < 2^32, a 16-byte aligned workspace of
 *   nvt_partition_plan_ws_bytes(n, P) bytes.  No result depends on timing: two runs on the same
 *   input are bit-identical.  n = 0 is a no-op (counts is not written).  Workgroups walk tiles of
 *   nvt_partition_tile_rows() = NVT_PARTITION_TILE rows.
 * nvt_partition_gather_many: ONE output partition of m rows from nsegs segments.  Segment s covers
 *   the output rows [segs[s].start, segs[s + 1].start) (the last one up to m; segs[0].start = 0,
 *   starts ascending, empty segments allowed) and output row j of it is row
 *   segs[s].idx[j - segs[s].start] of the segment's source -- idx is a slice of one input
 *   partition's perm.  `segs` and the per-column tables src / src_valid are DEVICE arrays of nsegs
 *   entries (the caller uploads them once for all its launches); the descriptors themselves are
 *   host memory.  src_valid is NULL (no segment has a bitmap: dst_valid must be NULL) or a table
 *   whose NULL entries mean "all valid"; then dst_valid (ceil(m / 64) * 8 bytes, 8-byte aligned) is
 *   written whole, bits past m zero.  At most NVT_PARTITION_MAX_COLS columns per launch and
 *   NVT_PARTITION_MAX_SEGS segments; m = 0 is a no-op.  Every entry is stream-ordered. */
#define NVT_PARTITION_MAX 4096
#define NVT_PARTITION_TILE 512
#define NVT_PARTITION_MAX_COLS 16
#define NVT_PARTITION_MAX_SEGS 1024
typedef struct nvt_partition_seg {
  const int64_t *idx;       /* source rows of the segment's output rows          */
  uint64_t start;           /* first output row of the segment                   */
} nvt_partition_seg;
typedef struct nvt_partition_col {
  const void *const *src;          /* DEVICE table [nsegs]: the column in each segment's source */
  const uint8_t *const *src_valid; /* DEVICE table [nsegs] of bitmaps (entries may be NULL), or NULL */
  void *dst;                       /* m values                                    */
  uint8_t *dst_valid;              /* bitmap of ceil(m / 64) * 8 bytes, with src_valid */
  int32_t width;                   /* bytes per value: 1, 2, 4 or 8               */
  int32_t reserved;
} nvt_partition_col;
int nvt_partition_tile_rows(void);
int nvt_partition_ids(const uint64_t *tags, uint64_t n, uint32_t P, uint32_t *pid, void *stream);
int nvt_partition_plan_ws_bytes(uint64_t n, uint32_t P, uint64_t *bytes);
int nvt_partition_plan(const uint32_t *pid, uint64_t n, uint32_t P, int64_t *perm, uint64_t *counts, void *ws,
                       uint64_t ws_bytes, void *stream);
int nvt_partition_gather_many(const nvt_partition_col *cols, int ncols, const nvt_partition_seg *segs, int nsegs,
                              uint64_t m, void *stream);

/* ---- dense labels of a low-cardinality key: Dataset.to_parquet(partition_on=...) ----
 * nvt_key_labels: `tags`, `nulls` and `words` are what nvt_join_hash produced for the same n rows
 *   (`words` [nkeys][n] is read only for nkeys >= 2).  Two rows have the same key when their tags
 *   are equal; with nkeys == 1 a row with nulls[i] != 0 belongs to the null key whatever its tag
 *   (with more components the tag fingerprints the null bits).  Every 64-bit tag is a legal key.
 *     label[i]      rank of row i's key among the distinct keys ordered by their first row
 *                   (row 0's key is label 0); the labels feed nvt_partition_plan
 *     first_row[l]  that first row, for l < D; entries from D on are not written
 *     state[0]      D, the number of distinct keys
 *     state[1]      0 ok | 1 more than NVT_LABEL_MAX distinct keys (label and first_row are then
 *                   unspecified; nothing is written outside the outputs) | 2 with nkeys >= 2, two
 *                   rows with equal tags whose words or null bits differ (a fingerprint collision)
 *   No result depends on timing: first rows come from atomicMin and the ranks are taken over first
 *   rows, so two runs on the same input are bit-identical.  n < 2^32; n = 0 is a no-op (nothing is
 *   written); the call is stream-ordered; the workspace of nvt_key_labels_ws_bytes(n) bytes is
 *   16-byte aligned.  Workgroups walk tiles of nvt_key_labels_tile_rows() = NVT_LABEL_TILE rows. */
#define NVT_LABEL_MAX 4096            /* = NVT_PARTITION_MAX */
#define NVT_LABEL_TILE 2048
int nvt_key_labels_tile_rows(void);
int nvt_key_labels_ws_bytes(uint64_t n, uint64_t *bytes);
int nvt_key_labels(const uint64_t *tags, const uint8_t *nulls, const uint64_t *words, int nkeys, uint64_t n,
                   uint32_t *label, uint32_t *first_row, uint64_t *state, void *ws, uint64_t ws_bytes,
                   void *stream);

/* ---- device dataloader: batch gather of a chunk (nvtabular.loader.torch.TorchAsyncItr) ----
 * nvt_batch_take_many: dst[j * dst_stride] = cast(src[index[j]]) for the m output rows of every
 *   descriptor, ONE launch per NVT_TAKE_MAX_COLS descriptors (the entry loops).  index: m int64 on
 *   the device, or NULL for the identity (then m <= n_src).  The index is read once per row and
 *   used for every column of the launch.
 *   dtypes: src_dtype NVT_F32 .. NVT_I16 (a bool column is NVT_U8); dst_dtype equal to src_dtype, or
 *   NVT_I64 from any integer source, or NVT_F32 / NVT_F64 from any source.  Casts are C++
 *   conversions (round to nearest even; numpy's astype bit for bit).
 *   nulls: a source row whose bit in src_valid is clear, or an index[j] outside [0, n_src), writes 0
 *   to an integer destination and NaN to a float destination; a NaN source stays NaN.  An
 *   out-of-range index is never dereferenced.  dst_valid, when given, is the gathered bitmap
 *   (out-of-range rows clear their bit): ceil(m / 64) * 8 bytes, 8-byte aligned, written in whole
 *   64-bit words, bits past m zero.
 *   layout: dst_stride (elements, >= 1) = 1 is a contiguous column; dst_stride = k with dst at
 *   column c of a row-major [m, k] matrix is the stacked layout.  When the descriptors of ONE
 *   launch cover every column of such a matrix exactly once (4- or 8-byte elements, 16-byte aligned
 *   matrix, rows of at most NVT_TAKE_STAGE_ROW_BYTES bytes, at most NVT_TAKE_MAX_GROUPS matrices
 *   per launch), a tile of 256 rows is staged in LDS and written out in 16-byte stores; any other
 *   strided descriptor is written element by element.  src / dst aligned to their element size.
 * nvt_take_list_offsets: out_offsets[0] = 0, out_offsets[j + 1] = out_offsets[j] + the length of
 *   row index[j] (an out-of-range index is an empty row; index NULL = identity); out_offsets[m] is
 *   the number of output leaves, which the caller reads back to size them.  ws:
 *   nvt_take_list_ws_bytes(m) bytes, 8-byte aligned.
 * nvt_take_list_many: the leaves of up to NVT_LIST_MAX_COLS columns per launch that share
 *   `offsets`; the work is spread over the `total` OUTPUT leaves (row of a leaf: a search in
 *   out_offsets), same casts and null policy, leaf bitmaps carried when dst_valid is given
 *   (ceil(total / 64) * 8 bytes).  dst_stride must be 1.  total = 0 is a no-op.
 * Every entry is stream-ordered and does not synchronise; m = 0 is a no-op. */
#define NVT_TAKE_MAX_COLS 64
#define NVT_TAKE_MAX_GROUPS 4
#define NVT_TAKE_STAGE_ROW_BYTES 256
typedef struct nvt_take_col {
  const void *src;          /* n_src values (leaves: the column's leaves)       */
  const uint8_t *src_valid; /* bitmap or NULL                                   */
  void *dst;                /* first element written                            */
  uint8_t *dst_valid;       /* gathered bitmap, 8-byte aligned, or NULL         */
  int64_t dst_stride;       /* elements between two output rows, >= 1           */
  int32_t src_dtype;        /* NVT_F32 .. NVT_I16                               */
  int32_t dst_dtype;
} nvt_take_col;
int nvt_batch_take_many(const int64_t *index, uint64_t m, uint64_t n_src, const nvt_take_col *cols, int ncols,
                        void *stream);
int nvt_take_list_ws_bytes(uint64_t m, uint64_t *bytes);
int nvt_take_list_offsets(const int64_t *offsets, uint64_t n_src, const int64_t *index, uint64_t m,
                          int64_t *out_offsets, void *ws, uint64_t ws_bytes, void *stream);
int nvt_take_list_many(const nvt_take_col *cols, int ncols, const int64_t *offsets, const int64_t *index,
                       const int64_t *out_offsets, uint64_t m, uint64_t total, void *stream);
/* The same three gathers over SEVERAL sources: a chunk of partitions that is shuffled as a whole.
 * index[j] is a row of the concatenation of nsrc sources (1 <= nsrc <= NVT_TAKE_MAX_SOURCES);
 * src_begin[0 .. nsrc] (device int64, non-decreasing, src_begin[0] = 0) holds the first row of every
 * source and src_begin[nsrc] the number of rows: a row outside [0, src_begin[nsrc]) is out of range
 * and never dereferenced.  src_begin[s] == src_begin[s + 1] is an empty source, whose pointers may
 * be NULL.  n_total is the host's copy of src_begin[nsrc]; it only guards the identity index.
 * The source tables live in DEVICE memory, so the number of sources is not bounded by the kernel
 * arguments:
 *   nvt_batch_take_multi: cols[c].src points at nsrc records nvt_take_src on the device, one per
 *     source (sources of one column may differ in bitmap and dtype; a source without a bitmap is
 *     all valid); cols[c].src_valid and cols[c].src_dtype are ignored.  The caller keeps every
 *     (source dtype, dst_dtype) pair inside the casts of nvt_batch_take_many; they are not visible
 *     to the host here.  Layout, staging, null policy and dst_valid exactly as nvt_batch_take_many.
 *   nvt_take_list_offsets_multi: offsets = device array of nsrc pointers to the sources' offsets
 *     (src rows + 1 entries each, offsets[s][0] may be non-zero).  ws as nvt_take_list_offsets.
 *   nvt_take_list_multi: the leaves; cols[c].src points at nsrc records nvt_take_src that describe
 *     the LEAVES of every source (leaf 0 = the leaf at offsets[s][0]).
 * A lane finds its source by a binary search in src_begin, staged in LDS up to 1024 sources. */
#define NVT_TAKE_MAX_SOURCES 4096
typedef struct nvt_take_src {
  const void *src;
  const uint8_t *src_valid; /* bitmap or NULL (all valid)                       */
  int64_t src_dtype;        /* NVT_F32 .. NVT_I16                               */
} nvt_take_src;
int nvt_batch_take_multi(const int64_t *index, uint64_t m, const int64_t *src_begin, int nsrc, uint64_t n_total,
                         const nvt_take_col *cols, int ncols, void *stream);
int nvt_take_list_offsets_multi(const int64_t *const *offsets, const int64_t *src_begin, int nsrc, uint64_t n_total,
                                const int64_t *index, uint64_t m, int64_t *out_offsets, void *ws, uint64_t ws_bytes,
                                void *stream);
int nvt_take_list_multi(const nvt_take_col *cols, int ncols, const int64_t *const *offsets, const int64_t *src_begin,
                        int nsrc, const int64_t *index, const int64_t *out_offsets, uint64_t m, uint64_t total,
                        void *stream);

/* ---- delimited text (CSV / TSV) parsed on the device (nvtabular_amd/csv_text.py) ----
 * `text` is one byte range of a file that ends in '\n': nbytes < 2^31 bytes, 16-byte aligned and
 * readable up to the next multiple of 16 (the bytes past nbytes are never looked at).  sep is a
 * byte other than '\n' and quote; quote is a byte or -1 (no quoting).  A separator or newline
 * counts only outside quotes; a doubled quote inside a quoted field toggles the state twice.
 * `state` is NVT_CSV_STATE_WORDS uint64 on the device, 8-byte aligned (NVT_CSV_ST_*).
 * nvt_csv_count: pass 1 over tiles of NVT_CSV_TILE bytes + the scan of the tile records in ws
 *   (nvt_csv_ws_bytes(nbytes) bytes, 16-byte aligned).  Writes state: FIELDS, ROWS, PARITY (1 =
 *   the text ends inside a quoted field), BAD_ROW / QUOTE_ROW / BAD_FIELD = UINT64_MAX, SLOW = 0.
 *   The caller reads FIELDS and ROWS back to size field_end.
 * nvt_csv_index: pass 2 with the ws nvt_csv_count left.  field_end[i] (uint32) = position of the
 *   i-th separator or newline, for the nfields = state[FIELDS] of them: field k of row r is the
 *   bytes [field_end[r * ncols + k - 1] + 1, field_end[r * ncols + k]) (field 0 of row 0 starts
 *   at byte 0).  The first row whose newline is not separator (row + 1) * ncols - 1 is posted to
 *   state[BAD_ROW], the first row with a newline inside quotes to state[QUOTE_ROW] (atomic min).
 * nvt_csv_parse_many: one lane per row parses field cols[i].k of every row as cols[i].dtype
 *   (NVT_F32, NVT_F64, NVT_I32, NVT_I64), NVT_CSV_MAX_COLS descriptors per launch (the entry
 *   loops).  A '\r' that ends the last field of a row is dropped and quotes around a field are
 *   stripped.  An empty field is a null: 0 (NaN for floats) and a clear bit in out_valid
 *   (ceil(nrows / 64) * 8 bytes, 8-byte aligned, written in whole words, bits past nrows zero).
 *   Floats are bit-equal to strtod, NVT_F32 is that double rounded once; a field the device
 *   parser declines (csv_parse_f64 in nvt_csv_parse.hpp) gets 0, a set bit in `slow` (same shape
 *   as out_valid) and is counted in state[SLOW]: the caller parses those.  The smallest
 *   row << 24 | k << 2 | code (code NVT_CSV_INVALID or NVT_CSV_OVERFLOW) of the fields that do
 *   not parse goes to state[BAD_FIELD].  Needs nrows * ncols <= state[FIELDS] of the index.
 * nvt_csv_str_offsets: field k of every row as a string column: byte length after unquoting and
 *   collapsing doubled quotes, scanned into Arrow int32 offsets[nrows + 1] (offsets[nrows] = the
 *   chars total), and validity (a field that is empty after unquoting is null).  A quoted field
 *   with a quote inside that is not doubled is posted to state[BAD_FIELD] like a number that does
 *   not parse (code NVT_CSV_INVALID).  ws: nvt_csv_str_ws_bytes(nrows) bytes, 8-byte aligned.
 * nvt_csv_str_copy: the chars of that column at the offsets nvt_csv_str_offsets wrote.
 * nvt_csv_parse_f64_host / nvt_csv_parse_i64_host: the device's scalar parsers run on the host
 *   (tests): NVT_CSV_OK with *out set, NVT_CSV_DECLINED, NVT_CSV_INVALID or NVT_CSV_OVERFLOW.
 * Every device entry is stream-ordered and does not synchronise; nbytes = 0 / nrows = 0 is a
 * no-op. */
#define NVT_CSV_TILE 4096
#define NVT_CSV_SCAN_STEP 256   /* tile records one step of the tile scan covers */
#define NVT_CSV_MAX_COLS 64
#define NVT_CSV_STATE_WORDS 8
#define NVT_CSV_ST_FIELDS 0
#define NVT_CSV_ST_ROWS 1
#define NVT_CSV_ST_PARITY 2
#define NVT_CSV_ST_BAD_ROW 3
#define NVT_CSV_ST_QUOTE_ROW 4
#define NVT_CSV_ST_BAD_FIELD 5
#define NVT_CSV_ST_SLOW 6
#define NVT_CSV_OK 0
#define NVT_CSV_DECLINED 1
#define NVT_CSV_INVALID 2
#define NVT_CSV_OVERFLOW 3
typedef struct nvt_csv_col {
  void *out;            /* nrows values of dtype                                  */
  uint8_t *out_valid;   /* bitmap, ceil(nrows / 64) * 8 bytes, 8-byte aligned    */
  uint8_t *slow;        /* float dtypes: bitmap of the declined fields; else NULL */
  uint32_t k;           /* field of the row, < ncols                             */
  int32_t dtype;        /* NVT_F32, NVT_F64, NVT_I32 or NVT_I64                  */
} nvt_csv_col;
int nvt_csv_ws_bytes(uint64_t nbytes, uint64_t *bytes);
int nvt_csv_count(const uint8_t *text, uint64_t nbytes, int sep, int quote, void *ws, uint64_t ws_bytes,
                  uint64_t *state, void *stream);
int nvt_csv_index(const uint8_t *text, uint64_t nbytes, int sep, int quote, uint32_t ncols, const void *ws,
                  uint64_t ws_bytes, uint32_t *field_end, uint64_t nfields, uint64_t *state, void *stream);
int nvt_csv_parse_many(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                       uint32_t ncols, int quote, const nvt_csv_col *cols, int ndesc, uint64_t *state,
                       void *stream);
int nvt_csv_str_ws_bytes(uint64_t nrows, uint64_t *bytes);
int nvt_csv_str_offsets(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                        uint32_t ncols, uint32_t k, int quote, int32_t *offsets, uint8_t *out_valid, void *ws,
                        uint64_t ws_bytes, uint64_t *state, void *stream);
int nvt_csv_str_copy(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                     uint32_t ncols, uint32_t k, int quote, const int32_t *offsets, uint8_t *chars,
                     uint64_t chars_bytes, void *stream);
int nvt_csv_parse_f64_host(const char *text, int len, double *out);
int nvt_csv_parse_i64_host(const char *text, int len, int64_t *out);

/* ---- datetime columns (nvtabular_amd/kernels_datetime.py) ----
 * A datetime column is int64 counts since 1970-01-01T00:00:00 in a unit (NVT_DT_S / _MS / _US /
 * _NS); a null is a clear bit in `valid`, whatever its slot holds.
 * nvt_dt_field: out[i] = calendar field `field` of ts[i] on the proleptic Gregorian calendar
 *   (NVT_DT_WEEKDAY: Monday = 0; NVT_DT_DAYOFYEAR and NVT_DT_QUARTER from 1), 0 for a null row.
 *   Counts before the epoch round down: 1969-12-31 23:59:59 is on day -1.  No signed overflow for
 *   any int64 input; the results are specified for years 1 to 9999.  ts 8-byte aligned, valid NULL
 *   or ceil(n / 8) bytes, out 4-byte aligned.  Stream-ordered; n = 0 is a no-op.
 * nvt_dt_fields_host: the same function looped on the host (no nulls).
 * nvt_csv_parse_datetime: field cols[i].k of every row of an indexed CSV partition (nvt_csv_index)
 *   as int64 nanoseconds (cols[i].dtype NVT_I64, slow unused), launched after nvt_csv_parse_many
 *   with the same arguments.  Grammar: YYYY-MM-DD[(T| )HH:MM[:SS[.f{1,9}]]], nothing else.  The
 *   empty field is a null (0 and a clear bit in out_valid); NVT_CSV_INVALID (wrong shape, a day the
 *   month does not have, hour 24, second 60, a zone suffix, blanks) and NVT_CSV_OVERFLOW (outside
 *   int64 nanoseconds, or INT64_MIN itself) are posted to state[BAD_FIELD] as nvt_csv_parse_many
 *   posts them.
 * nvt_csv_parse_datetime_host: the scalar parser run on the host (tests). */
#define NVT_DT_S 0
#define NVT_DT_MS 1
#define NVT_DT_US 2
#define NVT_DT_NS 3
#define NVT_DT_YEAR 0
#define NVT_DT_MONTH 1
#define NVT_DT_DAY 2
#define NVT_DT_HOUR 3
#define NVT_DT_MINUTE 4
#define NVT_DT_SECOND 5
#define NVT_DT_WEEKDAY 6
#define NVT_DT_DAYOFYEAR 7
#define NVT_DT_QUARTER 8
int nvt_dt_field(const int64_t *ts, const uint8_t *valid, uint64_t n, int unit, int field, int32_t *out,
                 void *stream);
int nvt_dt_fields_host(const int64_t *ts, uint64_t n, int unit, int field, int32_t *out);
int nvt_csv_parse_datetime(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                           uint32_t ncols, int quote, const nvt_csv_col *cols, int ndesc, uint64_t *state,
                           void *stream);
int nvt_csv_parse_datetime_host(const char *text, int len, int64_t *out_ns);

/* ---- small utilities used by the host layer ---- */
/* widen an int32/uint8 key column to int64 (multi-key tables take int64 components) */
int nvt_widen_i64(const void *src, int dtype, uint64_t n, int64_t *out, void *stream);
/* count set bits of a validity bitmap over n rows (null bookkeeping, meta.*.parquet) */
int nvt_popcount(const uint8_t *valid, uint64_t n, uint64_t *out_device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NVT_HIP_H */
