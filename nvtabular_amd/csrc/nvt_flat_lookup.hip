// Flat-index lookups and lookup images: the transform side of Groupby, JoinGroupby and
// TargetEncoding on a flat range table (built by nvt_flat_index_build, nvt_vocab_order.hip) whose
// labels are group ids.
//
//  * flat_lookup*: key -> group id, alone or followed by the group's statistics (gather, te).
//  * lookup images: ONE packed record per group that holds every operator's values in their
//    output dtype (flat_lookup_image_kernel reads it; image_pack / jg_image / te_image write an
//    operator's byte range).  What the records hold is defined once in nvt_image.hpp; the key
//    directory (nvt_keydir.hip) reads and writes the same records.
#include "nvt_common.hpp"
#include "nvt_image.hpp"
#include "nvt_prof.hpp"
#include "nvt_range.hpp"

namespace nvt {

// key -> position in the sorted list through a flat range table whose labels are the positions
// (groupby group ids, join_groupby.py:198-203 / target_encoding.py:350-371: the reference's left
// merge on the key column).  Probing runs forward from the key's home slot; the entries along a
// run are in key order, so a larger key ends an unsuccessful probe as an empty slot does.
struct FlatIndexView {
  RangeMap map;
  int64_t offset;  // table key = column key - offset (0 for int32 columns)
  bool has_min;
  int64_t null_group;  // group of the rows whose key is null (-1: none; aux word LO + 10 holds it + 1)
  const unsigned long long *table;
  uint64_t slots;
};

__device__ __forceinline__ FlatIndexView flat_view(const int32_t *__restrict__ aux,
                                                   const unsigned long long *table, uint64_t slots,
                                                   int64_t offset) {
  FlatIndexView v;
  v.map = load_map(aux);
  v.offset = offset;
  v.has_min = aux[NVT_RANGE_AUX_LO + 6] != 0;
  v.null_group = (int64_t)aux[NVT_RANGE_AUX_LO + 10] - 1;
  v.table = table;
  v.slots = slots;
  return v;
}

template <typename K>
__device__ __forceinline__ int64_t flat_probe(const FlatIndexView &v, const K *__restrict__ keys,
                                              const uint8_t *__restrict__ valid, uint64_t i) {
  int64_t kv;
  if (!bit_valid(valid, i)) return v.null_group;   // null keys are one group (groupby dropna=False)
  if (__builtin_sub_overflow((int64_t)keys[i], v.offset, &kv)) return -1;
  if (kv < (int64_t)INT32_MIN || kv > (int64_t)INT32_MAX) return -1;
  const int32_t k = (int32_t)kv;
  if (k == INT32_MIN) return v.has_min ? 0 : -1;
  const uint64_t home = v.map.fine(k);
  if (home >= v.slots) return -1;
  unsigned long long w = 0;
  const uint64_t sl = flat_find_from(v.table, v.slots, home, k, v.table[home], &w);
  return sl == ~0ull ? -1 : (int64_t)(uint32_t)(w >> 32);
}

template <typename K>
__global__ __launch_bounds__(kBlock) void flat_lookup_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n,
    const int32_t *__restrict__ aux, const unsigned long long *__restrict__ table, uint64_t slots,
    int64_t offset, int64_t *__restrict__ out) {
  const FlatIndexView v = flat_view(aux, table, slots, offset);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    out[i] = flat_probe(v, keys, valid, i);
}

// JoinGroupby.transform in one pass (join_groupby.py:198-217): probe, then the group's record
// of `ncols` float64 statistics (one 32-byte sector for count / sum / mean / std) instead of a
// group-id column in HBM and one random gather per statistic.
constexpr int kGatherMaxCols = 16;
struct GatherOuts {
  void *out[kGatherMaxCols];
  int dtype[kGatherMaxCols];
  double miss[kGatherMaxCols];
};

template <typename OUT>
__device__ __forceinline__ void gather_store(void *out, uint64_t i, double x) {
  reinterpret_cast<OUT *>(out)[i] = (OUT)x;
}

template <typename K, int NC>
__global__ __launch_bounds__(kBlock) void flat_lookup_gather_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n,
    const int32_t *__restrict__ aux, const unsigned long long *__restrict__ table, uint64_t slots,
    int64_t offset, const double *__restrict__ records, GatherOuts o, unsigned long long *unseen) {
  const FlatIndexView v = flat_view(aux, table, slots, offset);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  bool any_unseen = false;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t g = flat_probe(v, keys, valid, i);
    any_unseen |= g < 0;
    double x[NC];
    const double *rec = records + (uint64_t)(g < 0 ? 0 : g) * NC;
    if constexpr (NC % 2 == 0) {  // records are 16-byte aligned: two statistics per load
#pragma unroll
      for (int c = 0; c < NC; c += 2) {
        const double2 p = *reinterpret_cast<const double2 *>(rec + c);
        x[c] = p.x;
        x[c + 1] = p.y;
      }
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = rec[c];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {  // compile-time c: descriptors stay in scalar registers
      const double y = g < 0 ? o.miss[c] : x[c];
      switch (o.dtype[c]) {
        case NVT_F32: gather_store<float>(o.out[c], i, y); break;
        case NVT_F64: gather_store<double>(o.out[c], i, y); break;
        case NVT_I32: gather_store<int32_t>(o.out[c], i, y); break;
        default: gather_store<int64_t>(o.out[c], i, y); break;
      }
    }
  }
  if (unseen && __ballot(any_unseen) != 0ull && lane_id() == 0) atomicOr(unseen, 1ull);
}

template <typename K>
static int launch_gather(int ncols, unsigned grid, hipStream_t s, const K *keys, const uint8_t *valid,
                         uint64_t n, const int32_t *aux, const unsigned long long *tab,
                         uint64_t capacity, int64_t offset, const double *records,
                         const GatherOuts &o, unsigned long long *flag) {
#define NVT_G(NC)                                                                                 \
  case NC:                                                                                        \
    flat_lookup_gather_kernel<K, NC><<<grid, kBlock, 0, s>>>(keys, valid, n, aux, tab, capacity, \
                                                             offset, records, o, flag);          \
    break;
  switch (ncols) {
    NVT_G(1) NVT_G(2) NVT_G(3) NVT_G(4) NVT_G(5) NVT_G(6) NVT_G(7) NVT_G(8)
    NVT_G(9) NVT_G(10) NVT_G(11) NVT_G(12) NVT_G(13) NVT_G(14) NVT_G(15) NVT_G(16)
    default: return NVT_EINVAL;
  }
#undef NVT_G
  return NVT_OK;
}

// TargetEncoding.transform in one pass (target_encoding.py:341-371): probe, then the group's
// record {sum, count, (sum_f, count_f) for every fold} -- 16 * (kfold + 1) contiguous bytes.
// A (group, fold) pair without rows is the reference's unmatched [fold, key] merge: y_mean.
template <typename K, typename OUT>
__global__ __launch_bounds__(kBlock) void flat_lookup_te_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n,
    const int32_t *__restrict__ aux, const unsigned long long *__restrict__ table, uint64_t slots,
    int64_t offset, const uint8_t *__restrict__ fold, unsigned kfold,
    const double *__restrict__ records, double p, double y_mean, OUT *__restrict__ out) {
  const FlatIndexView v = flat_view(aux, table, slots, offset);
  const unsigned stride_rec = 2 * (kfold + 1);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t g = flat_probe(v, keys, valid, i);
    double r = y_mean;
    if (g >= 0) {
      const double *rec = records + (uint64_t)g * stride_rec;
      const double2 tot = *reinterpret_cast<const double2 *>(rec);
      if (fold) {
        const double2 f = *reinterpret_cast<const double2 *>(rec + 2 + 2 * (unsigned)fold[i]);
        if (f.y > 0.0) r = (tot.x - f.x + p * y_mean) / (tot.y - f.y + p);
      } else {
        r = (tot.x + p * y_mean) / (tot.y + p);
      }
    }
    out[i] = (OUT)r;
  }
}

// ---- lookup images: ONE probe and ONE record per row for every operator on a key column ----
// JoinGroupby.transform and TargetEncoding.transform on the same key column are two left merges
// on the same key in the reference (join_groupby.py:198-217, target_encoding.py:341-371).  Here
// every such operator ("consumer") owns a byte range of ONE packed per-group record whose values
// are already what a row receives, in the OUTPUT dtype: JoinGroupby's statistics cast to
// float32 / int32, TargetEncoding's smoothed value for every fold ((kfold + 1) values: slot 0 =
// no fold, slot 1 + f = rows of fold f) -- the formula depends on (group, fold) only, so
// evaluating it per group at the end of the fit gives the row's value bit for bit.  A row then
// costs one random sector for the probe and one for its record (<= 64 bytes), whatever the
// number of operators and statistics; the kernel moves 4- or 8-byte words, it does not convert.
template <typename K, int MAXC>
__global__ __launch_bounds__(kBlock) void flat_lookup_image_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n,
    const int32_t *__restrict__ aux, const unsigned long long *__restrict__ table, uint64_t slots,
    int64_t offset, const int32_t *__restrict__ gid_in, int32_t *__restrict__ gid_out,
    const uint8_t *__restrict__ image, uint32_t stride_bytes, int ncols, ImageOuts o,
    unsigned long long *unseen) {
  const FlatIndexView v = flat_view(aux, table, slots, offset);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  bool any_unseen = false;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t g = gid_in ? (int64_t)gid_in[i] : flat_probe(v, keys, valid, i);
    if (gid_out) gid_out[i] = (int32_t)g;
    any_unseen |= g < 0;
    const uint8_t *rec = image + (uint64_t)(g < 0 ? 0 : g) * stride_bytes;
    uint64_t x[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {  // all loads first: they hit the one sector of the record
      if (c < ncols) {
        uint32_t at = o.off[c];
        if (o.fold[c]) at += (1u + (uint32_t)o.fold[c][i]) * o.fstride[c];
        x[c] = o.size[c] == 8 ? *reinterpret_cast<const uint64_t *>(rec + at)
                              : (uint64_t)*reinterpret_cast<const uint32_t *>(rec + at);
      }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < ncols) {
        const uint64_t y = g < 0 ? o.miss[c] : x[c];
        if (o.size[c] == 8) __builtin_nontemporal_store(y, reinterpret_cast<uint64_t *>(o.out[c]) + i);
        else __builtin_nontemporal_store((uint32_t)y, reinterpret_cast<uint32_t *>(o.out[c]) + i);
      }
    }
  }
  if (unseen && __ballot(any_unseen) != 0ull && lane_id() == 0) atomicOr(unseen, 1ull);
}

// image[g * stride + off + 4|8 * c] = (dst dtype) src[c][g]: a consumer's statistics (float64 /
// int64 arrays of one value per group) written into its byte range of the records
struct ImagePackArgs {
  const void *src[kImageMaxCols];
  int src_dtype[kImageMaxCols];  // NVT_F64 / NVT_I64
  int dst_dtype[kImageMaxCols];  // NVT_F32 / NVT_F64 / NVT_I32 / NVT_I64
  uint32_t off[kImageMaxCols];
};

__global__ __launch_bounds__(kBlock) void image_pack_kernel(ImagePackArgs a, int ncols, uint64_t groups,
                                                            uint8_t *__restrict__ image,
                                                            uint32_t stride_bytes) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += stride) {
    uint8_t *rec = image + g * stride_bytes;
    for (int c = 0; c < ncols; ++c) {
      const bool is_int = a.src_dtype[c] == NVT_I64;
      const double x = is_int ? 0.0 : reinterpret_cast<const double *>(a.src[c])[g];
      const int64_t xi = is_int ? reinterpret_cast<const int64_t *>(a.src[c])[g] : 0;
      image_store(rec + a.off[c], a.dst_dtype[c], x, xi, is_int);
    }
  }
}

// JoinGroupby's byte range straight from the fit's accumulators (join_groupby.py:175-217 over
// categorify.py:1087-1131 _bottom_level_groupby): count, sum, mean = sum / n, var = (sumsq -
// sum * sum / n) / max(n - 1, 1) (NaN for n = 1), std = sqrt(var), min, max -- evaluated per group
// in float64 like the column-wise path (ops/_groupby.py derive_stats), stored in the output dtype.
__global__ __launch_bounds__(kBlock) void jg_image_kernel(JgImageArgs a, int ncols, uint64_t groups,
                                                          uint8_t *__restrict__ image, uint32_t stride_bytes) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += stride) {
    uint8_t *rec = image + g * stride_bytes;
    const int64_t ni = a.count[g];
    for (int c = 0; c < ncols; ++c) {
      bool is_int;
      const double x = jg_stat(a, c, g, ni, &is_int);
      image_store(rec + a.off[c], a.dst_dtype[c], x, ni, is_int);
    }
  }
}

// TargetEncoding's byte range: (kfold + 1) values per group from the fit's statistics -- totals
// {count, sum}[g] and the dense per-(group, fold) {count, sum}[g * kfold + f] of the sort path
// (nvt_sgb_reduce) -- exactly the expression nvt_te_apply_folds evaluates per row
// (target_encoding.py:350-371), once per (group, fold).  A thread per value: the fold arrays are
// read in memory order, a record's values leave as one contiguous run.
template <typename OUT>
__global__ __launch_bounds__(kBlock) void te_image_kernel(
    const int64_t *__restrict__ tot_count, const double *__restrict__ tot_sum,
    const int64_t *__restrict__ fold_count, const double *__restrict__ fold_sum, unsigned kfold,
    uint64_t groups, double p, double y_mean, uint8_t *__restrict__ image, uint32_t stride_bytes,
    uint32_t off) {
  const unsigned per = kfold + 1;
  const uint64_t total = groups * per, stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const uint64_t g = e / per;
    const unsigned slot = (unsigned)(e - g * per);
    const double r = te_value(tot_count, tot_sum, fold_count, fold_sum, kfold, g, slot, p, y_mean);
    *reinterpret_cast<OUT *>(image + g * stride_bytes + off + slot * sizeof(OUT)) = (OUT)r;
  }
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_flat_lookup(const void *keys, int dtype, const uint8_t *valid, uint64_t n, const int32_t *aux,
                    const void *table, uint64_t capacity, int64_t key_offset, int64_t *out,
                    void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(keys && aux && table && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_lookup", n * (dtype == NVT_I64 ? 8ull : 4ull), s);
  const unsigned grid = stream_grid(n, kBlock * 2);
  const unsigned long long *tab = reinterpret_cast<const unsigned long long *>(table);
  switch (dtype) {
    case NVT_I32:
      flat_lookup_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)keys, valid, n, aux, tab, capacity,
                                                          key_offset, out);
      break;
    case NVT_I64:
      flat_lookup_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)keys, valid, n, aux, tab, capacity,
                                                          key_offset, out);
      break;
    default:
      set_error("nvt_flat_lookup: key dtype must be int32 / int64 (got %d)", dtype);
      return NVT_EINVAL;
  }
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}


int nvt_flat_lookup_gather(const void *keys, int dtype, const uint8_t *valid, uint64_t n,
                           const int32_t *aux, const void *table, uint64_t capacity,
                           int64_t key_offset, const double *records, int ncols, void *const *outs,
                           const int *out_dtypes, const double *miss, uint64_t *unseen, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(keys && aux && table && records && outs && out_dtypes && miss, "null pointer");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= kGatherMaxCols, "1..16 statistics per call");
  GatherOuts o;
  memset(&o, 0, sizeof(o));
  for (int c = 0; c < ncols; ++c) {
    NVT_CHECK_ARG(outs[c], "null output column");
    NVT_CHECK_ARG(out_dtypes[c] == NVT_F32 || out_dtypes[c] == NVT_F64 || out_dtypes[c] == NVT_I32 ||
                      out_dtypes[c] == NVT_I64, "output dtype must be f32 / f64 / i32 / i64");
    o.out[c] = outs[c];
    o.dtype[c] = out_dtypes[c];
    o.miss[c] = miss[c];
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_lookup", n * (dtype == NVT_I64 ? 8ull : 4ull), s);
  const unsigned grid = stream_grid(n, kBlock * 2);
  const unsigned long long *tab = reinterpret_cast<const unsigned long long *>(table);
  unsigned long long *flag = reinterpret_cast<unsigned long long *>(unseen);
  int rc;
  if (dtype == NVT_I32)
    rc = launch_gather<int32_t>(ncols, grid, s, (const int32_t *)keys, valid, n, aux, tab, capacity,
                                key_offset, records, o, flag);
  else if (dtype == NVT_I64)
    rc = launch_gather<int64_t>(ncols, grid, s, (const int64_t *)keys, valid, n, aux, tab, capacity,
                                key_offset, records, o, flag);
  else {
    set_error("nvt_flat_lookup_gather: key dtype must be int32 / int64 (got %d)", dtype);
    return NVT_EINVAL;
  }
  if (rc) return rc;
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_flat_lookup_te(const void *keys, int dtype, const uint8_t *valid, uint64_t n, const int32_t *aux,
                       const void *table, uint64_t capacity, int64_t key_offset, const uint8_t *fold,
                       int kfold, const double *records, double p_smooth, double y_mean, void *out,
                       int out_dtype, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(keys && aux && table && records && out, "null pointer");
  NVT_CHECK_ARG(kfold >= 1 && kfold <= 256 && ((kfold > 1) == (fold != nullptr)), "fold ids come with kfold > 1");
  NVT_CHECK_ARG(dtype == NVT_I32 || dtype == NVT_I64, "key dtype must be int32 / int64");
  NVT_CHECK_ARG(out_dtype == NVT_F32 || out_dtype == NVT_F64, "out dtype must be f32 / f64");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("te_apply", n * (dtype == NVT_I64 ? 8ull : 4ull), s);
  const unsigned grid = stream_grid(n, kBlock * 2);
  const unsigned long long *tab = reinterpret_cast<const unsigned long long *>(table);
  const unsigned kf = fold ? (unsigned)kfold : 0u;  // record stride 2 * (kf + 1)
#define NVT_TE_LAUNCH(K, OUT)                                                                   \
  flat_lookup_te_kernel<K, OUT><<<grid, kBlock, 0, s>>>((const K *)keys, valid, n, aux, tab,    \
                                                        capacity, key_offset, fold, kf, records, \
                                                        p_smooth, y_mean, (OUT *)out)
  if (dtype == NVT_I32 && out_dtype == NVT_F32) NVT_TE_LAUNCH(int32_t, float);
  else if (dtype == NVT_I32) NVT_TE_LAUNCH(int32_t, double);
  else if (out_dtype == NVT_F32) NVT_TE_LAUNCH(int64_t, float);
  else NVT_TE_LAUNCH(int64_t, double);
#undef NVT_TE_LAUNCH
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_flat_lookup_image(const void *keys, int dtype, const uint8_t *valid, uint64_t n,
                          const int32_t *aux, const void *table, uint64_t capacity, int64_t key_offset,
                          const int32_t *gid_in, int32_t *gid_out, const void *image,
                          uint32_t stride_bytes, int ncols, void *const *outs,
                          const uint8_t *const *folds, const uint32_t *offs, const uint32_t *sizes,
                          const uint64_t *miss_bits, uint64_t *unseen, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(aux && table && image && outs && offs && sizes && miss_bits, "null pointer");
  NVT_CHECK_ARG(keys || gid_in, "keys or group ids");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= kImageMaxCols, "1..24 outputs");
  NVT_CHECK_ARG(stride_bytes >= 8 && stride_bytes % 8 == 0, "record stride: a multiple of 8 bytes");
  NVT_CHECK_ARG(dtype == NVT_I32 || dtype == NVT_I64, "key dtype must be int32 / int64");
  ImageOuts o;
  memset(&o, 0, sizeof(o));
  for (int c = 0; c < ncols; ++c) {
    NVT_CHECK_ARG(outs[c], "null output");
    NVT_CHECK_ARG(sizes[c] == 4 || sizes[c] == 8, "values are 4 or 8 bytes");
    NVT_CHECK_ARG(offs[c] % sizes[c] == 0, "value offsets are aligned to the value size");
    o.out[c] = outs[c];
    o.fold[c] = folds ? folds[c] : nullptr;
    o.miss[c] = miss_bits[c];
    o.off[c] = offs[c];
    o.fstride[c] = sizes[c];
    o.size[c] = sizes[c];
    // (with a fold column the caller guarantees off + (kfold + 1) * size <= stride)
    NVT_CHECK_ARG((uint64_t)offs[c] + sizes[c] <= stride_bytes, "value outside the record");
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_lookup", n * (dtype == NVT_I64 ? 8ull : 4ull), s);
  const unsigned grid = stream_grid(n, kBlock * 2);
  const unsigned long long *tab = reinterpret_cast<const unsigned long long *>(table);
  unsigned long long *flag = reinterpret_cast<unsigned long long *>(unseen);
  const uint8_t *img = reinterpret_cast<const uint8_t *>(image);
#define NVT_IMG(K, MAXC)                                                                          \
  flat_lookup_image_kernel<K, MAXC><<<grid, kBlock, 0, s>>>((const K *)keys, valid, n, aux, tab,  \
                                                            capacity, key_offset, gid_in, gid_out, \
                                                            img, stride_bytes, ncols, o, flag)
#define NVT_IMG_K(K)                    \
  do {                                  \
    if (ncols <= 2) NVT_IMG(K, 2);      \
    else if (ncols <= 4) NVT_IMG(K, 4); \
    else if (ncols <= 8) NVT_IMG(K, 8); \
    else if (ncols <= 16) NVT_IMG(K, 16); \
    else NVT_IMG(K, 24);                \
  } while (0)
  if (dtype == NVT_I32) NVT_IMG_K(int32_t);
  else NVT_IMG_K(int64_t);
#undef NVT_IMG_K
#undef NVT_IMG
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_image_pack(const void *const *src, const int *src_dtypes, const int *dst_dtypes,
                   const uint32_t *offs, int ncols, uint64_t groups, void *image,
                   uint32_t stride_bytes, void *stream) {
  if (groups == 0 || ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(src && src_dtypes && dst_dtypes && offs && image, "null pointer");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= kImageMaxCols, "1..24 columns");
  ImagePackArgs a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < ncols; ++c) {
    NVT_CHECK_ARG(src[c], "null source column");
    NVT_CHECK_ARG(src_dtypes[c] == NVT_F64 || src_dtypes[c] == NVT_I64, "sources are float64 / int64");
    const int d = dst_dtypes[c];
    NVT_CHECK_ARG(d == NVT_F32 || d == NVT_F64 || d == NVT_I32 || d == NVT_I64, "values are f32 / f64 / i32 / i64");
    const uint32_t sz = (d == NVT_F32 || d == NVT_I32) ? 4u : 8u;
    NVT_CHECK_ARG(offs[c] % sz == 0 && (uint64_t)offs[c] + sz <= stride_bytes, "value outside the record");
    a.src[c] = src[c];
    a.src_dtype[c] = src_dtypes[c];
    a.dst_dtype[c] = d;
    a.off[c] = offs[c];
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_index", groups * 8ull * ncols, s);
  image_pack_kernel<<<stream_grid(groups, kBlock, 8), kBlock, 0, s>>>(
      a, ncols, groups, reinterpret_cast<uint8_t *>(image), stride_bytes);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_jg_image(const int64_t *count, const double *const *sum, const double *const *sumsq,
                 const double *const *mn, const double *const *mx, int nvals, const int *kinds,
                 const int *vals, const int *dst_dtypes, const uint32_t *offs, int ncols, uint64_t groups,
                 void *image, uint32_t stride_bytes, void *stream) {
  if (groups == 0 || ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(count && kinds && vals && dst_dtypes && offs && image, "null pointer");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= kImageMaxCols, "1..24 columns");
  NVT_CHECK_ARG(nvals >= 0 && nvals <= kJgMaxVals, "0..8 value columns");
  JgImageArgs a;
  memset(&a, 0, sizeof(a));
  a.count = count;
  for (int j = 0; j < nvals; ++j) {
    a.sum[j] = sum ? sum[j] : nullptr;
    a.sumsq[j] = sumsq ? sumsq[j] : nullptr;
    a.mn[j] = mn ? mn[j] : nullptr;
    a.mx[j] = mx ? mx[j] : nullptr;
  }
  for (int c = 0; c < ncols; ++c) {
    const int k = kinds[c], j = vals[c], d = dst_dtypes[c];
    NVT_CHECK_ARG(k >= 0 && k <= 6, "statistic kind 0..6");
    NVT_CHECK_ARG(k == 0 || (j >= 0 && j < nvals), "value column out of range");
    NVT_CHECK_ARG(k == 0 || a.sum[j] || k == 3 || k == 4, "null sum array");
    NVT_CHECK_ARG((k != 3 || a.mn[j]) && (k != 4 || a.mx[j]) && (k < 5 || (a.sum[j] && a.sumsq[j])),
                  "null accumulator array for a requested statistic");
    NVT_CHECK_ARG(d == NVT_F32 || d == NVT_F64 || d == NVT_I32 || d == NVT_I64, "values are f32 / f64 / i32 / i64");
    const uint32_t sz = (d == NVT_F32 || d == NVT_I32) ? 4u : 8u;
    NVT_CHECK_ARG(offs[c] % sz == 0 && (uint64_t)offs[c] + sz <= stride_bytes, "value outside the record");
    a.kind[c] = k;
    a.val[c] = k == 0 ? 0 : j;
    a.dst_dtype[c] = d;
    a.off[c] = offs[c];
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_index", groups * 8ull * ncols, s);
  jg_image_kernel<<<stream_grid(groups, kBlock, 8), kBlock, 0, s>>>(a, ncols, groups,
                                                                    reinterpret_cast<uint8_t *>(image), stride_bytes);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_te_image(const int64_t *tot_count, const double *tot_sum, const int64_t *fold_count,
                 const double *fold_sum, int kfold, uint64_t groups, double p_smooth, double y_mean,
                 int out_dtype, void *image, uint32_t stride_bytes, uint32_t off, void *stream) {
  if (groups == 0) return NVT_OK;
  NVT_CHECK_ARG(tot_count && tot_sum && image, "null pointer");
  NVT_CHECK_ARG(kfold >= 0 && kfold <= 256, "kfold must be 0 (no folds) .. 256");
  NVT_CHECK_ARG(kfold == 0 || (fold_count && fold_sum), "fold statistics come with kfold > 0");
  NVT_CHECK_ARG(out_dtype == NVT_F32 || out_dtype == NVT_F64, "out dtype must be f32 / f64");
  const uint32_t sz = out_dtype == NVT_F32 ? 4u : 8u;
  NVT_CHECK_ARG(off % sz == 0 && (uint64_t)off + (uint64_t)(kfold + 1) * sz <= stride_bytes,
                "values outside the record");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_index", groups * 16ull * (kfold + 1), s);
  const unsigned grid = stream_grid(groups * (uint64_t)(kfold + 1), kBlock * 2, 8);
  uint8_t *img = reinterpret_cast<uint8_t *>(image);
  if (out_dtype == NVT_F32)
    te_image_kernel<float><<<grid, kBlock, 0, s>>>(tot_count, tot_sum, fold_count, fold_sum, (unsigned)kfold,
                                                   groups, p_smooth, y_mean, img, stride_bytes, off);
  else
    te_image_kernel<double><<<grid, kBlock, 0, s>>>(tot_count, tot_sum, fold_count, fold_sum, (unsigned)kfold,
                                                    groups, p_smooth, y_mean, img, stride_bytes, off);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
