// ---- Groupby operator (groupby.py:236-263): row order ---------------------------------------
// rows are ordered by (group id, sort columns) with the stable radix sort of nvt_sort.hip over
// packed (key32 << 32 | row) words -- a 64-bit sort key takes two passes of 32 bits -- and every
// conventional aggregate comes from ONE wave-level segmented reduction over the ordered rows
// (nvt_seg_aggregate, nvt_segreduce.hip, writing straight into the output arrays).
#include "nvt_groupby.hpp"
#include "nvt_prof.hpp"

namespace nvt {

template <typename T>
__device__ __forceinline__ uint64_t sortable_bits(T v);
template <>
__device__ __forceinline__ uint64_t sortable_bits<int64_t>(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ull;
}
template <>
__device__ __forceinline__ uint64_t sortable_bits<int32_t>(int32_t v) {
  return sortable_bits<int64_t>((int64_t)v);
}
template <>
__device__ __forceinline__ uint64_t sortable_bits<uint8_t>(uint8_t v) {
  return sortable_bits<int64_t>((int64_t)v);
}
template <>
__device__ __forceinline__ uint64_t sortable_bits<double>(double v) {
  // -0.0 == +0.0 for every comparison sort (numpy, pandas): ONE image, so that a stable sort
  // keeps the two in row order (float32 columns come through here too)
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
template <>
__device__ __forceinline__ uint64_t sortable_bits<float>(float v) {
  return sortable_bits<double>((double)v);
}

// out[i] = order-preserving 64-bit image of x[i]; nulls / NaN sort LAST for either direction
// (pandas sort_values na_position="last"); descending = complemented image
template <typename T>
__global__ __launch_bounds__(kBlock) void sort_key_kernel(const T *__restrict__ x,
                                                          const uint8_t *__restrict__ valid,
                                                          uint64_t n, int ascending,
                                                          uint64_t *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const T v = x[i];
    const bool ok = bit_valid(valid, i) && !is_nan(v);
    uint64_t b = sortable_bits<T>(v);
    if (!ascending) b = ~b;
    out[i] = ok ? (b == ~0ull ? b - 1 : b) : ~0ull;
  }
}

// words[i] = (hi32(i) << 32) | row(i) with row(i) = perm ? low 32 bits of perm[i] : i and
// hi32 = 32-bit chunk `chunk` (0 = low, 1 = high) of src64[row] -- or, for group ids, the id
// itself with -1 (null key) mapped to `null_hi` so that those rows sort last
__global__ __launch_bounds__(kBlock) void pack_words_kernel(const uint64_t *__restrict__ src64,
                                                            const int64_t *__restrict__ gid,
                                                            const uint64_t *__restrict__ perm,
                                                            uint64_t n, int chunk, uint32_t null_hi,
                                                            uint64_t *__restrict__ words) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t row = perm ? (uint32_t)perm[i] : (uint32_t)i;
    uint32_t hi;
    if (gid) {
      const int64_t g = gid[row];
      hi = g < 0 ? null_hi : (uint32_t)g;
    } else {
      hi = (uint32_t)(src64[row] >> (32 * chunk));
    }
    words[i] = ((uint64_t)hi << 32) | row;
  }
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_sort_key_u64(const void *x, int dtype, const uint8_t *valid, uint64_t n, int ascending,
                     uint64_t *out, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(x && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = stream_grid(n, kBlock * 4);
  switch (dtype) {
    case NVT_F32: sort_key_kernel<float><<<grid, kBlock, 0, s>>>((const float *)x, valid, n, ascending, out); break;
    case NVT_F64: sort_key_kernel<double><<<grid, kBlock, 0, s>>>((const double *)x, valid, n, ascending, out); break;
    case NVT_I32: sort_key_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)x, valid, n, ascending, out); break;
    case NVT_I64: sort_key_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)x, valid, n, ascending, out); break;
    case NVT_U8: sort_key_kernel<uint8_t><<<grid, kBlock, 0, s>>>((const uint8_t *)x, valid, n, ascending, out); break;
    default:
      set_error("nvt_sort_key_u64: unsupported dtype %d", dtype);
      return NVT_EINVAL;
  }
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_order_rows_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  *bytes = WordsWs(nullptr, n).bytes;
  return NVT_OK;
}

// Stable refinement of a row order: perm_out = rows of perm_in (NULL: 0..n-1) re-ordered by
//   key64 (both 32-bit halves, two radix sorts)                  when key64 != NULL
//   group id (ids in [0, ngroups), -1 = null key -> sorted last)  when gid != NULL
// perm_in / perm_out: uint64 row indices (may alias).  ws: nvt_order_rows_ws_bytes(n).
int nvt_order_rows(const uint64_t *key64, const int64_t *gid, uint64_t ngroups,
                   const uint64_t *perm_in, uint64_t n, uint64_t *perm_out, void *ws, void *stream) {
  if (n == 0) return NVT_OK;  // (first: the columns of an empty frame have no address)
  NVT_CHECK_ARG((key64 != nullptr) != (gid != nullptr), "exactly one of key64 / gid");
  NVT_CHECK_ARG(perm_out && ws, "null pointer");
  NVT_CHECK_ARG(n < (1ull << 30) && ngroups < (1ull << 31), "at most 2^30-1 rows");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_order", 0, s);
  const WordsWs w(ws, n);
  const unsigned grid = stream_grid(n, kBlock * 4);
  const uint64_t *cur = perm_in;
  const int rounds = key64 ? 2 : 1;
  for (int r = 0; r < rounds; ++r) {
    int hi_bits = 32;
    if (gid) {
      hi_bits = 1;
      while ((1ull << hi_bits) <= ngroups) ++hi_bits;  // ids 0..ngroups (ngroups = null marker)
    }
    pack_words_kernel<<<grid, kBlock, 0, s>>>(key64, gid, cur, n, r, (uint32_t)ngroups, w.words);
    NVT_CHECK_LAUNCH();
    uint64_t *sorted = nullptr;
    int rc = sort_words_bits(w.words, n, 32, 32 + hi_bits, w.sort_tmp, &sorted, s);
    if (rc) return rc;
    // the low halves are the new row order (kept as the 64-bit words: consumers mask them)
    NVT_CHECK_HIP(hipMemcpyAsync(perm_out, sorted, n * 8, hipMemcpyDeviceToDevice, s));
    cur = perm_out;
  }
  return NVT_OK;
}

}  // extern "C"
