// What the units of the groupby family share: the accumulator view and the row arguments their
// kernels take by value, the value loads / stores, the segmented reduction's launch
// (nvt_segreduce.hip) and the `words | sort scratch` workspace.
//   nvt_groupby.hip         hash table for 1..3 int64 keys (nvt_gb_*)
//   nvt_segreduce.hip       gb_segreduce_kernel, nvt_seg_aggregate
//   nvt_order_rows.hip      row order of the Groupby operator (nvt_sort_key_u64, nvt_order_rows)
//   nvt_sorted_groupby.hip  groupby of one 32-bit key by sorting (nvt_sgb_*), the count merge
#pragma once
#include "nvt_common.hpp"
#include "nvt_internal.hpp"

struct nvt_gb_head;  // nvt_groupby.hip: the 16-byte slot header of the hash table

namespace nvt {

constexpr int kMaxKeys = 3;
constexpr int kMaxVals = 8;

// (a by-value kernel argument: the members' order is the kernels' argument layout)
struct GbView {
  int nkeys, nvals, flags;
  uint64_t mask, cap;
  nvt_gb_head *head;
  long long *keys;  // components 1 .. nkeys-1
  unsigned long long *size, *count;
  double *sum, *sumsq, *vmin, *vmax;
  uint64_t *state;
  unsigned long long *vcount;  // [nvals][cap] non-null values per column (nvt_seg_aggregate only)
};

struct GbRowArgs {
  const int64_t *keys[kMaxKeys];
  const uint8_t *key_valid[kMaxKeys];
  const void *vals[kMaxVals];
  const uint8_t *val_valid[kMaxVals];
  int vdtype[kMaxVals];
  // sort path (gb_segreduce_kernel): a value column in the order of the words -- written by the
  // first aggregate of a pass that gathers it by row (sorted_out), read back streaming by the
  // next aggregate on the same words (sorted_in) instead of a second random gather
  const void *sorted_in[kMaxVals];
  void *sorted_out[kMaxVals];
};

__device__ __forceinline__ void atomic_min_f64(double *addr, double v) {
  unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
  unsigned long long old = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (v < __longlong_as_double((long long)old)) {
    unsigned long long prev = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
    if (prev == old) break;
    old = prev;
  }
}
__device__ __forceinline__ void atomic_max_f64(double *addr, double v) {
  unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
  unsigned long long old = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (v > __longlong_as_double((long long)old)) {
    unsigned long long prev = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
    if (prev == old) break;
    old = prev;
  }
}

__device__ __forceinline__ bool load_val(const void *p, int dtype, uint64_t i, double *out) {
  switch (dtype) {
    case NVT_F32: {
      float v = reinterpret_cast<const float *>(p)[i];
      *out = (double)v;
      return v == v;
    }
    case NVT_F64: {
      double v = reinterpret_cast<const double *>(p)[i];
      *out = v;
      return v == v;
    }
    case NVT_I32:
      *out = (double)reinterpret_cast<const int32_t *>(p)[i];
      return true;
    case NVT_I64:
      *out = (double)reinterpret_cast<const int64_t *>(p)[i];
      return true;
    case NVT_U8:
      *out = (double)reinterpret_cast<const uint8_t *>(p)[i];
      return true;
  }
  return false;
}

// the value as load_val read it, back in its own dtype (exact: v came from that dtype; NaN stays NaN)
__device__ __forceinline__ void store_val(void *p, int dtype, uint64_t i, double v) {
  switch (dtype) {
    case NVT_F32: reinterpret_cast<float *>(p)[i] = (float)v; break;
    case NVT_F64: reinterpret_cast<double *>(p)[i] = v; break;
    case NVT_I32: reinterpret_cast<int32_t *>(p)[i] = (int32_t)v; break;
    case NVT_I64: reinterpret_cast<int64_t *>(p)[i] = (int64_t)v; break;
    case NVT_U8: reinterpret_cast<uint8_t *>(p)[i] = (uint8_t)v; break;
  }
}

// ---- host side ----------------------------------------------------------------------------------
// NVT_CHECK_ARG for a helper that checks on behalf of the entry point `who`
inline int bad_arg(const char *who, const char *msg) {
  set_error("%s: %s", who, msg);
  return NVT_EINVAL;
}

// nvt_segreduce.hip.  One gb_segreduce_kernel<excl, SQ, MM> over n words ordered by slot, SQ / MM
// from the arrays the view carries; excl: see the kernel
void segreduce_launch(const GbView &t, const GbRowArgs &a, uint64_t n, const uint64_t *words,
                      uint32_t slot_div, bool excl, hipStream_t s);
// The row arguments of an entry point `who`: nkeys key columns (keys may be null when nkeys == 0)
// and nvals value columns, every column checked; the optional lists may be null as a whole
int row_args(GbRowArgs &a, const char *who, int nkeys, const int64_t *const *keys,
             const uint8_t *const *key_valid, int nvals, const void *const *vals, const int *vdtypes,
             const uint8_t *const *val_valid, const void *const *sorted_in = nullptr,
             void *const *sorted_out = nullptr);
// A view over plain arrays indexed by group (no table behind it): [cap] size / count,
// [nvals][cap] the rest; any of them may be null
GbView dense_view(uint64_t cap, int nvals, uint64_t *size, uint64_t *count, uint64_t *vcount,
                  double *sum, double *sumsq, double *vmin, double *vmax);

// words[n] | scratch of sort_words_bits: the workspace of nvt_gb_update's sort path and of
// nvt_order_rows.  bytes is what their _ws_bytes report, laid out from a null base (so the
// addresses are computed as integers)
struct WordsWs {
  uint64_t *words;
  void *sort_tmp;
  uint64_t bytes;
  WordsWs(void *base, uint64_t n)
      : words(reinterpret_cast<uint64_t *>(base)),
        sort_tmp(reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(base) + pad256(n * 8))),
        bytes(pad256(n * 8) + sort_words_tmp_bytes(n) + 512) {}
};

}  // namespace nvt
