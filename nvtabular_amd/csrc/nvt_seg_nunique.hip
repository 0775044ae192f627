// Groupby nunique: distinct non-null values per group, for rows that arrive ordered by group
// (words = group << 32 | row, the input of nvt_seg_aggregate).  pandas groupby(...).nunique().
//
// Per value column, on the caller's stream:
//   1. nu_key_kernel      position i of the words -> key[i], an INJECTIVE order-preserving image
//                         of the value on its own type (-0.0 folded into +0.0), and gid[i], the
//                         group of the entry or the null marker `ngroups` when the entry does not
//                         count (null key, null value, NaN); also the first sort words
//                         (low half of the key << 32 | i)
//   2. radix refinements  stable LSD sorts of (32-bit chunk << 32 | i) words with the sort of
//                         nvt_sort.hip: by the key's low half, by its high half (64-bit types
//                         only), then by gid -- the order inside a group is by value, the entries
//                         that do not count sort behind the last group
//   3. nu_count_kernel    an entry counts when it is the first of its group or its key differs
//                         from the key in front of it; the flags are summed per group by a
//                         wave-level segmented reduction with one atomic per run of a wave's chunk
// nvt_sort_key_u64 is not used for step 1: it reserves one image for nulls, so two int64 values
// at the end of the range share an image and a stable sort may interleave them.  Here the nulls
// leave through the group id instead and every one of the 2^64 images is a value's own.
// Launches per column: the key kernel, one repack per further refinement, the count kernel and
// the sorts' own (a histogram, a base scan and one scatter per 8 sorted bits: the gid sort takes
// as many scatters as a group id has bytes, 1..4).  No host loop over groups, no read-back.
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"

namespace nvt {

constexpr int kNuMaxCols = 8;

template <typename T>
__device__ __forceinline__ uint64_t nu_image(T v);
template <>
__device__ __forceinline__ uint64_t nu_image<uint8_t>(uint8_t v) { return v; }
template <>
__device__ __forceinline__ uint64_t nu_image<int32_t>(int32_t v) {
  return (uint32_t)v ^ 0x80000000u;
}
template <>
__device__ __forceinline__ uint64_t nu_image<int64_t>(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ull;
}
template <>
__device__ __forceinline__ uint64_t nu_image<float>(float v) {
  if (v == 0.0f) v = 0.0f;  // -0.0 == +0.0: one value
  const uint32_t b = __float_as_uint(v);
  return (b >> 31) ? (uint32_t)~b : (b | 0x80000000u);
}
template <>
__device__ __forceinline__ uint64_t nu_image<double>(double v) {
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nu_key_kernel(const uint64_t *__restrict__ words,
                                                        const T *__restrict__ x,
                                                        const uint8_t *__restrict__ valid,
                                                        uint64_t n, uint32_t ngroups,
                                                        uint64_t *__restrict__ key,
                                                        uint32_t *__restrict__ gid,
                                                        uint64_t *__restrict__ sort_words) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint64_t w = words[i];
    const uint32_t row = (uint32_t)w;
    uint64_t k = 0;
    uint32_t g = ngroups;
    if ((w >> 32) < ngroups && bit_valid(valid, row)) {  // (rows of null keys are not read)
      const T v = x[row];
      if (!is_nan(v)) {
        k = nu_image<T>(v);
        g = (uint32_t)(w >> 32);
      }
    }
    key[i] = k;
    gid[i] = g;
    sort_words[i] = (k << 32) | i;
  }
}

// the next refinement's words from the order so far: (high half of the key | gid) << 32 | i
__global__ __launch_bounds__(kBlock) void nu_repack_kernel(const uint64_t *order,
                                                           const uint64_t *__restrict__ key,
                                                           const uint32_t *__restrict__ gid,
                                                           uint64_t n, uint64_t *sort_words) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
    const uint64_t i = order[j] & 0xFFFFFFFFull;
    const uint64_t hi = gid ? (uint64_t)gid[i] : key[i] >> 32;
    sort_words[j] = (hi << 32) | i;
  }
}

// sorted[j] = gid << 32 | i, ordered by (gid, key[i]).  Every wave walks one contiguous chunk in
// rows of 64 and carries the run that reaches the end of a row into the next one, like
// gb_segreduce_kernel: one atomic per run of a chunk.
__global__ __launch_bounds__(kBlock) void nu_count_kernel(const uint64_t *__restrict__ sorted,
                                                          const uint64_t *__restrict__ key,
                                                          uint64_t n, uint32_t ngroups,
                                                          unsigned long long *__restrict__ out) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  const unsigned lane = lane_id();
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint64_t wave0 = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  const uint64_t per_wave = ((n + nwaves - 1) / nwaves + kWave - 1) / kWave * kWave;
  const uint64_t chunk_begin = wave0 * per_wave;
  const uint64_t chunk_end = (wave0 + 1) * per_wave < n ? (wave0 + 1) * per_wave : n;
  const unsigned long long below = (2ull << lane) - 1ull;  // lanes 0 .. lane
  uint32_t c_g = kNone;   // the carried run (wave-uniform): its group and its count so far
  unsigned c_cnt = 0;
  for (uint64_t base = chunk_begin; base < chunk_end; base += kWave) {
    const uint64_t j = base + lane;
    const bool act = j < chunk_end;
    const uint64_t w = act ? sorted[j] : ~0ull;
    uint32_t g = (uint32_t)(w >> 32);
    if (!act || g >= ngroups) g = kNone;  // entries nobody counts
    const unsigned long long k = g != kNone ? key[w & 0xFFFFFFFFull] : 0ull;
    // the entry in front: the lane below, or for lane 0 the last word of the previous row
    const uint32_t rg = __shfl_up(g, 1, 64);
    uint32_t pg = rg;
    unsigned long long pk = __shfl_up(k, 1, 64);
    if (lane == 0) {
      pg = kNone;
      if (j > 0 && act) {
        const uint64_t pw = sorted[j - 1];
        pg = (uint32_t)(pw >> 32);
        if (pg >= ngroups) pg = kNone;
        pk = pg != kNone ? key[pw & 0xFFFFFFFFull] : 0ull;
      }
    }
    const bool first = g != kNone && (pg != g || pk != k);
    // runs of this row (lane 0 starts one as far as the row is concerned)
    const unsigned long long heads = __ballot(lane == 0 || rg != g);
    const unsigned start = 63u - (unsigned)__clzll(heads & below);
    const unsigned long long run = below & ~((1ull << start) - 1ull);  // lanes start .. lane
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    unsigned cnt = (unsigned)__popcll(__ballot(first) & run);
    // the carried run continues in this row's first run, or is finished
    const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    const bool cont = c_g != kNone && c_g == g0;
    if (c_g != kNone && !cont && lane == 0 && c_cnt) atomicAdd(&out[c_g], (unsigned long long)c_cnt);
    if (cont && start == 0) cnt += c_cnt;
    // runs that end inside the row: written by their last lane
    if (g != kNone && tail && lane < 63 && cnt) atomicAdd(&out[g], (unsigned long long)cnt);
    c_g = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
    c_cnt = (unsigned)__builtin_amdgcn_readlane((int)cnt, 63);
  }
  if (c_g != kNone && lane == 0 && c_cnt) atomicAdd(&out[c_g], (unsigned long long)c_cnt);
}

// key bits of a dtype's image, 0 = unknown dtype
static int nu_key_bits(int dtype) {
  switch (dtype) {
    case NVT_U8: return 8;
    case NVT_I32: case NVT_F32: return 32;
    case NVT_I64: case NVT_F64: return 64;
    default: return 0;
  }
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_seg_nunique_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  // key[n] u64 | gid[n] u32 | sort words[n] u64 | radix sort scratch
  *bytes = 2 * pad256(n * 8) + pad256(n * 4) + sort_words_tmp_bytes(n) + 512;
  return NVT_OK;
}

int nvt_seg_nunique(const uint64_t *words, uint64_t n, uint64_t ngroups, const void *const *vals,
                    const int *vdtypes, const uint8_t *const *val_valid, int ncols, uint64_t *out,
                    void *ws, void *stream) {
  if (n == 0 || ngroups == 0) return NVT_OK;  // (first: the columns of an empty frame have no address)
  NVT_CHECK_ARG(ncols >= 0 && ncols <= kNuMaxCols, "ncols must be 0..8");
  if (ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(words && vals && vdtypes && out && ws, "null pointer");
  NVT_CHECK_ARG(n < (1ull << 30) && ngroups < (1ull << 31), "at most 2^30-1 rows");
  for (int c = 0; c < ncols; ++c) {
    NVT_CHECK_ARG(vals[c], "null value column");
    if (!nu_key_bits(vdtypes[c])) {
      set_error("nvt_seg_nunique: unsupported dtype %d", vdtypes[c]);
      return NVT_EINVAL;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_nunique", 0, s);
  char *p = reinterpret_cast<char *>(ws);
  uint64_t *key = reinterpret_cast<uint64_t *>(p);
  p += pad256(n * 8);
  uint64_t *sort_words = reinterpret_cast<uint64_t *>(p);
  p += pad256(n * 8);
  uint32_t *gid = reinterpret_cast<uint32_t *>(p);
  p += pad256(n * 4);
  void *sort_tmp = p;
  int gid_bits = 1;
  while ((1ull << gid_bits) <= ngroups) ++gid_bits;  // ids 0..ngroups (ngroups = null marker)
  const unsigned grid = stream_grid(n, kBlock * 4);
  const uint32_t ng = (uint32_t)ngroups;
  for (int c = 0; c < ncols; ++c) {
    const uint8_t *valid = val_valid ? val_valid[c] : nullptr;
    switch (vdtypes[c]) {
      case NVT_F32: nu_key_kernel<float><<<grid, kBlock, 0, s>>>(words, (const float *)vals[c], valid, n, ng, key, gid, sort_words); break;
      case NVT_F64: nu_key_kernel<double><<<grid, kBlock, 0, s>>>(words, (const double *)vals[c], valid, n, ng, key, gid, sort_words); break;
      case NVT_I32: nu_key_kernel<int32_t><<<grid, kBlock, 0, s>>>(words, (const int32_t *)vals[c], valid, n, ng, key, gid, sort_words); break;
      case NVT_I64: nu_key_kernel<int64_t><<<grid, kBlock, 0, s>>>(words, (const int64_t *)vals[c], valid, n, ng, key, gid, sort_words); break;
      default: nu_key_kernel<uint8_t><<<grid, kBlock, 0, s>>>(words, (const uint8_t *)vals[c], valid, n, ng, key, gid, sort_words); break;
    }
    NVT_CHECK_LAUNCH();
    const int key_bits = nu_key_bits(vdtypes[c]);
    uint64_t *sorted = nullptr;
    int rc = sort_words_bits(sort_words, n, 32, 32 + (key_bits < 32 ? key_bits : 32), sort_tmp, &sorted, s);
    if (rc) return rc;
    if (key_bits > 32) {
      nu_repack_kernel<<<grid, kBlock, 0, s>>>(sorted, key, nullptr, n, sort_words);
      NVT_CHECK_LAUNCH();
      rc = sort_words_bits(sort_words, n, 32, 64, sort_tmp, &sorted, s);
      if (rc) return rc;
    }
    nu_repack_kernel<<<grid, kBlock, 0, s>>>(sorted, key, gid, n, sort_words);
    NVT_CHECK_LAUNCH();
    rc = sort_words_bits(sort_words, n, 32, 32 + gid_bits, sort_tmp, &sorted, s);
    if (rc) return rc;
    nu_count_kernel<<<stream_grid(n, kBlock * 4, 8), kBlock, 0, s>>>(
        sorted, key, n, ng, reinterpret_cast<unsigned long long *>(out) + (uint64_t)c * ngroups);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
