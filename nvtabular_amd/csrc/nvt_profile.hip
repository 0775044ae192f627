// Column profile and narrowing casts: ops.DataStats / ops.ReduceDtypeSize.
//
// nvt_col_profile_many: rows, valid rows, min, max, sum and sum of squares of every column of a
// partition in ONE read of the column (blockIdx.y = column, per-block partials, one small final
// launch; no atomics, so a result does not depend on scheduling).  It keeps the grid and the
// row-to-lane mapping of moments_many_kernel (nvt_cont.hip): a pure stream, 4 independent 16-byte
// loads in flight per lane.  Min / max are taken on an order-preserving signed integer key of the
// value's own width, so int64 never passes through a double and -0.0 < +0.0 is decided the same way
// wherever the zeros sit.
// nvt_cast_many: int32 / int64 -> int8 / int16 / int32 and float64 -> float32, one launch for all
// columns; a lane reads the 32 .. 128 contiguous input bytes of one 16-byte store.
//
// Reference: data_stats.py:52-92, reduce_dtype_size.py:40-56.
#include <limits>
#include <type_traits>

#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr int kMaxCols = NVT_PROFILE_MAX_COLS;
constexpr unsigned kMaxGrid = 1024;  // stream_grid(.., .., 4): the widest launch
constexpr int kSlots = 5;            // partial rows: valid rows, min key, max key, sum, sum of squares
static_assert((uint64_t)kMaxCols * kSlots * kMaxGrid * 8 == NVT_PROFILE_SCRATCH_BYTES, "scratch size");

// 16 bytes of a column.  A16: the address is 16-byte aligned (non-temporal, as load_vec of
// nvt_cont.hip); otherwise only as aligned as T and the compiler picks the widest legal load.
template <typename T, bool A16>
__device__ __forceinline__ void load16(const T *p, T (&v)[16 / sizeof(T)]) {
  if constexpr (A16) {
    typedef int v4i_ntl __attribute__((ext_vector_type(4)));
    v4i_ntl raw = __builtin_nontemporal_load(reinterpret_cast<const v4i_ntl *>(p));
    memcpy(v, &raw, 16);
  } else {
    memcpy(v, p, 16);
  }
}

// Order-preserving signed key of a value, of the value's own width: integers as they are, floats
// with the magnitude bits of a negative value flipped (an involution: the sign bit stays).
__device__ __forceinline__ int32_t flip32(int32_t b) { return b ^ ((b >> 31) & 0x7FFFFFFF); }
__device__ __forceinline__ long long flip64(long long b) { return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll); }
__device__ __forceinline__ int32_t ord_key(int32_t v) { return v; }
__device__ __forceinline__ long long ord_key(int64_t v) { return (long long)v; }
__device__ __forceinline__ int32_t ord_key(float v) { return flip32(__float_as_int(v)); }
__device__ __forceinline__ long long ord_key(double v) { return flip64(__double_as_longlong(v)); }

// The five partial rows are combined by one function: 0 integer sum, 1 signed min, 2 signed max,
// 3 / 4 float64 sum (bits carried in the same 64-bit slots).
typedef unsigned long long slot_t;
__device__ __forceinline__ slot_t slot_neutral(int q) {
  return q == 1 ? (slot_t)INT64_MAX : q == 2 ? (slot_t)INT64_MIN : 0ull;
}
__device__ __forceinline__ slot_t slot_comb(int q, slot_t a, slot_t b) {
  switch (q) {
    case 0: return a + b;
    case 1: return (long long)b < (long long)a ? b : a;
    case 2: return (long long)b > (long long)a ? b : a;
    default: return (slot_t)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
  }
}
__device__ __forceinline__ slot_t slot_wave(int q, slot_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = slot_comb(q, v, __shfl_down(v, off, 64));
  return v;
}

struct ProfCol {
  const void *x;
  const uint8_t *valid;
  uint64_t n;
  long long *counts;
  void *extrema;
  double *sums;
  int dtype;
  unsigned grid;  // the blocks that share this column (its own stream_grid)
};
struct ProfBatch {
  ProfCol c[kMaxCols];
};

template <typename T, bool A16>
__device__ __forceinline__ void profile_body(const ProfCol &c, slot_t *__restrict__ partials,
                                             slot_t (*red)[kBlock / kWave]) {
  // (the blocks past the column's own grid add neutral elements: what a block reads, and the
  // result, do not depend on what else is in the batch)
  const unsigned nblk = c.grid;
  if (blockIdx.x >= nblk) {
    if (threadIdx.x < kSlots) partials[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = slot_neutral(threadIdx.x);
    return;
  }
  const T *__restrict__ x = reinterpret_cast<const T *>(c.x);
  const uint8_t *__restrict__ valid = c.valid;
  const uint64_t n = c.n;
  constexpr int VEC = 16 / sizeof(T);
  using KeyT = decltype(ord_key(T()));
  KeyT mn = std::numeric_limits<KeyT>::max(), mx = std::numeric_limits<KeyT>::min();
  unsigned long long cnt = 0;
  double sum = 0, sq = 0;
  auto acc = [&](T raw, bool ok) {
    if (!ok || is_nan(raw)) return;
    const KeyT k = ord_key(raw);
    mn = k < mn ? k : mn;
    mx = k > mx ? k : mx;
    const double v = (double)raw;
    cnt += 1;
    sum += v;
    sq += v * v;
  };
  const uint64_t nvec = n / VEC;
  const uint64_t stride = (uint64_t)nblk * kBlock;
  constexpr int U = 4;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i0 < nvec; i0 += stride * U) {
    T v[U][VEC];
    unsigned vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = i0 + (uint64_t)u * stride;
      vb[u] = 0;
      if (i < nvec) {
        load16<T, A16>(x + i * VEC, v[u]);
        // (row i * VEC is a multiple of VEC = 2 or 4: its VEC bits sit in one byte)
        vb[u] = 0x100u | (valid != nullptr ? (unsigned)valid[(i * VEC) >> 3] : 0xFFu);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!vb[u]) continue;
      const uint64_t row = (i0 + (uint64_t)u * stride) * VEC;
      const unsigned vbits = (vb[u] & 0xFFu) >> (row & 7);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc(v[u][j], (vbits >> j) & 1);
    }
  }
  for (uint64_t i = nvec * VEC + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    acc(x[i], bit_valid(valid, i));

  // a lane that saw no row holds the limits of its OWN key width: widen to the 64-bit markers
  slot_t part[kSlots] = {cnt, cnt ? (slot_t)(long long)mn : slot_neutral(1),
                         cnt ? (slot_t)(long long)mx : slot_neutral(2),
                         (slot_t)__double_as_longlong(sum), (slot_t)__double_as_longlong(sq)};
  const unsigned w = threadIdx.x / kWave;
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    const slot_t t = slot_wave(q, part[q]);
    if (lane_id() == 0) red[q][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < kSlots) {
    const int q = threadIdx.x;
    slot_t t = slot_neutral(q);
    for (int k = 0; k < kBlock / kWave; ++k) t = slot_comb(q, t, red[q][k]);
    partials[(uint64_t)q * gridDim.x + blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kBlock) void col_profile_many_kernel(ProfBatch b, slot_t *partials) {
  const ProfCol &c = b.c[blockIdx.y];
  slot_t *p = partials + (uint64_t)blockIdx.y * kSlots * gridDim.x;
  __shared__ slot_t red[kSlots][kBlock / kWave];
  const bool a16 = (reinterpret_cast<uintptr_t>(c.x) & 15) == 0;   // (block-uniform)
#define NVT_PROFILE_BODY(T)                    \
  do {                                         \
    if (a16)                                   \
      profile_body<T, true>(c, p, red);        \
    else                                       \
      profile_body<T, false>(c, p, red);       \
  } while (0)
  switch (c.dtype) {
    case NVT_F32: NVT_PROFILE_BODY(float); break;
    case NVT_F64: NVT_PROFILE_BODY(double); break;
    case NVT_I32: NVT_PROFILE_BODY(int32_t); break;
    default: NVT_PROFILE_BODY(int64_t); break;
  }
#undef NVT_PROFILE_BODY
}

// one workgroup per column: the partial rows in a fixed order, then the fold into the caller's
// accumulators
__global__ __launch_bounds__(kBlock) void col_profile_final_kernel(ProfBatch b, const slot_t *__restrict__ partials,
                                                                   unsigned nblocks) {
  const ProfCol &c = b.c[blockIdx.x];
  const slot_t *p = partials + (uint64_t)blockIdx.x * kSlots * nblocks;
  __shared__ slot_t red[kBlock / kWave];
  slot_t tot[kSlots];
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    slot_t t = slot_neutral(q);
    for (unsigned i = threadIdx.x; i < nblocks; i += kBlock) t = slot_comb(q, t, p[(uint64_t)q * nblocks + i]);
    t = slot_wave(q, t);
    if (lane_id() == 0) red[threadIdx.x / kWave] = t;
    __syncthreads();
    tot[q] = slot_neutral(q);
    for (int k = 0; k < kBlock / kWave; ++k) tot[q] = slot_comb(q, tot[q], red[k]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  c.counts[0] += (long long)c.n;
  c.counts[1] += (long long)tot[0];
  c.sums[0] += __longlong_as_double((long long)tot[3]);
  c.sums[1] += __longlong_as_double((long long)tot[4]);
  if (tot[0] == 0) return;   // no valid row: the extrema stay as they are
  long long kmn = (long long)tot[1], kmx = (long long)tot[2];
  if (c.dtype == NVT_I32 || c.dtype == NVT_I64) {
    long long *e = reinterpret_cast<long long *>(c.extrema);
    e[0] = kmn < e[0] ? kmn : e[0];
    e[1] = kmx > e[1] ? kmx : e[1];
    return;
  }
  if (c.dtype == NVT_F32) {   // the float's key -> the key of the same value as a double
    kmn = ord_key((double)__int_as_float(flip32((int32_t)kmn)));
    kmx = ord_key((double)__int_as_float(flip32((int32_t)kmx)));
  }
  double *e = reinterpret_cast<double *>(c.extrema);
  const double pmn = e[0], pmx = e[1];   // NaN = nothing folded in yet
  if (pmn == pmn && ord_key(pmn) < kmn) kmn = ord_key(pmn);
  if (pmx == pmx && ord_key(pmx) > kmx) kmx = ord_key(pmx);
  e[0] = __longlong_as_double(flip64(kmn));
  e[1] = __longlong_as_double(flip64(kmx));
}

// ---- narrowing casts ------------------------------------------------------------------------------
struct CastCol {
  const void *src;
  void *dst;
  uint64_t n;
  int pair;       // CastPair
  unsigned grid;  // the blocks that share this column
};
struct CastBatch {
  CastCol c[kMaxCols];
};
enum CastPair { kI32I8, kI32I16, kI64I8, kI64I16, kI64I32, kF64F32, kNoPair };

inline int cast_pair(int src, int dst) {
  if (src == NVT_I32) return dst == NVT_I8 ? kI32I8 : dst == NVT_I16 ? kI32I16 : kNoPair;
  if (src == NVT_I64) return dst == NVT_I8 ? kI64I8 : dst == NVT_I16 ? kI64I16 : dst == NVT_I32 ? kI64I32 : kNoPair;
  if (src == NVT_F64) return dst == NVT_F32 ? kF64F32 : kNoPair;
  return kNoPair;
}
inline int cast_src_bytes(int pair) { return pair == kI32I8 || pair == kI32I16 ? 4 : 8; }
inline int cast_dst_bytes(int pair) { return pair == kI32I8 || pair == kI64I8 ? 1 : pair == kI64I32 || pair == kF64F32 ? 4 : 2; }

// static_cast is the whole conversion: an integer keeps its low bits (two's complement wrap, what
// numpy's astype does), a double is rounded to the nearest float, ties to even, overflow to +-inf.
template <typename S, typename D, bool A16>
__device__ __forceinline__ void cast_body(const CastCol &c) {
  if (blockIdx.x >= c.grid) return;
  const S *__restrict__ src = reinterpret_cast<const S *>(c.src);
  D *__restrict__ dst = reinterpret_cast<D *>(c.dst);
  constexpr int NOUT = 16 / sizeof(D);   // values of one 16-byte store
  constexpr int SV = 16 / sizeof(S);     // values of one 16-byte load
  constexpr int NLD = NOUT / SV;
  // (16-byte stores need a 16-byte aligned output: otherwise every value goes the scalar way)
  const uint64_t nvec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 ? c.n / NOUT : 0;
  const uint64_t stride = (uint64_t)c.grid * kBlock;
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  for (uint64_t i = tid; i < nvec; i += stride) {
    S v[NLD][SV];
#pragma unroll
    for (int l = 0; l < NLD; ++l) load16<S, A16>(src + i * NOUT + l * SV, v[l]);
    D o[NOUT];
#pragma unroll
    for (int l = 0; l < NLD; ++l)
#pragma unroll
      for (int j = 0; j < SV; ++j) o[l * SV + j] = static_cast<D>(v[l][j]);
    typedef int v4i __attribute__((ext_vector_type(4)));
    v4i raw;
    memcpy(&raw, o, 16);
    *reinterpret_cast<v4i *>(dst + i * NOUT) = raw;
  }
  for (uint64_t i = nvec * NOUT + tid; i < c.n; i += stride) dst[i] = static_cast<D>(src[i]);
}

__global__ __launch_bounds__(kBlock) void cast_many_kernel(CastBatch b) {
  const CastCol &c = b.c[blockIdx.y];
  const bool a16 = (reinterpret_cast<uintptr_t>(c.src) & 15) == 0;   // (block-uniform)
#define NVT_CAST_BODY(S, D)          \
  do {                               \
    if (a16)                         \
      cast_body<S, D, true>(c);      \
    else                             \
      cast_body<S, D, false>(c);     \
  } while (0)
  switch (c.pair) {
    case kI32I8: NVT_CAST_BODY(int32_t, int8_t); break;
    case kI32I16: NVT_CAST_BODY(int32_t, int16_t); break;
    case kI64I8: NVT_CAST_BODY(int64_t, int8_t); break;
    case kI64I16: NVT_CAST_BODY(int64_t, int16_t); break;
    case kI64I32: NVT_CAST_BODY(int64_t, int32_t); break;
    default: NVT_CAST_BODY(double, float); break;
  }
#undef NVT_CAST_BODY
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_col_profile_many(const nvt_profile_col *cols, int ncols, void *partials, void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  NVT_CHECK_ARG(partials && (reinterpret_cast<uintptr_t>(partials) & 7) == 0, "null or misaligned partials");
  // every descriptor is checked before the first launch
  for (int i = 0; i < ncols; ++i) {
    const nvt_profile_col &c = cols[i];
    NVT_CHECK_ARG(c.dtype == NVT_F32 || c.dtype == NVT_F64 || c.dtype == NVT_I32 || c.dtype == NVT_I64,
                  "unsupported dtype");
    NVT_CHECK_ARG(c.counts && c.extrema && c.sums, "null accumulator");
    const uintptr_t esz = c.dtype == NVT_F32 || c.dtype == NVT_I32 ? 4 : 8;
    NVT_CHECK_ARG(c.n == 0 || (c.x && (reinterpret_cast<uintptr_t>(c.x) & (esz - 1)) == 0),
                  "x must be non-null and aligned to its element size");
  }
  hipStream_t s = (hipStream_t)stream;
  slot_t *p = reinterpret_cast<slot_t *>(partials);
  for (int c0 = 0; c0 < ncols; c0 += kMaxCols) {   // (the batches run in stream order: one scratch block)
    const int nc = ncols - c0 < kMaxCols ? ncols - c0 : kMaxCols;
    ProfBatch b;
    memset(&b, 0, sizeof(b));
    unsigned grid = 1;
    uint64_t bytes = 0;
    int live = 0;
    for (int i = 0; i < nc; ++i) {
      const nvt_profile_col &c = cols[c0 + i];
      if (c.n == 0) continue;
      const uint64_t esz = c.dtype == NVT_F32 || c.dtype == NVT_I32 ? 4 : 8;
      ProfCol &m = b.c[live++];
      m.x = c.x;
      m.valid = c.valid;
      m.n = c.n;
      m.counts = reinterpret_cast<long long *>(c.counts);
      m.extrema = c.extrema;
      m.sums = c.sums;
      m.dtype = c.dtype;
      m.grid = stream_grid(c.n / (16 / esz) + 1, kBlock * 4, 4);
      grid = m.grid > grid ? m.grid : grid;
      bytes += c.n * esz;
    }
    if (!live) continue;
    NVT_PROF("col_profile", bytes, s);
    col_profile_many_kernel<<<dim3(grid, live), kBlock, 0, s>>>(b, p);
    NVT_CHECK_LAUNCH();
    col_profile_final_kernel<<<live, kBlock, 0, s>>>(b, p, grid);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_cast_many(const nvt_cast_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  for (int i = 0; i < ncols; ++i) {
    const nvt_cast_col &c = cols[i];
    const int pair = cast_pair(c.src_dtype, c.dst_dtype);
    NVT_CHECK_ARG(pair != kNoPair,
                  "unsupported cast: int32 -> int8/int16, int64 -> int8/int16/int32 and float64 -> float32 only");
    NVT_CHECK_ARG(c.n == 0 || (c.src && c.dst), "null src/dst");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.src) & (cast_src_bytes(pair) - 1)) == 0 &&
                      (reinterpret_cast<uintptr_t>(c.dst) & (cast_dst_bytes(pair) - 1)) == 0,
                  "src/dst must be aligned to their element size");
  }
  hipStream_t s = (hipStream_t)stream;
  for (int c0 = 0; c0 < ncols; c0 += kMaxCols) {
    const int nc = ncols - c0 < kMaxCols ? ncols - c0 : kMaxCols;
    CastBatch b;
    memset(&b, 0, sizeof(b));
    unsigned grid = 1;
    uint64_t bytes = 0;
    int live = 0;
    for (int i = 0; i < nc; ++i) {
      const nvt_cast_col &c = cols[c0 + i];
      if (c.n == 0) continue;
      CastCol &m = b.c[live++];
      m.src = c.src;
      m.dst = c.dst;
      m.n = c.n;
      m.pair = cast_pair(c.src_dtype, c.dst_dtype);
      // one 16-byte store per lane and trip
      m.grid = stream_grid(c.n / (16 / cast_dst_bytes(m.pair)) + 1, kBlock * 2, 8);
      grid = m.grid > grid ? m.grid : grid;
      bytes += c.n * (uint64_t)(cast_src_bytes(m.pair) + cast_dst_bytes(m.pair));
    }
    if (!live) continue;
    NVT_PROF("cast", bytes, s);
    cast_many_kernel<<<dim3(grid, live), kBlock, 0, s>>>(b);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
