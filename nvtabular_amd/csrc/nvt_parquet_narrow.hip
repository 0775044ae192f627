// Parquet, flat int8 / int16 / bool columns: the device half of both directions ("Narrow
// and bool columns in the parquet path").
//
//   out: parquet has no 8- or 16-bit physical type -- an int8 / int16 column is an INT32 column whose
//     values are sign-extended (nvt_pq_widen_i32_many: every narrow column of a row group in one
//     launch; behind it the chunk IS an int32 chunk for the dictionary, snappy and statistics
//     code), and a BOOLEAN page holds its non-null values one per bit (nvt_pq_bool_pack: a wave
//     takes 64 values of a page and its ballot is 8 bytes of the page).
//   in: the host decoders stage such chunks as int32 values / one byte per bool, non-null ones only;
//     nvt_expand_narrow gives every row its slot like nvt_expand_valid and narrows on the way.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr int kWidenMaxCols = 32;
struct WidenCol {
  const void *src;
  int32_t *dst;
  uint64_t n;
  int wide;       // the source is int16 (else int8)
  unsigned grid;  // the blocks that share this column
};
struct WidenBatch {
  WidenCol c[kWidenMaxCols];
};

// dst is 4-byte aligned only: the values in front of its first 16-byte boundary and behind the
// last full group of 4 go one by one, the rest as one 16-byte store per lane and trip.  The source
// is read value by value (it is aligned to its element size only) and never outside [src, src + n).
template <typename S>
__device__ __forceinline__ void widen_body(const WidenCol &c) {
  if (blockIdx.x >= c.grid) return;
  const S *__restrict__ src = reinterpret_cast<const S *>(c.src);
  int32_t *__restrict__ dst = c.dst;
  uint64_t head = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / 4;
  if (head > c.n) head = c.n;
  const uint64_t nvec = (c.n - head) / 4;
  const uint64_t stride = (uint64_t)c.grid * kBlock;
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (tid < head) dst[tid] = (int32_t)src[tid];
  typedef int v4i __attribute__((ext_vector_type(4)));
  for (uint64_t i = tid; i < nvec; i += stride) {
    const S *p = src + head + i * 4;
    v4i o;
    o.x = (int32_t)p[0];
    o.y = (int32_t)p[1];
    o.z = (int32_t)p[2];
    o.w = (int32_t)p[3];
    *reinterpret_cast<v4i *>(dst + head + i * 4) = o;
  }
  for (uint64_t i = head + nvec * 4 + tid; i < c.n; i += stride) dst[i] = (int32_t)src[i];
}

__global__ __launch_bounds__(kBlock) void widen_many_kernel(WidenBatch b) {
  const WidenCol &c = b.c[blockIdx.y];
  if (c.wide)
    widen_body<int16_t>(c);
  else
    widen_body<int8_t>(c);
}

// Page p = blockIdx.y (+ k gridDim.y): its values [page_start[p], page_start[p + 1]) are taken 64 at
// a time by the waves of the gridDim.x blocks; the ballot of "value != 0" is the 8 bytes the group
// owns in the page, written by lanes 0 .. 7 one byte each (a page starts at ANY byte of `out`).  A
// lane behind the page's last value votes 0: the tail bits of the last byte are 0.
constexpr unsigned kPackBlocks = 64;
__global__ __launch_bounds__(kBlock) void bool_pack_kernel(const uint8_t *__restrict__ vals,
                                                           const int64_t *__restrict__ page_start,
                                                           const int64_t *__restrict__ byte_at, uint64_t npages,
                                                           uint8_t *__restrict__ out) {
  const unsigned lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / kWave);
  for (uint64_t p = blockIdx.y; p < npages; p += gridDim.y) {
    const int64_t lo = page_start[p], hi = page_start[p + 1];
    if (hi <= lo) continue;  // (uniform)
    const uint64_t cnt = (uint64_t)(hi - lo);
    const uint8_t *src = vals + lo;
    uint8_t *dst = out + byte_at[p];
    const uint64_t nbytes = (cnt + 7) / 8;
    for (uint64_t g = wave; g * 64 < cnt; g += nwaves) {  // (uniform per wave)
      const uint64_t i = g * 64 + lane;
      const bool one = i < cnt && src[i] != 0;
      const uint64_t bits = __ballot(one);
      const uint64_t at = g * 8 + lane;
      if (lane < 8 && at < nbytes) dst[at] = (uint8_t)(bits >> (8 * lane));
    }
  }
}

// valid rows in the 4096 rows (64 bitmap words) of every wave-tile
constexpr int kTileRows = 64 * 64;
__global__ __launch_bounds__(kBlock) void narrow_count_kernel(const uint64_t *__restrict__ bitmap, uint64_t n,
                                                              unsigned *__restrict__ tile_cnt, uint64_t ntiles) {
  const unsigned lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (wave >= ntiles) return;
  const uint64_t nwords = (n + 63) / 64;
  const uint64_t wi = wave * 64 + lane;
  uint64_t word = wi < nwords ? bitmap[wi] : 0ull;
  const uint64_t row0 = wi * 64;
  if (row0 + 64 > n) word &= row0 >= n ? 0ull : ((1ull << (n - row0)) - 1ull);  // bits behind the column
  unsigned pc = (unsigned)__popcll(word);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pc += __shfl_down(pc, off, 64);
  if (lane == 0) tile_cnt[wave] = pc;
}

// out[i] = bit i ? (D) packed[valid rows in front of i] : 0.  The walk of nvt_expand_valid: lane l
// owns bitmap word l of the wave's 64 for the rank prefix, then the wave goes through the words,
// lane r writing row 64 w + r.
template <typename S, typename D>
__global__ __launch_bounds__(kBlock) void expand_narrow_kernel(const S *__restrict__ packed,
                                                               const uint64_t *__restrict__ bitmap, uint64_t n,
                                                               const unsigned *__restrict__ tile_base,
                                                               D *__restrict__ out) {
  const unsigned lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  const uint64_t nwords = (n + 63) / 64;
  const uint64_t w0 = wave * 64;
  if (w0 >= nwords) return;
  uint64_t word = (w0 + lane < nwords) ? bitmap[w0 + lane] : 0ull;
  const uint64_t row0 = (w0 + lane) * 64;
  if (row0 + 64 > n) word &= row0 >= n ? 0ull : ((1ull << (n - row0)) - 1ull);
  const unsigned pc = (unsigned)__popcll(word);
  unsigned inc = pc;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += o;
  }
  const uint64_t wbase = (uint64_t)tile_base[wave] + inc - pc;
  for (int w = 0; w < 64; ++w) {
    if (w0 + w >= nwords) break;  // (uniform)
    const uint64_t bits = __shfl(word, w, 64);
    const uint64_t base = __shfl(wbase, w, 64);
    const uint64_t row = (w0 + w) * 64 + lane;
    if (row < n) {
      const bool v = (bits >> lane) & 1ull;
      const uint64_t rank = base + (uint64_t)__popcll(bits & ((1ull << lane) - 1ull));
      out[row] = v ? static_cast<D>(packed[rank]) : (D)0;
    }
  }
}

// no bitmap: the pure narrowing copy
template <typename S, typename D>
__global__ __launch_bounds__(kBlock) void narrow_copy_kernel(const S *__restrict__ packed, uint64_t n,
                                                             D *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    out[i] = static_cast<D>(packed[i]);
}

template <typename S, typename D>
int expand_narrow_launch(const void *packed, const uint64_t *bm, uint64_t n, void *out, void *ws, hipStream_t s) {
  if (bm == nullptr) {
    narrow_copy_kernel<S, D><<<stream_grid(n, kBlock * 4), kBlock, 0, s>>>((const S *)packed, n, (D *)out);
    NVT_CHECK_LAUNCH();
    return NVT_OK;
  }
  const uint64_t ntiles = (n + kTileRows - 1) / kTileRows;
  unsigned *tile = reinterpret_cast<unsigned *>(ws);
  unsigned long long *chunk_tot =
      reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ws) + ((ntiles * 4 + 255) & ~255ull));
  const unsigned grid = (unsigned)((ntiles + (kBlock / kWave) - 1) / (kBlock / kWave));
  narrow_count_kernel<<<grid, kBlock, 0, s>>>(bm, n, tile, ntiles);
  NVT_CHECK_LAUNCH();
  const int rc = exclusive_scan_u32(tile, ntiles, chunk_tot, s);
  if (rc) return rc;
  expand_narrow_kernel<S, D><<<grid, kBlock, 0, s>>>((const S *)packed, bm, n, tile, (D *)out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_widen_i32_many(const nvt_pq_widen_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  for (int i = 0; i < ncols; ++i) {   // every descriptor is checked before the first launch
    const nvt_pq_widen_col &c = cols[i];
    NVT_CHECK_ARG(c.src_dtype == NVT_I8 || c.src_dtype == NVT_I16, "src_dtype is NVT_I8 or NVT_I16");
    NVT_CHECK_ARG(c.n == 0 || (c.src && c.dst), "null src/dst");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.src) & (c.src_dtype == NVT_I16 ? 1 : 0)) == 0 &&
                      (reinterpret_cast<uintptr_t>(c.dst) & 3) == 0,
                  "src/dst must be aligned to their element size");
  }
  hipStream_t s = (hipStream_t)stream;
  for (int c0 = 0; c0 < ncols; c0 += kWidenMaxCols) {
    const int nc = ncols - c0 < kWidenMaxCols ? ncols - c0 : kWidenMaxCols;
    WidenBatch b;
    memset(&b, 0, sizeof(b));
    unsigned grid = 1;
    uint64_t bytes = 0;
    int live = 0;
    for (int i = 0; i < nc; ++i) {
      const nvt_pq_widen_col &c = cols[c0 + i];
      if (c.n == 0) continue;
      WidenCol &m = b.c[live++];
      m.src = c.src;
      m.dst = c.dst;
      m.n = c.n;
      m.wide = c.src_dtype == NVT_I16;
      m.grid = stream_grid(c.n / 4 + 1, kBlock * 2, 8);
      grid = m.grid > grid ? m.grid : grid;
      bytes += c.n * (uint64_t)(4 + (m.wide ? 2 : 1));
    }
    if (!live) continue;
    NVT_PROF("pq_widen", bytes, s);
    widen_many_kernel<<<dim3(grid, live), kBlock, 0, s>>>(b);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_pq_bool_pack(const uint8_t *vals, const int64_t *page_start, const int64_t *byte_at, uint64_t npages,
                     uint8_t *out, void *stream) {
  if (npages == 0) return NVT_OK;
  NVT_CHECK_ARG(page_start && byte_at, "null page table");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(page_start) & 7) == 0 && (reinterpret_cast<uintptr_t>(byte_at) & 7) == 0,
                "page tables must be 8-byte aligned");
  NVT_CHECK_ARG(vals && out, "null vals/out");
  NVT_CHECK_ARG(npages < (1ull << 31), "fewer than 2^31 pages");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_bool_pack", 0, s);
  const unsigned gy = (unsigned)(npages < 1024 ? npages : 1024);
  bool_pack_kernel<<<dim3(kPackBlocks, gy), kBlock, 0, s>>>(vals, page_start, byte_at, npages, out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_expand_narrow(const void *packed, int src_size, int dst_size, const uint8_t *bitmap, uint64_t n, void *out,
                      void *ws, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG((src_size == 4 && (dst_size == 1 || dst_size == 2)) || (src_size == 1 && dst_size == 1),
                "sizes are 4 -> 1, 4 -> 2 or 1 -> 1");
  NVT_CHECK_ARG(out && (bitmap == nullptr || ws), "null pointer");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(bitmap) & 7) == 0, "bitmap must be 8-byte aligned");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & (uintptr_t)(src_size - 1)) == 0 &&
                    (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(dst_size - 1)) == 0,
                "packed/out must be aligned to their element size");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "ws must be 8-byte aligned");
  NVT_CHECK_ARG(n < (1ull << 32), "fewer than 2^32 rows");
  NVT_CHECK_ARG(packed || bitmap, "null packed values without a bitmap");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("parquet_expand_narrow", n * (uint64_t)dst_size, s);
  const uint64_t *bm = reinterpret_cast<const uint64_t *>(bitmap);
  if (src_size == 1) return expand_narrow_launch<uint8_t, uint8_t>(packed, bm, n, out, ws, s);
  if (dst_size == 1) return expand_narrow_launch<int32_t, int8_t>(packed, bm, n, out, ws, s);
  return expand_narrow_launch<int32_t, int16_t>(packed, bm, n, out, ws, s);
}

}  // extern "C"
