// Session features on list columns (ops.ListSlice / ops.ValueCount) and ops.DifferenceLag.
//
// ListSlice: row i of the output is row[start:end] of the input, as Python slices it.
//   1. slice_len_kernel: per 2048-row tile the sliced lengths, scanned inside the tile (written to
//      out_offsets as tile-local exclusive prefixes) and the tile's total (uint64);
//      scan_totals_kernel (nvt_scan.hpp) scans the totals; slice_add_kernel adds the tile bases and
//      writes out_offsets[n] = the number of output leaves.  Everything is 64 bits wide: a column
//      may hold more than 2^32 leaves.  (pad = true needs none of this: row i starts at i * width.)
//   2. slice_move_kernel: work is distributed over OUTPUT leaves in tiles of 2048, one leaf per lane
//      and round, so stores are coalesced and a row of ten million leaves beside a million empty
//      rows costs what a uniform frame costs.  The row of a leaf is a division (pad) or a search in
//      the new offsets: two lanes find the first and the last row of the tile in global memory, the
//      rows between them are staged in LDS and every lane searches there (a tile that spans more
//      than kStage rows -- long runs of empty rows -- searches global memory between the two
//      bounds instead).  Row and source position are found once per leaf and used for every column
//      of the batch; a wave's 64 leaves make one validity word (__ballot), stored whole.
// ValueCount: len_minmax_kernel folds min / max of offsets[i + 1] - offsets[i] into int64[2].
// DifferenceLag: lag_kernel, one lane per row, every (column, shift) output of the batch.
#include "nvt_common.hpp"
#include "nvt_list_tile.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr uint64_t kTile = kListTile;       // rows (lengths) or output leaves (move) per tile
constexpr int kStage = kListStage;          // new offsets of one tile's rows held in LDS
constexpr int kMaxCols = NVT_LIST_MAX_COLS;
constexpr int kMaxKeys = NVT_LAG_MAX_KEYS;

__host__ __device__ inline uint64_t ntiles_of(uint64_t n) { return list_ntiles(n); }

struct Slice {
  int64_t start, end;
};

// row[start:end] of a row of L leaves: first kept leaf and their number
__device__ __forceinline__ void slice_row(const Slice &s, int64_t L, int64_t &first, int64_t &cnt) {
  int64_t a = s.start < 0 ? (L + s.start > 0 ? L + s.start : 0) : (s.start < L ? s.start : L);
  int64_t e = s.end < 0 ? (L + s.end > 0 ? L + s.end : 0) : (s.end < L ? s.end : L);
  first = a;
  cnt = e > a ? e - a : 0;
}

// ---- new offsets --------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void slice_len_kernel(const int64_t *__restrict__ off, uint64_t n, Slice s,
                                                           int64_t *__restrict__ out,
                                                           unsigned long long *__restrict__ tile_tot) {
  __shared__ uint64_t wsum[kBlock / kWave];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  const uint64_t nt = ntiles_of(n);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r0 = t * kTile + (uint64_t)threadIdx.x * 8;  // 8 consecutive rows per lane
    uint64_t len[8], tot = 0;
    int64_t prev = r0 < n ? off[r0] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      len[j] = 0;
      if (r0 + j < n) {
        const int64_t next = off[r0 + j + 1];
        int64_t first, cnt;
        slice_row(s, next - prev, first, cnt);
        len[j] = (uint64_t)cnt;
        prev = next;
      }
      tot += len[j];
    }
    const uint64_t inc = wave_incl_scan(tot);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t run = inc - tot;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (r0 + j < n) out[r0 + j] = (int64_t)run;
      run += len[j];
    }
    if (threadIdx.x == kBlock - 1) tile_tot[t] = run;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void slice_add_kernel(int64_t *__restrict__ out, uint64_t n,
                                                           const unsigned long long *__restrict__ tile_base,
                                                           const int64_t *__restrict__ off, Slice s) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const int64_t v = out[i] + (int64_t)tile_base[i / kTile];
    out[i] = v;
    if (i == n - 1) {  // out[n] = the start of the last row + its sliced length
      int64_t first, cnt;
      slice_row(s, off[n] - off[n - 1], first, cnt);
      out[n] = v + cnt;
    }
  }
}

// ---- leaves -------------------------------------------------------------------------------------
struct LCol {
  const void *src;
  void *dst;
  const uint8_t *src_valid;
  uint64_t *dst_valid;
  uint64_t pad_bits;
  int width, pad_;
};
struct LBatch {
  LCol c[kMaxCols];
  int ncols;
};

template <bool PAD>
__global__ __launch_bounds__(kBlock) void slice_move_kernel(LBatch b, const int64_t *__restrict__ off, uint64_t n,
                                                            Slice s, const int64_t *__restrict__ noff,
                                                            uint64_t total, uint64_t width, int small) {
  __shared__ int64_t soff[kStage];
  __shared__ uint64_t sbound[2];
  const unsigned lane = lane_id();
  const int64_t o0 = off[0];
  const uint64_t nt = ntiles_of(total);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t p0 = t * kTile;
    const uint64_t p1 = p0 + kTile < total ? p0 + kTile : total;
    uint64_t rlo = 0, rhi = 0;
    bool staged = false;
    if (!PAD) {
      if (threadIdx.x < 2)
        sbound[threadIdx.x] = row_of(noff, 0, n - 1, (int64_t)(threadIdx.x == 0 ? p0 : p1 - 1));
      __syncthreads();
      rlo = sbound[0];
      rhi = sbound[1];
      staged = rhi - rlo + 2 <= (uint64_t)kStage;  // (block-uniform)
      if (staged)
        for (uint64_t k = threadIdx.x; k < rhi - rlo + 2; k += kBlock) soff[k] = noff[rlo + k];
      __syncthreads();
    }
    for (uint64_t q = p0 + threadIdx.x; q < p0 + kTile; q += kBlock) {  // (q - lane is a multiple of 64)
      const bool live = q < p1;
      uint64_t row = 0, k = 0;
      if (live) {
        if (PAD) {
          if (small) {
            row = (unsigned)q / (unsigned)width;
            k = (unsigned)q - (unsigned)row * (unsigned)width;
          } else {
            row = q / width;
            k = q - row * width;
          }
        } else if (staged) {
          const uint64_t j = row_of(soff, 0, rhi - rlo, (int64_t)q);
          row = rlo + j;
          k = q - (uint64_t)soff[j];
        } else {
          row = row_of(noff, rlo, rhi, (int64_t)q);
          k = q - (uint64_t)noff[row];
        }
      }
      bool take = false;
      uint64_t si = 0;
      if (live) {
        const int64_t a = off[row];
        int64_t first, cnt;
        slice_row(s, off[row + 1] - a, first, cnt);
        take = (int64_t)k < cnt;  // (pad = false: always)
        si = (uint64_t)(a - o0 + first) + k;
      }
      for (int ci = 0; ci < b.ncols; ++ci) {
        const LCol &c = b.c[ci];
        if (live) {
          if (c.width == 8)
            ((uint64_t *)c.dst)[q] = take ? ((const uint64_t *)c.src)[si] : c.pad_bits;
          else if (c.width == 4)
            ((uint32_t *)c.dst)[q] = take ? ((const uint32_t *)c.src)[si] : (uint32_t)c.pad_bits;
          else
            ((uint8_t *)c.dst)[q] = take ? ((const uint8_t *)c.src)[si] : (uint8_t)c.pad_bits;
        }
        if (c.dst_valid != nullptr) {  // (block-uniform: every lane of the wave reaches the ballot)
          const bool ok = live && (!take || bit_valid(c.src_valid, si));
          const uint64_t word = __ballot(ok);
          if (lane == 0 && q < p1) c.dst_valid[q >> 6] = word;
        }
      }
    }
    __syncthreads();
  }
}

// ---- ValueCount -----------------------------------------------------------------------------------
struct MCol {
  const int64_t *off;
  uint64_t n;
  long long *acc;
};
struct MBatch {
  MCol c[kMaxCols];
};

__global__ __launch_bounds__(kBlock) void len_minmax_kernel(MBatch b) {
  const MCol c = b.c[blockIdx.y];
  __shared__ long long smin[kBlock / kWave], smax[kBlock / kWave];
  long long mn = INT64_MAX, mx = INT64_MIN;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < c.n; i += (uint64_t)gridDim.x * kBlock) {
    const long long d = c.off[i + 1] - c.off[i];
    mn = d < mn ? d : mn;
    mx = d > mx ? d : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long a = __shfl_xor(mn, o, 64), z = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = z > mx ? z : mx;
  }
  if (lane_id() == 0) {
    smin[threadIdx.x / kWave] = mn;
    smax[threadIdx.x / kWave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBlock / kWave; ++k) {
      mn = smin[k] < mn ? smin[k] : mn;
      mx = smax[k] > mx ? smax[k] : mx;
    }
    if (mn <= mx) {  // (a block that saw no row has nothing to add)
      atomicMin(&c.acc[0], mn);
      atomicMax(&c.acc[1], mx);
    }
  }
}

// ---- DifferenceLag --------------------------------------------------------------------------------
struct GKey {
  const void *x;
  const uint8_t *valid;
  int dtype, pad_;
};
struct GCol {
  const void *x;
  const uint8_t *valid;
  float *out;
  int64_t shift;
  int dtype, pad_;
};
struct GBatch {
  GKey k[kMaxKeys];
  GCol c[kMaxCols];
  int nkeys, ncols;
};

// partition column `k` is non-null and equal at rows i and j
__device__ __forceinline__ bool key_same(const GKey &k, uint64_t i, uint64_t j) {
  if (!bit_valid(k.valid, i) || !bit_valid(k.valid, j)) return false;
  switch (k.dtype) {
    case NVT_F32: return ((const float *)k.x)[i] == ((const float *)k.x)[j];    // (NaN: never equal)
    case NVT_F64: return ((const double *)k.x)[i] == ((const double *)k.x)[j];
    case NVT_I32: return ((const int32_t *)k.x)[i] == ((const int32_t *)k.x)[j];
    case NVT_I64: return ((const int64_t *)k.x)[i] == ((const int64_t *)k.x)[j];
    default: return ((const uint8_t *)k.x)[i] == ((const uint8_t *)k.x)[j];
  }
}

// x[i] - x[j] as pandas computes it: integers go to float64 first, float64 subtracts in float64,
// float32 in float32; the result is rounded to float32
__device__ __forceinline__ float lag_diff(const GCol &c, uint64_t i, uint64_t j) {
  switch (c.dtype) {
    case NVT_F32: return ((const float *)c.x)[i] - ((const float *)c.x)[j];
    case NVT_F64: return (float)(((const double *)c.x)[i] - ((const double *)c.x)[j]);
    case NVT_I32: return (float)((double)((const int32_t *)c.x)[i] - (double)((const int32_t *)c.x)[j]);
    case NVT_I64: return (float)((double)((const int64_t *)c.x)[i] - (double)((const int64_t *)c.x)[j]);
    default: return (float)((double)((const uint8_t *)c.x)[i] - (double)((const uint8_t *)c.x)[j]);
  }
}

__global__ __launch_bounds__(kBlock) void lag_kernel(GBatch b, uint64_t n) {
  const float nan = __builtin_nanf("");
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    int64_t shift = 0;
    bool same = false;
    uint64_t j = i;
    for (int ci = 0; ci < b.ncols; ++ci) {
      const GCol &c = b.c[ci];
      if (ci == 0 || c.shift != shift) {  // (descriptors of one shift are adjacent: the host sorts them)
        shift = c.shift;
        // j = i - shift inside [0, n); |shift| >= n leaves no row
        same = shift >= 0 ? (uint64_t)shift <= i : (uint64_t)(-(shift + 1)) < n - 1 - i;
        j = same ? (uint64_t)((int64_t)i - shift) : i;
        for (int q = 0; same && q < b.nkeys; ++q) same = key_same(b.k[q], i, j);
      }
      float v = nan;
      if (same && bit_valid(c.valid, i) && bit_valid(c.valid, j)) v = lag_diff(c, i, j);
      c.out[i] = v;
    }
  }
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_list_slice_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  *bytes = (ntiles_of(n) + 1) * 8;
  return NVT_OK;
}

int nvt_list_slice_offsets(const int64_t *offsets, uint64_t n, int64_t start, int64_t end, int64_t *out_offsets,
                           void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(offsets && out_offsets, "null pointer");
  NVT_CHECK_ARG(n > 0, "n must be positive");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace must be 8-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (ntiles_of(n) + 1) * 8, "workspace smaller than nvt_list_slice_ws_bytes(n)");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t nt = ntiles_of(n);
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(ws);
  const Slice sl{start, end};
  NVT_PROF("list_slice_offsets", (n + 1) * 32, s);
  slice_len_kernel<<<stream_grid(nt, 1), kBlock, 0, s>>>(offsets, n, sl, out_offsets, tot);
  NVT_CHECK_LAUNCH();
  scan_totals_kernel<<<1, kBlock, 0, s>>>(tot, nt);
  NVT_CHECK_LAUNCH();
  slice_add_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(out_offsets, n, tot, offsets, sl);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_list_slice_many(const nvt_list_col *cols, int ncols, const int64_t *offsets, uint64_t n, int64_t start,
                        int64_t end, const int64_t *out_offsets, uint64_t total, uint64_t pad_width,
                        void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  NVT_CHECK_ARG(out_offsets == nullptr || pad_width == 0, "out_offsets (ragged) or pad_width (padded), not both");
  NVT_CHECK_ARG(out_offsets != nullptr || pad_width > 0, "out_offsets (ragged) or pad_width (padded) is needed");
  NVT_CHECK_ARG(pad_width == 0 || (total / pad_width == n && total % pad_width == 0),
                "total must be n * pad_width");
  for (int i = 0; i < ncols; ++i) {
    const nvt_list_col &c = cols[i];
    NVT_CHECK_ARG(c.width == 1 || c.width == 4 || c.width == 8, "width must be 1, 4 or 8 bytes");
    NVT_CHECK_ARG(c.dst_valid || !c.src_valid, "a column with src_valid needs dst_valid");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.dst_valid) & 7) == 0, "dst_valid must be 8-byte aligned");
    NVT_CHECK_ARG(total == 0 || (c.src && c.dst) || (c.dst && pad_width), "null pointer");
  }
  if (total == 0 || n == 0) return NVT_OK;
  NVT_CHECK_ARG(offsets, "null offsets");
  hipStream_t s = (hipStream_t)stream;
  const Slice sl{start, end};
  const unsigned grid = stream_grid(ntiles_of(total), 1);
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    LBatch b;
    memset(&b, 0, sizeof(b));
    b.ncols = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
    uint64_t bytes = (n + 1) * 8;
    for (int j = 0; j < b.ncols; ++j) {
      const nvt_list_col &c = cols[i0 + j];
      LCol &d = b.c[j];
      d.src = c.src;
      d.dst = c.dst;
      d.src_valid = c.src_valid;
      d.dst_valid = reinterpret_cast<uint64_t *>(c.dst_valid);
      d.pad_bits = c.pad_bits;
      d.width = c.width;
      bytes += total * (uint64_t)c.width * 2 + (c.dst_valid ? total / 4 : 0);
    }
    NVT_PROF("list_slice_many", bytes, s);
    if (pad_width)
      slice_move_kernel<true><<<grid, kBlock, 0, s>>>(b, offsets, n, sl, nullptr, total, pad_width,
                                                      total <= 0xFFFFFFFFull);
    else
      slice_move_kernel<false><<<grid, kBlock, 0, s>>>(b, offsets, n, sl, out_offsets, total, 0, 0);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_list_len_minmax(const nvt_list_len_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  for (int i = 0; i < ncols; ++i)
    NVT_CHECK_ARG(cols[i].n == 0 || (cols[i].offsets && cols[i].acc), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    MBatch b;
    memset(&b, 0, sizeof(b));
    const int k = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
    uint64_t maxn = 0, bytes = 0;
    for (int j = 0; j < k; ++j) {
      const nvt_list_len_col &c = cols[i0 + j];
      b.c[j] = MCol{c.offsets, c.n, reinterpret_cast<long long *>(c.acc)};
      maxn = c.n > maxn ? c.n : maxn;
      bytes += (c.n + 1) * 8;
    }
    if (maxn == 0) continue;
    NVT_PROF("list_len_minmax", bytes, s);
    len_minmax_kernel<<<dim3(stream_grid(maxn, kBlock * 8, 4), k), kBlock, 0, s>>>(b);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_difference_lag_many(const nvt_lag_key *keys, int nkeys, const nvt_lag_col *cols, int ncols, uint64_t n,
                            void *stream) {
  NVT_CHECK_ARG(nkeys >= 0 && nkeys <= kMaxKeys, "at most 4 partition columns");
  NVT_CHECK_ARG(keys || nkeys == 0, "null partition descriptors");
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  for (int i = 0; i < nkeys; ++i) {
    NVT_CHECK_ARG(keys[i].dtype >= NVT_F32 && keys[i].dtype <= NVT_U8, "unsupported partition dtype");
    NVT_CHECK_ARG(keys[i].x || n == 0, "null partition column");
  }
  for (int i = 0; i < ncols; ++i) {
    NVT_CHECK_ARG(cols[i].dtype >= NVT_F32 && cols[i].dtype <= NVT_U8, "unsupported dtype");
    NVT_CHECK_ARG((cols[i].x && cols[i].out) || n == 0, "null pointer");
  }
  if (n == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  // descriptors of one shift side by side (stable: the batch keeps the caller's order otherwise)
  NVT_CHECK_ARG(ncols <= 1024, "at most 1024 outputs per call");
  int order[1024];
  for (int i = 0; i < ncols; ++i) order[i] = i;
  for (int i = 1; i < ncols; ++i) {
    const int v = order[i];
    int j = i;
    while (j > 0 && cols[order[j - 1]].shift > cols[v].shift) {
      order[j] = order[j - 1];
      --j;
    }
    order[j] = v;
  }
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    GBatch b;
    memset(&b, 0, sizeof(b));
    b.nkeys = nkeys;
    b.ncols = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
    uint64_t bytes = 0;
    for (int q = 0; q < nkeys; ++q) {
      b.k[q] = GKey{keys[q].x, keys[q].valid, keys[q].dtype, 0};
      bytes += n * (keys[q].dtype == NVT_U8 ? 1 : (keys[q].dtype == NVT_F32 || keys[q].dtype == NVT_I32) ? 4 : 8);
    }
    for (int j = 0; j < b.ncols; ++j) {
      const nvt_lag_col &c = cols[order[i0 + j]];
      b.c[j] = GCol{c.x, c.valid, c.out, c.shift, c.dtype, 0};
      bytes += n * (4 + (c.dtype == NVT_U8 ? 1 : (c.dtype == NVT_F32 || c.dtype == NVT_I32) ? 4 : 8));
    }
    NVT_PROF("difference_lag_many", bytes, s);
    lag_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(b, n);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
