// Row-wise sparse similarity (ops.ColumnSimilarity): out[i] = <row left[i] of L, row right[i] of R>
// for two CSR feature matrices, and the preparation that turns a COO matrix into the CSR read here.
//
// Preparation (nvt_similarity_prepare, then nvt_similarity_coalesce), entry by entry on the COO form:
//   count_pack     cnt[col] += 1 (the tf-idf document counts);  words = col << 32 | entry
//   sort           stable word sort (nvt_sort.hip) on the column bits, the words are re-packed as
//                  row << 32 | entry and sorted on the row bits: the entries in (row, col) order
//   weight         w = data (tf-idf: * log(N / cnt[col])) in that order, its key row << 32 | col, and
//                  sumsq[row] += w^2: the lanes of a wave that share a row add up in a segmented
//                  shuffle scan and one lane per (wave, row) does the atomic, so a row of thousands
//                  of entries is summed as a tree and not as one long chain of roundings
//   flag_norm      w /= sqrt(sumsq[row]) (cosine, tf-idf); head flag of every (row, col) run
//   scan           exclusive scan of the flags (nvt_scan.hpp): the output slot of every run, the
//                  coalesced nnz in state[0] -- the one number the host reads to size the CSR
//   coalesce       the head of a run sums it into its slot;  indptr[r] = slot of the first key >= r << 32
// An entry outside the shape is counted in state[1] and treated as (0, 0): nothing is addressed
// through it, and the host raises on the count.
//
// Similarity (nvt_row_similarity): search, not merge.
//   class pass     one lane per data row: ids checked against the bitmaps and the shapes, NaN / 0.0
//                  written for the rows that need no product; every other row index is appended to
//                  the list of its class (shorter row s <= 8, <= 64, longer): ballot-compacted in the
//                  wave, one reservation per workgroup, round of 1024 rows and class.  Order inside
//                  a list is free: a row owns its output.
//   dot<W>         W = 4, 16, 64 lanes own one data row of the class: they stride over the SHORTER CSR
//                  row with coalesced loads, each lane binary-searches its column in the longer row
//                  and multiplies on a hit; the group adds up with __shfl_xor and its first lane
//                  stores.  No LDS, no atomics, no dependency between entries.  The launches take
//                  their sizes from the class counters on the device: a capped grid whose groups
//                  stride over the list, so nothing is read back.
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr uint64_t kMaxDim = (1ull << 31) - 1;      // data rows, shape[0], shape[1]: int32 indices
constexpr uint64_t kMaxEntries = (1ull << 30) - 1;  // what the word sort takes

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int bits_for(uint64_t count) {  // bits that hold 0 .. count - 1 (at least 1)
  int b = 1;
  while ((1ull << b) < count) ++b;
  return b;
}

// rank of this lane among the lanes below it whose bit is set in `word`
__device__ __forceinline__ unsigned lane_rank(uint64_t word) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
}

// ---- preparation ------------------------------------------------------------------------------
struct PrepWs {
  unsigned *col_cnt;          // [n_cols]
  double *row_sq;             // [n_rows]   (directly behind col_cnt: one clearing pass)
  uint64_t clear_words;       // 32-bit words of the two accumulators
  uint64_t *words;            // [nnz]      the words handed to the sort
  void *sort_tmp;
  uint64_t *keys;             // [nnz]      row << 32 | col in (row, col) order
  double *w;                  // [nnz]      weights in that order
  unsigned *pos;              // [nnz + 1]  head flags, then their exclusive scan
  unsigned long long *chunk;  // the scan's chunk totals
  uint64_t bytes;
};

PrepWs prep_ws(const void *ws, uint64_t nnz, uint64_t n_rows, uint64_t n_cols) {
  PrepWs p;
  uint8_t *b = (uint8_t *)ws;
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    uint8_t *q = b + at;
    at += pad256(bytes);
    return q;
  };
  p.col_cnt = reinterpret_cast<unsigned *>(take(n_cols * 4));
  p.row_sq = reinterpret_cast<double *>(take(n_rows * 8));
  p.clear_words = at / 4;
  p.words = reinterpret_cast<uint64_t *>(take(nnz * 8));
  p.sort_tmp = take(sort_words_tmp_bytes(nnz));
  p.keys = reinterpret_cast<uint64_t *>(take(nnz * 8));
  p.w = reinterpret_cast<double *>(take(nnz * 8));
  p.pos = reinterpret_cast<unsigned *>(take((nnz + 1) * 4));
  p.chunk = reinterpret_cast<unsigned long long *>(take(scan_chunks(nnz + 1) * 8));
  p.bytes = at;
  return p;
}

__global__ __launch_bounds__(kBlock) void sim_clear_kernel(unsigned *__restrict__ acc, uint64_t nwords,
                                                           uint64_t *__restrict__ state) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * kBlock)
    acc[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < 2) state[threadIdx.x] = 0;
}

// (row, col) of entry e, or (0, 0) for an entry outside the shape
__device__ __forceinline__ bool entry_at(const int64_t *__restrict__ rows, const int64_t *__restrict__ cols, uint64_t e,
                                         uint64_t n_rows, uint64_t n_cols, uint32_t &r, uint32_t &c) {
  const uint64_t rr = (uint64_t)rows[e], cc = (uint64_t)cols[e];
  const bool ok = rr < n_rows && cc < n_cols;
  r = ok ? (uint32_t)rr : 0u;
  c = ok ? (uint32_t)cc : 0u;
  return ok;
}

__global__ __launch_bounds__(kBlock) void sim_count_pack_kernel(const int64_t *__restrict__ rows,
                                                                const int64_t *__restrict__ cols, uint64_t nnz,
                                                                uint64_t n_rows, uint64_t n_cols,
                                                                unsigned *__restrict__ col_cnt,
                                                                uint64_t *__restrict__ words,
                                                                uint64_t *__restrict__ state) {
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * kBlock) {
    uint32_t r, c;
    if (entry_at(rows, cols, e, n_rows, n_cols, r, c))
      atomicAdd(&col_cnt[c], 1u);
    else
      atomicAdd(reinterpret_cast<unsigned long long *>(&state[1]), 1ull);
    words[e] = ((uint64_t)c << 32) | e;
  }
}

// column-ordered words -> row << 32 | entry (`sorted` may be `words` itself: one lane per slot)
__global__ __launch_bounds__(kBlock) void sim_repack_kernel(const uint64_t *sorted, const int64_t *__restrict__ rows,
                                                            const int64_t *__restrict__ cols, uint64_t nnz,
                                                            uint64_t n_rows, uint64_t n_cols, uint64_t *words) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nnz; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t e = (uint32_t)sorted[j];
    uint32_t r, c;
    entry_at(rows, cols, e, n_rows, n_cols, r, c);
    words[j] = ((uint64_t)r << 32) | e;
  }
}

__global__ __launch_bounds__(kBlock) void sim_weight_kernel(const uint64_t *__restrict__ sorted,
                                                            const int64_t *__restrict__ rows,
                                                            const int64_t *__restrict__ cols,
                                                            const double *__restrict__ data, uint64_t nnz,
                                                            uint64_t n_rows, uint64_t n_cols,
                                                            const unsigned *__restrict__ col_cnt, int metric,
                                                            uint64_t *__restrict__ keys, double *__restrict__ w,
                                                            double *__restrict__ row_sq) {
  const int lane = (int)lane_id();
  for (uint64_t j0 = (uint64_t)blockIdx.x * kBlock; j0 < nnz; j0 += (uint64_t)gridDim.x * kBlock) {
    const uint64_t j = j0 + threadIdx.x;
    const bool active = j < nnz;
    uint32_t r = 0xFFFFFFFFu, c = 0;  // (no row has this number: the lanes past nnz form their own run)
    double v = 0.0;
    if (active) {
      const uint32_t e = (uint32_t)sorted[j];
      entry_at(rows, cols, e, n_rows, n_cols, r, c);
      v = data[e];
      if (metric == NVT_SIM_TFIDF) v *= log((double)n_rows / (double)col_cnt[c]);
      keys[j] = ((uint64_t)r << 32) | c;
      w[j] = v;
    }
    if (metric == NVT_SIM_INNER) continue;
    // the lanes of one row are neighbours: inclusive scan of w^2 that stops at the row's first lane
    const uint32_t before = __shfl_up(r, 1, 64);
    const uint64_t heads = __ballot(lane == 0 || before != r);
    const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    double s = v * v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(s, off, 64);
      if (lane - off >= start) s += o;
    }
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1);
    if (active && last) atomicAdd(&row_sq[r], s);
  }
}

__global__ __launch_bounds__(kBlock) void sim_flag_norm_kernel(const uint64_t *__restrict__ keys, uint64_t nnz,
                                                               const double *__restrict__ row_sq, int metric,
                                                               double *__restrict__ w, unsigned *__restrict__ pos) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nnz; j += (uint64_t)gridDim.x * kBlock) {
    const uint64_t key = keys[j];
    pos[j] = (j == 0 || keys[j - 1] != key) ? 1u : 0u;
    if (metric != NVT_SIM_INNER) w[j] = w[j] / sqrt(row_sq[key >> 32]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) pos[nnz] = 0u;
}

__global__ void sim_total_kernel(const unsigned *__restrict__ pos, uint64_t nnz, uint64_t *__restrict__ state) {
  state[0] = pos[nnz];
}

__global__ __launch_bounds__(kBlock) void sim_coalesce_kernel(const uint64_t *__restrict__ keys,
                                                              const double *__restrict__ w,
                                                              const unsigned *__restrict__ pos, uint64_t nnz,
                                                              uint64_t nnz_out, int32_t *__restrict__ indices,
                                                              double *__restrict__ weights) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nnz; j += (uint64_t)gridDim.x * kBlock) {
    const uint64_t slot = pos[j];
    if (pos[j + 1] == slot || slot >= nnz_out) continue;  // not the head of a run
    const uint64_t key = keys[j];
    double s = w[j];
    for (uint64_t k = j + 1; k < nnz && keys[k] == key; ++k) s += w[k];
    indices[slot] = (int32_t)(uint32_t)key;
    weights[slot] = s;
  }
}

__global__ __launch_bounds__(kBlock) void sim_indptr_kernel(const uint64_t *__restrict__ keys,
                                                            const unsigned *__restrict__ pos, uint64_t nnz,
                                                            uint64_t n_rows, int64_t *__restrict__ indptr) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r <= n_rows; r += (uint64_t)gridDim.x * kBlock) {
    const uint64_t want = r << 32;
    uint64_t lo = 0, len = nnz;  // the first entry whose key is not below `want`
    while (len > 0) {
      const uint64_t half = len >> 1;
      if (keys[lo + half] < want) {
        lo += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    indptr[r] = (int64_t)pos[lo];  // (lo <= nnz, and pos[nnz] is the total)
  }
}

// ---- similarity -------------------------------------------------------------------------------
constexpr int kClasses = 3;
constexpr int64_t kShort4 = 8, kShort16 = 64;  // shorter row <= 8: W = 4; <= 64: W = 16; longer: W = 64

struct SimWs {
  unsigned *count;           // [kClasses] rows appended so far
  unsigned *list[kClasses];  // [n] each
};

uint64_t sim_ws_bytes(uint64_t n) { return 256 + kClasses * pad256(n * 4); }

SimWs sim_ws(void *ws, uint64_t n) {
  SimWs w;
  uint8_t *b = (uint8_t *)ws;
  w.count = reinterpret_cast<unsigned *>(b);
  for (int k = 0; k < kClasses; ++k) w.list[k] = reinterpret_cast<unsigned *>(b + 256 + k * pad256(n * 4));
  return w;
}

__global__ void sim_zero_counts_kernel(unsigned *count) {
  if (threadIdx.x < kClasses) count[threadIdx.x] = 0u;
}

// A workgroup classes kTileRows rows per round and reserves their list slots with ONE atomic per class:
// one atomic per wave and class put 625 000 additions on one counter for 40 M short rows and made this
// pass cost twice the products (profiles/column_similarity_notes.md).
constexpr int kRowsPerLane = 4;
constexpr uint64_t kTileRows = (uint64_t)kBlock * kRowsPerLane;

template <typename T>
__global__ __launch_bounds__(kBlock) void sim_class_kernel(const T *__restrict__ left,
                                                           const uint8_t *__restrict__ left_valid,
                                                           const T *__restrict__ right,
                                                           const uint8_t *__restrict__ right_valid, uint64_t n,
                                                           nvt_csr L, nvt_csr R, double *__restrict__ out, SimWs w) {
  __shared__ unsigned wave_cnt[kBlock / kWave][kClasses];
  __shared__ unsigned base[kClasses];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kTileRows; i0 < n; i0 += (uint64_t)gridDim.x * kTileRows) {
    int cls[kRowsPerLane];
    unsigned rank[kRowsPerLane];            // among the wave's rows of the same class in this round
    unsigned mine[kClasses] = {0u, 0u, 0u};  // the wave's rows per class (uniform over the wave)
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
      const uint64_t i = i0 + (uint64_t)r * kBlock + threadIdx.x;
      cls[r] = -1;
      rank[r] = 0u;
      if (i < n) {
        const uint64_t a = (uint64_t)(int64_t)left[i], b = (uint64_t)(int64_t)right[i];  // negative: huge
        if (!bit_valid(left_valid, i) || !bit_valid(right_valid, i) || a >= L.rows || b >= R.rows) {
          out[i] = __longlong_as_double(0x7FF8000000000000ll);
        } else {
          const int64_t la = L.indptr[a + 1] - L.indptr[a], lb = R.indptr[b + 1] - R.indptr[b];
          const int64_t s = la < lb ? la : lb;
          if (s <= 0)
            out[i] = 0.0;
          else
            cls[r] = s <= kShort4 ? 0 : (s <= kShort16 ? 1 : 2);
        }
      }
#pragma unroll
      for (int k = 0; k < kClasses; ++k) {
        const uint64_t mask = __ballot(cls[r] == k);
        if (cls[r] == k) rank[r] = mine[k] + lane_rank(mask);
        mine[k] += (unsigned)__popcll(mask);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kClasses; ++k) wave_cnt[wave][k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < kClasses) {
      unsigned total = 0;
      for (int v = 0; v < kBlock / kWave; ++v) total += wave_cnt[v][threadIdx.x];
      base[threadIdx.x] = total ? atomicAdd(&w.count[threadIdx.x], total) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
      if (cls[r] < 0) continue;
      unsigned at = base[cls[r]] + rank[r];
      for (unsigned v = 0; v < wave; ++v) at += wave_cnt[v][cls[r]];
      w.list[cls[r]][at] = (unsigned)(i0 + (uint64_t)r * kBlock + threadIdx.x);
    }
    __syncthreads();  // (the counts are rewritten in the next round)
  }
}

template <int W, typename T>
__global__ __launch_bounds__(kBlock) void sim_dot_kernel(const T *__restrict__ left, const T *__restrict__ right,
                                                         nvt_csr L, nvt_csr R, const unsigned *__restrict__ list,
                                                         const unsigned *__restrict__ count,
                                                         double *__restrict__ out) {
  constexpr unsigned kGroups = kBlock / W;
  const unsigned total = *count;
  const unsigned sub = threadIdx.x % W;
  for (uint64_t g = (uint64_t)blockIdx.x * kGroups + threadIdx.x / W; g < total; g += (uint64_t)gridDim.x * kGroups) {
    const unsigned i = list[g];
    const int64_t a = (int64_t)left[i], b = (int64_t)right[i];
    const int64_t pa = L.indptr[a], la = L.indptr[a + 1] - pa;
    const int64_t pb = R.indptr[b], lb = R.indptr[b + 1] - pb;
    const bool left_short = la <= lb;
    const int32_t *__restrict__ si = left_short ? L.indices + pa : R.indices + pb;
    const double *__restrict__ sw = left_short ? L.weights + pa : R.weights + pb;
    const int32_t *__restrict__ li = left_short ? R.indices + pb : L.indices + pa;
    const double *__restrict__ lw = left_short ? R.weights + pb : L.weights + pa;
    const int64_t s = left_short ? la : lb, l = left_short ? lb : la;
    double acc = 0.0;
    for (int64_t k = sub; k < s; k += W) {
      const int32_t c = si[k];
      int64_t lo = 0, len = l;  // the first entry of the longer row whose column is not below c
      while (len > 0) {
        const int64_t half = len >> 1;
        if (li[lo + half] < c) {
          lo += half + 1;
          len -= half + 1;
        } else {
          len = half;
        }
      }
      if (lo < l && li[lo] == c) acc += sw[k] * lw[lo];
    }
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, W);
    if (sub == 0) out[i] = acc;
  }
}

template <typename T>
int launch_similarity(const void *left, const uint8_t *left_valid, const void *right, const uint8_t *right_valid,
                      uint64_t n, const nvt_csr &L, const nvt_csr &R, double *out, const SimWs &w, hipStream_t s) {
  const T *a = reinterpret_cast<const T *>(left), *b = reinterpret_cast<const T *>(right);
  sim_zero_counts_kernel<<<1, kWave, 0, s>>>(w.count);
  NVT_CHECK_LAUNCH();
  sim_class_kernel<T><<<stream_grid(n, kTileRows), kBlock, 0, s>>>(a, left_valid, b, right_valid, n, L, R, out, w);
  NVT_CHECK_LAUNCH();
  sim_dot_kernel<4, T><<<stream_grid(n, kBlock / 4), kBlock, 0, s>>>(a, b, L, R, w.list[0], w.count + 0, out);
  NVT_CHECK_LAUNCH();
  sim_dot_kernel<16, T><<<stream_grid(n, kBlock / 16), kBlock, 0, s>>>(a, b, L, R, w.list[1], w.count + 1, out);
  NVT_CHECK_LAUNCH();
  sim_dot_kernel<64, T><<<stream_grid(n, kBlock / 64), kBlock, 0, s>>>(a, b, L, R, w.list[2], w.count + 2, out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int check_shape(uint64_t nnz, uint64_t n_rows, uint64_t n_cols) {
  NVT_CHECK_ARG(nnz <= kMaxEntries, "nnz must be below 2^30");
  NVT_CHECK_ARG(n_rows >= 1 && n_rows <= kMaxDim && n_cols >= 1 && n_cols <= kMaxDim,
                "n_rows and n_cols must be 1 to 2^31 - 1");
  return NVT_OK;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_similarity_prepare_ws_bytes(uint64_t nnz, uint64_t n_rows, uint64_t n_cols, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  const int rc = check_shape(nnz, n_rows, n_cols);
  if (rc) return rc;
  *bytes = prep_ws(nullptr, nnz, n_rows, n_cols).bytes;
  return NVT_OK;
}

int nvt_similarity_prepare(const int64_t *rows, const int64_t *cols, const double *data, uint64_t nnz,
                           uint64_t n_rows, uint64_t n_cols, int metric, void *ws, uint64_t ws_bytes,
                           uint64_t *state, void *stream) {
  const int rc = check_shape(nnz, n_rows, n_cols);
  if (rc) return rc;
  NVT_CHECK_ARG(metric == NVT_SIM_INNER || metric == NVT_SIM_COSINE || metric == NVT_SIM_TFIDF, "unknown metric");
  NVT_CHECK_ARG(state && ws, "null state / workspace");
  NVT_CHECK_ARG((rows && cols && data) || nnz == 0, "null rows / cols / data");
  NVT_CHECK_ARG(aligned_to(rows, 8) && aligned_to(cols, 8) && aligned_to(data, 8) && aligned_to(state, 8),
                "rows, cols, data and state must be 8-byte aligned");
  NVT_CHECK_ARG(aligned_to(ws, 256), "workspace must be 256-byte aligned");
  const PrepWs p = prep_ws(ws, nnz, n_rows, n_cols);
  NVT_CHECK_ARG(ws_bytes >= p.bytes, "workspace smaller than nvt_similarity_prepare_ws_bytes");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("similarity_prepare", nnz * 24, s);
  sim_clear_kernel<<<stream_grid(p.clear_words, kBlock * 4), kBlock, 0, s>>>(p.col_cnt, p.clear_words, state);
  NVT_CHECK_LAUNCH();
  if (nnz == 0) return NVT_OK;  // (state = {0, 0}: an empty matrix)
  const unsigned grid = stream_grid(nnz, kBlock * 4);
  sim_count_pack_kernel<<<grid, kBlock, 0, s>>>(rows, cols, nnz, n_rows, n_cols, p.col_cnt, p.words, state);
  NVT_CHECK_LAUNCH();
  uint64_t *sorted = nullptr;
  int sr = sort_words_bits(p.words, nnz, 32, 32 + bits_for(n_cols), p.sort_tmp, &sorted, s);
  if (sr) return sr;
  sim_repack_kernel<<<grid, kBlock, 0, s>>>(sorted, rows, cols, nnz, n_rows, n_cols, p.words);
  NVT_CHECK_LAUNCH();
  sr = sort_words_bits(p.words, nnz, 32, 32 + bits_for(n_rows), p.sort_tmp, &sorted, s);
  if (sr) return sr;
  sim_weight_kernel<<<grid, kBlock, 0, s>>>(sorted, rows, cols, data, nnz, n_rows, n_cols, p.col_cnt, metric, p.keys,
                                            p.w, p.row_sq);
  NVT_CHECK_LAUNCH();
  sim_flag_norm_kernel<<<grid, kBlock, 0, s>>>(p.keys, nnz, p.row_sq, metric, p.w, p.pos);
  NVT_CHECK_LAUNCH();
  sr = exclusive_scan_u32(p.pos, nnz + 1, p.chunk, s);
  if (sr) return sr;
  sim_total_kernel<<<1, 1, 0, s>>>(p.pos, nnz, state);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_similarity_coalesce(const void *ws, uint64_t ws_bytes, uint64_t nnz, uint64_t n_rows, uint64_t n_cols,
                            uint64_t nnz_out, int64_t *indptr, int32_t *indices, double *weights, void *stream) {
  const int rc = check_shape(nnz, n_rows, n_cols);
  if (rc) return rc;
  NVT_CHECK_ARG(nnz >= 1 && nnz_out >= 1 && nnz_out <= nnz, "nnz_out must be 1 to nnz");
  NVT_CHECK_ARG(ws && indptr && indices && weights, "null pointer");
  NVT_CHECK_ARG(aligned_to(ws, 256), "workspace must be 256-byte aligned");
  NVT_CHECK_ARG(aligned_to(indptr, 8) && aligned_to(indices, 4) && aligned_to(weights, 8),
                "indptr, indices and weights must be aligned to their types");
  const PrepWs p = prep_ws(ws, nnz, n_rows, n_cols);
  NVT_CHECK_ARG(ws_bytes >= p.bytes, "workspace smaller than nvt_similarity_prepare_ws_bytes");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("similarity_coalesce", nnz * 20 + nnz_out * 12 + n_rows * 8, s);
  sim_coalesce_kernel<<<stream_grid(nnz, kBlock * 4), kBlock, 0, s>>>(p.keys, p.w, p.pos, nnz, nnz_out, indices,
                                                                      weights);
  NVT_CHECK_LAUNCH();
  sim_indptr_kernel<<<stream_grid(n_rows + 1, kBlock * 4), kBlock, 0, s>>>(p.keys, p.pos, nnz, n_rows, indptr);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_row_similarity_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  NVT_CHECK_ARG(n <= kMaxDim, "n must be below 2^31");
  *bytes = sim_ws_bytes(n);
  return NVT_OK;
}

int nvt_row_similarity(const void *left, const uint8_t *left_valid, const void *right, const uint8_t *right_valid,
                       int dtype, uint64_t n, const nvt_csr *left_csr, const nvt_csr *right_csr, double *out,
                       void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(dtype == NVT_I32 || dtype == NVT_I64, "id dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(n <= kMaxDim, "n must be below 2^31");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(left && right && out && ws, "null ids / out / workspace");
  NVT_CHECK_ARG(left_csr && right_csr, "null feature matrix");
  const uintptr_t width = dtype == NVT_I32 ? 4 : 8;
  NVT_CHECK_ARG(aligned_to(left, width) && aligned_to(right, width) && aligned_to(out, 8),
                "ids and out must be aligned to their types");
  NVT_CHECK_ARG(aligned_to(ws, 256), "workspace must be 256-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= sim_ws_bytes(n), "workspace smaller than nvt_row_similarity_ws_bytes(n)");
  for (const nvt_csr *m : {left_csr, right_csr}) {
    NVT_CHECK_ARG(m->indptr && m->rows >= 1 && m->rows <= kMaxDim,
                  "a feature matrix needs indptr and 1 to 2^31 - 1 rows");
    NVT_CHECK_ARG(aligned_to(m->indptr, 8) && aligned_to(m->indices, 4) && aligned_to(m->weights, 8),
                  "indptr, indices and weights must be aligned to their types");
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("row_similarity", n * (2 * width + 8 + 32), s);
  const SimWs w = sim_ws(ws, n);
  const nvt_csr &L = *left_csr, &R = *right_csr;
  return dtype == NVT_I32 ? launch_similarity<int32_t>(left, left_valid, right, right_valid, n, L, R, out, w, s)
                          : launch_similarity<int64_t>(left, left_valid, right, right_valid, n, L, R, out, w, s);
}

}  // extern "C"
