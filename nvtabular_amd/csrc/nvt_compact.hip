// Row compaction (ops.Filter / ops.Dropna): a keep mask, a plan, and one launch that moves the kept
// rows of every column.
//
// A plan covers n rows in tiles of kTile = 2048.  Its workspace (nvt_compact_ws_bytes) holds
//   words  uint64[ntiles * 32]   the keep mask, bit i of word i / 64 = row i (bits past n are 0)
//   base   uint32[ntiles + 1]    kept rows per tile; after nvt_compact_plan the exclusive scan of
//                                them: tile t's kept rows go to [base[t], base[t + 1]), base[ntiles] = m
//   chunk  uint64[...]           the scan's chunk totals (nvt_scan.hpp)
// The producers (a bool mask, the null test of Dropna, the terms of a Dataset filter, the leaf
// expansion of a list column) write
// the words and the per-tile counts in one pass; the scan has no inter-workgroup waits and the data
// path no global atomics except the two boundary words of a tile's validity run, which are merged
// with atomicOr into a bitmap zeroed first (OR does not depend on the order: the bits come out the
// same on every run).
#include "nvt_common.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr uint64_t kTile = 2048;                 // rows per tile: 256 threads x 8
constexpr int kTileWords = (int)(kTile / 64);    // mask words per tile
constexpr int kMaxCols = NVT_COMPACT_MAX_COLS;   // descriptors per launch (kernel arguments < 4 KiB)
constexpr unsigned kGridCap = 2048;              // workgroups per launch; the rest is grid-strided
constexpr uint64_t kMaxRows = (1ull << 32) - kTile;  // tile bases are uint32

__host__ __device__ inline uint64_t up256(uint64_t b) { return (b + 255) & ~255ull; }
__host__ __device__ inline uint64_t ntiles_of(uint64_t n) { return (n + kTile - 1) / kTile; }

struct Plan {
  uint64_t *words;
  unsigned *base;
  unsigned long long *chunk;
  uint64_t ntiles;
};

__host__ __device__ inline Plan plan_of(const void *ws, uint64_t n) {
  Plan p;
  uint8_t *b = (uint8_t *)ws;
  p.ntiles = ntiles_of(n);
  p.words = reinterpret_cast<uint64_t *>(b);
  b += p.ntiles * (kTile / 8);
  p.base = reinterpret_cast<unsigned *>(b);
  b += up256((p.ntiles + 1) * 4);
  p.chunk = reinterpret_cast<unsigned long long *>(b);
  return p;
}

uint64_t plan_bytes(uint64_t n) {
  const uint64_t nt = ntiles_of(n);
  return nt * (kTile / 8) + up256((nt + 1) * 4) + up256(scan_chunks(nt + 1) * 8);
}

__device__ __forceinline__ bool row_kept(const Plan &p, uint64_t r) { return (p.words[r >> 6] >> (r & 63)) & 1; }

// kept rows of the plan before position `pos` (pos <= n)
__device__ uint64_t plan_rank(const Plan &p, uint64_t n, uint64_t pos) {
  if (n == 0) return 0;
  const uint64_t t = pos / kTile;
  if (t >= p.ntiles) return p.base[p.ntiles];
  uint64_t r = p.base[t];
  for (uint64_t w = t * kTileWords; w < (pos >> 6); ++w) r += __popcll(p.words[w]);
  const unsigned sh = pos & 63;
  if (sh) r += __popcll(p.words[pos >> 6] & ((1ull << sh) - 1));
  return r;
}

// rank of this lane among the lanes below it whose bit is set in `word` (v_mbcnt_lo / _hi)
__device__ __forceinline__ unsigned lane_rank(uint64_t word) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
}

__device__ __forceinline__ uint64_t bit_range(unsigned lo, unsigned hi) {  // bits [lo, hi), hi - lo >= 1
  const unsigned len = hi - lo;
  return (len >= 64 ? ~0ull : ((1ull << len) - 1)) << lo;
}

// ---- keep-mask producers ----------------------------------------------------------------------
// Tile t: wave w, round k takes mask word t * 32 + 4 k + w, one row per lane; the per-tile count
// goes to base[t], and workgroup 0 writes base[ntiles] = 0 (the scan's last entry becomes m).
template <typename Keep>
__device__ __forceinline__ void produce_tiles(uint64_t n, const Plan &p, bool accumulate, Keep keep_row) {
  __shared__ unsigned wcnt[kBlock / kWave];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  for (uint64_t t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    unsigned cnt = 0;
#pragma unroll 2
    for (int k = 0; k < kTileWords / (kBlock / kWave); ++k) {
      const uint64_t wi = t * kTileWords + (uint64_t)k * (kBlock / kWave) + w;
      const uint64_t row = wi * 64 + lane;
      bool keep = row < n;
      if (keep && accumulate) keep = (p.words[wi] >> lane) & 1;
      if (keep) keep = keep_row(row);
      const uint64_t word = __ballot(keep);
      if (lane == 0) p.words[wi] = word;
      cnt += (unsigned)__popcll(word);
    }
    if (lane == 0) wcnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) p.base[t] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) p.base[p.ntiles] = 0;
}

__global__ __launch_bounds__(kBlock) void keep_mask_kernel(const uint8_t *__restrict__ mask, uint64_t n, Plan p) {
  produce_tiles(n, p, false, [&](uint64_t row) { return mask[row] != 0; });
}

struct NaCol {
  const void *x;
  const uint8_t *valid;
  int dtype;
};
struct NaBatch {
  NaCol c[kMaxCols];
  int ncols;
};

// Dropna: a row is kept iff every column is valid there (bitmap bit 1, and not NaN for floats)
__global__ __launch_bounds__(kBlock) void keep_dropna_kernel(NaBatch b, uint64_t n, Plan p, int accumulate) {
  produce_tiles(n, p, accumulate != 0, [&](uint64_t row) {
    for (int j = 0; j < b.ncols; ++j) {
      const NaCol &c = b.c[j];
      if (!bit_valid(c.valid, row)) return false;
      if (c.dtype == NVT_F32 && is_nan(((const float *)c.x)[row])) return false;
      if (c.dtype == NVT_F64 && is_nan(((const double *)c.x)[row])) return false;
    }
    return true;
  });
}

// Dataset(filters=): a row is kept iff in some conjunction every term holds.  The descriptors are
// kernel arguments (scalar loads: the term loop is uniform); the row's value lives in two scalars,
// reloaded only when a term names another column than the term before it, so terms on one column
// share a load.  A conjunction no lane of the wave still satisfies skips its remaining terms.
struct FCol {
  const void *x;
  const uint8_t *valid;
  int dtype;
};
struct FTerm {
  int col, op, conj, set_len;
  uint64_t set_off;
  union {
    int64_t i;
    double f;
  } value;
};
struct FBatch {
  FCol c[NVT_FILTER_MAX_COLS];
  FTerm t[NVT_FILTER_MAX_TERMS];
  const uint64_t *sets;
  int nterms;
};

template <typename T>
__device__ __forceinline__ bool term_holds(const FTerm &t, const uint64_t *__restrict__ sets, T v, T c) {
  switch (t.op) {
    case NVT_FILTER_EQ: return v == c;
    case NVT_FILTER_NE: return v != c;
    case NVT_FILTER_LT: return v < c;
    case NVT_FILTER_LE: return v <= c;
    case NVT_FILTER_GT: return v > c;
    case NVT_FILTER_GE: return v >= c;
    default: {  // NVT_FILTER_IN / NVT_FILTER_NOT_IN: the lower bound of v in the term's sorted run
      const T *s = reinterpret_cast<const T *>(sets + t.set_off);
      int lo = 0, len = t.set_len;
      while (len > 0) {
        const int half = len >> 1;
        if (s[lo + half] < v) {
          lo += half + 1;
          len -= half + 1;
        } else {
          len = half;
        }
      }
      const bool in = lo < t.set_len && s[lo] == v;  // (a NaN is below nothing and equals nothing)
      return in == (t.op == NVT_FILTER_IN);
    }
  }
}

__global__ __launch_bounds__(kBlock) void keep_terms_kernel(FBatch b, uint64_t n, Plan p) {
  produce_tiles(n, p, false, [&](uint64_t row) {
    bool any = false, acc = false;
    int conj = -1, loaded = -1;
    int64_t vi = 0;
    double vf = 0.0;
    bool ok = false, flt = false;
    for (int k = 0; k < b.nterms; ++k) {
      const FTerm &t = b.t[k];
      if (t.conj != conj) {
        any |= acc;
        acc = true;
        conj = t.conj;
      }
      if (__ballot(acc) == 0) continue;  // (uniform over the lanes that are rows)
      if (t.col != loaded) {
        const FCol &c = b.c[t.col];
        loaded = t.col;
        ok = bit_valid(c.valid, row);
        flt = c.dtype == NVT_F32 || c.dtype == NVT_F64;
        switch (c.dtype) {
          case NVT_F32: vf = (double)((const float *)c.x)[row]; break;
          case NVT_F64: vf = ((const double *)c.x)[row]; break;
          case NVT_I32: vi = ((const int32_t *)c.x)[row]; break;
          case NVT_I64: vi = ((const int64_t *)c.x)[row]; break;
          case NVT_U8: vi = ((const uint8_t *)c.x)[row]; break;
          case NVT_I8: vi = ((const int8_t *)c.x)[row]; break;
          default: vi = ((const int16_t *)c.x)[row]; break;  // NVT_I16
        }
      }
      bool holds = t.op == NVT_FILTER_NOT_IN;  // a null fails every term but `not in`
      if (ok) holds = flt ? term_holds<double>(t, b.sets, vf, t.value.f) : term_holds<int64_t>(t, b.sets, vi, t.value.i);
      acc = acc && holds;
    }
    return any || acc;
  });
}

// List column: leaf word wi is kept where a kept row's leaf range covers it.  One lane per leaf
// word (a binary search for the row holding its first leaf, then the rows that start inside it),
// plain stores; the two tiles of a wave sum their counts over 32 lanes each.
__global__ __launch_bounds__(kBlock) void keep_expand_kernel(const int64_t *__restrict__ off, uint64_t n, Plan rows,
                                                             uint64_t nl, Plan leaves) {
  const int64_t o0 = off[0];
  const uint64_t nwords = leaves.ntiles * kTileWords;  // a multiple of 32: tiles never straddle half-waves
  const unsigned lane = lane_id();
  for (uint64_t b0 = (uint64_t)blockIdx.x * kBlock; b0 < nwords; b0 += (uint64_t)gridDim.x * kBlock) {
    const uint64_t wi = b0 + threadIdx.x;
    uint64_t word = 0;
    const uint64_t p0 = wi * 64;
    if (wi < nwords && p0 < nl) {
      const uint64_t p1 = p0 + 64 < nl ? p0 + 64 : nl;
      uint64_t lo = 0, hi = n;  // the last row r < n with off[r] <= p0 (off[0] - o0 = 0 <= p0)
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)(off[mid] - o0) <= p0) lo = mid;
        else hi = mid;
      }
      for (uint64_t r = lo; r < n; ++r) {
        const uint64_t a = (uint64_t)(off[r] - o0);
        if (a >= p1) break;
        const uint64_t e = (uint64_t)(off[r + 1] - o0);
        if (e > p0 && row_kept(rows, r)) {
          const uint64_t s = a > p0 ? a : p0, f = e < p1 ? e : p1;
          word |= bit_range((unsigned)(s - p0), (unsigned)(f - p0));
        }
      }
    }
    if (wi < nwords) leaves.words[wi] = word;
    unsigned c = (unsigned)__popcll(word);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((lane & 31) == 0 && wi < nwords) leaves.base[wi / kTileWords] = c;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) leaves.base[leaves.ntiles] = 0;
}

__global__ void plan_total_kernel(const unsigned *base, uint64_t ntiles, uint64_t *out_m) {
  *out_m = base[ntiles];
}

// ---- compaction -------------------------------------------------------------------------------
struct CCol {
  const void *src;
  void *dst;
  const uint8_t *src_valid;
  uint32_t *dst_valid;
  const void *plan;
  uint64_t n;
  int width, vec;
};
struct CBatch {
  CCol c[kMaxCols];
};

__global__ __launch_bounds__(kBlock) void compact_zero_kernel(CBatch b) {
  const CCol &c = b.c[blockIdx.y];
  if (c.dst_valid == nullptr || c.n == 0) return;
  const Plan p = plan_of(c.plan, c.n);
  const uint64_t m = p.base[p.ntiles];
  const uint64_t nw = (m + 63) / 64 * 2;  // bitmaps are padded to 8 bytes
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nw; i += (uint64_t)gridDim.x * kBlock)
    c.dst_valid[i] = 0u;
}

// Kept values of one tile -> LDS in output order -> one coalesced pass to dst[base, base + cnt).
// Loads are 16 bytes wide where the column is 16-byte aligned and the vector lies below n.
template <typename T>
__device__ __forceinline__ void move_tile(const T *__restrict__ src, T *__restrict__ dst, uint64_t n, bool vec,
                                          uint64_t row0, uint64_t base, unsigned cnt, const uint64_t *sw,
                                          const unsigned *spre, T *stage) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int NV = (int)kTile / V;
  for (int v = threadIdx.x; v < NV; v += kBlock) {
    const int p = v * V;
    const uint64_t word = sw[p >> 6];
    const unsigned sh = p & 63;
    unsigned bits = (unsigned)((word >> sh) & ((1ull << V) - 1));
    if (!bits) continue;
    unsigned o = spre[p >> 6] + (unsigned)__popcll(word & ((1ull << sh) - 1));
    const uint64_t r = row0 + p;
    if (vec && r + V <= n) {
      union {
        uint4 u;
        T e[V];
      } x;
      x.u = *reinterpret_cast<const uint4 *>(src + r);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if ((bits >> j) & 1) stage[o++] = x.e[j];
    } else {
      for (int j = 0; j < V; ++j)
        if ((bits >> j) & 1) stage[o++] = src[r + j];  // (a set bit is a row below n)
    }
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < cnt; i += kBlock) dst[base + i] = stage[i];
}

__global__ __launch_bounds__(kBlock) void compact_kernel(CBatch b) {
  const CCol &c = b.c[blockIdx.y];
  __shared__ uint64_t sw[kTileWords];
  __shared__ unsigned spre[kTileWords + 1];
  __shared__ unsigned sbits[kTile / 32 + 4];
  __shared__ uint64_t stage[kTile];
  if (c.n == 0) return;
  const Plan p = plan_of(c.plan, c.n);
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  for (uint64_t t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    if (threadIdx.x < kTileWords) sw[threadIdx.x] = p.words[t * kTileWords + threadIdx.x];
    if (threadIdx.x < kTile / 32 + 4) sbits[threadIdx.x] = 0u;
    const uint64_t base = p.base[t];
    const unsigned cnt = p.base[t + 1] - (unsigned)base;
    __syncthreads();
    if (w == 0) {  // exclusive prefix of the 32 words' popcounts
      unsigned v = lane < (unsigned)kTileWords ? (unsigned)__popcll(sw[lane]) : 0u;
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const unsigned u = __shfl_up(v, o, 64);
        if (lane >= (unsigned)o) v += u;
      }
      if (lane < (unsigned)kTileWords) spre[lane + 1] = v;
      if (lane == 0) spre[0] = 0u;
    }
    __syncthreads();
    if (cnt == 0) continue;  // (block-uniform; the next tile's first barrier orders the LDS reuse)
    const uint64_t row0 = t * kTile;
    if (c.width == 8)
      move_tile<uint64_t>((const uint64_t *)c.src, (uint64_t *)c.dst, c.n, c.vec, row0, base, cnt, sw, spre,
                          stage);
    else if (c.width == 4)
      move_tile<uint32_t>((const uint32_t *)c.src, (uint32_t *)c.dst, c.n, c.vec, row0, base, cnt, sw, spre,
                          reinterpret_cast<uint32_t *>(stage));
    else
      move_tile<uint8_t>((const uint8_t *)c.src, (uint8_t *)c.dst, c.n, c.vec, row0, base, cnt, sw, spre,
                         reinterpret_cast<uint8_t *>(stage));
    if (c.src_valid != nullptr) {
      // validity: wave w takes words w, w + 4, ...; lane l's bit goes to output bit (its rank among
      // the word's kept lanes); the word's bits are OR-reduced over the wave and lane 0 merges the
      // run into the tile's LDS bitmap, which starts at bit (base & 31) of global word base / 32
      const unsigned s = (unsigned)(base & 31);
      for (int k = w; k < kTileWords; k += kBlock / kWave) {
        const uint64_t word = sw[k];
        if (word == 0) continue;
        const uint64_t row = row0 + (uint64_t)k * 64 + lane;
        const bool keep = (word >> lane) & 1;
        uint64_t bit = (keep && bit_valid(c.src_valid, row)) ? (1ull << lane_rank(word)) : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bit |= __shfl_xor(bit, o, 64);
        if (lane == 0 && bit) {
          const unsigned pos = s + spre[k], wi = pos >> 5, sh = pos & 31;
          const uint64_t lo = bit << sh;
          const unsigned hi = sh ? (unsigned)(bit >> (64 - sh)) : 0u;
          atomicOr(&sbits[wi], (unsigned)lo);
          atomicOr(&sbits[wi + 1], (unsigned)(lo >> 32));
          if (hi) atomicOr(&sbits[wi + 2], hi);
        }
      }
      __syncthreads();
      const unsigned nw = (s + cnt + 31) >> 5;
      uint32_t *out = c.dst_valid + (base >> 5);
      for (unsigned i = threadIdx.x; i < nw; i += kBlock) {
        const unsigned v = sbits[i];
        if (i == 0 || i == nw - 1) {
          if (v) atomicOr(&out[i], v);  // shared with the neighbouring tiles' runs
        } else {
          out[i] = v;
        }
      }
    }
    __syncthreads();
  }
}

// new offsets of a list column: kept row i (output row j) starts at the rank of its first leaf
// among the kept leaves; out[m] = the number of kept leaves
__global__ __launch_bounds__(kBlock) void compact_offsets_kernel(const int64_t *__restrict__ off, uint64_t n,
                                                                 Plan rows, Plan leaves, uint64_t nl,
                                                                 int64_t *__restrict__ out) {
  const int64_t o0 = off[0];
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    if (!row_kept(rows, i)) continue;
    out[plan_rank(rows, n, i)] = (int64_t)plan_rank(leaves, nl, (uint64_t)(off[i] - o0));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[rows.base[rows.ntiles]] = nl ? (int64_t)leaves.base[leaves.ntiles] : 0;
}

inline bool a256(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 255) == 0; }

int check_ws(const void *ws, uint64_t ws_bytes, uint64_t n) {
  NVT_CHECK_ARG(n <= kMaxRows, "n must be below 2^32 - 2048 rows");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG(a256(ws), "workspace must be 256-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= plan_bytes(n), "workspace smaller than nvt_compact_ws_bytes(n)");
  return NVT_OK;
}

unsigned tile_grid(uint64_t ntiles, unsigned cap = kGridCap) {
  return (unsigned)(ntiles < cap ? (ntiles ? ntiles : 1) : cap);
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_compact_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  NVT_CHECK_ARG(n <= kMaxRows, "n must be below 2^32 - 2048 rows");
  *bytes = plan_bytes(n);
  return NVT_OK;
}

int nvt_compact_keep_mask(const uint8_t *mask, uint64_t n, void *ws, uint64_t ws_bytes, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(mask, "null mask");
  const int rc = check_ws(ws, ws_bytes, n);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan_of(ws, n);
  NVT_PROF("compact_keep", n + p.ntiles * (kTile / 8 + 4), s);
  keep_mask_kernel<<<tile_grid(p.ntiles), kBlock, 0, s>>>(mask, n, p);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_compact_keep_dropna(const nvt_dropna_col *cols, int ncols, uint64_t n, void *ws, uint64_t ws_bytes,
                            void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  uint64_t bytes = 0;
  for (int i = 0; i < ncols; ++i) {
    const nvt_dropna_col &c = cols[i];
    NVT_CHECK_ARG(c.dtype >= NVT_F32 && c.dtype <= NVT_U8, "unsupported dtype");
    const bool flt = c.dtype == NVT_F32 || c.dtype == NVT_F64;
    NVT_CHECK_ARG(!flt || c.x || n == 0, "null x of a float column");
    bytes += (c.valid ? n / 8 : 0) + (flt ? n * (c.dtype == NVT_F32 ? 4 : 8) : 0);
  }
  if (n == 0) return NVT_OK;
  const int rc = check_ws(ws, ws_bytes, n);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan_of(ws, n);
  NVT_PROF("compact_keep", bytes + p.ntiles * (kTile / 8 + 4), s);
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {  // more than kMaxCols columns: AND into the mask
    NaBatch b;
    memset(&b, 0, sizeof(b));
    b.ncols = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
    for (int j = 0; j < b.ncols; ++j) b.c[j] = NaCol{cols[i0 + j].x, cols[i0 + j].valid, cols[i0 + j].dtype};
    keep_dropna_kernel<<<tile_grid(p.ntiles), kBlock, 0, s>>>(b, n, p, i0 > 0);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_compact_keep_terms(const nvt_filter_col *cols, int ncols, const nvt_filter_term *terms, int nterms,
                           const void *sets, uint64_t set_words, uint64_t n, void *ws, uint64_t ws_bytes,
                           void *stream) {
  NVT_CHECK_ARG(cols && terms, "null descriptors");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= NVT_FILTER_MAX_COLS, "ncols must be 1 to NVT_FILTER_MAX_COLS");
  NVT_CHECK_ARG(nterms >= 1 && nterms <= NVT_FILTER_MAX_TERMS, "nterms must be 1 to NVT_FILTER_MAX_TERMS");
  NVT_CHECK_ARG(sets || set_words == 0, "null sets");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(sets) & 7) == 0, "sets must be 8-byte aligned");
  static const int kWidth[] = {4, 8, 4, 8, 1, 1, 2};  // NVT_F32 .. NVT_I16
  uint64_t bytes = 0;
  for (int j = 0; j < ncols; ++j) {
    const nvt_filter_col &c = cols[j];
    NVT_CHECK_ARG(c.dtype >= NVT_F32 && c.dtype <= NVT_I16, "unsupported dtype");
    NVT_CHECK_ARG(c.x || n == 0, "null x");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.x) & (kWidth[c.dtype] - 1)) == 0, "x must be aligned to its dtype");
    bytes += n * kWidth[c.dtype] + (c.valid ? n / 8 : 0);
  }
  for (int k = 0; k < nterms; ++k) {
    const nvt_filter_term &t = terms[k];
    NVT_CHECK_ARG(t.col >= 0 && t.col < ncols, "a term's col is no descriptor");
    NVT_CHECK_ARG(t.op >= NVT_FILTER_EQ && t.op <= NVT_FILTER_NOT_IN, "unknown op");
    NVT_CHECK_ARG(t.conj >= 0 && (k == 0 || t.conj >= terms[k - 1].conj), "terms must be sorted by conj");
    if (t.op == NVT_FILTER_IN || t.op == NVT_FILTER_NOT_IN) {
      NVT_CHECK_ARG(t.set_len >= 0, "set_len must not be negative");
      NVT_CHECK_ARG(t.set_off <= set_words && (uint64_t)t.set_len <= set_words - t.set_off,
                    "set_off + set_len lies past set_words");
    }
  }
  if (n == 0) return NVT_OK;
  const int rc = check_ws(ws, ws_bytes, n);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan_of(ws, n);
  FBatch b;
  memset(&b, 0, sizeof(b));
  for (int j = 0; j < ncols; ++j) b.c[j] = FCol{cols[j].x, cols[j].valid, cols[j].dtype};
  for (int k = 0; k < nterms; ++k) {
    const nvt_filter_term &t = terms[k];
    FTerm &d = b.t[k];
    d.col = t.col;
    d.op = t.op;
    d.conj = t.conj;
    d.set_len = t.set_len;
    d.set_off = t.set_off;
    d.value.i = t.value.i;
  }
  b.sets = reinterpret_cast<const uint64_t *>(sets);
  b.nterms = nterms;
  NVT_PROF("compact_keep_terms", bytes + p.ntiles * (kTile / 8 + 4), s);
  keep_terms_kernel<<<tile_grid(p.ntiles), kBlock, 0, s>>>(b, n, p);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_compact_plan(uint64_t n, void *ws, uint64_t ws_bytes, uint64_t *out_m, void *stream) {
  if (n == 0) return NVT_OK;
  const int rc = check_ws(ws, ws_bytes, n);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan_of(ws, n);
  NVT_PROF("compact_plan", (p.ntiles + 1) * 8, s);
  const int sr = exclusive_scan_u32(p.base, p.ntiles + 1, p.chunk, s);
  if (sr) return sr;
  if (out_m) {
    plan_total_kernel<<<1, 1, 0, s>>>(p.base, p.ntiles, out_m);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_compact_list_keep(const int64_t *offsets, uint64_t n, const void *row_plan, uint64_t n_leaves,
                          void *leaf_ws, uint64_t leaf_ws_bytes, void *stream) {
  if (n == 0 || n_leaves == 0) return NVT_OK;
  NVT_CHECK_ARG(offsets && row_plan, "null pointer");
  NVT_CHECK_ARG(n <= kMaxRows, "n must be below 2^32 - 2048 rows");
  NVT_CHECK_ARG(a256(row_plan), "row plan must be 256-byte aligned");
  const int rc = check_ws(leaf_ws, leaf_ws_bytes, n_leaves);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const Plan leaves = plan_of(leaf_ws, n_leaves);
  NVT_PROF("compact_list_keep", (n + 1) * 8 + leaves.ntiles * (kTile / 8 + 4), s);
  keep_expand_kernel<<<stream_grid(leaves.ntiles * kTileWords, kBlock), kBlock, 0, s>>>(
      offsets, n, plan_of(row_plan, n), n_leaves, leaves);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_compact_list_offsets(const int64_t *offsets, uint64_t n, const void *row_plan, const void *leaf_plan,
                             uint64_t n_leaves, int64_t *out_offsets, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(offsets && row_plan && out_offsets && (leaf_plan || n_leaves == 0), "null pointer");
  NVT_CHECK_ARG(n <= kMaxRows && n_leaves <= kMaxRows, "n and n_leaves must be below 2^32 - 2048");
  NVT_CHECK_ARG(a256(row_plan) && (n_leaves == 0 || a256(leaf_plan)), "plans must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("compact_list_offsets", n * 16, s);
  compact_offsets_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(
      offsets, n, plan_of(row_plan, n), plan_of(n_leaves ? leaf_plan : row_plan, n_leaves), n_leaves,
      out_offsets);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_compact_many(const nvt_compact_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  for (int i = 0; i < ncols; ++i) {
    const nvt_compact_col &c = cols[i];
    NVT_CHECK_ARG(c.width == 1 || c.width == 4 || c.width == 8, "width must be 1, 4 or 8 bytes");
    NVT_CHECK_ARG(c.n <= kMaxRows, "n must be below 2^32 - 2048 rows");
    NVT_CHECK_ARG(!c.dst_valid == !c.src_valid, "src_valid and dst_valid go together");
    if (c.n == 0) continue;
    NVT_CHECK_ARG(c.src && c.dst && c.plan, "null pointer");
    NVT_CHECK_ARG(a256(c.plan), "plan must be 256-byte aligned");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.dst_valid) & 3) == 0, "dst_valid must be 4-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    CBatch b;
    memset(&b, 0, sizeof(b));
    const int k = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
    uint64_t maxn = 0, bytes = 0;
    bool bitmaps = false;
    for (int j = 0; j < k; ++j) {
      const nvt_compact_col &c = cols[i0 + j];
      CCol &d = b.c[j];
      d.src = c.src;
      d.dst = c.dst;
      d.src_valid = c.src_valid;
      d.dst_valid = reinterpret_cast<uint32_t *>(c.dst_valid);
      d.plan = c.plan;
      d.n = c.n;
      d.width = c.width;
      d.vec = (reinterpret_cast<uintptr_t>(c.src) & 15) == 0;
      maxn = c.n > maxn ? c.n : maxn;
      bitmaps |= c.src_valid != nullptr && c.n > 0;
      bytes += c.n * (uint64_t)c.width * 2 + (c.src_valid ? c.n / 4 : 0) + ntiles_of(c.n) * (kTile / 8);
    }
    if (maxn == 0) continue;
    NVT_PROF("compact_many", bytes, s);
    if (bitmaps) {
      compact_zero_kernel<<<dim3(stream_grid(maxn / 32 + 1, kBlock, 1), k), kBlock, 0, s>>>(b);
      NVT_CHECK_LAUNCH();
    }
    const unsigned gx = tile_grid(ntiles_of(maxn), kGridCap / k > 0 ? kGridCap / k : 1);
    compact_kernel<<<dim3(gx, k), kBlock, 0, s>>>(b);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
