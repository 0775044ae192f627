// Batch gather of a dataloader chunk (nvtabular_amd/kernels_loader.py, loader/torch.py).
//
// take_kernel: one lane per OUTPUT row and tile of 256 rows.  The lane reads index[j] once
//   (coalesced), checks it against n_src and then walks every column of the launch: the source
//   reads are the shuffle's random reads, everything else is in row order.  A wave's 64 rows make
//   one validity word (__ballot), stored whole.
//   Stacked output (several columns of the launch are the columns of one row-major [m, k] matrix):
//   a lane storing its own element would write 64 addresses k elements apart.  Instead the lanes
//   write their elements into an LDS image of the tile's 256 rows -- the tile is one contiguous byte
//   range of the matrix that starts on a 16-byte boundary, since 256 * row bytes is a multiple of
//   16 -- and the block then copies the image out flat, 16 bytes per lane and step
//   (ds_read_b128 from consecutive slots: conflict-free; one global_store_dwordx4 per lane).
//   The LDS writes are one element per lane, a row apart: for rows of 13 floats (13 dwords, odd)
//   they are conflict-free, for rows of 26 int64 (52 dwords, gcd(52, 32) = 4) 4-way; that costs a
//   few LDS cycles per element next to a random HBM read per element and was left alone.
// Lists: take_len_kernel / scan_totals_kernel / take_add_kernel give the new offsets as
//   nvt_list_slice_offsets does; take_move_kernel spreads the work over the OUTPUT leaves, the row
//   of a leaf found by the staged search of slice_move_kernel (nvt_list_tile.hpp).
// Sources: every kernel is a template over WHERE a row comes from.  OneSource is the single-source
//   entry: the row number is the index and the descriptor carries src / src_valid / src_dtype.
//   MultiSource is a chunk of several partitions: index[j] is a row of their concatenation, the
//   source s is found by a search in src_begin[0 .. nsrc] (the last s with src_begin[s] <= i, which
//   steps over empty sources), and {src, src_valid, src_dtype} of (column, s) is read from a table
//   in device memory: [ncols][nsrc] records of nvt_take_src, the descriptor's src pointing at its
//   column's row of the table.  src_begin is copied into LDS once per block when it fits (behind
//   the tile image of take_kernel, whose dynamic LDS stays within 64 KiB; a static array of
//   kSrcStage entries in the list kernels) and searched in memory otherwise.  Casts, null policy,
//   ballots and staging are the one copy both instantiations share.
#include "nvt_common.hpp"
#include "nvt_list_tile.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr int kTakeCols = NVT_TAKE_MAX_COLS;
constexpr int kTakeGroups = NVT_TAKE_MAX_GROUPS;
constexpr int kListCols = NVT_LIST_MAX_COLS;

struct TCol {
  const void *src;
  const uint8_t *src_valid;
  void *dst;
  uint64_t *dst_valid;
  int64_t stride;  // plain: elements between rows; member of a staged matrix: byte offset in the row
  int sd, dd;
};
struct TGroup {
  void *base;  // row 0 of the matrix
  int first, count, row_bytes, pad_;
};
struct TBatch {
  TCol c[kTakeCols];  // [0, nplain): stored by their lane; then the members of g[0], g[1], ...
  TGroup g[kTakeGroups];
  int nplain, ngroups;
};
struct LBatch {
  TCol c[kListCols];
  int ncols;
};

__host__ __device__ inline int dt_size(int d) {
  switch (d) {
    case NVT_F32:
    case NVT_I32: return 4;
    case NVT_F64:
    case NVT_I64: return 8;
    case NVT_I16: return 2;
    default: return 1;
  }
}
inline bool dt_known(int d) { return d >= NVT_F32 && d <= NVT_I16; }
inline bool dt_float(int d) { return d == NVT_F32 || d == NVT_F64; }

// *p = (destination type) v, or the null of the destination type
template <typename S>
__device__ __forceinline__ void put_as(S v, bool ok, int dd, void *p) {
  switch (dd) {
    case NVT_F32: *(float *)p = ok ? (float)v : __builtin_nanf(""); break;
    case NVT_F64: *(double *)p = ok ? (double)v : __builtin_nan(""); break;
    case NVT_I64: *(int64_t *)p = ok ? (int64_t)v : 0; break;
    case NVT_I32: *(int32_t *)p = ok ? (int32_t)v : 0; break;
    case NVT_I16: *(int16_t *)p = ok ? (int16_t)v : (int16_t)0; break;
    case NVT_I8: *(int8_t *)p = ok ? (int8_t)v : (int8_t)0; break;
    default: *(uint8_t *)p = ok ? (uint8_t)v : (uint8_t)0; break;
  }
}
template <typename S>
__device__ __forceinline__ void take_as(const void *src, uint64_t i, bool ok, int dd, void *p) {
  S v = S(0);
  if (ok) v = ((const S *)src)[i];  // (a null or out-of-range row is never read)
  put_as<S>(v, ok, dd, p);
}
__device__ __forceinline__ void take_one(const void *src, int sd, int dd, uint64_t i, bool ok, void *p) {
  switch (sd) {
    case NVT_F32: take_as<float>(src, i, ok, dd, p); break;
    case NVT_F64: take_as<double>(src, i, ok, dd, p); break;
    case NVT_I32: take_as<int32_t>(src, i, ok, dd, p); break;
    case NVT_I64: take_as<int64_t>(src, i, ok, dd, p); break;
    case NVT_I16: take_as<int16_t>(src, i, ok, dd, p); break;
    case NVT_I8: take_as<int8_t>(src, i, ok, dd, p); break;
    default: take_as<uint8_t>(src, i, ok, dd, p); break;
  }
}

// ---- where a row comes from -------------------------------------------------------------------------
constexpr int kSrcStage = 1024 + 1;  // entries of src_begin a block holds in LDS

struct Row {
  unsigned s;   // source
  uint64_t i;   // row inside it
};
struct OneSource {
  static constexpr bool kMulti = false;
  uint64_t n;              // rows of the source
  const int64_t *off;      // list kernels: its offsets
  __device__ __forceinline__ void stage(int64_t *) {}
  __device__ __forceinline__ bool find(int64_t i, Row &r) const {
    r.s = 0;
    r.i = (uint64_t)i;
    return (uint64_t)i < n;
  }
  __device__ __forceinline__ const int64_t *offsets(unsigned) const { return off; }
  __device__ __forceinline__ void source(const TCol &c, unsigned, const void *&src, const uint8_t *&valid,
                                         int &sd) const {
    src = c.src;
    valid = c.src_valid;
    sd = c.sd;
  }
};
struct MultiSource {
  static constexpr bool kMulti = true;
  const int64_t *begin;        // src_begin[0 .. nsrc]; after stage(): the copy that is searched
  const int64_t *const *offs;  // list kernels: offsets of every source
  unsigned nsrc;               // >= 1
  int staged;                  // src_begin fits the LDS the launch set aside (host's decision)
  __device__ __forceinline__ void stage(int64_t *lds) {
    if (!staged) return;  // (block-uniform)
    for (unsigned k = threadIdx.x; k <= nsrc; k += kBlock) lds[k] = begin[k];
    __syncthreads();
    begin = lds;
  }
  __device__ __forceinline__ bool find(int64_t i, Row &r) const {
    r.s = 0;
    r.i = 0;
    if (i < 0 || i >= begin[nsrc]) return false;
    r.s = (unsigned)row_of(begin, 0, nsrc - 1, i);
    r.i = (uint64_t)(i - begin[r.s]);
    return true;
  }
  __device__ __forceinline__ const int64_t *offsets(unsigned s) const { return offs[s]; }
  __device__ __forceinline__ void source(const TCol &c, unsigned s, const void *&src, const uint8_t *&valid,
                                         int &sd) const {
    const nvt_take_src &t = reinterpret_cast<const nvt_take_src *>(c.src)[s];
    src = t.src;
    valid = t.src_valid;
    sd = t.src_dtype;
  }
};

// one element of column c: read (never for a null or out-of-range row), cast, stored at p
template <typename R>
__device__ __forceinline__ bool take_elem(const R &r, const TCol &c, const Row &at, bool in, bool live, void *p) {
  const void *src = nullptr;
  const uint8_t *valid = nullptr;
  int sd = NVT_U8;
  if (in) r.source(c, at.s, src, valid, sd);
  const bool ok = in && bit_valid(valid, at.i);
  if (live) take_one(src, sd, c.dd, at.i, ok, p);
  return ok;
}

constexpr int kTakeTile = kBlock;  // rows per tile: one per lane

template <typename R>
__global__ __launch_bounds__(kBlock) void take_kernel(TBatch b, R r, const int64_t *__restrict__ index, uint64_t m,
                                                      unsigned image_bytes) {
  extern __shared__ uint4 stage[];
  const unsigned lane = lane_id();
  r.stage(reinterpret_cast<int64_t *>(reinterpret_cast<char *>(stage) + image_bytes));
  const uint64_t nt = (m + kTakeTile - 1) / kTakeTile;
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r0 = t * kTakeTile, j = r0 + threadIdx.x;
    const bool live = j < m;
    int64_t i = -1;
    if (live) i = index != nullptr ? index[j] : (int64_t)j;
    Row at;
    const bool in = r.find(i, at) && live;
    for (int ci = 0; ci < b.nplain; ++ci) {
      const TCol &c = b.c[ci];
      const bool ok = take_elem(r, c, at, in, live, (char *)c.dst + j * (uint64_t)c.stride * dt_size(c.dd));
      if (c.dst_valid != nullptr) {  // (block-uniform: every lane of the wave reaches the ballot)
        const uint64_t word = __ballot(ok);
        if (lane == 0 && live) c.dst_valid[j >> 6] = word;
      }
    }
    for (int gi = 0; gi < b.ngroups; ++gi) {
      const TGroup &g = b.g[gi];
      char *image = reinterpret_cast<char *>(stage);
      for (int ci = g.first; ci < g.first + g.count; ++ci) {
        const TCol &c = b.c[ci];
        const bool ok = take_elem(r, c, at, in, live, image + (uint64_t)threadIdx.x * g.row_bytes + c.stride);
        if (c.dst_valid != nullptr) {
          const uint64_t word = __ballot(ok);
          if (lane == 0 && live) c.dst_valid[j >> 6] = word;
        }
      }
      __syncthreads();
      const uint64_t rows = m - r0 < (uint64_t)kTakeTile ? m - r0 : (uint64_t)kTakeTile;
      const unsigned bytes = (unsigned)rows * (unsigned)g.row_bytes;
      char *out = (char *)g.base + r0 * (uint64_t)g.row_bytes;  // (16-byte aligned)
      for (unsigned o = threadIdx.x * 16; o + 16 <= bytes; o += kBlock * 16)
        *reinterpret_cast<uint4 *>(out + o) = *reinterpret_cast<const uint4 *>(image + o);
      const unsigned tail = bytes & ~15u;  // (rows are whole 4-byte words: at most 3 of them are left)
      if (tail + threadIdx.x * 4 < bytes)
        *reinterpret_cast<uint32_t *>(out + tail + threadIdx.x * 4) =
            *reinterpret_cast<const uint32_t *>(image + tail + threadIdx.x * 4);
      __syncthreads();
    }
  }
}

// ---- lists: new offsets ---------------------------------------------------------------------------
template <typename R>
__device__ __forceinline__ uint64_t take_len(const R &r, const int64_t *index, uint64_t j) {
  const int64_t i = index != nullptr ? index[j] : (int64_t)j;
  Row at;
  if (!r.find(i, at)) return 0;
  const int64_t *off = r.offsets(at.s);
  return (uint64_t)(off[at.i + 1] - off[at.i]);
}

// src_begin of the list kernels' block (MultiSource only: OneSource keeps no such array)
template <typename R>
__device__ __forceinline__ void stage_sources(R &r) {
  if constexpr (R::kMulti) {
    __shared__ int64_t sbegin[kSrcStage];
    r.stage(sbegin);
  }
}

template <typename R>
__global__ __launch_bounds__(kBlock) void take_len_kernel(R r, const int64_t *__restrict__ index, uint64_t m,
                                                          int64_t *__restrict__ out,
                                                          unsigned long long *__restrict__ tile_tot) {
  __shared__ uint64_t wsum[kBlock / kWave];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  stage_sources(r);
  const uint64_t nt = list_ntiles(m);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r0 = t * kListTile + (uint64_t)threadIdx.x * 8;  // 8 consecutive rows per lane
    uint64_t len[8], tot = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      len[k] = r0 + k < m ? take_len(r, index, r0 + k) : 0;
      tot += len[k];
    }
    const uint64_t inc = wave_incl_scan(tot);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t run = inc - tot;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (r0 + k < m) out[r0 + k] = (int64_t)run;
      run += len[k];
    }
    if (threadIdx.x == kBlock - 1) tile_tot[t] = run;
    __syncthreads();
  }
}

template <typename R>
__global__ __launch_bounds__(kBlock) void take_add_kernel(int64_t *__restrict__ out, uint64_t m,
                                                          const unsigned long long *__restrict__ tile_base, R r,
                                                          const int64_t *__restrict__ index) {
  // (r is not staged: one lane of the launch searches src_begin, in memory)
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
    const int64_t v = out[j] + (int64_t)tile_base[j / kListTile];
    out[j] = v;
    if (j == m - 1) out[m] = v + (int64_t)take_len(r, index, j);
  }
}

// ---- lists: leaves --------------------------------------------------------------------------------
template <typename R>
__global__ __launch_bounds__(kBlock) void take_move_kernel(LBatch b, R r, const int64_t *__restrict__ index,
                                                           const int64_t *__restrict__ noff, uint64_t m,
                                                           uint64_t total) {
  __shared__ int64_t soff[kListStage];
  __shared__ uint64_t sbound[2];
  const unsigned lane = lane_id();
  stage_sources(r);
  int64_t o0 = 0;  // (one source: its first offset, read once)
  if constexpr (!R::kMulti) o0 = r.off[0];
  const uint64_t nt = list_ntiles(total);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t p0 = t * kListTile;
    const uint64_t p1 = p0 + kListTile < total ? p0 + kListTile : total;
    if (threadIdx.x < 2) sbound[threadIdx.x] = row_of(noff, 0, m - 1, (int64_t)(threadIdx.x == 0 ? p0 : p1 - 1));
    __syncthreads();
    const uint64_t rlo = sbound[0], rhi = sbound[1];
    const bool staged = rhi - rlo + 2 <= (uint64_t)kListStage;  // (block-uniform)
    if (staged)
      for (uint64_t k = threadIdx.x; k < rhi - rlo + 2; k += kBlock) soff[k] = noff[rlo + k];
    __syncthreads();
    for (uint64_t q = p0 + threadIdx.x; q < p0 + kListTile; q += kBlock) {  // (q - lane is a multiple of 64)
      const bool live = q < p1;
      Row at{0, 0};  // the leaf's source and its place among that source's leaves
      if (live) {
        uint64_t row, k;
        if (staged) {
          const uint64_t r = row_of(soff, 0, rhi - rlo, (int64_t)q);
          row = rlo + r;
          k = q - (uint64_t)soff[r];
        } else {
          row = row_of(noff, rlo, rhi, (int64_t)q);
          k = q - (uint64_t)noff[row];
        }
        // (a row that holds a leaf is not empty: its index is inside the source)
        const int64_t i = index != nullptr ? index[row] : (int64_t)row;
        r.find(i, at);
        const int64_t *off = r.offsets(at.s);
        at.i = (uint64_t)(off[at.i] - (R::kMulti ? off[0] : o0)) + k;
      }
      for (int ci = 0; ci < b.ncols; ++ci) {
        const TCol &c = b.c[ci];
        const bool ok = take_elem(r, c, at, live, live, (char *)c.dst + q * dt_size(c.dd));
        if (c.dst_valid != nullptr) {  // (block-uniform: every lane of the wave reaches the ballot)
          const uint64_t word = __ballot(ok);
          if (lane == 0 && live) c.dst_valid[q >> 6] = word;
        }
      }
    }
    __syncthreads();
  }
}

// the checks every descriptor of both gathers passes before a launch
// (multi: src is the column's row of the source table, the source dtypes live there)
int check_take_col(const char *fn, const nvt_take_col &c, bool rows, bool strided, bool multi = false) {
#define TAKE_ARG(cond, msg)                 \
  do {                                      \
    if (!(cond)) {                          \
      nvt::set_error("%s: %s", fn, msg);    \
      return NVT_EINVAL;                    \
    }                                       \
  } while (0)
  TAKE_ARG(multi || dt_known(c.src_dtype), "src_dtype must be NVT_F32 .. NVT_I16");
  TAKE_ARG(dt_known(c.dst_dtype), "dst_dtype must be NVT_F32 .. NVT_I16");
  TAKE_ARG(multi || c.dst_dtype == c.src_dtype || dt_float(c.dst_dtype) ||
               (c.dst_dtype == NVT_I64 && !dt_float(c.src_dtype)),
           "dst_dtype must be src_dtype, NVT_I64 from an integer source, or NVT_F32 / NVT_F64");
  TAKE_ARG(c.dst_stride >= 1, "dst_stride must be at least 1");
  TAKE_ARG(strided || c.dst_stride == 1, "dst_stride must be 1 for leaves");
  TAKE_ARG(!rows || (c.src && c.dst), multi ? "null source table / dst" : "null src / dst");
  TAKE_ARG((reinterpret_cast<uintptr_t>(c.src) & (multi ? 7 : dt_size(c.src_dtype) - 1)) == 0,
           multi ? "source table must be 8-byte aligned" : "src must be aligned to its element size");
  TAKE_ARG((reinterpret_cast<uintptr_t>(c.dst) & (dt_size(c.dst_dtype) - 1)) == 0,
           "dst must be aligned to its element size");
  TAKE_ARG((reinterpret_cast<uintptr_t>(c.dst_valid) & 7) == 0, "dst_valid must be 8-byte aligned");
#undef TAKE_ARG
  return NVT_OK;
}

TCol to_tcol(const nvt_take_col &c) {
  return TCol{c.src, c.src_valid, c.dst, reinterpret_cast<uint64_t *>(c.dst_valid), c.dst_stride, c.src_dtype,
              c.dst_dtype};
}

// Descriptors [0, k) of one launch -> TBatch: the columns that make up whole matrices go behind the
// others, matrix by matrix.  Returns the LDS bytes the launch needs.
unsigned plan_batch(const nvt_take_col *cols, int k, TBatch &b) {
  memset(&b, 0, sizeof(b));
  int group_of[kTakeCols];
  for (int i = 0; i < k; ++i) group_of[i] = -1;
  unsigned lds = 0;
  int members = 0;
  for (int a = 0; a < k && b.ngroups < kTakeGroups; ++a) {
    const nvt_take_col &ca = cols[a];
    const int es = dt_size(ca.dst_dtype);
    if (group_of[a] != -1 || ca.dst_stride < 2 || es < 4) continue;
    const uint64_t row_bytes = (uint64_t)ca.dst_stride * es;
    if (row_bytes > NVT_TAKE_STAGE_ROW_BYTES) continue;
    // every column of the launch that lies in the same row as `a`
    int set[kTakeCols], ns = 0;
    uintptr_t base = reinterpret_cast<uintptr_t>(ca.dst);
    for (int j = a; j < k; ++j) {
      const nvt_take_col &cj = cols[j];
      if (group_of[j] != -1 || cj.dst_stride != ca.dst_stride || cj.dst_dtype != ca.dst_dtype) continue;
      const uintptr_t pa = reinterpret_cast<uintptr_t>(ca.dst), pj = reinterpret_cast<uintptr_t>(cj.dst);
      if ((pj > pa ? pj - pa : pa - pj) >= row_bytes) continue;
      set[ns++] = j;
      base = pj < base ? pj : base;
    }
    bool whole = ns == ca.dst_stride && (base & 15) == 0;
    uint64_t seen[4] = {0, 0, 0, 0};  // (a row holds at most 256 / 4 = 64 elements)
    for (int q = 0; q < ns && whole; ++q) {
      const uint64_t d = reinterpret_cast<uintptr_t>(cols[set[q]].dst) - base;
      const uint64_t e = d / es;
      whole = d < row_bytes && d % es == 0 && !((seen[e >> 6] >> (e & 63)) & 1);
      seen[e >> 6] |= 1ull << (e & 63);
    }
    if (!whole) continue;
    for (int q = 0; q < ns; ++q) group_of[set[q]] = b.ngroups;
    b.g[b.ngroups] = TGroup{reinterpret_cast<void *>(base), 0, ns, (int)row_bytes, 0};
    members += ns;
    ++b.ngroups;
    lds = (unsigned)(row_bytes * kTakeTile) > lds ? (unsigned)(row_bytes * kTakeTile) : lds;
  }
  b.nplain = k - members;
  int at = 0;
  for (int i = 0; i < k; ++i)
    if (group_of[i] == -1) b.c[at++] = to_tcol(cols[i]);
  for (int g = 0; g < b.ngroups; ++g) {
    b.g[g].first = at;
    for (int i = 0; i < k; ++i)
      if (group_of[i] == g) {
        b.c[at] = to_tcol(cols[i]);
        b.c[at].stride = (int64_t)(reinterpret_cast<uintptr_t>(cols[i].dst) - reinterpret_cast<uintptr_t>(b.g[g].base));
        ++at;
      }
  }
  return lds;
}

int check_sources(const char *fn, const int64_t *src_begin, int nsrc) {
  if (nsrc < 1 || nsrc > NVT_TAKE_MAX_SOURCES) {
    nvt::set_error("%s: nsrc must be in [1, NVT_TAKE_MAX_SOURCES = %d]", fn, NVT_TAKE_MAX_SOURCES);
    return NVT_EINVAL;
  }
  if (!src_begin || (reinterpret_cast<uintptr_t>(src_begin) & 7) != 0) {
    nvt::set_error("%s: %s", fn, src_begin ? "src_begin must be 8-byte aligned" : "null src_begin");
    return NVT_EINVAL;
  }
  return NVT_OK;
}

// the launches of nvt_batch_take_many / _multi: one per kTakeCols descriptors.  `extra` = LDS bytes
// behind the tile image for the staged src_begin, given up when the two pass 64 KiB together.
template <typename R>
int launch_take(const char *name, R r, const int64_t *index, uint64_t m, const nvt_take_col *cols, int ncols,
                unsigned extra, hipStream_t s) {
  const unsigned grid = stream_grid((m + kTakeTile - 1) / kTakeTile, 1);
  for (int i0 = 0; i0 < ncols; i0 += kTakeCols) {
    const int k = ncols - i0 < kTakeCols ? ncols - i0 : kTakeCols;
    TBatch b;
    const unsigned lds = plan_batch(cols + i0, k, b);
    uint64_t bytes = index ? m * 8 : 0;
    for (int j = 0; j < k; ++j) {
      const nvt_take_col &c = cols[i0 + j];
      const int ss = R::kMulti ? dt_size(c.dst_dtype) : dt_size(c.src_dtype);  // (multi: per source, not known here)
      bytes += m * (uint64_t)(ss + dt_size(c.dst_dtype)) + (c.dst_valid ? m / 4 : 0);
    }
    unsigned more = extra;
    if constexpr (R::kMulti) {
      if (lds + extra > 65536u) more = 0;
      r.staged = more != 0;
    }
    NVT_PROF(name, bytes, s);
    take_kernel<R><<<grid, kBlock, lds + more, s>>>(b, r, index, m, lds);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

template <typename R>
int launch_take_offsets(R r, const int64_t *index, uint64_t m, int64_t *out_offsets, unsigned long long *tot,
                        hipStream_t s) {
  const uint64_t nt = list_ntiles(m);
  take_len_kernel<R><<<stream_grid(nt, 1), kBlock, 0, s>>>(r, index, m, out_offsets, tot);
  NVT_CHECK_LAUNCH();
  scan_totals_kernel<<<1, kBlock, 0, s>>>(tot, nt);
  NVT_CHECK_LAUNCH();
  if constexpr (R::kMulti) r.staged = 0;
  take_add_kernel<R><<<stream_grid(m, kBlock), kBlock, 0, s>>>(out_offsets, m, tot, r, index);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

template <typename R>
int launch_take_leaves(const char *name, R r, const nvt_take_col *cols, int ncols, const int64_t *index,
                       const int64_t *out_offsets, uint64_t m, uint64_t total, hipStream_t s) {
  const unsigned grid = stream_grid(list_ntiles(total), 1);
  for (int i0 = 0; i0 < ncols; i0 += kListCols) {
    LBatch b;
    memset(&b, 0, sizeof(b));
    b.ncols = ncols - i0 < kListCols ? ncols - i0 : kListCols;
    uint64_t bytes = (m + 1) * 8;
    for (int j = 0; j < b.ncols; ++j) {
      const nvt_take_col &c = cols[i0 + j];
      b.c[j] = to_tcol(c);
      const int ss = R::kMulti ? dt_size(c.dst_dtype) : dt_size(c.src_dtype);
      bytes += total * (uint64_t)(ss + dt_size(c.dst_dtype)) + (c.dst_valid ? total / 4 : 0);
    }
    NVT_PROF(name, bytes, s);
    take_move_kernel<R><<<grid, kBlock, 0, s>>>(b, r, index, out_offsets, m, total);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_batch_take_many(const int64_t *index, uint64_t m, uint64_t n_src, const nvt_take_col *cols, int ncols,
                        void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must not be negative");
  NVT_CHECK_ARG(cols || ncols == 0, "null descriptors");
  NVT_CHECK_ARG(index || m <= n_src, "index == NULL (identity) needs m <= n_src");
  for (int i = 0; i < ncols; ++i) {
    const int rc = check_take_col(__func__, cols[i], m > 0, true);
    if (rc != NVT_OK) return rc;
  }
  if (m == 0 || ncols == 0) return NVT_OK;
  return launch_take("batch_take_many", OneSource{n_src, nullptr}, index, m, cols, ncols, 0, (hipStream_t)stream);
}

int nvt_batch_take_multi(const int64_t *index, uint64_t m, const int64_t *src_begin, int nsrc, uint64_t n_total,
                         const nvt_take_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must not be negative");
  NVT_CHECK_ARG(cols || ncols == 0, "null descriptors");
  const int rs = check_sources(__func__, src_begin, nsrc);
  if (rs != NVT_OK) return rs;
  NVT_CHECK_ARG(index || m <= n_total, "index == NULL (identity) needs m <= n_total");
  for (int i = 0; i < ncols; ++i) {
    const int rc = check_take_col(__func__, cols[i], m > 0, true, true);
    if (rc != NVT_OK) return rc;
  }
  if (m == 0 || ncols == 0) return NVT_OK;
  const unsigned extra = nsrc + 1 <= kSrcStage ? (unsigned)(nsrc + 1) * 8u : 0u;
  return launch_take("batch_take_multi", MultiSource{src_begin, nullptr, (unsigned)nsrc, 0}, index, m, cols, ncols,
                     extra, (hipStream_t)stream);
}

int nvt_take_list_ws_bytes(uint64_t m, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  *bytes = (list_ntiles(m) + 1) * 8;
  return NVT_OK;
}

int nvt_take_list_offsets(const int64_t *offsets, uint64_t n_src, const int64_t *index, uint64_t m,
                          int64_t *out_offsets, void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(out_offsets, "null out_offsets");
  NVT_CHECK_ARG(offsets || n_src == 0, "null offsets");
  NVT_CHECK_ARG(index || m <= n_src, "index == NULL (identity) needs m <= n_src");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace must be 8-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (list_ntiles(m) + 1) * 8, "workspace smaller than nvt_take_list_ws_bytes(m)");
  if (m == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(ws);
  NVT_PROF("take_list_offsets", m * 40, s);
  return launch_take_offsets(OneSource{n_src, offsets}, index, m, out_offsets, tot, s);
}

int nvt_take_list_offsets_multi(const int64_t *const *offsets, const int64_t *src_begin, int nsrc, uint64_t n_total,
                                const int64_t *index, uint64_t m, int64_t *out_offsets, void *ws, uint64_t ws_bytes,
                                void *stream) {
  NVT_CHECK_ARG(out_offsets, "null out_offsets");
  const int rc = check_sources(__func__, src_begin, nsrc);
  if (rc != NVT_OK) return rc;
  NVT_CHECK_ARG(offsets, "null offsets table");
  NVT_CHECK_ARG(index || m <= n_total, "index == NULL (identity) needs m <= n_total");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace must be 8-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (list_ntiles(m) + 1) * 8, "workspace smaller than nvt_take_list_ws_bytes(m)");
  if (m == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("take_list_offsets_multi", m * 40, s);
  return launch_take_offsets(MultiSource{src_begin, offsets, (unsigned)nsrc, nsrc + 1 <= kSrcStage}, index, m,
                             out_offsets, reinterpret_cast<unsigned long long *>(ws), s);
}

int nvt_take_list_many(const nvt_take_col *cols, int ncols, const int64_t *offsets, const int64_t *index,
                       const int64_t *out_offsets, uint64_t m, uint64_t total, void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must not be negative");
  NVT_CHECK_ARG(cols || ncols == 0, "null descriptors");
  for (int i = 0; i < ncols; ++i) {
    const int rc = check_take_col(__func__, cols[i], total > 0, false);
    if (rc != NVT_OK) return rc;
  }
  if (total == 0 || m == 0 || ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(offsets && out_offsets, "null offsets / out_offsets");
  // (n = 0: the leaf kernel never asks whether a row is inside -- a row that holds a leaf is)
  return launch_take_leaves("take_list_many", OneSource{0, offsets}, cols, ncols, index, out_offsets, m, total,
                            (hipStream_t)stream);
}

int nvt_take_list_multi(const nvt_take_col *cols, int ncols, const int64_t *const *offsets, const int64_t *src_begin,
                        int nsrc, const int64_t *index, const int64_t *out_offsets, uint64_t m, uint64_t total,
                        void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must not be negative");
  NVT_CHECK_ARG(cols || ncols == 0, "null descriptors");
  const int rs = check_sources(__func__, src_begin, nsrc);
  if (rs != NVT_OK) return rs;
  for (int i = 0; i < ncols; ++i) {
    const int rc = check_take_col(__func__, cols[i], total > 0, false, true);
    if (rc != NVT_OK) return rc;
  }
  if (total == 0 || m == 0 || ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(offsets && out_offsets, "null offsets table / out_offsets");
  return launch_take_leaves("take_list_multi", MultiSource{src_begin, offsets, (unsigned)nsrc, nsrc + 1 <= kSrcStage},
                            cols, ncols, index, out_offsets, m, total, (hipStream_t)stream);
}

}  // extern "C"
