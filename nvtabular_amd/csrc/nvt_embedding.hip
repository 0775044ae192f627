// Embedding layers (nvtabular_amd/kernels_embedding.py, framework_utils.torch.layers): the fused
// forward of all tables of a layer and one sparse, coalesced, deterministic gradient per table.
//
// Tables are float32 [rows, dim], one allocation each; a launch gets them by value (TableSet: at most
// NVT_EMB_MAX_TABLES descriptors in the kernel arguments, read with wave-uniform indices, i.e. through
// scalar registers).  A column whose dim, first output column and row pitch are multiples of 4 (and
// whose pointers are 16-byte aligned) moves float4, every other column dwords (Vec<4> / Vec<1>).
// lanes per (row, column) pair = vector units of the column rounded up to a power of two, at most 64:
// a dim-16 column puts 16 pairs into a wave, a dim-512 column takes two trips of a whole wave.
//
// gather_cat     a workgroup owns 64 batch rows: their ids are read once with coalesced loads, checked
//                against the table and kept in LDS as uint32 row numbers (kBadRow: out of range); then
//                column by column the groups of the workgroup copy (row, column) pairs.  The column
//                loop is uniform over the workgroup, so the descriptor sits in scalar registers.
// bag            blockIdx.y = column, one group per bag: fp32 accumulators in registers, values added
//                in value order; offsets are clamped to [0, nvalues] before they address anything.
// grad_plan      entry e (single-hot: b * ntables + c, bags: the values of all columns one after the
//                other) -> word global_row << 32 | e, global_row numbering the rows of all tables
//                consecutively and = total rows for an entry that counts for nothing (id out of range,
//                value outside every bag).  Stable word sort on the row bits (nvt_sort.hip): positions
//                ascend inside a row.  Two head flags per sorted slot -- first of its row; first of its
//                UNIT: first of its row or slot % NVT_EMB_CHUNK == 0 -- and their scans number the
//                unique rows (segments) and the units.  A unit never holds more than NVT_EMB_CHUNK
//                entries, so the id that a third of the batch carries is summed by many groups.
// grad_reduce    one group per unit sums grad_out[b, slice] over the unit's entries in position order;
//                the only unit of its row writes the row's gradient, every other unit a partial sum,
//                and grad_fold adds the partial sums of a row in unit order.  No atomics: the bits of
//                the result depend on the input alone.
// An id is compared with its table's row count before anything is addressed through it.
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr unsigned kTileRows = 64;            // batch rows of one gather workgroup
constexpr uint32_t kBadRow = 0xFFFFFFFFu;     // (total rows <= 2^32 - 2: no table has this row)
constexpr uint64_t kMaxTotalRows = 0xFFFFFFFEull;
constexpr uint64_t kMaxEntries = (1ull << 30) - 1;  // what the word sort takes
constexpr uint64_t kMaxBatch = (1ull << 31) - 1;
constexpr uint32_t kChunk = NVT_EMB_CHUNK;

struct TableSet {
  nvt_emb_table t[NVT_EMB_MAX_TABLES];
  uint8_t vec[NVT_EMB_MAX_TABLES];  // 1: float4 accesses
};
struct BagSet {
  nvt_emb_bag_col c[NVT_EMB_MAX_TABLES];
};
struct OutSet {
  nvt_emb_grad_out o[NVT_EMB_MAX_TABLES];
};
struct RowBase {
  uint64_t row[NVT_EMB_MAX_TABLES + 1];  // first global row of every table; [ntables] = total rows
};
struct EntryBase {
  uint64_t entry[NVT_EMB_MAX_TABLES + 1];  // bags: first entry of every column
};

template <int V>
struct Vec;
template <>
struct Vec<1> {
  using T = float;
};
template <>
struct Vec<4> {
  using T = float4;
};
__device__ __forceinline__ void acc_add(float &a, float v, float s) { a += v * s; }
__device__ __forceinline__ void acc_add(float4 &a, float4 v, float s) {
  a.x += v.x * s;
  a.y += v.y * s;
  a.z += v.z * s;
  a.w += v.w * s;
}
__device__ __forceinline__ void acc_zero(float &a) { a = 0.0f; }
__device__ __forceinline__ void acc_zero(float4 &a) { a = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

__host__ __device__ __forceinline__ unsigned group_lanes(uint32_t dim, bool vec) {
  const uint32_t units = vec ? dim / 4 : dim;
  unsigned l = 1;
  while (l < units && l < (unsigned)kWave) l <<= 1;
  return l;
}

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int bits_for(uint64_t count) {  // bits that hold 0 .. count - 1 (at least 1)
  int b = 1;
  while ((1ull << b) < count) ++b;
  return b;
}

// ---- forward: single-hot ----------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void gather_column(const nvt_emb_table t, const uint32_t *rows_lds, unsigned c,
                                              unsigned ntables, unsigned nrows, uint64_t r0, float *__restrict__ out,
                                              uint64_t out_cols) {
  using E = typename Vec<V>::T;
  const unsigned units = t.dim / V, lanes = group_lanes(t.dim, V == 4), groups = kBlock / lanes;
  const unsigned g = threadIdx.x / lanes, sub = threadIdx.x % lanes;
  for (unsigned r = g; r < nrows; r += groups) {
    const uint32_t id = rows_lds[r * ntables + c];
    const E *__restrict__ src = reinterpret_cast<const E *>(t.weight + (uint64_t)id * t.dim);
    E *__restrict__ dst = reinterpret_cast<E *>(out + (r0 + r) * out_cols + t.out_col);
    for (unsigned j = sub; j < units; j += lanes) {
      E v;
      acc_zero(v);
      if (id != kBadRow) v = src[j];
      dst[j] = v;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void emb_gather_cat_kernel(const T *__restrict__ ids, uint64_t batch, TableSet ts,
                                                                unsigned ntables, float *__restrict__ out,
                                                                uint64_t out_cols, unsigned long long *__restrict__ oor) {
  __shared__ uint32_t rows_lds[kTileRows * NVT_EMB_MAX_TABLES];
  __shared__ uint64_t limit[NVT_EMB_MAX_TABLES];
  if (threadIdx.x < ntables) limit[threadIdx.x] = ts.t[threadIdx.x].rows;
  __syncthreads();
  for (uint64_t r0 = (uint64_t)blockIdx.x * kTileRows; r0 < batch; r0 += (uint64_t)gridDim.x * kTileRows) {
    const unsigned nrows = (unsigned)(batch - r0 < kTileRows ? batch - r0 : kTileRows);
    const unsigned nids = nrows * ntables;
    unsigned bad = 0;
    for (unsigned i = threadIdx.x; i < nids; i += kBlock) {
      const uint64_t id = (uint64_t)(int64_t)ids[r0 * ntables + i];  // negative: huge
      const bool ok = id < limit[i % ntables];
      rows_lds[i] = ok ? (uint32_t)id : kBadRow;
      bad += ok ? 0u : 1u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if (lane_id() == 0 && bad) atomicAdd(oor, (unsigned long long)bad);
    __syncthreads();
    for (unsigned c = 0; c < ntables; ++c) {
      if (ts.vec[c])
        gather_column<4>(ts.t[c], rows_lds, c, ntables, nrows, r0, out, out_cols);
      else
        gather_column<1>(ts.t[c], rows_lds, c, ntables, nrows, r0, out, out_cols);
    }
    __syncthreads();  // (the ids are rewritten in the next round)
  }
}

// ---- forward: bags ----------------------------------------------------------------------------
__device__ __forceinline__ void bag_range(const int64_t *__restrict__ offsets, uint64_t b, uint64_t nvalues,
                                          uint64_t &s, uint64_t &e) {
  const int64_t a = offsets[b], z = offsets[b + 1];
  s = a < 0 ? 0 : ((uint64_t)a > nvalues ? nvalues : (uint64_t)a);
  e = z < 0 ? 0 : ((uint64_t)z > nvalues ? nvalues : (uint64_t)z);
  if (e < s) e = s;
}

template <typename T, int V>
__device__ __forceinline__ void bag_column(const nvt_emb_table t, const nvt_emb_bag_col col, uint64_t batch, int mode,
                                           float *__restrict__ out, uint64_t out_cols,
                                           unsigned long long *__restrict__ oor) {
  using E = typename Vec<V>::T;
  const T *__restrict__ values = reinterpret_cast<const T *>(col.values);
  const unsigned units = t.dim / V, lanes = group_lanes(t.dim, V == 4), groups = kBlock / lanes;
  const unsigned g = threadIdx.x / lanes, sub = threadIdx.x % lanes;
  for (uint64_t b = (uint64_t)blockIdx.x * groups + g; b < batch; b += (uint64_t)gridDim.x * groups) {
    uint64_t s, e;
    bag_range(col.offsets, b, col.nvalues, s, e);
    const float scale = (mode == NVT_EMB_MEAN && e > s) ? 1.0f / (float)(e - s) : 1.0f;
    E *__restrict__ dst = reinterpret_cast<E *>(out + b * out_cols + t.out_col);
    unsigned bad = 0;
    for (unsigned j = sub; j < units; j += lanes) {
      E acc;
      acc_zero(acc);
      for (uint64_t k = s; k < e; ++k) {
        const uint64_t id = (uint64_t)(int64_t)values[k];
        if (id < t.rows)
          acc_add(acc, reinterpret_cast<const E *>(t.weight + id * t.dim)[j], 1.0f);
        else if (j == 0)
          ++bad;
      }
      E res;
      acc_zero(res);
      acc_add(res, acc, scale);
      dst[j] = res;
    }
    if (bad) atomicAdd(oor, (unsigned long long)bad);  // (only the lane that owns unit 0 counts)
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void emb_bag_kernel(BagSet bs, TableSet ts, uint64_t batch, int mode,
                                                         float *__restrict__ out, uint64_t out_cols,
                                                         unsigned long long *__restrict__ oor) {
  const unsigned c = blockIdx.y;
  if (ts.vec[c])
    bag_column<T, 4>(ts.t[c], bs.c[c], batch, mode, out, out_cols, oor);
  else
    bag_column<T, 1>(ts.t[c], bs.c[c], batch, mode, out, out_cols, oor);
}

// ---- backward: plan ---------------------------------------------------------------------------
struct GradMeta {  // written by emb_meta_kernel, read by the reduce and fold launches
  uint32_t seg_base[NVT_EMB_MAX_TABLES + 1];    // first segment (unique row) of every table
  uint32_t unit_base[NVT_EMB_MAX_TABLES + 1];   // first unit of every table
  uint32_t unit_block[NVT_EMB_MAX_TABLES + 1];  // first workgroup of every table in the reduce launch
  uint32_t seg_block[NVT_EMB_MAX_TABLES + 1];   // ... in the fold launch
  uint64_t pbase[NVT_EMB_MAX_TABLES + 1];       // first float of every table's partial sums
};

struct GradWs {
  GradMeta *meta;
  uint64_t *words;          // [n]
  void *sort_tmp;
  uint32_t *epos;           // [n]      entry of every sorted slot
  uint32_t *row_pos;        // [n + 1]  row-head flags, then their exclusive scan
  uint32_t *unit_pos;       // [n + 1]  unit-head flags, then their exclusive scan
  uint32_t *unit_start;     // [n + 1]  first slot of every unit; [units] = slots that count
  uint32_t *unit_row;       // [n]      global row of every unit
  uint32_t *unit_seg;       // [n]      segment of every unit
  uint32_t *seg_unit;       // [n + 1]  first unit of every segment; [segments] = units
  uint32_t *bag_of;         // [n]      bags: the bag of every entry
  float *inv_len;           // [n]      bags: 1 / length of that bag
  unsigned long long *chunk;  // the scans' chunk totals
  uint64_t bytes;
};

GradWs grad_ws(const void *ws, uint64_t n) {
  GradWs w;
  uint8_t *b = (uint8_t *)ws;
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    uint8_t *q = b + at;
    at += pad256(bytes);
    return q;
  };
  w.meta = reinterpret_cast<GradMeta *>(take(sizeof(GradMeta)));
  w.words = reinterpret_cast<uint64_t *>(take(n * 8));
  w.sort_tmp = take(sort_words_tmp_bytes(n));
  w.epos = reinterpret_cast<uint32_t *>(take(n * 4));
  w.row_pos = reinterpret_cast<uint32_t *>(take((n + 1) * 4));
  w.unit_pos = reinterpret_cast<uint32_t *>(take((n + 1) * 4));
  w.unit_start = reinterpret_cast<uint32_t *>(take((n + 1) * 4));
  w.unit_row = reinterpret_cast<uint32_t *>(take(n * 4));
  w.unit_seg = reinterpret_cast<uint32_t *>(take(n * 4));
  w.seg_unit = reinterpret_cast<uint32_t *>(take((n + 1) * 4));
  w.bag_of = reinterpret_cast<uint32_t *>(take(n * 4));
  w.inv_len = reinterpret_cast<float *>(take(n * 4));
  w.chunk = reinterpret_cast<unsigned long long *>(take(scan_chunks(n + 1) * 8));
  w.bytes = at;
  return w;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void emb_pack_ids_kernel(const T *__restrict__ ids, uint64_t n, RowBase base,
                                                              unsigned ntables, uint64_t *__restrict__ words) {
  __shared__ uint64_t limit[NVT_EMB_MAX_TABLES], first[NVT_EMB_MAX_TABLES];
  if (threadIdx.x < ntables) {
    limit[threadIdx.x] = base.row[threadIdx.x + 1] - base.row[threadIdx.x];
    first[threadIdx.x] = base.row[threadIdx.x];
  }
  __syncthreads();
  const uint64_t total = base.row[ntables];
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (uint64_t)gridDim.x * kBlock) {
    const unsigned c = (unsigned)(e % ntables);
    const uint64_t id = (uint64_t)(int64_t)ids[e];
    const uint64_t row = id < limit[c] ? first[c] + id : total;
    words[e] = (row << 32) | e;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void emb_pack_bags_kernel(BagSet bs, uint64_t n, uint64_t batch, RowBase base,
                                                               EntryBase ebase, unsigned ntables,
                                                               uint64_t *__restrict__ words,
                                                               uint32_t *__restrict__ bag_of,
                                                               float *__restrict__ inv_len) {
  const uint64_t total = base.row[ntables];
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (uint64_t)gridDim.x * kBlock) {
    unsigned c = 0;
    while (c + 1 < ntables && e >= ebase.entry[c + 1]) ++c;
    const nvt_emb_bag_col col = bs.c[c];
    const uint64_t k = e - ebase.entry[c];
    // the bag of value k: the last one whose start is not behind k
    uint64_t lo = 0, len = batch + 1;  // the first offset that is greater than k
    while (len > 0) {
      const uint64_t half = len >> 1;
      const int64_t o = col.offsets[lo + half];
      if (o <= (int64_t)k) {
        lo += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    uint64_t row = total;
    uint32_t bag = 0;
    float inv = 0.0f;
    if (lo >= 1 && lo <= batch) {
      uint64_t s, z;
      bag_range(col.offsets, lo - 1, col.nvalues, s, z);
      const uint64_t id = (uint64_t)(int64_t) reinterpret_cast<const T *>(col.values)[k];
      if (k >= s && k < z && id < base.row[c + 1] - base.row[c]) {
        row = base.row[c] + id;
        bag = (uint32_t)(lo - 1);
        inv = 1.0f / (float)(z - s);
      }
    }
    words[e] = (row << 32) | e;
    bag_of[e] = bag;
    inv_len[e] = inv;
  }
}

__global__ __launch_bounds__(kBlock) void emb_flag_kernel(const uint64_t *__restrict__ sorted, uint64_t n,
                                                          uint32_t bad_row, uint32_t *__restrict__ epos,
                                                          uint32_t *__restrict__ row_flag,
                                                          uint32_t *__restrict__ unit_flag) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * kBlock) {
    uint32_t rf = 0, uf = 0;
    if (j < n) {
      const uint64_t w = sorted[j];
      const uint32_t row = (uint32_t)(w >> 32);
      epos[j] = (uint32_t)w;
      if (row != bad_row) {
        rf = (j == 0 || (uint32_t)(sorted[j - 1] >> 32) != row) ? 1u : 0u;
        uf = (rf || j % kChunk == 0) ? 1u : 0u;
      }
    }
    row_flag[j] = rf;
    unit_flag[j] = uf;
  }
}

__global__ __launch_bounds__(kBlock) void emb_units_kernel(const uint64_t *__restrict__ sorted, uint64_t n,
                                                           uint32_t bad_row, const uint32_t *__restrict__ row_pos,
                                                           const uint32_t *__restrict__ unit_pos,
                                                           uint32_t *__restrict__ unit_start,
                                                           uint32_t *__restrict__ unit_row,
                                                           uint32_t *__restrict__ unit_seg,
                                                           uint32_t *__restrict__ seg_unit) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t row = (uint32_t)(sorted[j] >> 32);
    if (row == bad_row) continue;
    const uint32_t u = unit_pos[j], s = row_pos[j];
    const bool row_head = row_pos[j + 1] != s;
    if (unit_pos[j + 1] != u) {
      unit_start[u] = (uint32_t)j;
      unit_row[u] = row;
      unit_seg[u] = row_head ? s : s - 1;
      if (row_head) seg_unit[s] = u;
    }
    if (j + 1 == n || (uint32_t)(sorted[j + 1] >> 32) == bad_row) {  // the last slot that counts
      unit_start[unit_pos[n]] = (uint32_t)(j + 1);
      seg_unit[row_pos[n]] = unit_pos[n];
    }
  }
}

constexpr int kMetaBlock = 128;  // (one thread per table and one more)
static_assert(NVT_EMB_MAX_TABLES + 1 <= kMetaBlock, "emb_meta_kernel: one thread per table boundary");
// state: {segments, units, reduce workgroups, fold workgroups, floats of partial sums, segments of
// every table}
__global__ __launch_bounds__(kMetaBlock) void emb_meta_kernel(const uint64_t *__restrict__ sorted, uint64_t n,
                                                                      TableSet ts, RowBase base, unsigned ntables,
                                                                      const uint32_t *__restrict__ row_pos,
                                                                      const uint32_t *__restrict__ unit_pos,
                                                                      GradMeta *__restrict__ meta,
                                                                      int64_t *__restrict__ state) {
  __shared__ uint32_t seg_at[NVT_EMB_MAX_TABLES + 1], unit_at[NVT_EMB_MAX_TABLES + 1];
  if (threadIdx.x <= ntables) {
    const uint64_t want = base.row[threadIdx.x];
    uint64_t lo = 0, len = n;  // the first slot whose row is not below `want`
    while (len > 0) {
      const uint64_t half = len >> 1;
      if ((sorted[lo + half] >> 32) < want) {
        lo += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    seg_at[threadIdx.x] = row_pos[lo];
    unit_at[threadIdx.x] = unit_pos[lo];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t ublock = 0, sblock = 0;
  uint64_t pfloats = 0;
  for (unsigned c = 0; c < ntables; ++c) {
    const unsigned groups = kBlock / group_lanes(ts.t[c].dim, ts.vec[c]);
    const uint32_t segs = seg_at[c + 1] - seg_at[c], units = unit_at[c + 1] - unit_at[c];
    meta->seg_base[c] = seg_at[c];
    meta->unit_base[c] = unit_at[c];
    meta->unit_block[c] = ublock;
    meta->seg_block[c] = sblock;
    meta->pbase[c] = pfloats;
    ublock += (units + groups - 1) / groups;
    sblock += (segs + groups - 1) / groups;
    pfloats += ((uint64_t)units * ts.t[c].dim + 3) & ~3ull;
    state[5 + c] = segs;
  }
  meta->seg_base[ntables] = seg_at[ntables];
  meta->unit_base[ntables] = unit_at[ntables];
  meta->unit_block[ntables] = ublock;
  meta->seg_block[ntables] = sblock;
  meta->pbase[ntables] = pfloats;
  state[0] = seg_at[ntables];
  state[1] = unit_at[ntables];
  state[2] = ublock;
  state[3] = sblock;
  state[4] = (int64_t)pfloats;
}

// ---- backward: reduce and fold ------------------------------------------------------------------
struct GradArgs {
  const GradMeta *meta;
  const uint32_t *epos, *unit_start, *unit_row, *unit_seg, *seg_unit, *bag_of;
  const float *inv_len;
  const float *grad_out;
  float *partials;
  uint64_t out_cols;
  unsigned ntables;
  int bags, mean;
};

// where the gradient of segment `seg` (local row `row`) of table c goes, or nullptr
__device__ __forceinline__ float *grad_row(const nvt_emb_grad_out o, const nvt_emb_table t, uint32_t seg_local,
                                           uint32_t row, unsigned sub) {
  if (o.ids == nullptr) return o.values + (uint64_t)row * t.dim;  // dense: row < t.rows by construction
  if (seg_local >= o.count) return nullptr;
  if (sub == 0) o.ids[seg_local] = (int64_t)row;
  return o.values + (uint64_t)seg_local * t.dim;
}

template <int V>
__device__ __forceinline__ void reduce_unit(const GradArgs a, const nvt_emb_table t, const nvt_emb_grad_out o,
                                            unsigned c, uint32_t first_row) {
  using E = typename Vec<V>::T;
  const GradMeta *__restrict__ m = a.meta;
  const unsigned units = t.dim / V, lanes = group_lanes(t.dim, V == 4), groups = kBlock / lanes;
  const unsigned g = threadIdx.x / lanes, sub = threadIdx.x % lanes;
  const uint32_t local = (blockIdx.x - m->unit_block[c]) * groups + g;
  if (local >= m->unit_base[c + 1] - m->unit_base[c]) return;
  const uint32_t u = m->unit_base[c] + local;
  const uint32_t j0 = a.unit_start[u], j1 = a.unit_start[u + 1], seg = a.unit_seg[u];
  float *dst;
  if (a.seg_unit[seg] == u && a.seg_unit[seg + 1] == u + 1)  // the only unit of its row
    dst = grad_row(o, t, seg - m->seg_base[c], a.unit_row[u] - first_row, sub);
  else
    dst = a.partials + m->pbase[c] + (uint64_t)local * t.dim;
  if (dst == nullptr) return;
  for (unsigned j = sub; j < units; j += lanes) {
    E acc;
    acc_zero(acc);
    for (uint32_t k = j0; k < j1; ++k) {
      const uint32_t e = a.epos[k];
      const uint64_t b = a.bags ? a.bag_of[e] : e / a.ntables;
      const float s = a.mean ? a.inv_len[e] : 1.0f;
      acc_add(acc, reinterpret_cast<const E *>(a.grad_out + b * a.out_cols + t.out_col)[j], s);
    }
    reinterpret_cast<E *>(dst)[j] = acc;
  }
}

__global__ __launch_bounds__(kBlock) void emb_grad_reduce_kernel(GradArgs a, TableSet ts, OutSet outs, RowBase base) {
  unsigned c = 0;
  while (c + 1 < a.ntables && blockIdx.x >= a.meta->unit_block[c + 1]) ++c;
  if (ts.vec[c])
    reduce_unit<4>(a, ts.t[c], outs.o[c], c, (uint32_t)base.row[c]);
  else
    reduce_unit<1>(a, ts.t[c], outs.o[c], c, (uint32_t)base.row[c]);
}

template <int V>
__device__ __forceinline__ void fold_segment(const GradArgs a, const nvt_emb_table t, const nvt_emb_grad_out o,
                                             unsigned c, uint32_t first_row) {
  using E = typename Vec<V>::T;
  const GradMeta *__restrict__ m = a.meta;
  const unsigned units = t.dim / V, lanes = group_lanes(t.dim, V == 4), groups = kBlock / lanes;
  const unsigned g = threadIdx.x / lanes, sub = threadIdx.x % lanes;
  const uint32_t local = (blockIdx.x - m->seg_block[c]) * groups + g;
  if (local >= m->seg_base[c + 1] - m->seg_base[c]) return;
  const uint32_t seg = m->seg_base[c] + local;
  const uint32_t u0 = a.seg_unit[seg], u1 = a.seg_unit[seg + 1];
  if (u1 - u0 <= 1) return;  // written by its only unit
  float *dst = grad_row(o, t, local, a.unit_row[u0] - first_row, sub);
  if (dst == nullptr) return;
  const float *__restrict__ part = a.partials + m->pbase[c] + (uint64_t)(u0 - m->unit_base[c]) * t.dim;
  for (unsigned j = sub; j < units; j += lanes) {
    E acc;
    acc_zero(acc);
    for (uint32_t u = 0; u < u1 - u0; ++u) acc_add(acc, reinterpret_cast<const E *>(part + (uint64_t)u * t.dim)[j], 1.0f);
    reinterpret_cast<E *>(dst)[j] = acc;
  }
}

__global__ __launch_bounds__(kBlock) void emb_grad_fold_kernel(GradArgs a, TableSet ts, OutSet outs, RowBase base) {
  unsigned c = 0;
  while (c + 1 < a.ntables && blockIdx.x >= a.meta->seg_block[c + 1]) ++c;
  if (ts.vec[c])
    fold_segment<4>(a, ts.t[c], outs.o[c], c, (uint32_t)base.row[c]);
  else
    fold_segment<1>(a, ts.t[c], outs.o[c], c, (uint32_t)base.row[c]);
}

// ---- host side ----------------------------------------------------------------------------------
// The descriptors of a layer: checked, copied into the launch arguments, the float4 columns marked.
// float4 or dwords follows from the layout alone, so the plan and the reduce of one backward agree;
// what a float4 column touches (`io`: the [batch, out_cols] matrix the slices lie in) is 16-byte aligned.
int check_tables(const nvt_emb_table *tables, int ntables, uint64_t out_cols, const float *io, TableSet *ts,
                 RowBase *base) {
  NVT_CHECK_ARG(tables, "null descriptors");
  NVT_CHECK_ARG(ntables >= 1 && ntables <= NVT_EMB_MAX_TABLES, "1 to NVT_EMB_MAX_TABLES tables");
  NVT_CHECK_ARG(out_cols >= 1 && out_cols <= (1ull << 31), "out_cols must be 1 to 2^31");
  uint64_t total = 0;
  for (int c = 0; c < ntables; ++c) {
    const nvt_emb_table &t = tables[c];
    NVT_CHECK_ARG(t.weight && aligned_to(t.weight, 4), "null or unaligned table");
    NVT_CHECK_ARG(t.dim >= 1, "dim must be at least 1");
    NVT_CHECK_ARG(t.rows >= 1 && t.rows <= kMaxTotalRows, "a table has 1 to 2^32 - 2 rows");
    NVT_CHECK_ARG((uint64_t)t.out_col + t.dim <= out_cols, "a slice ends behind out_cols");
    total += t.rows;
    NVT_CHECK_ARG(total <= kMaxTotalRows, "the tables of a layer hold fewer than 2^32 - 1 rows together");
    ts->t[c] = t;
    ts->vec[c] = t.dim % 4 == 0 && t.out_col % 4 == 0 && out_cols % 4 == 0;
    NVT_CHECK_ARG(!ts->vec[c] || (aligned_to(t.weight, 16) && aligned_to(io, 16)),
                  "a table and a matrix read as float4 must be 16-byte aligned");
    base->row[c] = total - t.rows;
  }
  base->row[ntables] = total;
  return NVT_OK;
}

int check_bags(const nvt_emb_bag_col *cols, int ntables, int id_dtype, BagSet *bs, EntryBase *base,
               uint64_t *entries) {
  NVT_CHECK_ARG(cols, "null bag columns");
  const uintptr_t width = id_dtype == NVT_I32 ? 4 : 8;
  uint64_t n = 0;
  for (int c = 0; c < ntables; ++c) {
    NVT_CHECK_ARG(cols[c].offsets && aligned_to(cols[c].offsets, 8), "null or unaligned offsets");
    NVT_CHECK_ARG(cols[c].nvalues <= kMaxEntries, "fewer than 2^30 values");
    NVT_CHECK_ARG((cols[c].values || cols[c].nvalues == 0) && aligned_to(cols[c].values, width),
                  "null or unaligned values");
    bs->c[c] = cols[c];
    base->entry[c] = n;
    n += cols[c].nvalues;
    NVT_CHECK_ARG(n <= kMaxEntries, "fewer than 2^30 values in all columns together");
  }
  base->entry[ntables] = n;
  *entries = n;
  return NVT_OK;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_emb_gather_cat(const void *ids, int id_dtype, uint64_t batch, const nvt_emb_table *tables, int ntables,
                       float *out, uint64_t out_cols, int64_t *out_of_range, void *stream) {
  NVT_CHECK_ARG(id_dtype == NVT_I32 || id_dtype == NVT_I64, "id dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(batch <= kMaxBatch, "batch must be below 2^31");
  TableSet ts;
  RowBase base;
  const int rc = check_tables(tables, ntables, out_cols, out, &ts, &base);
  if (rc) return rc;
  NVT_CHECK_ARG(batch * (uint64_t)ntables <= kMaxEntries, "fewer than 2^30 ids");
  if (batch == 0) return NVT_OK;
  NVT_CHECK_ARG(ids && out && out_of_range, "null ids / out / counter");
  NVT_CHECK_ARG(aligned_to(ids, id_dtype == NVT_I32 ? 4 : 8) && aligned_to(out, 4) && aligned_to(out_of_range, 8),
                "ids, out and the counter must be aligned to their types");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("emb_gather_cat", batch * (ntables * (id_dtype == NVT_I32 ? 4 : 8) + 8 * out_cols), s);
  unsigned long long *oor = reinterpret_cast<unsigned long long *>(out_of_range);
  const unsigned grid = stream_grid(batch, kTileRows);
  if (id_dtype == NVT_I32)
    emb_gather_cat_kernel<int32_t><<<grid, kBlock, 0, s>>>(reinterpret_cast<const int32_t *>(ids), batch, ts,
                                                            (unsigned)ntables, out, out_cols, oor);
  else
    emb_gather_cat_kernel<int64_t><<<grid, kBlock, 0, s>>>(reinterpret_cast<const int64_t *>(ids), batch, ts,
                                                            (unsigned)ntables, out, out_cols, oor);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_emb_bag(const nvt_emb_bag_col *cols, int id_dtype, uint64_t batch, const nvt_emb_table *tables, int ntables,
                int mode, float *out, uint64_t out_cols, int64_t *out_of_range, void *stream) {
  NVT_CHECK_ARG(id_dtype == NVT_I32 || id_dtype == NVT_I64, "id dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(mode == NVT_EMB_SUM || mode == NVT_EMB_MEAN, "mode must be NVT_EMB_SUM or NVT_EMB_MEAN");
  NVT_CHECK_ARG(batch <= kMaxBatch, "batch must be below 2^31");
  TableSet ts;
  RowBase base;
  EntryBase ebase;
  BagSet bs;
  uint64_t entries = 0;
  int rc = check_tables(tables, ntables, out_cols, out, &ts, &base);
  if (rc) return rc;
  rc = check_bags(cols, ntables, id_dtype, &bs, &ebase, &entries);
  if (rc) return rc;
  if (batch == 0) return NVT_OK;
  NVT_CHECK_ARG(out && out_of_range, "null out / counter");
  NVT_CHECK_ARG(aligned_to(out, 4) && aligned_to(out_of_range, 8), "out and the counter must be aligned to their types");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("emb_bag", entries * 8 + batch * (8 * ntables + 4 * out_cols), s);
  unsigned long long *oor = reinterpret_cast<unsigned long long *>(out_of_range);
  const dim3 grid(stream_grid(batch, 4), (unsigned)ntables);
  if (id_dtype == NVT_I32)
    emb_bag_kernel<int32_t><<<grid, kBlock, 0, s>>>(bs, ts, batch, mode, out, out_cols, oor);
  else
    emb_bag_kernel<int64_t><<<grid, kBlock, 0, s>>>(bs, ts, batch, mode, out, out_cols, oor);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_emb_grad_ws_bytes(uint64_t entries, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  NVT_CHECK_ARG(entries <= kMaxEntries, "fewer than 2^30 entries");
  *bytes = grad_ws(nullptr, entries).bytes;
  return NVT_OK;
}

int nvt_emb_grad_plan(const void *ids, const nvt_emb_bag_col *cols, int id_dtype, uint64_t batch,
                      const nvt_emb_table *tables, int ntables, uint64_t out_cols, void *ws, uint64_t ws_bytes,
                      int64_t *state, void *stream) {
  NVT_CHECK_ARG(id_dtype == NVT_I32 || id_dtype == NVT_I64, "id dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(batch >= 1 && batch <= kMaxBatch, "batch must be 1 to 2^31 - 1");
  NVT_CHECK_ARG((ids != nullptr) != (cols != nullptr), "either ids or bag columns");
  TableSet ts;
  RowBase base;
  EntryBase ebase;
  BagSet bs;
  uint64_t n = 0;
  int rc = check_tables(tables, ntables, out_cols, nullptr, &ts, &base);
  if (rc) return rc;
  if (ids) {
    n = batch * (uint64_t)ntables;
    NVT_CHECK_ARG(n <= kMaxEntries, "fewer than 2^30 ids");
    NVT_CHECK_ARG(aligned_to(ids, id_dtype == NVT_I32 ? 4 : 8), "ids must be aligned to their type");
  } else {
    rc = check_bags(cols, ntables, id_dtype, &bs, &ebase, &n);
    if (rc) return rc;
  }
  NVT_CHECK_ARG(ws && state, "null workspace / state");
  NVT_CHECK_ARG(aligned_to(ws, 256) && aligned_to(state, 8), "workspace 256-byte, state 8-byte aligned");
  const GradWs w = grad_ws(ws, n);
  NVT_CHECK_ARG(ws_bytes >= w.bytes, "workspace smaller than nvt_emb_grad_ws_bytes");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("emb_grad_plan", n * 64, s);
  const uint32_t bad_row = (uint32_t)base.row[ntables];
  uint64_t *sorted = w.words;
  if (n) {
    const unsigned grid = stream_grid(n, kBlock * 4);
    if (ids && id_dtype == NVT_I32)
      emb_pack_ids_kernel<int32_t><<<grid, kBlock, 0, s>>>(reinterpret_cast<const int32_t *>(ids), n, base,
                                                            (unsigned)ntables, w.words);
    else if (ids)
      emb_pack_ids_kernel<int64_t><<<grid, kBlock, 0, s>>>(reinterpret_cast<const int64_t *>(ids), n, base,
                                                            (unsigned)ntables, w.words);
    else if (id_dtype == NVT_I32)
      emb_pack_bags_kernel<int32_t><<<grid, kBlock, 0, s>>>(bs, n, batch, base, ebase, (unsigned)ntables, w.words,
                                                             w.bag_of, w.inv_len);
    else
      emb_pack_bags_kernel<int64_t><<<grid, kBlock, 0, s>>>(bs, n, batch, base, ebase, (unsigned)ntables, w.words,
                                                             w.bag_of, w.inv_len);
    NVT_CHECK_LAUNCH();
    rc = sort_words_bits(w.words, n, 32, 32 + bits_for(base.row[ntables] + 1), w.sort_tmp, &sorted, s);
    if (rc) return rc;
  }
  emb_flag_kernel<<<stream_grid(n + 1, kBlock * 4), kBlock, 0, s>>>(sorted, n, bad_row, w.epos, w.row_pos, w.unit_pos);
  NVT_CHECK_LAUNCH();
  rc = exclusive_scan_u32(w.row_pos, n + 1, w.chunk, s);
  if (rc) return rc;
  rc = exclusive_scan_u32(w.unit_pos, n + 1, w.chunk, s);
  if (rc) return rc;
  if (n) {
    emb_units_kernel<<<stream_grid(n, kBlock * 4), kBlock, 0, s>>>(sorted, n, bad_row, w.row_pos, w.unit_pos,
                                                                   w.unit_start, w.unit_row, w.unit_seg, w.seg_unit);
    NVT_CHECK_LAUNCH();
  }
  emb_meta_kernel<<<1, kMetaBlock, 0, s>>>(sorted, n, ts, base, (unsigned)ntables,
                                                                          w.row_pos, w.unit_pos, w.meta, state);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_emb_grad_reduce(int bags, uint64_t batch, uint64_t entries, const nvt_emb_table *tables, int ntables, int mode,
                        const float *grad_out, uint64_t out_cols, const void *ws, uint64_t ws_bytes,
                        const int64_t *counts, float *partials, uint64_t partial_floats,
                        const nvt_emb_grad_out *outs, void *stream) {
  NVT_CHECK_ARG(mode == NVT_EMB_SUM || mode == NVT_EMB_MEAN, "mode must be NVT_EMB_SUM or NVT_EMB_MEAN");
  NVT_CHECK_ARG(batch >= 1 && batch <= kMaxBatch, "batch must be 1 to 2^31 - 1");
  NVT_CHECK_ARG(entries <= kMaxEntries, "fewer than 2^30 entries");
  TableSet ts;
  RowBase base;
  OutSet os;
  int rc = check_tables(tables, ntables, out_cols, grad_out, &ts, &base);
  if (rc) return rc;
  NVT_CHECK_ARG(bags || entries == batch * (uint64_t)ntables, "single-hot: entries = batch * ntables");
  NVT_CHECK_ARG(grad_out && ws && counts && outs, "null grad_out / workspace / counts / outputs");
  NVT_CHECK_ARG(aligned_to(ws, 256) && aligned_to(grad_out, 4), "workspace 256-byte, grad_out 4-byte aligned");
  const GradWs w = grad_ws(ws, entries);
  NVT_CHECK_ARG(ws_bytes >= w.bytes, "workspace smaller than nvt_emb_grad_ws_bytes");
  const uint64_t segs = (uint64_t)counts[0], units = (uint64_t)counts[1], ublocks = (uint64_t)counts[2],
                 sblocks = (uint64_t)counts[3], pfloats = (uint64_t)counts[4];
  NVT_CHECK_ARG(segs <= units && units <= entries && ublocks <= units && sblocks <= segs,
                "counts are not what nvt_emb_grad_plan wrote");
  NVT_CHECK_ARG(partial_floats >= pfloats && (partials || pfloats == 0) && aligned_to(partials, 16),
                "partial sums: 16-byte aligned, counts[4] floats");
  uint64_t sum = 0;
  for (int c = 0; c < ntables; ++c) {
    const nvt_emb_grad_out &o = outs[c];
    NVT_CHECK_ARG(counts[5 + c] >= 0 && (uint64_t)counts[5 + c] <= segs, "counts are not what nvt_emb_grad_plan wrote");
    sum += (uint64_t)counts[5 + c];
    NVT_CHECK_ARG(o.ids == nullptr || o.count == (uint64_t)counts[5 + c], "a sparse output holds counts[5 + c] rows");
    NVT_CHECK_ARG((o.values && aligned_to(o.values, ts.vec[c] ? 16 : 4)) || (o.ids && o.count == 0),
                  "null or unaligned gradient");
    NVT_CHECK_ARG(aligned_to(o.ids, 8), "unaligned gradient ids");
    os.o[c] = o;
  }
  NVT_CHECK_ARG(sum == segs, "counts are not what nvt_emb_grad_plan wrote");
  if (units == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("emb_grad_reduce", entries * (8 + 4 * out_cols / ntables), s);
  GradArgs a;
  a.meta = w.meta;
  a.epos = w.epos;
  a.unit_start = w.unit_start;
  a.unit_row = w.unit_row;
  a.unit_seg = w.unit_seg;
  a.seg_unit = w.seg_unit;
  a.bag_of = w.bag_of;
  a.inv_len = w.inv_len;
  a.grad_out = grad_out;
  a.partials = partials;
  a.out_cols = out_cols;
  a.ntables = (unsigned)ntables;
  a.bags = bags ? 1 : 0;
  a.mean = (bags && mode == NVT_EMB_MEAN) ? 1 : 0;
  emb_grad_reduce_kernel<<<(unsigned)ublocks, kBlock, 0, s>>>(a, ts, os, base);
  NVT_CHECK_LAUNCH();
  if (units > segs) {  // some row has more than one unit
    emb_grad_fold_kernel<<<(unsigned)sblocks, kBlock, 0, s>>>(a, ts, os, base);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
