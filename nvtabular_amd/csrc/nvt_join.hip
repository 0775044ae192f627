// Hash join of partitions against an external table (ops.JoinExternal).
//
// Keys.  Every key component is reduced to a canonical 64-bit word plus a null bit (canon below):
// NVT_JOIN_INT compares by value (any integer width, string surrogates), NVT_JOIN_FLOAT by the bits
// of the double value (-0.0 -> 0.0; an integer column is converted to double, as pandas' merge does
// when one side is float).  A null component is a validity bit 0 or a NaN; nulls match nulls.
//
// Table.  Open addressing in HBM, 16-byte slots {tag, first, count}, linear probing from
// fmix64(tag), load <= 0.5.  One key component: tag = the word itself (stored whole, no
// verification); its null rows are one group kept outside the table (null_first / null_count).
// Two to four components: tag = a fingerprint of the words and null bits, and a hit is verified
// against the grouped canonical words of the external table.  `empty` is a tag value no external
// key has (the host picks it); a left key whose tag equals it cannot match.
//
// The external rows are grouped by key (a stable sort on the host side), so the rows of a key are
// the positions [first, first + count) of the grouped payload columns, in external order.
//
// Output validity words are built with __ballot over 64 consecutive rows of a wave; lane 0 writes
// each 8-byte word with an ordinary store, so bits past the row count are 0 and no atomics touch
// the outputs.
#include "nvt_common.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr int kMaxKeys = NVT_JOIN_MAX_KEYS;
constexpr int kMaxCols = NVT_JOIN_MAX_COLS;

struct JKey {
  const void *x;
  const uint8_t *valid;
  int dtype, mode;
};
struct JKeys {
  JKey k[kMaxKeys];
  int nkeys;
};

struct JIndex {
  const uint4 *slots;
  uint64_t mask;  // capacity - 1
  uint64_t empty;
  const uint64_t *words;  // [nkeys][n_ext] (nkeys >= 2)
  const uint8_t *nulls;   // [n_ext]       (nkeys >= 2)
  uint64_t n_ext;
  uint64_t null_first, null_count;
};

struct JCol {
  const void *src;
  const uint8_t *src_valid;
  void *dst;
  uint64_t *dst_valid;
  int width;
};
struct JBatch {
  JCol c[kMaxCols];
  int ncols;
};

__device__ __forceinline__ uint64_t float_word(double d, bool &null) {
  if (d != d) null = true;
  if (null) return 0;
  if (d == 0.0) d = 0.0;  // -0.0 == 0.0
  return (uint64_t)__double_as_longlong(d);
}

__device__ __forceinline__ uint64_t canon(const JKey &k, uint64_t row, bool &null) {
  null = !bit_valid(k.valid, row);
  if (k.dtype == NVT_F32) return float_word((double)((const float *)k.x)[row], null);
  if (k.dtype == NVT_F64) return float_word(((const double *)k.x)[row], null);
  int64_t v;
  if (k.dtype == NVT_I32) v = ((const int32_t *)k.x)[row];
  else if (k.dtype == NVT_I64) v = ((const int64_t *)k.x)[row];
  else v = ((const uint8_t *)k.x)[row];
  if (k.mode == NVT_JOIN_FLOAT) return float_word((double)v, null);
  return null ? 0 : (uint64_t)v;
}

// The null bits are mixed before the first word meets them: XOR-ed in raw, bit k of `nulls` and
// bit k of w[0] + constant cancel, and the ordinary keys (0, null) and (2, 0) share a tag.
__device__ __forceinline__ uint64_t tuple_tag(const uint64_t *w, unsigned nulls, int nkeys) {
  uint64_t h = fmix64(0x243F6A8885A308D3ull ^ nulls);
#pragma unroll
  for (int j = 0; j < kMaxKeys; ++j)
    if (j < nkeys) h = fmix64(h ^ (w[j] + 0x9E3779B97F4A7C15ull * (uint64_t)(j + 1)));
  return h;
}

// the words, null bits and tag of one row's key
__device__ __forceinline__ uint64_t row_key(const JKeys &ks, uint64_t row, uint64_t *w, unsigned &nulls) {
  nulls = 0;
#pragma unroll
  for (int j = 0; j < kMaxKeys; ++j) {
    w[j] = 0;
    if (j < ks.nkeys) {
      bool nl;
      w[j] = canon(ks.k[j], row, nl);
      nulls |= (unsigned)nl << j;
    }
  }
  return ks.nkeys == 1 ? w[0] : tuple_tag(w, nulls, ks.nkeys);
}

// grouped position of the first external row matching `row`'s key, or -1; cnt = its row count
__device__ __forceinline__ int64_t probe_row(const JIndex &ix, const JKeys &ks, uint64_t row, uint32_t &cnt) {
  uint64_t w[kMaxKeys];
  unsigned nulls;
  const uint64_t tag = row_key(ks, row, w, nulls);
  cnt = 0;
  if (ks.nkeys == 1 && nulls) {
    if (ix.null_count == 0) return -1;
    cnt = (uint32_t)ix.null_count;
    return (int64_t)ix.null_first;
  }
  if (tag == ix.empty) return -1;
  uint64_t h = fmix64(tag) & ix.mask;
  for (uint64_t p = 0; p <= ix.mask; ++p) {
    const uint4 s = ix.slots[h];
    const uint64_t t = (uint64_t)s.x | ((uint64_t)s.y << 32);
    if (t == tag) {
      if (ks.nkeys > 1) {
        if (ix.nulls[s.z] != nulls) return -1;
#pragma unroll
        for (int j = 0; j < kMaxKeys; ++j)
          if (j < ks.nkeys && ix.words[(uint64_t)j * ix.n_ext + s.z] != w[j]) return -1;
      }
      cnt = s.w;
      return (int64_t)s.z;
    }
    if (t == ix.empty) return -1;
    h = (h + 1) & ix.mask;
  }
  return -1;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[row] = src[f] for every column (0 and a cleared validity bit where f < 0); one wave per 64
// consecutive rows, grid-strided.  `f_of(row)` gives the source position of an output row.
template <typename F>
__device__ __forceinline__ uint64_t gather_rows(uint64_t n, const JBatch &b, F f_of) {
  const uint64_t nchunks = (n + 63) / 64;
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / kWave);
  const unsigned lane = lane_id();
  uint64_t misses = 0;
  for (uint64_t c = wave; c < nchunks; c += nwaves) {
    const uint64_t row = c * 64 + lane;
    const bool in = row < n;
    const int64_t f = in ? f_of(row) : -1;
    const bool hit = f >= 0;
    misses += (uint64_t)__popcll(__ballot(in && !hit));
    for (int j = 0; j < b.ncols; ++j) {
      const JCol &g = b.c[j];
      if (in) {
        if (g.width == 8) {
          ((uint64_t *)g.dst)[row] = hit ? ((const uint64_t *)g.src)[f] : 0ull;
        } else if (g.width == 4) {
          ((uint32_t *)g.dst)[row] = hit ? ((const uint32_t *)g.src)[f] : 0u;
        } else {
          ((uint8_t *)g.dst)[row] = hit ? ((const uint8_t *)g.src)[f] : (uint8_t)0;
        }
      }
      if (g.dst_valid != nullptr) {
        const uint64_t word = __ballot(hit && bit_valid(g.src_valid, (uint64_t)f));
        if (lane == 0) g.dst_valid[c] = word;
      }
    }
  }
  return misses;  // (the same in every lane)
}

__global__ __launch_bounds__(kBlock) void hash_kernel(JKeys ks, uint64_t n, uint64_t *__restrict__ tag,
                                                      uint64_t *__restrict__ words, uint8_t *__restrict__ nulls) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    uint64_t w[kMaxKeys];
    unsigned nb;
    tag[i] = row_key(ks, i, w, nb);
    nulls[i] = (uint8_t)nb;
    if (words != nullptr) {
#pragma unroll
      for (int j = 0; j < kMaxKeys; ++j)
        if (j < ks.nkeys) words[(uint64_t)j * n + i] = w[j];
    }
  }
}

// one lane per distinct key: claim a slot with a 64-bit CAS on its tag, then write {first, count}
__global__ __launch_bounds__(kBlock) void insert_kernel(unsigned long long *slots, uint64_t mask, uint64_t empty,
                                                        const uint64_t *__restrict__ tags,
                                                        const uint32_t *__restrict__ first,
                                                        const uint32_t *__restrict__ count, uint64_t ng) {
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < ng; g += (uint64_t)gridDim.x * kBlock) {
    const uint64_t tag = tags[g];
    uint64_t h = fmix64(tag) & mask;
    for (uint64_t p = 0; p <= mask; ++p) {
      const unsigned long long prev = atomicCAS(&slots[2 * h], (unsigned long long)empty, (unsigned long long)tag);
      if (prev == empty) {
        slots[2 * h + 1] = (unsigned long long)first[g] | ((unsigned long long)count[g] << 32);
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

__global__ __launch_bounds__(kBlock) void probe_kernel(JIndex ix, JKeys ks, uint64_t n, int inner,
                                                       int64_t *__restrict__ out_first,
                                                       uint32_t *__restrict__ out_count,
                                                       uint8_t *__restrict__ out_keep,
                                                       unsigned long long *out_total) {
  uint64_t total = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    uint32_t cnt;
    const int64_t f = probe_row(ix, ks, i, cnt);
    const uint32_t c = inner ? cnt : (cnt > 1 ? cnt : 1u);
    out_first[i] = f;
    if (out_count) out_count[i] = c;
    if (out_keep) out_keep[i] = f >= 0;
    total += c;
  }
  if (out_total) {
    total = wave_sum_u64(total);
    if (lane_id() == 0 && total) atomicAdd(out_total, (unsigned long long)total);
  }
}

__global__ __launch_bounds__(kBlock) void probe_gather_kernel(JIndex ix, JKeys ks, uint64_t n, JBatch b,
                                                              unsigned long long *unmatched) {
  const uint64_t misses = gather_rows(n, b, [&](uint64_t row) {
    uint32_t cnt;
    return probe_row(ix, ks, row, cnt);
  });
  if (unmatched && lane_id() == 0 && misses) atomicAdd(unmatched, (unsigned long long)misses);
}

__global__ __launch_bounds__(kBlock) void gather_kernel(const int64_t *__restrict__ idx, uint64_t m, JBatch b) {
  gather_rows(m, b, [&](uint64_t row) { return idx[row]; });
}

// one lane per OUTPUT row: the left row is the last i with offsets[i] <= j (a bisection), so a key
// with 10^5 external rows spreads over as many lanes as it has output rows
__global__ __launch_bounds__(kBlock) void expand_kernel(const uint32_t *__restrict__ off,
                                                        const int64_t *__restrict__ first, uint64_t n, uint64_t m,
                                                        int64_t *__restrict__ out_left, int64_t *__restrict__ out_ext) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if ((uint64_t)off[mid] <= j) lo = mid;
      else hi = mid;
    }
    const int64_t f = first[lo];
    out_left[j] = (int64_t)lo;
    out_ext[j] = f >= 0 ? f + (int64_t)(j - off[lo]) : -1;
  }
}

int load_keys(const nvt_join_key *keys, int nkeys, uint64_t n, JKeys &ks) {
  NVT_CHECK_ARG(keys, "null key descriptors");
  NVT_CHECK_ARG(nkeys >= 1 && nkeys <= kMaxKeys, "nkeys must be 1 to 4");
  memset(&ks, 0, sizeof(ks));
  ks.nkeys = nkeys;
  for (int j = 0; j < nkeys; ++j) {
    const nvt_join_key &k = keys[j];
    NVT_CHECK_ARG(k.dtype >= NVT_F32 && k.dtype <= NVT_U8, "unsupported key dtype");
    NVT_CHECK_ARG(k.mode == NVT_JOIN_INT || k.mode == NVT_JOIN_FLOAT, "mode must be NVT_JOIN_INT or NVT_JOIN_FLOAT");
    NVT_CHECK_ARG(k.mode == NVT_JOIN_FLOAT || (k.dtype != NVT_F32 && k.dtype != NVT_F64),
                  "a float key column needs NVT_JOIN_FLOAT");
    NVT_CHECK_ARG(k.x || n == 0, "null key column");
    ks.k[j] = JKey{k.x, k.valid, k.dtype, k.mode};
  }
  return NVT_OK;
}

int load_index(const nvt_join_index *ix, int nkeys, JIndex &j) {
  NVT_CHECK_ARG(ix, "null index");
  NVT_CHECK_ARG(ix->slots, "null slot table");
  NVT_CHECK_ARG(ix->capacity >= 2 && (ix->capacity & (ix->capacity - 1)) == 0, "capacity must be a power of two");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ix->slots) & 15) == 0, "slots must be 16-byte aligned");
  NVT_CHECK_ARG(ix->nkeys == nkeys, "the index was built for another number of key columns");
  NVT_CHECK_ARG(nkeys == 1 || ix->n_ext == 0 || (ix->words && ix->nulls), "null verification words");
  NVT_CHECK_ARG(ix->null_count == 0 || ix->null_first + ix->null_count <= ix->n_ext, "null group out of range");
  j = JIndex{reinterpret_cast<const uint4 *>(ix->slots), ix->capacity - 1, ix->empty, ix->words, ix->nulls,
             ix->n_ext, ix->null_first, ix->null_count};
  return NVT_OK;
}

int load_cols(const nvt_join_col *cols, int ncols, bool need_valid, JBatch &b, uint64_t &bytes) {
  NVT_CHECK_ARG(cols, "null column descriptors");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= kMaxCols, "ncols must be 1 to 16");
  memset(&b, 0, sizeof(b));
  b.ncols = ncols;
  bytes = 0;
  for (int j = 0; j < ncols; ++j) {
    const nvt_join_col &c = cols[j];
    NVT_CHECK_ARG(c.width == 1 || c.width == 4 || c.width == 8, "width must be 1, 4 or 8 bytes");
    NVT_CHECK_ARG(c.src && c.dst, "null column");
    NVT_CHECK_ARG(c.dst_valid || !need_valid, "null dst_valid");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.dst_valid) & 7) == 0, "dst_valid must be 8-byte aligned");
    b.c[j] = JCol{c.src, c.src_valid, c.dst, reinterpret_cast<uint64_t *>(c.dst_valid), c.width};
    bytes += 2 * (uint64_t)c.width + (c.dst_valid ? 1 : 0);
  }
  return NVT_OK;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_join_table_bytes(uint64_t n_groups, uint64_t *capacity, uint64_t *bytes) {
  NVT_CHECK_ARG(capacity && bytes, "null output");
  NVT_CHECK_ARG(n_groups < (1ull << 32), "more than 2^32 distinct keys");
  uint64_t cap = 64;
  while (cap < 2 * n_groups) cap <<= 1;
  *capacity = cap;
  *bytes = cap * 16;
  return NVT_OK;
}

int nvt_join_hash(const nvt_join_key *keys, int nkeys, uint64_t n, uint64_t *out_tag, uint64_t *out_words,
                  uint8_t *out_nulls, void *stream) {
  JKeys ks;
  const int rc = load_keys(keys, nkeys, n, ks);
  if (rc) return rc;
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(out_tag && out_nulls, "null output");
  NVT_CHECK_ARG(nkeys == 1 || out_words, "null out_words");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_hash", n * (8ull * nkeys + 9), s);
  hash_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(ks, n, out_tag, nkeys > 1 ? out_words : nullptr, out_nulls);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_join_insert(void *slots, uint64_t capacity, uint64_t empty, const uint64_t *tags, const uint32_t *first,
                    const uint32_t *count, uint64_t n_groups, void *stream) {
  NVT_CHECK_ARG(slots, "null slot table");
  NVT_CHECK_ARG(capacity >= 2 && (capacity & (capacity - 1)) == 0, "capacity must be a power of two");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(slots) & 15) == 0, "slots must be 16-byte aligned");
  NVT_CHECK_ARG(n_groups <= capacity / 2, "load above 0.5");
  if (n_groups == 0) return NVT_OK;
  NVT_CHECK_ARG(tags && first && count, "null group arrays");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_insert", n_groups * 32, s);
  insert_kernel<<<stream_grid(n_groups, kBlock), kBlock, 0, s>>>((unsigned long long *)slots, capacity - 1, empty,
                                                                  tags, first, count, n_groups);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_join_probe(const nvt_join_index *ix, const nvt_join_key *keys, int nkeys, uint64_t n, int inner,
                   int64_t *out_first, uint32_t *out_count, uint8_t *out_keep, uint64_t *out_total, void *stream) {
  JKeys ks;
  int rc = load_keys(keys, nkeys, n, ks);
  if (rc) return rc;
  JIndex j;
  rc = load_index(ix, nkeys, j);
  if (rc) return rc;
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(out_first, "null out_first");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_probe", n * (8ull * nkeys + 16 + 13), s);
  probe_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(j, ks, n, inner != 0, out_first, out_count, out_keep,
                                                         (unsigned long long *)out_total);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_join_probe_gather(const nvt_join_index *ix, const nvt_join_key *keys, int nkeys, uint64_t n,
                          const nvt_join_col *cols, int ncols, uint64_t *unmatched, void *stream) {
  JKeys ks;
  int rc = load_keys(keys, nkeys, n, ks);
  if (rc) return rc;
  JIndex j;
  rc = load_index(ix, nkeys, j);
  if (rc) return rc;
  JBatch b;
  uint64_t per_row;
  rc = load_cols(cols, ncols, true, b, per_row);
  if (rc) return rc;
  if (n == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_probe_gather", n * (8ull * nkeys + 16 + per_row), s);
  probe_gather_kernel<<<stream_grid((n + 63) / 64, kBlock / kWave), kBlock, 0, s>>>(
      j, ks, n, b, (unsigned long long *)unmatched);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_join_scan_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  *bytes = scan_chunks(n + 1) * 8;
  return NVT_OK;
}

int nvt_join_offsets(uint32_t *counts, uint64_t n, void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(counts, "null counts");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace must be 8-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= scan_chunks(n + 1) * 8, "workspace smaller than nvt_join_scan_ws_bytes(n)");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_offsets", (n + 1) * 8, s);
  return exclusive_scan_u32(counts, n + 1, (unsigned long long *)ws, s);
}

int nvt_join_expand(const uint32_t *offsets, const int64_t *first, uint64_t n, uint64_t m, int64_t *out_left,
                    int64_t *out_ext, void *stream) {
  if (m == 0) return NVT_OK;
  NVT_CHECK_ARG(n > 0, "output rows from no left rows");
  NVT_CHECK_ARG(m < (1ull << 32), "output rows must be below 2^32");
  NVT_CHECK_ARG(offsets && first && out_left && out_ext, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_expand", m * 24, s);
  expand_kernel<<<stream_grid(m, kBlock), kBlock, 0, s>>>(offsets, first, n, m, out_left, out_ext);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_join_gather(const int64_t *idx, uint64_t m, const nvt_join_col *cols, int ncols, void *stream) {
  JBatch b;
  uint64_t per_row;
  const int rc = load_cols(cols, ncols, false, b, per_row);
  if (rc) return rc;
  if (m == 0) return NVT_OK;
  NVT_CHECK_ARG(idx, "null idx");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("join_gather", m * (8 + per_row), s);
  gather_kernel<<<stream_grid((m + 63) / 64, kBlock / kWave), kBlock, 0, s>>>(idx, m, b);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
