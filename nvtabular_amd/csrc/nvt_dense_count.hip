// Categorify.fit groupby-size WITHOUT global atomics: key column -> dense (key, count) list.
// Replaces categorify.py:955-1051 (_top_level_groupby, size only) and, with weights, the concat +
// re-groupby of :1054-1070.
//
// Why: the first version (nvt_count.hip: LDS front table + one global open-addressing table)
// spends its time in device-scope atomics -- 512-1024 workgroups flushing the same hot keys
// serialise at the memory-side atomic unit (36 distinct keys: 290 us; 1000 keys: 1 ms for a
// 45 M-row column whose stream takes 35 us), and every row of a high-cardinality column is 2
// random atomics.  LDS atomics, by contrast, run at near stream speed (micro-benchmark
// tools/micro/lds_count_probe.hip: 45 M keys, 36 distinct: 58 us = 3.1 TB/s).
//
// This unit is the driver: it decodes the path word of the C ABI (include/nvt_hip.h), checks the
// arguments and hands every column to the unit that owns its path.
//   0 / 6 / 7   nvt_count_lds.hip     the distinct keys fit workgroup-private LDS tables: one
//                                     counting launch (0: one key class, 6: the same for tiny
//                                     vocabularies, 7: two key classes) and one merge launch
//   1 / 2 / 3   nvt_count_part.hip    rows are hash-partitioned into 256 / 64 x 64 / 64 x 256
//                                     buckets, one LDS table per bucket
//   | HOT       nvt_hot_sample.hip,   paths 1 / 2 / 3, int32 keys without weights: the rows of a
//               nvt_count_part.hip    sampled set of hot keys are counted by the histogram pass and
//                                     leave the partition
//   9           nvt_range_count.hip   int32 keys without weights: buckets by key range, key-ordered
//                                     output (sampled by nvt_hot_sample.hip as well)
//   10          nvt_sort_count.hip    int32 keys without weights: radix sort + run lengths
// A path whose tables fill up raises NVT_ST_OVERFLOW bit0 and the caller reruns the column on a
// larger one.  nvt_lds_table.hpp holds the LDS table that paths 0 - 7 share.
#include <algorithm>
#include <vector>

#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"
#include "nvt_range.hpp"

namespace nvt {

// The path word, decoded: low byte = path, bit 4 = NVT_PATH_HOT, bits 8-15 = log2(buckets) of the
// range path, bit 16 = NVT_PATH_PIECES.
struct CountPath {
  int kind;  // 0, 6, 7, 1, 2, 3, NVT_PATH_RANGE or NVT_PATH_SORT
  bool hot, pieces;
  int nb_log2;
};

// Fills *p and returns nullptr, or returns why (path, key width, weights) is refused.  Every rule
// that depends on these three alone is here and nowhere else.
static const char *count_path(int path, int key_bytes, bool weighted, CountPath *p) {
  if (key_bytes != 4 && key_bytes != 8) return "key_bytes must be 4 or 8";
  *p = {path & 0xFF, false, false, 0};
  if (p->kind == NVT_PATH_SORT) {
    if (key_bytes != 4 || weighted) return "the sort path takes int32 keys without weights";
    return nullptr;
  }
  if (p->kind == NVT_PATH_RANGE) {
    if (key_bytes != 4 || weighted) return "the range path takes int32 keys without weights";
    p->nb_log2 = (path >> 8) & 0xFF;
    p->pieces = (path & NVT_PATH_PIECES) != 0;
    if (p->nb_log2 < 6 || p->nb_log2 > 10) return "range path: 64 .. 1024 buckets";
    return nullptr;
  }
  p->hot = (path & NVT_PATH_HOT) != 0;
  p->kind = path & ~NVT_PATH_HOT;
  const bool parted = p->kind >= 1 && p->kind <= 3;
  if (!(p->kind == 0 || p->kind == 6 || p->kind == 7 || parted))
    return "path must be 0 / 6 / 7 (LDS tables: one key class / tiny / two key classes) or "
           "1 / 2 / 3 (partitioned)";
  if (p->hot && !(parted && key_bytes == 4 && !weighted))
    return "the hot filter takes int32 keys without weights on paths 1 / 2 / 3";
  return nullptr;
}

// What is left to check of one column once its path is decoded; nullptr or the reason.
static const char *count_col_check(const CountPath &p, const nvt_count_col &c) {
  if (!c.state || !c.ws) return "null state/workspace";
  if (p.kind == NVT_PATH_RANGE && !c.hot_image)
    return "the range path needs the column's aux block (nvt_dense_count_many, hot_image)";
  if (p.kind == NVT_PATH_SORT && !c.hot_image)
    return "the sort path needs the column's histogram block";
  if (reinterpret_cast<uintptr_t>(c.keys) & 15) return "keys must be 16-byte aligned";
  if (c.n && !(c.keys && c.out_keys && c.out_counts)) return "null keys/out";
  if (p.kind != NVT_PATH_SORT && c.n >= (1ull << 32))
    return "at most 2^32-1 rows per call (32-bit LDS counters)";
  return nullptr;
}

// The single description of the workspace: every path's own layout walk (one walk per unit that
// yields size and pointers) behind one switch.
static uint64_t dense_ws_layout(const CountPath &p, int key_bytes, uint64_t n, bool weighted) {
  if (p.kind == NVT_PATH_SORT) return sort_count_ws_bytes(n);
  if (p.kind == NVT_PATH_RANGE) return range_count_ws_bytes(n, p.nb_log2);
  if (p.kind >= 1 && p.kind <= 3) return part_count_ws_bytes(p.kind, p.hot, key_bytes, weighted, n);
  return lds_count_ws_bytes(p.kind, key_bytes, weighted);
}

static const char *prof_name(const CountPath &p) {
  static const char *const kPlain[8] = {"dense_count_p0", "dense_count_p1", "dense_count_p2",
                                        "dense_count_p3", nullptr,          nullptr,
                                        "dense_count_p6", "dense_count_p7"};
  static const char *const kHot[4] = {nullptr, "dense_count_h1", "dense_count_h2", "dense_count_h3"};
  return p.hot ? kHot[p.kind] : kPlain[p.kind];
}

// paths 0 - 7: the unit that owns the path
template <typename K>
static int dense_count(const CountPath &p, const nvt_count_col &c, hipStream_t s) {
  if (p.kind >= 1 && p.kind <= 3) return part_count<K>(c, p.kind, p.hot, s);
  return lds_count<K>(c, p.kind, s);
}

// One checked column (count_path, count_col_check) on stream s.
static int count_column(const CountPath &p, const nvt_count_col &c, hipStream_t s, bool clear_state) {
  if (p.kind == NVT_PATH_SORT || p.kind == NVT_PATH_RANGE) {  // int32 keys (count_path)
    if (clear_state) NVT_CHECK_HIP(hipMemsetAsync(c.state, 0, NVT_STATE_WORDS * 8, s));
    if (c.n == 0) return NVT_OK;
    if (p.kind == NVT_PATH_SORT)
      return sort_count_i32((const int32_t *)c.keys, c.valid, c.n, c.ws, (unsigned *)c.hot_image,
                            (int32_t *)c.out_keys, c.out_counts, c.out_capacity, c.state, s);
    return range_count_i32((const int32_t *)c.keys, c.valid, c.n, p.nb_log2, c.ws, c.hot_image,
                           (int32_t *)c.out_keys, c.out_counts, c.out_capacity, c.range_table,
                           c.out_slots, c.state, s, p.pieces);
  }
  NVT_PROF(prof_name(p), c.n * c.key_bytes, s);
  if (clear_state) NVT_CHECK_HIP(hipMemsetAsync(c.state, 0, NVT_STATE_WORDS * 8, s));
  if (c.n == 0) return NVT_OK;
  return c.key_bytes == 4 ? dense_count<int32_t>(p, c, s) : dense_count<int64_t>(p, c, s);
}

// the single-column entry points: a descriptor without aux block or range table
static int count_single(const void *keys, const uint8_t *valid, const int64_t *weights, uint64_t n,
                        int key_bytes, int path, void *ws, void *out_keys, int64_t *out_counts,
                        uint64_t out_capacity, uint64_t *state, void *stream) {
  nvt_count_col c = {};
  c.keys = keys, c.valid = valid, c.weights = weights, c.n = n;
  c.key_bytes = key_bytes, c.path = path, c.ws = ws, c.state = state;
  c.out_keys = out_keys, c.out_counts = out_counts, c.out_capacity = out_capacity;
  CountPath p;
  const char *why = count_path(path, key_bytes, weights != nullptr, &p);
  if (!why) why = count_col_check(p, c);
  if (why) {
    set_error("dense_count: %s", why);
    return NVT_EINVAL;
  }
  return count_column(p, c, (hipStream_t)stream, true);
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_range_table_bytes(int nb_log2, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes && nb_log2 >= 6 && nb_log2 <= 10, "64 .. 1024 buckets");
  *bytes = (((uint64_t)1 << nb_log2) * kRpRegion + kRpGuard) * 8;
  return NVT_OK;
}
int nvt_dense_count_ws_bytes(int key_bytes, uint64_t n, int path, int weighted, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null bytes");
  CountPath p;
  if (const char *why = count_path(path, key_bytes, weighted != 0, &p)) {
    set_error("%s: %s", __func__, why);
    return NVT_EINVAL;
  }
  *bytes = dense_ws_layout(p, key_bytes, n, weighted != 0) + 64;
  return NVT_OK;
}
int nvt_dense_count_many(const nvt_count_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(ncols == 0 || cols, "null descriptors");
  // columns that were given DIFFERENT workspaces may run concurrently: each distinct ws pointer
  // (up to kSideStreams of them) gets an internal stream forked from / joined into `stream`, so
  // one column's short serial kernels (reduce / scan / offsets) hide under another's wide ones.
  // Columns sharing a workspace stay ordered on one stream.
  hipStream_t main_s = (hipStream_t)stream;
  std::vector<void *> wss;
  for (int i = 0; i < ncols; ++i)
    if (std::find(wss.begin(), wss.end(), cols[i].ws) == wss.end()) wss.push_back(cols[i].ws);
  if (wss.size() > (size_t)kSideStreams) {
    set_error("nvt_dense_count_many: at most %d distinct workspaces per call", kSideStreams);
    return NVT_EINVAL;
  }
  // every descriptor is checked before anything is put on a stream: a call that fails on its
  // arguments launches nothing
  std::vector<CountPath> paths(std::max(ncols, 0));
  for (int i = 0; i < ncols; ++i) {
    const char *why = count_path(cols[i].path, cols[i].key_bytes, cols[i].weights != nullptr, &paths[i]);
    if (!why) why = count_col_check(paths[i], cols[i]);
    if (why) {
      set_error("nvt_dense_count_many: %s (column %d)", why, i);
      return NVT_EINVAL;
    }
  }
  // state blocks laid out back to back (the usual case: one tensor, one row per column) are
  // cleared by ONE memset instead of one tiny fill kernel per column
  bool contiguous = ncols > 1;
  for (int i = 0; i < ncols && contiguous; ++i)
    contiguous = cols[i].state == cols[0].state + (uint64_t)i * NVT_STATE_WORDS;
  if (contiguous)
    NVT_CHECK_HIP(hipMemsetAsync(cols[0].state, 0, (uint64_t)ncols * NVT_STATE_WORDS * 8, main_s));
  SidePool *pool = nullptr;
  const bool fork = wss.size() > 1;
  if (fork) {
    int rc = side_pool(1, &pool);
    if (rc) return rc;
    NVT_CHECK_HIP(hipEventRecord(pool->fork, main_s));
    for (size_t k = 0; k < wss.size(); ++k) NVT_CHECK_HIP(hipStreamWaitEvent(pool->s[k], pool->fork, 0));
  }
  // hot-key samples of every filtered column: ONE launch (a workgroup per column) on the
  // caller's stream.  The internal streams were forked before it: columns that need no sample
  // start at once, a stream waits for the samples only in front of its first filtered column.
  auto sampled_here = [&](int i) {
    return (paths[i].hot || paths[i].kind == NVT_PATH_RANGE) && cols[i].hot_image && cols[i].n != 0;
  };
  bool sampled = false;
  {
    HotSampleBatch hb;
    int nh = 0;
    auto flush = [&]() -> int {
      if (nh) {
        NVT_PROF("dense_count_sample", 0, main_s);
        int rc = hot_sample_launch(hb, nh, main_s);
        if (rc) return rc;
        sampled = true;
      }
      nh = 0;
      return NVT_OK;
    };
    for (int i = 0; i < ncols; ++i) {
      if (!sampled_here(i)) continue;
      const nvt_count_col &c = cols[i];
      hb.c[nh++] = {(const int32_t *)c.keys, c.valid, c.n, c.hot_image, paths[i].nb_log2,
                    paths[i].pieces ? 1 : 0};
      if (nh == kHotBatch) {
        int rc = flush();
        if (rc) return rc;
      }
    }
    int rc = flush();
    if (rc) return rc;
  }
  bool waited[kSideStreams] = {false, false, false};
  int rc_all = NVT_OK;
  if (fork && sampled) NVT_CHECK_HIP(hipEventRecord(pool->aux, main_s));
  for (int i = 0; i < ncols; ++i) {
    const nvt_count_col &c = cols[i];
    hipStream_t cs = main_s;
    if (fork) {
      const size_t k = std::find(wss.begin(), wss.end(), c.ws) - wss.begin();
      cs = pool->s[k];
      if (sampled && (paths[i].hot || paths[i].kind == NVT_PATH_RANGE) && c.hot_image && !waited[k]) {
        NVT_CHECK_HIP(hipStreamWaitEvent(cs, pool->aux, 0));
        waited[k] = true;
      }
    }
    int rc = count_column(paths[i], c, cs, !contiguous);
    if (rc) {
      rc_all = rc;  // the columns launched so far keep running on the internal streams: they
      break;        // are joined below all the same, so the caller may free / reuse its buffers
    }
  }
  if (fork)
    for (size_t k = 0; k < wss.size(); ++k) {
      NVT_CHECK_HIP(hipEventRecord(pool->join[k], pool->s[k]));
      NVT_CHECK_HIP(hipStreamWaitEvent(main_s, pool->join[k], 0));
    }
  return rc_all;
}
int nvt_dense_count_i32(const int32_t *keys, const uint8_t *valid, const int64_t *weights,
                        uint64_t n, int path, void *ws, int32_t *out_keys, int64_t *out_counts,
                        uint64_t out_capacity, uint64_t *state, void *stream) {
  return count_single(keys, valid, weights, n, 4, path, ws, out_keys, out_counts, out_capacity,
                         state, stream);
}
int nvt_dense_count_i64(const int64_t *keys, const uint8_t *valid, const int64_t *weights,
                        uint64_t n, int path, void *ws, int64_t *out_keys, int64_t *out_counts,
                        uint64_t out_capacity, uint64_t *state, void *stream) {
  return count_single(keys, valid, weights, n, 8, path, ws, out_keys, out_counts, out_capacity,
                         state, stream);
}

}  // extern "C"
