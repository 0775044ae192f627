// Cross-file entry points of the kernel library (host side), used by the batched C-ABI calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nvt_hip.h"

namespace nvt {

// nvt_util.hip: per-device pools of internal streams that batched calls fork onto from / join
// into the caller's stream (`which` 0: vocabulary finalisation, 1: counting)
constexpr int kSideStreams = 3;
struct SidePool {
  int dev = -1, which = 0;
  hipStream_t s[kSideStreams];
  hipEvent_t fork, join[kSideStreams], aux;
};
int side_pool(int which, SidePool **out);

// nvt_sort.hip
int vocab_sort_any(int key_bytes, void *keys, int64_t *counts, uint64_t n, int64_t max_count,
                   void *tmp, hipStream_t s);
struct SmallSortDesc {
  int32_t *keys;
  int64_t *counts;
  unsigned n;
  void *tmp;  // 8 n bytes of scratch, or nullptr (n > 2048 is then sorted by one workgroup)
};
// int32 keys, 2 <= n <= 16384, 0 < max_count < 2^32: sorted by the batched small sort (chunks of
// 2048 in LDS, one workgroup each; longer lists are then merged by rank through their scratch)
bool vocab_sort_small_eligible(int key_bytes, uint64_t n, int64_t max_count);
int vocab_sort_small_batch(const SmallSortDesc *cols, int ncols, hipStream_t s);

// stable LSD radix sort of packed 64-bit words on the bit range [bit_lo, bit_hi); *result is
// `data` or a buffer inside tmp (sort_words_tmp_bytes(n) bytes)
uint64_t sort_words_tmp_bytes(uint64_t n);
int sort_words_bits(uint64_t *data, uint64_t n, int bit_lo, int bit_hi, void *tmp, uint64_t **result,
                    hipStream_t s);
// the packed rows of a key column ((key - bias) image << 32 | fold << rb | row) sorted by bits
// [rb, 64) without writing the unsorted words out first; *result = a buffer inside tmp
int sort_packed_keys(const void *keys, int key_dtype, int64_t key_bias, const uint8_t *fold, int rb,
                     uint64_t n, void *tmp, uint64_t **result, hipStream_t stream);

// nvt_hot_sample.hip: the sample in front of the hot filter (paths 1 / 2 / 3 | NVT_PATH_HOT) and of
// the range path; one launch, one workgroup per column, ncols <= kHotBatch
struct HotSampleCol {
  const int32_t *keys;
  const uint8_t *valid;
  uint64_t n;
  int32_t *image;
  int nb_log2;  // > 0: also derive the key ranges of the range path (image[NVT_RANGE_AUX_*])
  int pieces;   // range path: also decide on the piecewise map (NVT_PATH_PIECES: after an overflow)
};
constexpr int kHotBatch = 32;
struct HotSampleBatch {
  HotSampleCol c[kHotBatch];
};
int hot_sample_launch(const HotSampleBatch &batch, int ncols, hipStream_t s);

// nvt_count_lds.hip: paths 0 / 6 / 7 of nvt_dense_count_* (`kind`) for a column the driver
// (nvt_dense_count.hip) has checked, n > 0; K = int32_t or int64_t as c.key_bytes says
uint64_t lds_count_ws_bytes(int kind, int key_bytes, bool weighted);
template <typename K>
int lds_count(const nvt_count_col &c, int kind, hipStream_t s);

// nvt_count_part.hip: paths 1 / 2 / 3, with the hot filter in front when `hot` (c.hot_image = the
// column's sampled image, or nullptr: sampled here into the workspace)
uint64_t part_count_ws_bytes(int kind, bool hot, int key_bytes, bool weighted, uint64_t n);
template <typename K>
int part_count(const nvt_count_col &c, int kind, bool hot, hipStream_t s);

// nvt_range_count.hip: path NVT_PATH_RANGE of nvt_dense_count_* (aux = hot image + range
// parameters written by hot_sample_kernel + class histogram)
uint64_t range_count_ws_bytes(uint64_t n, int nb_log2);
int range_count_i32(const int32_t *keys, const uint8_t *valid, uint64_t n, int nb_log2, void *ws,
                    int32_t *aux, int32_t *out_keys, int64_t *out_cnt, uint64_t out_cap,
                    void *range_table, uint32_t *out_slots, uint64_t *state, hipStream_t s, bool pieces);

// nvt_sort_count.hip: path NVT_PATH_SORT of nvt_dense_count_* (radix sort + run lengths; hist =
// the column's uint32[256] class histogram block)
uint64_t sort_count_ws_bytes(uint64_t n);
int sort_count_i32(const int32_t *keys, const uint8_t *valid, uint64_t n, void *ws, unsigned *hist,
                   int32_t *out_keys, int64_t *out_cnt, uint64_t out_cap, uint64_t *state,
                   hipStream_t s);

// nvt_vocab_order.hip: vocabulary order of a KEY-SORTED (key, count) list (range path) in one stable
// counting pass on min(count, 255) + encode table filled in the same pass
uint64_t vocab_order_tmp_bytes(uint64_t n, uint64_t n_big);
int vocab_order_from_sorted(const int32_t *src_keys, const int64_t *src_cnts, uint64_t n,
                            const unsigned *cls_hist, uint64_t n_big, int64_t max_count,
                            int32_t *out_keys, int64_t *out_cnts, void *tmp, int64_t first_label,
                            void *table, uint64_t capacity, int64_t *sentinel_label,
                            const int32_t *range_aux, int range_nb_log2, hipStream_t s,
                            bool *tail_deferred, uint64_t flat_slots = 0,
                            const uint32_t *src_slots = nullptr);
// the same for several vocabularies that own a range table (dumped or flat): one launch per
// stage for ALL of them, class-255 tails included
struct OrderSortedJob {
  const int32_t *src_keys;
  const int64_t *src_cnts;
  uint64_t n;
  const unsigned *cls_hist;
  uint64_t n_big;
  int64_t max_count;
  int32_t *out_keys;
  int64_t *out_cnts;
  void *tmp;
  int64_t first_label;
  void *table;
  uint64_t capacity;
  int64_t *sentinel_label;
  const int32_t *range_aux;
  int range_nb_log2;
  uint64_t flat_slots;
  const uint32_t *src_slots;  // dumped table: the slot of every source entry, or nullptr (patch pass)
};
int vocab_order_sorted_batch(const OrderSortedJob *jobs, int njobs, hipStream_t s);
// LDS head image of an ordered int32 vocabulary for the cache-mode encode (nvt_encode_build.hip)
int encode_head_build(const int32_t *vocab_keys, uint64_t n, int64_t first_label, void *image,
                      hipStream_t s);
int encode_head_build_many(const int32_t *const *vocab_keys, const uint64_t *n, const int64_t *first_label,
                           void *const *images, int count, hipStream_t s);
// key-sorted list whose entries carry their 0-based position in the vocabulary order (multi-GPU:
// labelled shard by shard on the owners): ordered arrays + table without any ordering pass
int vocab_from_labels(const int32_t *src_keys, const int64_t *src_cnts, const int32_t *labels, uint64_t n,
                      int32_t *out_keys, int64_t *out_cnts, void *tmp, int64_t first_label, void *table,
                      uint64_t capacity, int64_t *sentinel_label, const int32_t *range_aux,
                      uint64_t flat_slots, hipStream_t s);
// the deferred part: sort of the n_big leading entries (class 255) + their labels
struct OrderTail {
  int32_t *keys;
  int64_t *counts;
  uint64_t n_big;
  int64_t first_label;
  void *table;
  uint64_t capacity;
  int64_t *sentinel_label;
  const int32_t *range_aux;
  void *tmp;   // the vocabulary's ordering workspace (its sort scratch serves the small sort)
  uint64_t n;  // entries of the whole vocabulary: what the workspace was laid out for
};
int vocab_order_tail_batch(const OrderTail *t, int nt, hipStream_t s);

// nvt_encode_build.hip
int encode_clear_any(int key_bytes, void *table, uint64_t capacity, int64_t *sentinel_label,
                     hipStream_t s);
// insert vocab[0 .. n) with labels first_label + i into an already cleared / partly filled table
int encode_insert_any(int key_bytes, const void *vocab, uint64_t n, int64_t first_label,
                      void *table, uint64_t capacity, int64_t *sentinel_label, hipStream_t s);
int encode_build_any(int key_bytes, const void *vocab, uint64_t n, int64_t first_label, void *table,
                     uint64_t capacity, int64_t *sentinel_label, int unique_keys, hipStream_t s);

}  // namespace nvt
