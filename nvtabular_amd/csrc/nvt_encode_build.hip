// Building what Categorify.transform probes: the hashed {key, label} table in HBM (clear + insert,
// whole or in the two halves the one-pass vocabulary ordering uses) and the prebuilt image of the
// LDS head of an ordered int32 vocabulary.  The row kernels are in nvt_encode.hip.
#include <limits>

#include "nvt_common.hpp"
#include "nvt_encode_table.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"

namespace nvt {

template <typename K>
__global__ __launch_bounds__(kBlock) void enc_clear_kernel(EncSlot<K> *table, uint64_t capacity,
                                                           int64_t *sentinel_label) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  EncSlot<K> e;
  e.key = EncTraits<K>::empty;
  e.label = std::numeric_limits<decltype(e.label)>::max();  // atomicMin target
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < capacity; i += stride)
    table[i] = e;
  if (blockIdx.x == 0 && threadIdx.x == 0) *sentinel_label = -1;
}

template <typename K>
__global__ __launch_bounds__(kBlock) void enc_build_kernel(const K *__restrict__ vocab, uint64_t n,
                                                           int64_t first_label, EncSlot<K> *table,
                                                           uint64_t mask, int64_t *sentinel_label) {
  constexpr K EMPTY = EncTraits<K>::empty;
  using C = typename EncTraits<K>::cas_t;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    K key = vocab[i];
    int64_t label = first_label + (int64_t)i;
    if (key == EMPTY) {
      // the sentinel key lives in a word of its own; a vocabulary may hold it more than once like
      // any other key, and the first (lowest) label wins here too: the cleared word is -1, the
      // largest value of an unsigned minimum (labels are never negative)
      atomicMin(reinterpret_cast<unsigned long long *>(sentinel_label), (unsigned long long)label);
      continue;
    }
    uint64_t slot = (uint64_t)slot_hash(key) & mask;
    while (true) {
      K prev = (K)atomicCAS(reinterpret_cast<C *>(&table[slot].key), (C)EMPTY, (C)key);
      if (prev == EMPTY || prev == key) {
        // duplicate vocabulary keys (user-supplied vocabs): first (lowest) label wins,
        // so every writer goes through atomicMin against the cleared max value
        using L = decltype(table[slot].label);
        if constexpr (sizeof(L) == 4)
          atomicMin(reinterpret_cast<int *>(&table[slot].label), (int)label);
        else
          atomicMin(reinterpret_cast<long long *>(&table[slot].label), (long long)label);
        break;
      }
      slot = (slot + 1) & mask;
    }
  }
}

// Vocabulary produced by fit: keys are unique, so an int32 slot {key,label} is claimed
// and filled by ONE 64-bit CAS (half the atomics of the general build above).
__global__ __launch_bounds__(kBlock) void enc_build_unique_i32_kernel(
    const int32_t *__restrict__ vocab, uint64_t n, int64_t first_label, EncSlot<int32_t> *table,
    uint64_t mask, int64_t *sentinel_label) {
  const unsigned long long EMPTY_SLOT =
      ((unsigned long long)(uint32_t)std::numeric_limits<int32_t>::max() << 32) |
      (unsigned long long)(uint32_t)INT32_MIN;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    int32_t key = vocab[i];
    int64_t label = first_label + (int64_t)i;
    if (key == INT32_MIN) {
      *sentinel_label = label;
      continue;
    }
    unsigned long long want = ((unsigned long long)(uint32_t)label << 32) | (uint32_t)key;
    uint64_t slot = (uint64_t)slot_hash(key) & mask;
    while (atomicCAS(reinterpret_cast<unsigned long long *>(&table[slot]), EMPTY_SLOT, want) !=
           EMPTY_SLOT)
      slot = (slot + 1) & mask;
  }
}

struct HeadJob {
  const int32_t *keys;
  unsigned char *image;
  int64_t first_label;
  uint32_t n_hot;
};
constexpr int kHeadJobsMax = 32;
struct HeadJobs {
  HeadJob j[kHeadJobsMax];
};

__global__ __launch_bounds__(kEncBS) void enc_head_build_many_kernel(HeadJobs jobs) {
  constexpr int kLdsBytes = kHeadLdsBytes<int32_t, true>;
  __shared__ __align__(16) unsigned char lraw[kLdsBytes];
  __shared__ long long s_sent;
  const HeadJob j = jobs.j[blockIdx.x];
  build_head<int32_t, true>(lraw, &s_sent, j.keys, j.n_hot, j.first_label);
  const int4 *src = reinterpret_cast<const int4 *>(lraw);
  int4 *dst = reinterpret_cast<int4 *>(j.image);
  for (int i = threadIdx.x; i < kLdsBytes / 16; i += kEncBS) dst[i] = src[i];
  if (threadIdx.x == 0) *reinterpret_cast<long long *>(j.image + kLdsBytes) = s_sent;
}

template <typename K>
int build_launch(const K *vocab, uint64_t n, int64_t first_label, void *table, uint64_t capacity,
                 int64_t *sentinel_label, int unique_keys, hipStream_t s) {
  NVT_CHECK_ARG(table && sentinel_label, "null table");
  NVT_CHECK_ARG(capacity >= 64 && (capacity & (capacity - 1)) == 0, "capacity must be 2^k >= 64");
  NVT_CHECK_ARG(capacity > n, "capacity must exceed the vocabulary size");
  NVT_CHECK_ARG(sizeof(K) == 8 || first_label + (int64_t)n < INT32_MAX, "labels overflow int32");
  // (a negative label reads as "not in the vocabulary" in every encode kernel, and would lose
  // against the cleared sentinel word in enc_build_kernel's unsigned minimum)
  NVT_CHECK_ARG(first_label >= 0, "first_label must not be negative");
  auto *t = reinterpret_cast<EncSlot<K> *>(table);
  NVT_PROF("encode_build", 0, s);
  enc_clear_kernel<K><<<stream_grid(capacity, kBlock * 4), kBlock, 0, s>>>(t, capacity,
                                                                           sentinel_label);
  NVT_CHECK_LAUNCH();
  if (n) {
    NVT_CHECK_ARG(vocab, "null vocabulary");
    if constexpr (sizeof(K) == 4) {
      if (unique_keys) {
        enc_build_unique_i32_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(
            vocab, n, first_label, t, capacity - 1, sentinel_label);
        NVT_CHECK_LAUNCH();
        return NVT_OK;
      }
    }
    enc_build_kernel<K><<<stream_grid(n, kBlock), kBlock, 0, s>>>(vocab, n, first_label, t,
                                                                  capacity - 1, sentinel_label);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int encode_build_any(int key_bytes, const void *vocab, uint64_t n, int64_t first_label, void *table,
                     uint64_t capacity, int64_t *sentinel_label, int unique_keys, hipStream_t s) {
  if (key_bytes == 4)
    return build_launch<int32_t>((const int32_t *)vocab, n, first_label, table, capacity,
                                 sentinel_label, unique_keys, s);
  return build_launch<int64_t>((const int64_t *)vocab, n, first_label, table, capacity,
                               sentinel_label, unique_keys, s);
}

// the two halves of a build, for callers that fill most of the table themselves (the one-pass
// vocabulary ordering, nvt_vocab_order.hip): clear, then insert a duplicate-free int32 key range
int encode_clear_any(int key_bytes, void *table, uint64_t capacity, int64_t *sentinel_label,
                     hipStream_t s) {
  NVT_CHECK_ARG(table && sentinel_label, "null table");
  NVT_CHECK_ARG(capacity >= 64, "capacity must be >= 64");  // (any size: flat range tables)
  NVT_PROF("encode_build", 0, s);
  if (key_bytes == 4)
    enc_clear_kernel<int32_t><<<stream_grid(capacity, kBlock * 4), kBlock, 0, s>>>(
        reinterpret_cast<EncSlot<int32_t> *>(table), capacity, sentinel_label);
  else
    enc_clear_kernel<int64_t><<<stream_grid(capacity, kBlock * 4), kBlock, 0, s>>>(
        reinterpret_cast<EncSlot<int64_t> *>(table), capacity, sentinel_label);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int encode_insert_any(int key_bytes, const void *vocab, uint64_t n, int64_t first_label,
                      void *table, uint64_t capacity, int64_t *sentinel_label, hipStream_t s) {
  NVT_CHECK_ARG(key_bytes == 4, "encode_insert_any: int32 keys");
  NVT_CHECK_ARG(table && sentinel_label && (n == 0 || vocab), "null pointer");
  NVT_CHECK_ARG(first_label + (int64_t)n < INT32_MAX, "labels overflow int32");
  if (n == 0) return NVT_OK;
  NVT_PROF("encode_build", 0, s);
  enc_build_unique_i32_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(
      (const int32_t *)vocab, n, first_label, reinterpret_cast<EncSlot<int32_t> *>(table),
      capacity - 1, sentinel_label);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

// head images of ORDERED int32 vocabularies (n > NVT_ENCODE_RESIDENT_I32: the launches that encode
// with them run in cache mode), NVT_ENCODE_HEAD_BYTES bytes each: ONE launch, a workgroup per
// vocabulary.  Entries with a null image / too few keys are skipped.
int encode_head_build_many(const int32_t *const *vocab_keys, const uint64_t *n, const int64_t *first_label,
                           void *const *images, int count, hipStream_t s) {
  const uint64_t cap = (uint64_t)kHead16Keys;
  HeadJobs jobs;
  int m = 0;
  auto flush = [&]() -> int {
    if (m == 0) return NVT_OK;
    NVT_PROF("vocab_order", 0, s);
    enc_head_build_many_kernel<<<m, kEncBS, 0, s>>>(jobs);
    NVT_CHECK_LAUNCH();
    m = 0;
    return NVT_OK;
  };
  for (int i = 0; i < count; ++i) {
    if (images[i] == nullptr || vocab_keys[i] == nullptr || n[i] <= NVT_ENCODE_RESIDENT_I32) continue;
    jobs.j[m].keys = vocab_keys[i];
    jobs.j[m].image = (unsigned char *)images[i];
    jobs.j[m].first_label = first_label[i];
    jobs.j[m].n_hot = (uint32_t)(n[i] < cap ? n[i] : cap);
    if (++m == kHeadJobsMax) {
      int rc = flush();
      if (rc) return rc;
    }
  }
  return flush();
}
int encode_head_build(const int32_t *vocab_keys, uint64_t n, int64_t first_label, void *image,
                      hipStream_t s) {
  return encode_head_build_many(&vocab_keys, &n, &first_label, &image, 1, s);
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_encode_table_bytes(int key_bytes, uint64_t capacity, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes && (key_bytes == 4 || key_bytes == 8), "key_bytes must be 4 or 8");
  *bytes = capacity * (key_bytes == 4 ? sizeof(EncSlot<int32_t>) : sizeof(EncSlot<int64_t>));
  return NVT_OK;
}
int nvt_encode_build_i32(const int32_t *vocab_keys, uint64_t n_vocab, int64_t first_label,
                         void *table, uint64_t capacity, int64_t *sentinel_label, int unique_keys,
                         void *stream) {
  return build_launch<int32_t>(vocab_keys, n_vocab, first_label, table, capacity, sentinel_label,
                               unique_keys, (hipStream_t)stream);
}
int nvt_encode_build_i64(const int64_t *vocab_keys, uint64_t n_vocab, int64_t first_label,
                         void *table, uint64_t capacity, int64_t *sentinel_label, int unique_keys,
                         void *stream) {
  return build_launch<int64_t>(vocab_keys, n_vocab, first_label, table, capacity, sentinel_label,
                               unique_keys, (hipStream_t)stream);
}

}  // extern "C"
