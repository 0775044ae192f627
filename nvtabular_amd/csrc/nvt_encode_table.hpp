// What the encode units share (nvt_encode_build.hip, nvt_hash_bucket.hip, nvt_encode.hip with its
// kernel headers nvt_encode_head.hpp / nvt_encode_pipe.hpp): the {key, label} slot of the probe
// tables, the 16-byte non-temporal accesses of the row kernels, and the LDS head of the
// frequency-ordered vocabulary -- its two layouts and the one routine that builds either.
#pragma once
#include "nvt_common.hpp"

namespace nvt {

template <typename K>
struct EncSlot;
template <>
struct EncSlot<int32_t> {
  int32_t key;
  int32_t label;
};
template <>
struct EncSlot<int64_t> {
  int64_t key;
  int64_t label;
};
template <typename K>
struct EncTraits;
template <>
struct EncTraits<int32_t> {
  static constexpr int32_t empty = INT32_MIN;
  static constexpr int vec = 4;
  using cas_t = int;
};
template <>
struct EncTraits<int64_t> {
  static constexpr int64_t empty = INT64_MIN;
  static constexpr int vec = 2;
  using cas_t = unsigned long long;
};

// 16 bytes of a stream that is touched once, loaded / stored non-temporally
typedef int nvt_v4i __attribute__((ext_vector_type(4)));
template <typename V>
__device__ __forceinline__ V nt_load16(const V *p) {
  static_assert(sizeof(V) == 16, "16-byte vectors only");
  nvt_v4i r = __builtin_nontemporal_load(reinterpret_cast<const nvt_v4i *>(p));
  V v;
  memcpy(&v, &r, 16);
  return v;
}
template <typename V>
__device__ __forceinline__ void nt_store16(V v, V *p) {
  static_assert(sizeof(V) == 16, "16-byte vectors only");
  nvt_v4i r;
  memcpy(&r, &v, 16);
  __builtin_nontemporal_store(r, reinterpret_cast<nvt_v4i *>(p));
}

constexpr int kEncBS = 1024;   // threads of a workgroup that holds the 128-144 KiB head
template <typename K>
struct HotCfg;
template <>
struct HotCfg<int32_t> {
  static constexpr int slots = 16384;  // 128 KiB of {key,label} int32 pairs
};
template <>
struct HotCfg<int64_t> {
  static constexpr int slots = 8192;  // 128 KiB of {key,label} int64 pairs
};

// TWO (int32 keys, cache mode only): the staged head of the vocabulary lives in a 2-choice,
// 2-slots-per-bucket table instead of a linear-probing one.  A lookup is exactly two
// independent LDS bucket reads whatever the load (a MISS in the linear table walks ~2.5 slots
// at 25 % load and ~8.5 at 75 %, which is why that table is only filled to a quarter), so the
// table can be filled to 7/8.  A key that finds both buckets full is simply not cached (the
// global table holds every key).  The head's labels are frequency ranks -- first_label + the
// position of the key among the n_hot most frequent ones -- so a slot needs the key and a 16-bit
// rank, 6 bytes: {key0, key1} int2 per bucket + one word of two 16-bit ranks, 12288 buckets
// (144 KiB of the CU's 160): 21504 hot keys at 7/8 load against 4096 in the linear table.  Fewer
// rows miss the head, and a miss is what the cache mode pays for (one random 64-byte sector each;
// VERDICT r04 item 4).  Bucket index: 15 hash bits h, (3 h) >> 3; both indices from 24-bit
// multiplies of the same two words (nvt_common.hpp: mul24_hash).
constexpr int kHead16Buckets = 12288;
constexpr int kHead16Keys = kHead16Buckets * 2 / 8 * 7;   // 21504 < 65536
__device__ __forceinline__ void two_buckets16(int32_t key, uint32_t &b1, uint32_t &b2) {
  const uint32_t k = (uint32_t)key, lo = k ^ (k >> 7), hi = k >> 8;
  const uint32_t h1 = ((__umul24(hi, 0x5BD1E9u) + __umul24(lo, 0x9E3779u)) >> 17) & 0x7FFFu;
  const uint32_t h2 = ((__umul24(hi, 0x7FEB35u) + __umul24(lo, 0x846CA7u)) >> 17) & 0x7FFFu;
  b1 = (h1 + 2u * h1) >> 3;
  b2 = (h2 + 2u * h2) >> 3;
  b2 = b2 == b1 ? (b1 ^ 1u) : b2;   // (12288 is even: b ^ 1 stays in range)
}
// first slot of the linear-probing LDS table
template <int SLOTS, typename K>
__device__ __forceinline__ uint32_t lds_home(K key) {
  if constexpr (sizeof(K) == 4) {
    static_assert(SLOTS <= 16384, "14 index bits");
    return (mul24_hash((int32_t)key) >> 18) & (SLOTS - 1);
  } else {
    return (uint32_t)(slot_hash(key) >> 13) & (SLOTS - 1);
  }
}

// The LDS head of a launch: the first n_hot keys of the frequency-ordered vocabulary.  Every
// workgroup of an encode launch used to build it for itself (clear 128-144 KiB, read the keys,
// CAS them in: ~22 us in front of each of the 13 cache-mode launches of a Criteo step, 0.25-0.3 ms
// per step measured by returning right behind it); nvt_vocab_finalize_many now builds it ONCE per
// vocabulary into a global image (enc_head_build_kernel, on the stream that orders the vocabulary:
// off the critical path) and the launch's workgroups copy the image with coalesced loads.
template <typename K, bool TWO>
__device__ __forceinline__ void build_head(unsigned char *lraw, long long *s_sent_p,
                                           const K *__restrict__ hot_keys, uint32_t n_hot,
                                           int64_t first_label) {
  constexpr K EMPTY = EncTraits<K>::empty;
  constexpr int SLOTS = HotCfg<K>::slots;
  using L = decltype(EncSlot<K>::label);
  using C = typename EncTraits<K>::cas_t;
  EncSlot<K> *lt = reinterpret_cast<EncSlot<K> *>(lraw);
  int2 *tkeys = reinterpret_cast<int2 *>(lraw);
  uint32_t *tlab = reinterpret_cast<uint32_t *>(lraw + kHead16Buckets * 8);
  long long &s_sent = *s_sent_p;
  if constexpr (TWO) {
    for (int i = threadIdx.x; i < kHead16Buckets; i += kEncBS) {
      tkeys[i] = make_int2((int)EMPTY, (int)EMPTY);
      tlab[i] = 0u;
    }
  } else {
    for (int i = threadIdx.x; i < SLOTS; i += kEncBS) {
      lt[i].key = EMPTY;
      lt[i].label = 0;
    }
  }
  if (threadIdx.x == 0) s_sent = -1;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_hot; i += kEncBS) {
    K key = hot_keys[i];
    if (key == EMPTY) {
      s_sent = first_label + (long long)i;
      continue;
    }
    if constexpr (TWO) {
      uint32_t b1, b2;
      two_buckets16((int32_t)key, b1, b2);
      const uint32_t cand[4] = {2 * b1, 2 * b1 + 1, 2 * b2, 2 * b2 + 1};   // key words of the int2 array
      int *kw = reinterpret_cast<int *>(tkeys);
      unsigned short *lw = reinterpret_cast<unsigned short *>(tlab);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int prev = atomicCAS(&kw[cand[c]], (int)EMPTY, (int)key);
        if (prev == (int)EMPTY) {
          lw[cand[c]] = (unsigned short)i;   // rank: i < n_hot <= kHead16Keys < 2^16
          break;
        }
      }
      continue;  // all four slots taken: not cached
    }
    uint32_t s = lds_home<SLOTS>(key);
    while (true) {
      K prev = (K)atomicCAS(reinterpret_cast<C *>(&lt[s].key), (C)EMPTY, (C)key);
      if (prev == EMPTY || prev == key) {
        if (prev == EMPTY) lt[s].label = (L)(first_label + (int64_t)i);
        break;
      }
      s = (s + 1) & (SLOTS - 1);
    }
  }
  __syncthreads();
}

// bytes of the LDS head: 2-choice buckets of 6-byte slots, or the linear table of {key, label} slots
template <typename K, bool TWO>
constexpr int kHeadLdsBytes = TWO ? kHead16Buckets * 12 : HotCfg<K>::slots * (int)sizeof(EncSlot<K>);

}  // namespace nvt
