// What the counting units share on the device: the workgroup-private LDS hash table of
// nvt_count_lds.hip (paths 0 / 6 / 7) and nvt_count_part.hip (paths 1 / 2 / 3), and the geometry
// of the read-only hot-key table that nvt_hot_sample.hip fills and nvt_count_part.hip reads.
// The library is built without relocatable device code, so every device function here is
// __forceinline__.
#pragma once
#include "nvt_common.hpp"

namespace nvt {

template <typename K>
struct DKey;
template <>
struct DKey<int32_t> {
  static constexpr int32_t empty = INT32_MIN;
  static constexpr int vec = 4;
  using cas_t = int;
};
template <>
struct DKey<int64_t> {
  static constexpr int64_t empty = INT64_MIN;
  static constexpr int vec = 2;
  using cas_t = unsigned long long;
};

// state words (uint64) written by these kernels
constexpr int DS_NULLS = NVT_ST_NULLS, DS_SENT = NVT_ST_SENTINEL, DS_OUT = NVT_ST_OCCUPIED,
              DS_OVF = NVT_ST_OVERFLOW, DS_ROWS = NVT_ST_ROWS;

constexpr int kLdsSlots = 8192;     // weighted stages / per-bucket tables (u64 or u32 counts)
constexpr int kLdsSlotsBig = 16384; // unweighted path S: int32 key + u32 count = 128 KiB, 1 WG / CU
constexpr int kLdsProbe = 512;  // linear-probing clusters reach ~25 slots at 37 % load; the real
                                // "table full" signal is lfill > max_fill, not the chain length

__host__ __device__ constexpr int max_fill(int slots) { return slots / 4 * 3; }

template <typename K>
__device__ __forceinline__ K lds_cas(K *addr, K expect, K val) {
  using C = typename DKey<K>::cas_t;
  return (K)atomicCAS(reinterpret_cast<C *>(addr), (C)expect, (C)val);
}

// (A wave-level "aggregate the lanes that share the first lane's key" pre-pass was tried to
// relieve same-address LDS atomics on hot keys; it cost more issue slots than it saved on
// every cardinality measured, see profiles/r01_notes.md.)
// Insert into a workgroup-private LDS table.  Returns false when no slot was found.
// `h` must be independent of whatever selected the rows that reach this table: path S
// uses the upper bits of slot_hash, path P the LOW bits of part_hash (its top bits chose
// the bucket; reusing slot_hash there clustered and overflowed 24-probe chains at 37 % load).
template <typename K, typename C, int SLOTS = kLdsSlots>
__device__ __forceinline__ bool lds_add(K *lkeys, C *lcnt, unsigned *lfill, K key, C w,
                                        uint32_t h) {
  constexpr K EMPTY = DKey<K>::empty;
#ifndef NVT_PROBE_UNROLL
#define NVT_PROBE_UNROLL 4
#endif
#pragma unroll NVT_PROBE_UNROLL
  for (int p = 0; p < kLdsProbe; ++p) {
    uint32_t s = (h + p) & (SLOTS - 1);
    K cur = lkeys[s];
    if (cur == EMPTY) {
      cur = lds_cas<K>(&lkeys[s], EMPTY, key);
      if (cur == EMPTY) {
        cur = key;
        atomicAdd(lfill, 1u);
      }
    }
    if (cur == key) {
      atomicAdd(&lcnt[s], w);
      return true;
    }
  }
  return false;
}

// Append the occupied LDS slots to (out_keys, out_cnt) at a range reserved with one
// atomic on *cursor.  All threads of the block must call this.
template <typename K, typename C, int BS, int SLOTS = kLdsSlots>
__device__ __forceinline__ void lds_flush(const K *lkeys, const C *lcnt, K *out_keys,
                                          int64_t *out_cnt, uint64_t out_cap,
                                          unsigned long long *cursor, uint64_t *state) {
  constexpr K EMPTY = DKey<K>::empty;
  __shared__ unsigned wsum[BS / kWave];
  __shared__ unsigned long long base_s;
  constexpr int PER = SLOTS / BS;
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  unsigned mine = 0;
  const int first = threadIdx.x * PER;
#pragma unroll 8
  for (int j = 0; j < PER; ++j) mine += (lkeys[first + j] != EMPTY);
  unsigned inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned o = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += o;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned wbase = 0, total = 0;
  for (unsigned i = 0; i < BS / kWave; ++i) {
    if (i < w) wbase += wsum[i];
    total += wsum[i];
  }
  if (threadIdx.x == 0) base_s = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
  __syncthreads();
  uint64_t pos = base_s + wbase + inc - mine;
  if (base_s + total > out_cap) {
    if (threadIdx.x == 0) atomicOr((unsigned long long *)&state[DS_OVF], 2ull);
    return;
  }
  unsigned long long mx = 0;
#pragma unroll 8
  for (int j = 0; j < PER; ++j) {
    K k = lkeys[first + j];
    if (k != EMPTY) {
      unsigned long long c = (unsigned long long)lcnt[first + j];
      out_keys[pos] = k;
      out_cnt[pos] = (int64_t)c;
      mx = c > mx ? c : mx;
      ++pos;
    }
  }
  // final list only: largest count, so the host can size the vocabulary sort without a
  // second round trip (one relaxed read, an atomic only when this block raises the max)
  if (cursor == reinterpret_cast<unsigned long long *>(&state[DS_OUT])) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      unsigned long long o = __shfl_down(mx, off, 64);
      mx = o > mx ? o : mx;
    }
    if (lane == 0 && mx > 0) {
      unsigned long long *gm = reinterpret_cast<unsigned long long *>(&state[NVT_ST_MAXCOUNT]);
      if (mx > __hip_atomic_load(gm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(gm, mx);
    }
  }
}

// Same, but into a caller-assigned region (no cursor): used for the per-chunk partial lists
// of split (skewed) buckets and for P3's atomic-free staging of its results.  *out_len
// receives the entry count; with `state` the largest count is folded into
// state[NVT_ST_MAXCOUNT].
template <typename K, typename C, int BS, int SLOTS = kLdsSlots>
__device__ __forceinline__ void lds_flush_region(const K *lkeys, const C *lcnt, K *out_keys,
                                                 int64_t *out_cnt, unsigned *out_len,
                                                 uint64_t *state = nullptr) {
  constexpr K EMPTY = DKey<K>::empty;
  __shared__ unsigned wsum2[BS / kWave];
  constexpr int PER = SLOTS / BS;
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  unsigned mine = 0;
  const int first = threadIdx.x * PER;
#pragma unroll 8
  for (int j = 0; j < PER; ++j) mine += (lkeys[first + j] != EMPTY);
  unsigned inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned o = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += o;
  }
  if (lane == 63) wsum2[w] = inc;
  __syncthreads();
  unsigned wbase = 0, total = 0;
  for (unsigned i = 0; i < BS / kWave; ++i) {
    if (i < w) wbase += wsum2[i];
    total += wsum2[i];
  }
  if (threadIdx.x == 0) *out_len = total;
  unsigned pos = wbase + inc - mine;
  unsigned long long mx = 0;
#pragma unroll 8
  for (int j = 0; j < PER; ++j) {
    K k = lkeys[first + j];
    if (k != EMPTY) {
      unsigned long long c = (unsigned long long)lcnt[first + j];
      out_keys[pos] = k;
      out_cnt[pos] = (int64_t)c;
      mx = c > mx ? c : mx;
      ++pos;
    }
  }
  if (state != nullptr) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      unsigned long long o = __shfl_down(mx, off, 64);
      mx = o > mx ? o : mx;
    }
    if (lane == 0 && mx > 0) {
      unsigned long long *gm = reinterpret_cast<unsigned long long *>(&state[NVT_ST_MAXCOUNT]);
      if (mx > __hip_atomic_load(gm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(gm, mx);
    }
  }
}

// workgroup size of the kernels that own one 96-128 KiB table per CU (lds_stage_kernel,
// part_merge_kernel)
constexpr int kStageBS = 1024;  // 16 waves

// ---- the hot-key table (hot filter of paths 1 / 2 / 3, hot image of the range path) -------------
// The table: buckets of NVT_HOT_WIDTH slots, ONE candidate bucket per key, so a lookup is one
// 8- or 16-byte LDS read.  A key whose bucket is full is simply not hot (2 choices x 2 slots
// kept ~8 % more keys and cost a second read per row: 2.37 vs 2.22 ms for the nine filtered
// path-1 columns).
#ifndef NVT_HOT_WIDTH
#define NVT_HOT_WIDTH 2
#endif
constexpr int kHotSlots = NVT_HOT_IMAGE_WORDS;  // 32 KiB of keys + 32 KiB of counters
constexpr int kHotWidth = NVT_HOT_WIDTH;
constexpr int kHotBuckets = kHotSlots / kHotWidth;
__device__ __forceinline__ uint32_t hot_bucket(int32_t key) { return hot_image_bucket(key, kHotBuckets - 1); }

}  // namespace nvt
