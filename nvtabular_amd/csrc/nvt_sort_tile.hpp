// What the radix sorts (nvt_sort.hip) and the vocabulary ordering (nvt_vocab_order.hip) share: the
// packed (count, key) word, the 4096-entry tile and its element order, the ballot ranking of equal
// digits and the status words of the decoupled look-back.
#pragma once
#include "nvt_common.hpp"

namespace nvt {

// peers = lanes of this wave holding the same digit (inactive lanes excluded)
__device__ __forceinline__ unsigned long long match_digit(unsigned digit, bool active) {
  unsigned long long peers = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    unsigned long long m = __ballot((digit >> b) & 1);
    peers &= ((digit >> b) & 1) ? m : ~m;
  }
  return peers;
}

//   comp = (~count32 << 32) | (key ^ 0x80000000)     ascending comp == (count desc, key asc)
constexpr int kS2BS = 256, kS2Rows = 16, kS2Tile = kS2BS * kS2Rows;  // 4096 entries

__device__ __forceinline__ uint64_t comp_make(int32_t key, int64_t cnt) {
  return ((uint64_t)(~(uint32_t)cnt) << 32) | (uint64_t)((uint32_t)key ^ 0x80000000u);
}
__device__ __forceinline__ int32_t comp_key(uint64_t c) { return (int32_t)((uint32_t)c ^ 0x80000000u); }
__device__ __forceinline__ int64_t comp_cnt(uint64_t c) { return (int64_t)(uint32_t)~(uint32_t)(c >> 32); }

// element (wave w, row r, lane l) of a tile: waves own contiguous 1024-element runs (stability)
__device__ __forceinline__ uint64_t s2_elem(uint64_t tile, unsigned w, unsigned r, unsigned l) {
  return tile * kS2Tile + (uint64_t)w * (kS2Rows * kWave) + (uint64_t)r * kWave + l;
}

// decoupled look-back: a status word is flag (2 bits) + count (30 bits)
constexpr unsigned kOsAgg = 1u << 30, kOsPrefix = 2u << 30, kOsMask = (1u << 30) - 1u;

}  // namespace nvt
