// Tile helpers of the list kernels (nvt_list.hip, nvt_loader.hip): rows and output leaves are
// walked in tiles of 2048, offsets are scanned 64 bits wide, the row of a leaf is a search in the
// new offsets.
#pragma once
#include "nvt_common.hpp"

namespace nvt {

constexpr uint64_t kListTile = 2048;        // rows (lengths) or output leaves (move) per tile
constexpr int kListStage = 2048 + 2;        // new offsets of one tile's rows held in LDS

__host__ __device__ inline uint64_t list_ntiles(uint64_t n) { return (n + kListTile - 1) / kListTile; }

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t u = __shfl_up(v, o, 64);
    if (lane_id() >= (unsigned)o) v += u;
  }
  return v;
}

// the row r in [lo, hi] with a[r] <= p < a[r + 1] (it exists: a[lo] <= p < a[hi + 1])
template <typename A>
__device__ __forceinline__ uint64_t row_of(const A a, uint64_t lo, uint64_t hi, int64_t p) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (a[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

}  // namespace nvt
