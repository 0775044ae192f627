// Dictionary pages of the PLAIN parquet writer: the distinct values of one column chunk in
// ascending order, and the chunk's values as bit-packed dictionary indices (RLE_DICTIONARY data
// pages of ONE bit-packed run each).  include/nvt_hip.h, "parquet dictionary pages", states the
// contract; DESIGN.md, "Dictionary pages in the PLAIN parquet writer", the reasons.
//
// nvt_pq_dict_build, on the caller's stream:
//   1. memset              state record 0, table keys "empty"
//   2. pd_insert_kernel    every value's key (the order-preserving image of nvt_seg_nunique: sign
//                          bit flipped) claims a slot of an open-addressing table in HBM with a
//                          64-bit CAS; the claims of a wave take their compact indices with ONE
//                          atomic.  More than max_entries claims (or a full table) set `overflow`,
//                          which every wave looks at before each tile.
//   3. pd_words_kernel +   the at most min(n, max_entries) claimed keys are ordered with the radix
//      sort_words_bits     sort of nvt_sort.hip: (low half << 32 | compact index), then for 64-bit
//                          keys (high half << 32 | compact index).  The sort's length is fixed on
//                          the host, so the entries past d are padding with all-ones halves: the
//                          sort is stable and they start behind the real entries, so they stay
//                          behind the one real key that can tie with them.
//   4. pd_rank_kernel      position j of the order: dictionary[j] = value, rank[slot] = j
// nvt_pq_dict_pack:
//   1. pd_pages_kernel     one wave: W from d, and per page the first output word and the first
//                          tile (prefix sums over the page table); checks the table and out_cap
//   2. pd_pack_kernel      a tile is kPdTile values of one page, i.e. 64 * W whole output words:
//                          the ranks are looked up into LDS, then every lane composes whole 32-bit
//                          words from the ranks that overlap them -- aligned, coalesced stores, no
//                          read-modify-write.  The last tile of a page also writes the page's zero
//                          padding up to its 16-byte boundary.
// The key that equals the table's empty marker (the image of INT64_MAX) has a slot of its own
// behind the table, claimed through state[2], as nvt_str_dedup does for its marker.
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"

namespace nvt {

constexpr unsigned long long kPdEmpty = ~0ull;
constexpr int kPdTile = 2048;                      // values per pack tile
constexpr uint64_t kPdMaxEntries = NVT_PQ_DICT_MAX_ENTRIES;

template <typename T>
__device__ __forceinline__ unsigned long long pd_image(T v);
template <>
__device__ __forceinline__ unsigned long long pd_image<int32_t>(int32_t v) {
  return (uint32_t)v ^ 0x80000000u;
}
template <>
__device__ __forceinline__ unsigned long long pd_image<int64_t>(int64_t v) {
  return (unsigned long long)v ^ 0x8000000000000000ull;
}
template <typename T>
__device__ __forceinline__ T pd_value(unsigned long long key);
template <>
__device__ __forceinline__ int32_t pd_value<int32_t>(unsigned long long key) {
  return (int32_t)((uint32_t)key ^ 0x80000000u);
}
template <>
__device__ __forceinline__ int64_t pd_value<int64_t>(unsigned long long key) {
  return (int64_t)(key ^ 0x8000000000000000ull);
}

// home slot: the top bits of a Fibonacci product (nslots = 2^(64 - shift))
__device__ __forceinline__ uint32_t pd_home(unsigned long long key, int shift) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift);
}

__host__ __device__ __forceinline__ int pd_width(uint64_t d) {
  int w = 1;
  while (w < 32 && (1ull << w) < d) ++w;
  return w;
}

// the table of a chunk of n values: nslots = 2 * next_pow2(min(n, max_entries)), at least 16
struct PdGeom {
  uint64_t cap;     // compact entries (and the length of the sort)
  uint64_t nslots;
  int shift;        // 64 - log2(nslots)
  uint64_t keys_at, rank_at, slot_of_at, words_at, sort_at, pages_at, bytes;
};
static PdGeom pd_geom(uint64_t n, uint64_t max_entries, uint64_t npages) {
  PdGeom g;
  g.cap = n < max_entries ? n : max_entries;
  if (g.cap < 1) g.cap = 1;
  int lg = 4;
  while ((1ull << lg) < 2 * g.cap) ++lg;
  g.nslots = 1ull << lg;
  g.shift = 64 - lg;
  uint64_t at = 0;
  g.keys_at = at;
  at += pad16((g.nslots + 1) * 8);
  g.rank_at = at;
  at += pad16((g.nslots + 1) * 4);
  g.slot_of_at = at;
  at += pad16(g.cap * 4);
  g.words_at = at;
  at += pad16(g.cap * 8);
  g.sort_at = at;
  at += pad16(sort_words_tmp_bytes(g.cap));
  g.pages_at = at;
  at += 2 * pad16((npages + 1) * 8);
  g.bytes = at;
  return g;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pd_insert_kernel(const T *__restrict__ x, uint64_t n,
                                                           uint64_t max_entries,
                                                           unsigned long long *keys,
                                                           uint32_t *__restrict__ slot_of,
                                                           uint32_t nslots, int shift,
                                                           unsigned long long *state) {
  const uint32_t mask = nslots - 1;
  const unsigned lane = lane_id();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += stride) {
    // (wave-uniform: the ballots below need whole waves)
    if (__any(__hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) return;
    const uint64_t i = base + threadIdx.x;
    bool active = i < n, claimed = false;
    unsigned long long key = 0;
    uint32_t slot = 0, steps = 0;
    if (active) {
      key = pd_image<T>(x[i]);
      if (key == kPdEmpty) {  // the marker's own slot, behind the table
        active = false;
        slot = nslots;
        claimed = atomicExch(&state[2], 1ull) == 0ull;
      } else {
        slot = pd_home(key, shift);
      }
    }
    while (__any(active)) {
      if (active) {
        unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kPdEmpty) {
          cur = atomicCAS(&keys[slot], kPdEmpty, key);
          if (cur == kPdEmpty) {
            claimed = true;
            cur = key;
          }
        }
        if (cur == key) {
          active = false;
        } else {
          slot = (slot + 1) & mask;
          if (++steps >= nslots) {  // a full table: only after more than max_entries claims
            active = false;
            atomicOr(&state[1], 1ull);
          }
        }
      }
    }
    const unsigned long long m = __ballot(claimed);
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      unsigned long long first = 0;
      if ((int)lane == leader) first = atomicAdd(&state[0], (unsigned long long)__popcll(m));
      first = __shfl(first, leader, 64);
      if (claimed) {
        const unsigned long long idx = first + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (idx < max_entries)
          slot_of[idx] = slot;
        else
          atomicOr(&state[1], 1ull);
      }
    }
  }
}

// the sort words of a refinement: (32-bit half of the key << 32 | compact index); `order` == nullptr:
// the first one, in compact order; else the next one, in the order so far
__global__ __launch_bounds__(kBlock) void pd_words_kernel(const uint64_t *order,
                                                          const unsigned long long *__restrict__ keys,
                                                          const uint32_t *__restrict__ slot_of,
                                                          const unsigned long long *__restrict__ state,
                                                          uint64_t cap, int half, uint64_t *words) {
  const uint64_t d = state[1] ? 0 : state[0];
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < cap; j += stride) {
    const uint64_t idx = order ? (order[j] & 0xFFFFFFFFull) : j;
    uint64_t h = 0xFFFFFFFFull;
    if (idx < d) h = (keys[slot_of[idx]] >> (32 * half)) & 0xFFFFFFFFull;
    words[j] = (h << 32) | idx;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pd_rank_kernel(const uint64_t *__restrict__ sorted,
                                                         const unsigned long long *__restrict__ keys,
                                                         const uint32_t *__restrict__ slot_of,
                                                         const unsigned long long *__restrict__ state,
                                                         uint64_t cap, uint32_t *__restrict__ rank,
                                                         T *__restrict__ dict) {
  const uint64_t d = state[1] ? 0 : state[0];
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < cap && j < d; j += stride) {
    const uint64_t idx = sorted[j] & 0xFFFFFFFFull;
    if (idx >= d) continue;  // (cannot be: the padding sorts behind the d entries)
    const uint32_t slot = slot_of[idx];
    rank[slot] = (uint32_t)j;
    dict[j] = pd_value<T>(keys[slot]);
  }
}

__device__ __forceinline__ unsigned long long pd_wave_incl(unsigned long long v) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long o = __shfl_up(v, off, 64);
    if (lane_id() >= (unsigned)off) v += o;
  }
  return v;
}

// one wave: word0[p] / tile0[p] = 32-bit output words / pack tiles in front of page p
__global__ __launch_bounds__(kWave) void pd_pages_kernel(const int64_t *__restrict__ page_start,
                                                         uint64_t npages, uint64_t n, uint64_t out_cap,
                                                         unsigned long long *state,
                                                         uint64_t *__restrict__ word0,
                                                         uint64_t *__restrict__ tile0) {
  const unsigned lane = lane_id();
  const uint64_t W = (uint64_t)pd_width(state[0]);
  unsigned long long carry_w = 0, carry_t = 0;
  bool bad = false;
  for (uint64_t base = 0; base < npages; base += kWave) {
    const uint64_t p = base + lane;
    unsigned long long qw = 0, tl = 0;
    if (p < npages) {
      const int64_t a = page_start[p], b = page_start[p + 1];
      if (a < 0 || b < a || (uint64_t)b > n) {
        bad = true;
      } else {
        const uint64_t nv = (uint64_t)(b - a);
        qw = (W * ((nv + 7) / 8) + 15) / 16 * 4;
        tl = (nv + kPdTile - 1) / kPdTile;
      }
    }
    const unsigned long long iw = pd_wave_incl(qw), it = pd_wave_incl(tl);
    if (p < npages) {
      word0[p] = carry_w + iw - qw;
      tile0[p] = carry_t + it - tl;
    }
    carry_w += __shfl(iw, 63, 64);
    carry_t += __shfl(it, 63, 64);
  }
  bad = __any(bad) || carry_w * 4 > out_cap;
  if (lane == 0) {
    word0[npages] = carry_w;
    tile0[npages] = carry_t;
    if (bad) atomicOr(&state[1], 2ull);  // a page table that is not one, or an output that is too small
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pd_pack_kernel(const T *__restrict__ x,
                                                         const int64_t *__restrict__ page_start,
                                                         uint64_t npages,
                                                         const unsigned long long *__restrict__ keys,
                                                         const uint32_t *__restrict__ rank,
                                                         uint32_t nslots, int shift,
                                                         const unsigned long long *__restrict__ state,
                                                         const uint64_t *__restrict__ word0,
                                                         const uint64_t *__restrict__ tile0,
                                                         uint32_t *__restrict__ out) {
  __shared__ uint32_t sr[kPdTile];
  if (state[1]) return;  // (overflow, or a bad page table: nothing is written)
  const uint32_t mask = nslots - 1;
  const int W = pd_width(state[0]);
  const uint64_t ntiles = tile0[npages];
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t lo = 0, hi = npages;  // the last page whose first tile is <= t: the one that holds t
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) / 2;
      if (tile0[mid] <= t) lo = mid; else hi = mid;
    }
    const uint64_t p = lo, tt = t - tile0[p];
    const uint64_t v0 = (uint64_t)page_start[p] + tt * kPdTile;
    const uint64_t left = (uint64_t)page_start[p + 1] - v0;
    const unsigned r = left < (uint64_t)kPdTile ? (unsigned)left : (unsigned)kPdTile;
    for (unsigned k = threadIdx.x; k < (unsigned)kPdTile; k += kBlock) {
      uint32_t rk = 0;
      if (k < r) {
        const unsigned long long key = pd_image<T>(x[v0 + k]);
        uint32_t slot = nslots;
        if (key != kPdEmpty) {
          slot = pd_home(key, shift);
          for (uint32_t steps = 0; keys[slot] != key && steps < nslots; ++steps) slot = (slot + 1) & mask;
        }
        rk = rank[slot];
      }
      sr[k] = rk;
    }
    __syncthreads();
    const uint64_t tile_w0 = tt * (uint64_t)(kPdTile / 32) * W;
    const uint64_t region = word0[p + 1] - word0[p] - tile_w0;   // words from the tile to the page's end
    const unsigned nw = region < (uint64_t)(kPdTile / 32) * W ? (unsigned)region : (unsigned)(kPdTile / 32) * W;
    uint32_t *dst = out + word0[p] + tile_w0;
    for (unsigned k = threadIdx.x; k < nw; k += kBlock) {
      const int bit0 = 32 * (int)k;
      int i = bit0 / W;
      int last = (bit0 + 31) / W;
      if (last > kPdTile - 1) last = kPdTile - 1;
      uint32_t w = 0;
      for (; i <= last; ++i) {
        const int sh = i * W - bit0;
        const uint32_t v = sr[i];
        w |= sh >= 0 ? (v << sh) : (v >> (-sh));
      }
      dst[k] = w;
    }
    __syncthreads();
  }
}

static int pd_itemsize(int dtype) { return dtype == NVT_I32 ? 4 : dtype == NVT_I64 ? 8 : 0; }

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_dict_ws_bytes(uint64_t n, uint64_t max_entries, uint64_t npages, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  NVT_CHECK_ARG(max_entries >= 1 && max_entries <= kPdMaxEntries, "max_entries must be 1..2^20");
  NVT_CHECK_ARG(n < (1ull << 31) && npages < (1ull << 31), "at most 2^31-1 values / pages");
  *bytes = pd_geom(n, max_entries, npages).bytes;
  return NVT_OK;
}

int nvt_pq_dict_build(const void *values, int dtype, uint64_t n, uint64_t max_entries, void *dict,
                      uint64_t *state, void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG(pd_itemsize(dtype), "dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(max_entries >= 1 && max_entries <= kPdMaxEntries, "max_entries must be 1..2^20");
  NVT_CHECK_ARG(n < (1ull << 31), "at most 2^31-1 values");
  NVT_CHECK_ARG(n == 0 || (values && dict && ws), "null pointer");
  const PdGeom g = pd_geom(n, max_entries, 0);
  NVT_CHECK_ARG(n == 0 || ws_bytes >= g.bytes, "workspace too small");
  NVT_CHECK_ARG(n == 0 || ((uintptr_t)ws % 16 == 0 && (uintptr_t)dict % 8 == 0), "ws 16-byte / dict 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_dict_build", n * (uint64_t)pd_itemsize(dtype), s);
  NVT_CHECK_HIP(hipMemsetAsync(state, 0, NVT_PQ_DICT_STATE_WORDS * 8, s));
  if (n == 0) return NVT_OK;
  char *p = reinterpret_cast<char *>(ws);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(p + g.keys_at);
  uint32_t *rank = reinterpret_cast<uint32_t *>(p + g.rank_at);
  uint32_t *slot_of = reinterpret_cast<uint32_t *>(p + g.slot_of_at);
  uint64_t *words = reinterpret_cast<uint64_t *>(p + g.words_at);
  void *sort_tmp = p + g.sort_at;
  unsigned long long *st = reinterpret_cast<unsigned long long *>(state);
  NVT_CHECK_HIP(hipMemsetAsync(keys, 0xFF, (g.nslots + 1) * 8, s));
  const unsigned grid = stream_grid(n, kBlock * 4);
  if (dtype == NVT_I32)
    pd_insert_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)values, n, max_entries, keys, slot_of, (uint32_t)g.nslots, g.shift, st);
  else
    pd_insert_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)values, n, max_entries, keys, slot_of, (uint32_t)g.nslots, g.shift, st);
  NVT_CHECK_LAUNCH();
  const unsigned cgrid = stream_grid(g.cap, kBlock * 4);
  uint64_t *sorted = nullptr;
  pd_words_kernel<<<cgrid, kBlock, 0, s>>>(nullptr, keys, slot_of, st, g.cap, 0, words);
  NVT_CHECK_LAUNCH();
  int rc = sort_words_bits(words, g.cap, 32, 64, sort_tmp, &sorted, s);
  if (rc) return rc;
  if (dtype == NVT_I64) {
    pd_words_kernel<<<cgrid, kBlock, 0, s>>>(sorted, keys, slot_of, st, g.cap, 1, words);
    NVT_CHECK_LAUNCH();
    rc = sort_words_bits(words, g.cap, 32, 64, sort_tmp, &sorted, s);
    if (rc) return rc;
  }
  if (dtype == NVT_I32)
    pd_rank_kernel<int32_t><<<cgrid, kBlock, 0, s>>>(sorted, keys, slot_of, st, g.cap, rank, (int32_t *)dict);
  else
    pd_rank_kernel<int64_t><<<cgrid, kBlock, 0, s>>>(sorted, keys, slot_of, st, g.cap, rank, (int64_t *)dict);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_pq_dict_pack(const void *values, int dtype, uint64_t n, uint64_t max_entries,
                     const int64_t *page_start, uint64_t npages, uint64_t *state, uint8_t *out,
                     uint64_t out_cap, void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG(pd_itemsize(dtype), "dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(max_entries >= 1 && max_entries <= kPdMaxEntries, "max_entries must be 1..2^20");
  NVT_CHECK_ARG(n < (1ull << 31) && npages < (1ull << 31), "at most 2^31-1 values / pages");
  if (n == 0 || npages == 0) return NVT_OK;  // (pages without values have no bytes)
  NVT_CHECK_ARG(values && page_start && out && ws, "null pointer");
  const PdGeom g = pd_geom(n, max_entries, npages);
  NVT_CHECK_ARG(ws_bytes >= g.bytes, "workspace too small");
  NVT_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)out % 16 == 0, "ws / out 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_dict_pack", n * (uint64_t)pd_itemsize(dtype), s);
  char *p = reinterpret_cast<char *>(ws);
  const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(p + g.keys_at);
  const uint32_t *rank = reinterpret_cast<const uint32_t *>(p + g.rank_at);
  uint64_t *word0 = reinterpret_cast<uint64_t *>(p + g.pages_at);
  uint64_t *tile0 = reinterpret_cast<uint64_t *>(p + g.pages_at + pad16((npages + 1) * 8));
  unsigned long long *st = reinterpret_cast<unsigned long long *>(state);
  pd_pages_kernel<<<1, kWave, 0, s>>>(page_start, npages, n, out_cap, st, word0, tile0);
  NVT_CHECK_LAUNCH();
  const unsigned grid = stream_grid(n / kPdTile + npages, 1);   // (an upper bound on the tiles)
  if (dtype == NVT_I32)
    pd_pack_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)values, page_start, npages, keys, rank, (uint32_t)g.nslots, g.shift, st, word0, tile0, reinterpret_cast<uint32_t *>(out));
  else
    pd_pack_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)values, page_start, npages, keys, rank, (uint32_t)g.nslots, g.shift, st, word0, tile0, reinterpret_cast<uint32_t *>(out));
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
