// String columns of the PLAIN parquet writer: the surrogates of a column chunk's non-null values
// become PLAIN BYTE_ARRAY pages (u32 length, little endian, then the bytes) on the device.
//
// The column's {surrogate -> string} dict travels to the device once as an entry table: keys
// (ascending) and the Arrow string buffers of the entries in key order (offsets int64[E + 1], chars
// padded to a 4-byte boundary: what nvt_str_hash / nvt_str_gather read).
//   1. entry_ids_kernel: one lane per value, binary search of its surrogate in the keys.
//   2. plan: the value at position j takes 4 + len(entry ids[j]) bytes.  plan_len_kernel scans the
//      sizes inside tiles of 2048 positions, 64 bits wide (a chunk may pass 4 GiB), scan_totals_kernel
//      (nvt_scan.hpp) scans the tile totals, plan_add_kernel adds the tile bases; plan_pages_kernel
//      reads pos at the page starts.
//   3. fill_kernel: kFillLanes lanes per value.  The value is the byte stream V = length | chars; a
//      lane takes one ALIGNED 4-byte word of the output and assembles the four bytes of V that fall
//      into it from two aligned words of the chars (v_alignbyte_b32), under the rule of
//      nvt_strings.hip: no word is loaded that holds no byte of the string.  A word that lies wholly
//      inside the value is stored whole; the first and the last word of a value are shared with its
//      neighbours and are stored byte by byte.  Destinations fall at every byte alignment, so do the
//      sources; a value of 100 000 bytes is a loop of the same lanes (correct, not fast).
#include "nvt_common.hpp"
#include "nvt_list_tile.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr uint64_t kPlanTile = kListTile;   // positions per tile of the size scan (256 lanes x 8)
constexpr int kFillLanes = 8;               // lanes per value: 32 output bytes per round

__global__ __launch_bounds__(kBlock) void entry_ids_kernel(const int64_t *__restrict__ keys, uint64_t E,
                                                           const int64_t *__restrict__ sur, uint64_t m,
                                                           int32_t *__restrict__ out, unsigned long long *bad) {
  unsigned long long miss = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
    const int64_t k = sur[j];
    uint64_t lo = 0, hi = E;   // first position with keys[pos] >= k
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (keys[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    const bool found = lo < E && keys[lo] == k;
    out[j] = found ? (int32_t)lo : 0;
    miss += !found;
  }
  for (int off = 32; off > 0; off >>= 1) miss += __shfl_down(miss, off, 64);
  if (lane_id() == 0 && miss) atomicAdd(bad, miss);
}

// bytes of entry `id` (0 for an id outside the table: never dereferenced)
__device__ __forceinline__ uint64_t entry_len(const int64_t *offsets, uint64_t E, int32_t id) {
  if ((uint64_t)(int64_t)id >= E) return 0;
  const int64_t b = offsets[id], e = offsets[(uint64_t)id + 1];
  return e > b ? (uint64_t)(e - b) : 0;
}

// pos[j] for j in [0, m]: tile-local exclusive prefix of the sizes; tile_tot[t] the tile's total
__global__ __launch_bounds__(kBlock) void plan_len_kernel(const int32_t *__restrict__ ids, uint64_t m,
                                                          const int64_t *__restrict__ offsets, uint64_t E,
                                                          uint64_t *__restrict__ pos,
                                                          unsigned long long *__restrict__ tile_tot) {
  __shared__ uint64_t wsum[kBlock / kWave];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  const uint64_t nt = list_ntiles(m + 1);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t j0 = t * kPlanTile + (uint64_t)threadIdx.x * 8;   // 8 consecutive positions per lane
    uint64_t len[8], tot = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      len[q] = j0 + q < m ? 4 + entry_len(offsets, E, ids[j0 + q]) : 0;
      tot += len[q];
    }
    const uint64_t inc = wave_incl_scan(tot);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t run = inc - tot;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (j0 + q <= m) pos[j0 + q] = run;
      run += len[q];
    }
    if (threadIdx.x == kBlock - 1) tile_tot[t] = run;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void plan_add_kernel(uint64_t *__restrict__ pos, uint64_t m,
                                                          const unsigned long long *__restrict__ tile_base) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= m; j += (uint64_t)gridDim.x * kBlock)
    pos[j] += tile_base[j / kPlanTile];
}

__global__ __launch_bounds__(kBlock) void plan_pages_kernel(const uint64_t *__restrict__ pos, uint64_t m,
                                                            const int64_t *__restrict__ page_start, uint64_t pages,
                                                            uint64_t *__restrict__ page_at) {
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p <= pages; p += (uint64_t)gridDim.x * kBlock) {
    const int64_t s = page_start[p];
    page_at[p] = pos[s < 0 ? 0 : ((uint64_t)s > m ? m : (uint64_t)s)];
  }
}

__global__ __launch_bounds__(kBlock) void fill_kernel(const int32_t *__restrict__ ids, uint64_t m,
                                                      const int64_t *__restrict__ offsets,
                                                      const uint8_t *__restrict__ chars, uint64_t E,
                                                      const uint64_t *__restrict__ pos, uint8_t *__restrict__ out,
                                                      uint64_t out_bytes) {
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kFillLanes);
  const uint32_t sub = threadIdx.x % kFillLanes;
  for (uint64_t j = (uint64_t)blockIdx.x * (kBlock / kFillLanes) + threadIdx.x / kFillLanes; j < m; j += groups) {
    const uint64_t dst = pos[j], end = pos[j + 1];
    const int32_t id = ids[j];
    const uint64_t L = entry_len(offsets, E, id);
    // a value that would end behind the buffer is not written; neither is one whose place is not
    // the 4 + L bytes the plan gives it
    if (end < dst || end > out_bytes || end - dst != 4 + L) continue;
    const uint8_t *p = chars + (L ? offsets[id] - offsets[0] : 0);
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p - sh);
    const int64_t nwords = L ? (int64_t)((sh + L + 3) >> 2) : 0;   // words holding a byte of the string
    const int64_t T = 4 + (int64_t)L;                               // bytes of V
    const uint64_t a0 = dst & ~3ull;
    for (uint64_t a = a0 + 4 * (uint64_t)sub; a < end; a += 4 * kFillLanes) {
      const int64_t r = (int64_t)a - (int64_t)dst;   // V[r .. r + 4) falls into this word (r >= -3)
      // chars bytes [r - 4, r) of the string start at byte sh + r - 4 of the aligned words
      const int64_t t = (int64_t)sh + r - 4;
      const int64_t qi = t >> 2;
      const uint32_t lo = (qi >= 0 && qi < nwords) ? w[qi] : 0u;
      const uint32_t hi = (qi + 1 >= 0 && qi + 1 < nwords) ? w[qi + 1] : 0u;
      const uint32_t val = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(t & 3));
      if (r >= 4 && r + 4 <= T) {
        *reinterpret_cast<uint32_t *>(out + a) = val;
        continue;
      }
      uint32_t word = 0, have = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t x = r + i;
        if (x < 0 || x >= T) continue;
        const uint32_t b = x < 4 ? (uint32_t)(L >> (8 * x)) & 0xFFu : (val >> (8 * i)) & 0xFFu;
        word |= b << (8 * i);
        have |= 1u << i;
      }
      if (have == 0xFu) {
        *reinterpret_cast<uint32_t *>(out + a) = word;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (have & (1u << i)) out[a + i] = (uint8_t)(word >> (8 * i));
      }
    }
  }
}

inline uint64_t plan_ws_bytes(uint64_t m) { return pad16(list_ntiles(m + 1) * 8) + 16; }

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_str_entry_ids(const int64_t *keys, uint64_t n_entries, const int64_t *surrogates, uint64_t m,
                         int32_t *out_ids, uint64_t *bad, void *stream) {
  NVT_CHECK_ARG(n_entries < (1ull << 31), "2^31 entries or more");
  if (m == 0) return NVT_OK;
  NVT_CHECK_ARG(surrogates && out_ids && bad && (keys || n_entries == 0), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_str_entry_ids", m * 12, s);
  entry_ids_kernel<<<stream_grid(m, kBlock * 4), kBlock, 0, s>>>(keys, n_entries, surrogates, m, out_ids,
                                                                 (unsigned long long *)bad);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_pq_byte_array_ws_bytes(uint64_t m, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null pointer");
  *bytes = plan_ws_bytes(m);
  return NVT_OK;
}

int nvt_pq_byte_array_plan(const int32_t *ids, uint64_t m, const int64_t *offsets, uint64_t n_entries,
                           const int64_t *page_start, uint64_t pages, uint64_t *pos, uint64_t *page_at, void *ws,
                           uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(n_entries < (1ull << 31), "2^31 entries or more");
  if (m == 0) return NVT_OK;
  NVT_CHECK_ARG(ids && offsets && pos && ws, "null pointer");
  NVT_CHECK_ARG(pages == 0 || (page_start && page_at), "null page table");
  NVT_CHECK_ARG(ws_bytes >= plan_ws_bytes(m), "workspace smaller than nvt_pq_byte_array_ws_bytes");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(pos) & 7) == 0,
                "ws / pos must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_byte_array_plan", m * 28, s);
  auto *tot = static_cast<unsigned long long *>(ws);
  const uint64_t nt = list_ntiles(m + 1);
  plan_len_kernel<<<stream_grid(nt, 1), kBlock, 0, s>>>(ids, m, offsets, n_entries, pos, tot);
  NVT_CHECK_LAUNCH();
  scan_totals_kernel<<<1, kBlock, 0, s>>>(tot, nt);
  NVT_CHECK_LAUNCH();
  plan_add_kernel<<<stream_grid(m + 1, kBlock * 4), kBlock, 0, s>>>(pos, m, tot);
  NVT_CHECK_LAUNCH();
  if (pages) {
    plan_pages_kernel<<<stream_grid(pages + 1, kBlock), kBlock, 0, s>>>(pos, m, page_start, pages, page_at);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_pq_byte_array_fill(const int32_t *ids, uint64_t m, const int64_t *offsets, const uint8_t *chars,
                           uint64_t n_entries, const uint64_t *pos, uint8_t *out, uint64_t out_bytes,
                           void *stream) {
  NVT_CHECK_ARG(n_entries < (1ull << 31), "2^31 entries or more");
  if (m == 0) return NVT_OK;
  NVT_CHECK_ARG(ids && offsets && chars && pos && out, "null pointer");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(chars) & 3) == 0, "chars must be 4-byte aligned");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "out must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_byte_array_fill", m * 28 + out_bytes, s);
  fill_kernel<<<stream_grid(m, kBlock / kFillLanes * 4), kBlock, 0, s>>>(ids, m, offsets, chars, n_entries, pos,
                                                                         out, out_bytes);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
