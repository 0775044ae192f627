// Vocabulary order: (count descending, key ascending) -- the two sort_values calls of
// categorify.py:1300,1316 with the deterministic tie rule.
//
//  * n <= 8192: one workgroup, bitonic network in LDS over the composite
//    (inverted count, key) -- most Criteo vocabularies are this small and a
//    multi-pass radix sort would be pure launch latency.
//  * larger: LSD radix sort, 8-bit digits over (key bytes, then inverted-count bytes);
//    passes whose digit is constant over the whole array are skipped (the high count
//    bytes almost always are).  Per pass: tile histogram -> scan -> stable scatter.
//    A tile is 2048 elements = 4 waves x 8 rows x 64 lanes; stability inside a tile
//    comes from ballot-matching equal digits in lane order (rank within a row), a
//    per-wave running digit counter in LDS (rows), and a 4-entry prefix over the waves.
#include <type_traits>

#include <cstdlib>

#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"
#include "nvt_sort_tile.hpp"

namespace nvt {

template <typename K>
__device__ __forceinline__ unsigned sort_digit(K key, int64_t cnt, int pass) {
  constexpr int KB = (int)sizeof(K);
  if (pass < KB) {
    using U = typename std::make_unsigned<K>::type;
    U u = (U)key ^ ((U)1 << (8 * KB - 1));  // signed order
    return (unsigned)((u >> (8 * pass)) & 0xFF);
  }
  uint64_t inv = ~(uint64_t)cnt;  // descending counts
  return (unsigned)((inv >> (8 * (pass - KB))) & 0xFF);
}

// ---- small: single-workgroup bitonic sort -------------------------------------
constexpr int kSmallMax = 8192;
constexpr int kSmallBS = 1024;

template <typename K>
__device__ __forceinline__ bool vocab_before(int64_t ca, K ka, int64_t cb, K kb) {
  return ca > cb || (ca == cb && ka < kb);
}

template <typename K>
__global__ __launch_bounds__(kSmallBS) void sort_small_kernel(K *keys, int64_t *counts, unsigned n) {
  __shared__ K sk[kSmallMax];
  __shared__ int64_t sc[kSmallMax];
  unsigned m = 1;
  while (m < n) m <<= 1;
  for (unsigned i = threadIdx.x; i < m; i += kSmallBS) {
    if (i < n) {
      sk[i] = keys[i];
      sc[i] = counts[i];
    } else {  // padding sorts last: count = INT64_MIN
      sk[i] = std::numeric_limits<K>::max();
      sc[i] = INT64_MIN;
    }
  }
  __syncthreads();
  for (unsigned size = 2; size <= m; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      for (unsigned t = threadIdx.x; t < m / 2; t += kSmallBS) {
        unsigned lo = 2 * t - (t & (stride - 1));
        unsigned hi = lo + stride;
        bool up = (lo & size) == 0;
        K ka = sk[lo], kb = sk[hi];
        int64_t ca = sc[lo], cb = sc[hi];
        bool swap = up ? vocab_before<K>(cb, kb, ca, ka) : vocab_before<K>(ca, ka, cb, kb);
        if (swap) {
          sk[lo] = kb;
          sk[hi] = ka;
          sc[lo] = cb;
          sc[hi] = ca;
        }
      }
      __syncthreads();
    }
  }
  for (unsigned i = threadIdx.x; i < n; i += kSmallBS) {
    keys[i] = sk[i];
    counts[i] = sc[i];
  }
}

// ---- large: LSD radix ------------------------------------------------------------
constexpr int kRows = 8;
constexpr int kTileSort = kBlock * kRows;  // 2048 elements

template <typename K>
__global__ __launch_bounds__(kBlock) void sort_pass_hist_kernel(const K *__restrict__ keys,
                                                                const int64_t *__restrict__ cnts,
                                                                uint64_t n,
                                                                unsigned long long *pass_hist) {
  constexpr int NP = (int)sizeof(K) + 8;
  __shared__ unsigned h[NP * 256];
  for (int i = threadIdx.x; i < NP * 256; i += kBlock) h[i] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    K k = keys[i];
    int64_t c = cnts[i];
#pragma unroll
    for (int p = 0; p < NP; ++p) atomicAdd(&h[p * 256 + sort_digit<K>(k, c, p)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NP * 256; i += kBlock)
    if (h[i]) atomicAdd(&pass_hist[i], (unsigned long long)h[i]);
}

// element index of (wave w, row r, lane l) inside a tile: waves own contiguous 512-element runs
__device__ __forceinline__ uint64_t tile_elem(uint64_t tile, unsigned w, unsigned r, unsigned l) {
  return tile * kTileSort + (uint64_t)w * (kRows * kWave) + (uint64_t)r * kWave + l;
}

template <typename K>
__global__ __launch_bounds__(kBlock) void sort_tile_hist_kernel(const K *__restrict__ keys,
                                                                const int64_t *__restrict__ cnts,
                                                                uint64_t n, int pass,
                                                                unsigned *tile_hist,
                                                                uint64_t ntiles) {
  constexpr int KB = (int)sizeof(K);
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned w = threadIdx.x / kWave, l = lane_id();
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    uint64_t i = tile_elem(blockIdx.x, w, r, l);
    if (i < n) {
      // only the array that holds this pass's digit is read
      unsigned d = pass < KB ? sort_digit<K>(keys[i], 0, pass) : sort_digit<K>((K)0, cnts[i], pass);
      atomicAdd(&h[d], 1u);
    }
  }
  __syncthreads();
  tile_hist[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

template <typename K>
__global__ __launch_bounds__(kBlock) void sort_scatter_kernel(
    const K *__restrict__ keys, const int64_t *__restrict__ cnts, uint64_t n, int pass,
    const unsigned *__restrict__ tile_off, uint64_t ntiles, K *out_keys, int64_t *out_cnts) {
  __shared__ unsigned wcnt[kBlock / kWave][256];
  const unsigned w = threadIdx.x / kWave, l = lane_id();
  for (int i = threadIdx.x; i < (kBlock / kWave) * 256; i += kBlock) (&wcnt[0][0])[i] = 0;
  __syncthreads();
  K k[kRows];
  int64_t c[kRows];
  unsigned dig[kRows], local[kRows];
  bool act[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    uint64_t i = tile_elem(blockIdx.x, w, r, l);
    act[r] = i < n;
    k[r] = act[r] ? keys[i] : (K)0;
    c[r] = act[r] ? cnts[i] : 0;
    dig[r] = sort_digit<K>(k[r], c[r], pass);
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    unsigned long long peers = match_digit(dig[r], act[r]);
    unsigned rank = __popcll(peers & ((1ull << l) - 1ull));
    unsigned before = act[r] ? wcnt[w][dig[r]] : 0;  // digits seen in earlier rows of this wave
    __builtin_amdgcn_wave_barrier();
    if (act[r] && rank == 0) wcnt[w][dig[r]] = before + (unsigned)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    local[r] = before + rank;
  }
  __syncthreads();
  {  // per digit: exclusive prefix over the 4 waves, seeded with the tile's global offset
    const unsigned d = threadIdx.x;
    unsigned run = tile_off[(uint64_t)d * ntiles + blockIdx.x];
#pragma unroll
    for (int q = 0; q < kBlock / kWave; ++q) {
      unsigned t = wcnt[q][d];
      wcnt[q][d] = run;
      run += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    if (act[r]) {
      unsigned dst = wcnt[w][dig[r]] + local[r];
      out_keys[dst] = k[r];
      out_cnts[dst] = c[r];
    }
  }
}

// ---- int32 keys with a known max count: LSD radix over ONE packed 64-bit word -------------
//   comp = (~count32 << 32) | (key ^ 0x80000000)     ascending comp == (count desc, key asc)
// (counts fit 32 bits: n rows < 2^32).  Against the generic path above this moves 8 B per
// entry instead of 12, uses 4096-entry tiles (a quarter of the per-tile histograms to scan)
// and -- the main point -- stages every tile through LDS in sorted order, so each digit's
// run leaves the tile as ONE coalesced burst: with 256 digits a 2048-entry tile wrote
// 8-entry (32 / 64 B) runs straight from registers and the key passes ran at a third of
// the speed of the (nearly sequential) count passes.
// The first pass reads (keys, counts) and packs; the last unpacks into (keys, counts).

template <bool FIRST>
__global__ __launch_bounds__(kS2BS) void sort2_hist_kernel(const uint64_t *__restrict__ comp,
                                                           const int32_t *__restrict__ keys,
                                                           const int64_t *__restrict__ cnts,
                                                           uint64_t n, int shift,
                                                           unsigned *tile_hist, uint64_t ntiles) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kS2Tile;
#pragma unroll 4
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = base + (uint64_t)r * kS2BS + threadIdx.x;  // any order: only counts matter
    const bool act = i < n;
    uint64_t c = 0;
    if (act) c = FIRST ? comp_make(keys[i], cnts[i]) : comp[i];
    const unsigned d = (unsigned)(c >> shift) & 0xFF;
    if (shift < 32) {
      if (act) atomicAdd(&h[d], 1u);  // key bytes: digits spread over 256 bins
    } else {
      // count passes see one or two digit values: aggregate equal digits per wave first
      const unsigned long long peers = match_digit(d, act);
      if (act && (peers & ((1ull << lane_id()) - 1ull)) == 0)
        atomicAdd(&h[d], (unsigned)__popcll(peers));
    }
  }
  __syncthreads();
  tile_hist[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kS2BS) void sort2_scatter_kernel(
    const uint64_t *__restrict__ comp, const int32_t *__restrict__ keys,
    const int64_t *__restrict__ cnts, uint64_t n, int shift, const unsigned *__restrict__ tile_off,
    const unsigned long long *__restrict__ chunk_base, uint64_t ntiles, uint64_t *out_comp,
    int32_t *out_keys, int64_t *out_cnts) {
  constexpr int NW = kS2BS / kWave;
  __shared__ unsigned wcnt[NW][256];
  __shared__ unsigned goff[256];
  __shared__ unsigned wtot[NW];
  __shared__ uint64_t stage[kS2Tile];
  const unsigned w = threadIdx.x / kWave, l = lane_id();
#pragma unroll
  for (int q = 0; q < NW; ++q) wcnt[q][threadIdx.x] = 0;
  __syncthreads();
  uint64_t c[kS2Rows];
  unsigned short local[kS2Rows];
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = s2_elem(blockIdx.x, w, r, l);
    c[r] = ~0ull;
    if (i < n) c[r] = FIRST ? comp_make(keys[i], cnts[i]) : comp[i];
  }
  const uint64_t tile_base = (uint64_t)blockIdx.x * kS2Tile;
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const bool act = s2_elem(blockIdx.x, w, r, l) < n;
    const unsigned d = (unsigned)(c[r] >> shift) & 0xFF;
    const unsigned long long peers = match_digit(d, act);
    const unsigned rank = __popcll(peers & ((1ull << l) - 1ull));
    const unsigned before = act ? wcnt[w][d] : 0;  // equal digits in earlier rows of this wave
    __builtin_amdgcn_wave_barrier();
    if (act && rank == 0) wcnt[w][d] = before + (unsigned)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    local[r] = (unsigned short)(before + rank);
  }
  __syncthreads();
  {  // thread d: tile-local start of digit d (block exclusive scan) + per-wave bases
    const unsigned d = threadIdx.x;
    unsigned t[NW], tot = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      t[q] = wcnt[q][d];
      tot += t[q];
    }
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o = __shfl_up(inc, off, 64);
      if (l >= (unsigned)off) inc += o;
    }
    if (l == 63) wtot[w] = inc;
    __syncthreads();
    unsigned wbase = 0;
    for (unsigned q = 0; q < w; ++q) wbase += wtot[q];
    const unsigned dstart = wbase + inc - tot;
    unsigned run = dstart;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      wcnt[q][d] = run;
      run += t[q];
    }
    goff[d] = scan_lookup(tile_off, chunk_base, (uint64_t)d * ntiles + blockIdx.x) - dstart;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    if (s2_elem(blockIdx.x, w, r, l) < n) {
      const unsigned d = (unsigned)(c[r] >> shift) & 0xFF;
      stage[wcnt[w][d] + local[r]] = c[r];
    }
  }
  __syncthreads();
  const unsigned tile_n = (unsigned)(n - tile_base < (uint64_t)kS2Tile ? n - tile_base : kS2Tile);
#pragma unroll 4
  for (int j = 0; j < kS2Rows; ++j) {
    const unsigned idx = j * kS2BS + threadIdx.x;
    if (idx < tile_n) {
      const uint64_t v = stage[idx];
      const unsigned d = (unsigned)(v >> shift) & 0xFF;
      const unsigned dst = goff[d] + idx;
      if (LAST) {
        out_keys[dst] = comp_key(v);
        out_cnts[dst] = comp_cnt(v);
      } else {
        out_comp[dst] = v;
      }
    }
  }
}

// ---- int32 keys, packed words, ONESWEEP: one histogram read + one scatter launch per pass ---
// The three-launch passes above (tile histogram -> device scan -> scatter) cost ~21-28 launches
// and two extra reads of the array per sort; Criteo's 26 vocabularies spent more time in the
// 7-17 us hist / scan kernels than in the scatters (profiles/r01_final_kernel_stats.csv).  Here:
//   os_hist_kernel    ONE read of (keys, counts): the digit histograms of EVERY pass
//   os_base_kernel    per pass: bucket totals -> exclusive scan = global digit bases
//   os_scatter_kernel per pass: tile ranks as in sort2_scatter_kernel; the tile's offset inside
//                     each digit bucket comes from a decoupled look-back over the preceding
//                     tiles' published (aggregate | inclusive prefix) words instead of a scanned
//                     per-tile histogram.  Tile ids are handed out by an atomic ticket, so a tile
//                     only ever waits for tiles that are already running (no deadlock whatever
//                     the dispatch order).  A status word is flag (2 bits) + count (30 bits):
//                     the data IS the flag (one relaxed agent-scope 4-byte store / load, the
//                     "R2 granule" form of cdna_hip_programming.md G16), so no fences are needed.
constexpr int kOsMaxPass = 8;
constexpr int kOsHistBlocks = 1024;  // 4 per CU: 256 left 4 waves per CU waiting for their loads

__global__ __launch_bounds__(kS2BS) void os_hist_kernel(const int32_t *__restrict__ keys,
                                                        const int64_t *__restrict__ cnts,
                                                        uint64_t n, int npass,
                                                        unsigned *__restrict__ block_hist) {
  __shared__ unsigned h[kOsMaxPass * 256];
  for (int i = threadIdx.x; i < npass * 256; i += kS2BS) h[i] = 0;
  __syncthreads();
  const unsigned l = lane_id();
  unsigned c255[kOsMaxPass];  // digit 0xFF of the upper count bytes (nearly every entry) in registers
#pragma unroll
  for (int p = 0; p < kOsMaxPass; ++p) c255[p] = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kS2BS;
  const uint64_t iters = (n + stride - 1) / stride;
  for (uint64_t it = 0; it < iters; ++it) {
    const uint64_t i = it * stride + (uint64_t)blockIdx.x * kS2BS + threadIdx.x;
    const bool act = i < n;
    const uint64_t c = act ? comp_make(keys[i], cnts[i]) : 0ull;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (act) atomicAdd(&h[p * 256 + ((unsigned)(c >> (8 * p)) & 0xFF)], 1u);
    if (npass > 4) {  // lowest count byte: a few hot digits -> aggregate equal digits per wave
      const unsigned d = (unsigned)(c >> 32) & 0xFF;
      const unsigned long long peers = match_digit(d, act);
      if (act && (peers & ((1ull << l) - 1ull)) == 0)
        atomicAdd(&h[4 * 256 + d], (unsigned)__popcll(peers));
    }
#pragma unroll
    for (int p = 5; p < kOsMaxPass; ++p) {
      if (p < npass && act) {
        const unsigned d = (unsigned)(c >> (8 * p)) & 0xFF;
        if (d == 0xFF)
          ++c255[p];
        else
          atomicAdd(&h[p * 256 + d], 1u);
      }
    }
  }
#pragma unroll
  for (int p = 5; p < kOsMaxPass; ++p) {
    if (p < npass) {
      unsigned v = c255[p];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (l == 0 && v) atomicAdd(&h[p * 256 + 0xFF], v);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < npass * 256; i += kS2BS)
    block_hist[(uint64_t)blockIdx.x * (kOsMaxPass * 256) + i] = h[i];
}

// one workgroup per pass: base[p][d] = number of entries whose digit (pass p) is < d
__global__ __launch_bounds__(256) void os_base_kernel(const unsigned *__restrict__ block_hist,
                                                      int nblocks, unsigned *__restrict__ base) {
  __shared__ unsigned wtot[4];
  const int p = blockIdx.x, d = threadIdx.x;
  unsigned tot = 0;
#pragma unroll 8
  for (int b = 0; b < nblocks; ++b) tot += block_hist[(uint64_t)b * (kOsMaxPass * 256) + p * 256 + d];
  unsigned inc = tot;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned o = __shfl_up(inc, off, 64);
    if (lane_id() >= (unsigned)off) inc += o;
  }
  const unsigned w = threadIdx.x / kWave;
  if (lane_id() == 63) wtot[w] = inc;
  __syncthreads();
  unsigned wb = 0;
  for (unsigned q = 0; q < w; ++q) wb += wtot[q];
  base[p * 256 + d] = wb + inc - tot;
}

// (LOAD: element index -> packed word; the kernels below differ only in where a word comes from)
template <bool LAST, typename LOAD>
__device__ __forceinline__ void os_scatter_body(
    LOAD load, uint64_t n, int shift, const unsigned *__restrict__ base,
    unsigned *status, unsigned *ticket, uint64_t *out_comp, int32_t *out_keys, int64_t *out_cnts) {
  constexpr int NW = kS2BS / kWave;
  __shared__ unsigned wcnt[NW][256];
  __shared__ unsigned goff[256];
  __shared__ unsigned wtot[NW];
  __shared__ unsigned s_tile;
  __shared__ uint64_t stage[kS2Tile];
  const unsigned w = threadIdx.x / kWave, l = lane_id();
  if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u);
#pragma unroll
  for (int q = 0; q < NW; ++q) wcnt[q][threadIdx.x] = 0;
  __syncthreads();
  const unsigned tile = s_tile;
  uint64_t c[kS2Rows];
  unsigned short local[kS2Rows];
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = s2_elem(tile, w, r, l);
    c[r] = ~0ull;
    if (i < n) c[r] = load(i);
  }
  const uint64_t tile_base = (uint64_t)tile * kS2Tile;
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const bool act = s2_elem(tile, w, r, l) < n;
    const unsigned d = (unsigned)(c[r] >> shift) & 0xFF;
    const unsigned long long peers = match_digit(d, act);
    const unsigned rank = __popcll(peers & ((1ull << l) - 1ull));
    const unsigned before = act ? wcnt[w][d] : 0;  // equal digits in earlier rows of this wave
    __builtin_amdgcn_wave_barrier();
    if (act && rank == 0) wcnt[w][d] = before + (unsigned)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    local[r] = (unsigned short)(before + rank);
  }
  __syncthreads();
  {  // thread d: tile count of digit d, tile-local start, look-back for the global offset
    const unsigned d = threadIdx.x;
    unsigned t[NW], tot = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      t[q] = wcnt[q][d];
      tot += t[q];
    }
    // publish this tile's aggregate first: the tiles behind us only need this word
    unsigned *my = status + (uint64_t)tile * 256 + d;
    __hip_atomic_store(my, (tile == 0 ? kOsPrefix : kOsAgg) | tot, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o = __shfl_up(inc, off, 64);
      if (l >= (unsigned)off) inc += o;
    }
    if (l == 63) wtot[w] = inc;
    __syncthreads();
    unsigned wbase = 0;
    for (unsigned q = 0; q < w; ++q) wbase += wtot[q];
    const unsigned dstart = wbase + inc - tot;
    unsigned run = dstart;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      wcnt[q][d] = run;
      run += t[q];
    }
    unsigned excl = 0;
    if (tile > 0) {
      unsigned tb = tile - 1;
      while (true) {
        const unsigned v = __hip_atomic_load(status + (uint64_t)tb * 256 + d, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        const unsigned f = v >> 30;
        if (f == 0) {
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        excl += v & kOsMask;
        if (f == 2) break;
        --tb;  // tile 0 always publishes a prefix: never runs below 0
      }
      __hip_atomic_store(my, kOsPrefix | (excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    goff[d] = base[d] + excl - dstart;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    if (s2_elem(tile, w, r, l) < n) {
      const unsigned d = (unsigned)(c[r] >> shift) & 0xFF;
      stage[wcnt[w][d] + local[r]] = c[r];
    }
  }
  __syncthreads();
  const unsigned tile_n = (unsigned)(n - tile_base < (uint64_t)kS2Tile ? n - tile_base : kS2Tile);
#pragma unroll 4
  for (int j = 0; j < kS2Rows; ++j) {
    const unsigned idx = j * kS2BS + threadIdx.x;
    if (idx < tile_n) {
      const uint64_t v = stage[idx];
      const unsigned d = (unsigned)(v >> shift) & 0xFF;
      const unsigned dst = goff[d] + idx;
      if (LAST) {
        out_keys[dst] = comp_key(v);
        out_cnts[dst] = comp_cnt(v);
      } else {
        out_comp[dst] = v;
      }
    }
  }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kS2BS) void os_scatter_kernel(
    const uint64_t *__restrict__ comp, const int32_t *__restrict__ keys,
    const int64_t *__restrict__ cnts, uint64_t n, int shift, const unsigned *__restrict__ base,
    unsigned *status, unsigned *ticket, uint64_t *out_comp, int32_t *out_keys, int64_t *out_cnts) {
  os_scatter_body<LAST>([=](uint64_t i) -> uint64_t { return FIRST ? comp_make(keys[i], cnts[i]) : comp[i]; },
                        n, shift, base, status, ticket, out_comp, out_keys, out_cnts);
}

// the word of row i of a key column as nvt_sgb_sort sorts it: (order-preserving 32-bit key image
// << 32) | fold << rb | row -- the first pass and the histogram read the COLUMN (4 / 8 + 1 bytes per
// row) instead of a packed copy of it (a pass that wrote 8 bytes per row and two that read them)
template <typename K>
struct PackedKeyWord {
  const K *keys;
  const uint8_t *fold;
  int64_t bias;
  int rb;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
    const uint64_t img = (uint32_t)((uint64_t)(int64_t)keys[i] - (uint64_t)bias);
    const uint64_t f = fold ? (uint64_t)fold[i] : 0ull;
    return (img << 32) | (f << rb) | i;
  }
};
template <typename K>
__global__ __launch_bounds__(kS2BS) void os_scatter_pack_kernel(
    PackedKeyWord<K> src, uint64_t n, int shift, const unsigned *__restrict__ base, unsigned *status,
    unsigned *ticket, uint64_t *out_comp) {
  os_scatter_body<false>(src, n, shift, base, status, ticket, out_comp, nullptr, nullptr);
}

// tmp layout: compA[n] | compB[n] | block_hist | base | status[npass][ntiles][256] | tickets
inline uint64_t os_tmp_bytes(uint64_t n) {
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile;
  return 2 * n * 8 + (uint64_t)kOsHistBlocks * kOsMaxPass * 256 * 4 + kOsMaxPass * 256 * 4 +
         (uint64_t)kOsMaxPass * ntiles * 256 * 4 + kOsMaxPass * 4 + 256;
}

inline int vocab_sort_onesweep(int32_t *keys, int64_t *counts, uint64_t n, int64_t max_count,
                               void *tmp, hipStream_t stream) {
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile;
  char *p = reinterpret_cast<char *>(tmp);
  uint64_t *bufs[2];
  bufs[0] = reinterpret_cast<uint64_t *>(p);
  p += n * 8;
  bufs[1] = reinterpret_cast<uint64_t *>(p);
  p += n * 8;
  unsigned *block_hist = reinterpret_cast<unsigned *>(p);
  p += (uint64_t)kOsHistBlocks * kOsMaxPass * 256 * 4;
  unsigned *base = reinterpret_cast<unsigned *>(p);
  p += kOsMaxPass * 256 * 4;
  unsigned *status = reinterpret_cast<unsigned *>(p);
  int count_bytes = 0;
  for (uint64_t m = (uint64_t)max_count; m; m >>= 8) ++count_bytes;
  const int npass = 4 + count_bytes;  // 4 key bytes, then the live bytes of ~count
  const uint64_t status_words = (uint64_t)npass * ntiles * 256;
  unsigned *tickets = status + status_words;
  NVT_CHECK_HIP(hipMemsetAsync(status, 0, (status_words + kOsMaxPass) * 4, stream));
  const unsigned hb = (unsigned)(ntiles < (uint64_t)kOsHistBlocks ? ntiles : kOsHistBlocks);
  os_hist_kernel<<<hb, kS2BS, 0, stream>>>(keys, counts, n, npass, block_hist);
  NVT_CHECK_LAUNCH();
  os_base_kernel<<<npass, 256, 0, stream>>>(block_hist, (int)hb, base);
  NVT_CHECK_LAUNCH();
  const uint64_t *src = nullptr;
  int flip = 0;
  for (int pass = 0; pass < npass; ++pass) {
    const int shift = 8 * pass;
    const bool first = pass == 0, last = pass == npass - 1;
    unsigned *st = status + (uint64_t)pass * ntiles * 256;
    uint64_t *dst = bufs[flip];
    if (first)
      os_scatter_kernel<true, false><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          nullptr, keys, counts, n, shift, base + pass * 256, st, tickets + pass, dst, nullptr,
          nullptr);
    else if (last)
      os_scatter_kernel<false, true><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          src, nullptr, nullptr, n, shift, base + pass * 256, st, tickets + pass, nullptr, keys,
          counts);
    else
      os_scatter_kernel<false, false><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          src, nullptr, nullptr, n, shift, base + pass * 256, st, tickets + pass, dst, nullptr,
          nullptr);
    NVT_CHECK_LAUNCH();
    src = dst;
    flip ^= 1;
  }
  return NVT_OK;
}

// ---- generic: stable LSD radix sort of packed 64-bit words on the bit range [bit_lo, bit_hi) ----
// (the onesweep scatter above with FIRST = LAST = false).  Used by the multi-key groupby update:
// words are (slot << 32 | row), sorted by slot, so that every group's rows become one run in
// row order.
template <typename LOAD>
__device__ __forceinline__ void os_hist_words_body(LOAD load, uint64_t n, int bit_lo, int npass,
                                                   unsigned *__restrict__ block_hist) {
  __shared__ unsigned h[kOsMaxPass * 256];
  for (int i = threadIdx.x; i < npass * 256; i += kS2BS) h[i] = 0;
  __syncthreads();
  const unsigned l = lane_id();
  const uint64_t stride = (uint64_t)gridDim.x * kS2BS;
  const uint64_t iters = (n + stride - 1) / stride;
  constexpr int U = 4;  // loads in flight per thread
  for (uint64_t it = 0; it < iters; it += U) {
    uint64_t cw[U];
    bool av[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t i = (it + u) * stride + (uint64_t)blockIdx.x * kS2BS + threadIdx.x;
      av[u] = (it + u) < iters && i < n;
      cw[u] = av[u] ? load(i) >> bit_lo : 0ull;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool act = av[u];
      const uint64_t c = cw[u];
#pragma unroll
      for (int p = 0; p < kOsMaxPass; ++p) {
        if (p < npass) {
          // sorted-by-group inputs are heavily skewed (one hot group = one digit value): a wave
          // whose 64 digits are all equal adds once; otherwise plain LDS atomics (a full
          // match-any aggregation per digit cost more than the conflicts it saved)
          const unsigned d = (unsigned)(c >> (8 * p)) & 0xFF;
          const unsigned long long am = __ballot(act);
          const unsigned d0 = __builtin_amdgcn_readfirstlane(d);
          if (am == ~0ull && __ballot(d == d0) == ~0ull) {
            if (l == 0) atomicAdd(&h[p * 256 + d0], 64u);
          } else if (act) {
            atomicAdd(&h[p * 256 + d], 1u);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < npass * 256; i += kS2BS)
    block_hist[(uint64_t)blockIdx.x * (kOsMaxPass * 256) + i] = h[i];
}

__global__ __launch_bounds__(kS2BS) void os_hist_words_kernel(const uint64_t *__restrict__ w,
                                                              uint64_t n, int bit_lo, int npass,
                                                              unsigned *__restrict__ block_hist) {
  os_hist_words_body([=](uint64_t i) -> uint64_t { return w[i]; }, n, bit_lo, npass, block_hist);
}
template <typename K>
__global__ __launch_bounds__(kS2BS) void os_hist_pack_kernel(PackedKeyWord<K> src, uint64_t n, int bit_lo,
                                                             int npass, unsigned *__restrict__ block_hist) {
  os_hist_words_body(src, n, bit_lo, npass, block_hist);
}

uint64_t sort_words_tmp_bytes(uint64_t n) { return os_tmp_bytes(n); }

// Sorts data[0..n) by bits [bit_lo, bit_hi) (stable).  *result = data or a buffer inside tmp.
// keys != nullptr: the words are the packed rows of a key column (PackedKeyWord: key image, fold,
// row) that nobody has written out -- the histogram and the first pass read the column.
static int sort_words_impl(uint64_t *data, const void *keys, int key_dtype, int64_t key_bias,
                           const uint8_t *fold, int rb, uint64_t n, int bit_lo, int bit_hi, void *tmp,
                           uint64_t **result, hipStream_t stream) {
  NVT_CHECK_ARG(n < (1ull << 30), "at most 2^30-1 words");
  const int npass = (bit_hi - bit_lo + 7) / 8;
  NVT_CHECK_ARG(npass >= 1 && npass <= kOsMaxPass, "bit range too wide");
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile;
  char *p = reinterpret_cast<char *>(tmp);
  uint64_t *bufs[2];
  bufs[0] = reinterpret_cast<uint64_t *>(p);
  p += n * 8;
  bufs[1] = reinterpret_cast<uint64_t *>(p);
  p += n * 8;
  unsigned *block_hist = reinterpret_cast<unsigned *>(p);
  p += (uint64_t)kOsHistBlocks * kOsMaxPass * 256 * 4;
  unsigned *base = reinterpret_cast<unsigned *>(p);
  p += kOsMaxPass * 256 * 4;
  unsigned *status = reinterpret_cast<unsigned *>(p);
  const uint64_t status_words = (uint64_t)npass * ntiles * 256;
  unsigned *tickets = status + status_words;
  NVT_CHECK_HIP(hipMemsetAsync(status, 0, (status_words + kOsMaxPass) * 4, stream));
  const unsigned hb = (unsigned)(ntiles < (uint64_t)kOsHistBlocks ? ntiles : kOsHistBlocks);
  const PackedKeyWord<int32_t> s32{reinterpret_cast<const int32_t *>(keys), fold, key_bias, rb};
  const PackedKeyWord<int64_t> s64{reinterpret_cast<const int64_t *>(keys), fold, key_bias, rb};
  if (!keys)
    os_hist_words_kernel<<<hb, kS2BS, 0, stream>>>(data, n, bit_lo, npass, block_hist);
  else if (key_dtype == NVT_I32)
    os_hist_pack_kernel<int32_t><<<hb, kS2BS, 0, stream>>>(s32, n, bit_lo, npass, block_hist);
  else
    os_hist_pack_kernel<int64_t><<<hb, kS2BS, 0, stream>>>(s64, n, bit_lo, npass, block_hist);
  NVT_CHECK_LAUNCH();
  os_base_kernel<<<npass, 256, 0, stream>>>(block_hist, (int)hb, base);
  NVT_CHECK_LAUNCH();
  const uint64_t *src = data;
  int flip = 0;
  for (int pass = 0; pass < npass; ++pass) {
    uint64_t *dst = bufs[flip];
    unsigned *st = status + (uint64_t)pass * ntiles * 256;
    if (pass == 0 && keys && key_dtype == NVT_I32)
      os_scatter_pack_kernel<int32_t><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          s32, n, bit_lo, base, st, tickets, dst);
    else if (pass == 0 && keys)
      os_scatter_pack_kernel<int64_t><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          s64, n, bit_lo, base, st, tickets, dst);
    else
      os_scatter_kernel<false, false><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          src, nullptr, nullptr, n, bit_lo + 8 * pass, base + pass * 256, st, tickets + pass, dst,
          nullptr, nullptr);
    NVT_CHECK_LAUNCH();
    src = dst;
    flip ^= 1;
  }
  *result = const_cast<uint64_t *>(src);
  return NVT_OK;
}

int sort_words_bits(uint64_t *data, uint64_t n, int bit_lo, int bit_hi, void *tmp, uint64_t **result,
                    hipStream_t stream) {
  *result = data;
  if (n <= 1 || bit_hi <= bit_lo) return NVT_OK;
  return sort_words_impl(data, nullptr, 0, 0, nullptr, 0, n, bit_lo, bit_hi, tmp, result, stream);
}

// The packed rows of a key column ((key - bias) image << 32 | fold << rb | row), sorted by
// bits [rb, 64) (key, then fold; stable): *result = a buffer inside tmp (sort_words_tmp_bytes(n)).
int sort_packed_keys(const void *keys, int key_dtype, int64_t key_bias, const uint8_t *fold, int rb,
                     uint64_t n, void *tmp, uint64_t **result, hipStream_t stream) {
  NVT_CHECK_ARG(keys && n >= 1 && rb >= 24 && rb <= 32, "keys / rows / row bits");
  return sort_words_impl(nullptr, keys, key_dtype, key_bias, fold, rb, n, rb, 64, tmp, result, stream);
}

// ---- all small vocabularies of a fit: the whole device sorts them ----------------------------
// packed words, ascending.  Every list is cut into chunks of kSmallChunk words; launch A sorts
// each chunk in LDS (16 KiB: many workgroups per CU), which finishes a list of one chunk.  The
// sorted chunks of a longer list go to its scratch as packed words, and launch B ranks every
// element among all chunks of its list -- its index in its own chunk + a binary search in each
// other chunk, equal words ordered by chunk -- and writes it out unpacked at that rank.  No
// workgroup waits for another.  (One 1024-thread workgroup per list over 128 KiB of LDS kept 13
// of 256 CUs busy for ~120 us; a caller without scratch still gets that kernel.)
constexpr int kSmallPackedMax = 16384;
constexpr int kSmallChunk = 2048, kSmallRankBS = 256;
constexpr int kSmallMaxChunks = kSmallPackedMax / kSmallChunk;
struct SmallCol {
  int32_t *keys;
  int64_t *counts;
  uint64_t *tmp;  // kSmallChunk < n: n packed words (the sorted chunks between the two launches)
  unsigned n;
};
constexpr int kSmallBatch = 64;
struct SmallBatch {
  SmallCol c[kSmallBatch];
  unsigned chunk_start[kSmallBatch + 1];  // launch A: first workgroup of every list
  unsigned rank_start[kSmallBatch + 1];   // launch B: the same (lists of one chunk take none)
  int ncols;
};
__device__ __forceinline__ int small_col_of(const unsigned *start, int n, unsigned b) {
  int c = 0;
  while (c + 1 < n && b >= start[c + 1]) ++c;
  return c;
}
__global__ __launch_bounds__(kSmallBS) void sort_small_packed_many_kernel(SmallBatch b) {
  __shared__ uint64_t sv[kSmallPackedMax];
  const SmallCol col = b.c[blockIdx.x];
  const unsigned n = col.n;
  unsigned m = 1;
  while (m < n) m <<= 1;
  for (unsigned i = threadIdx.x; i < m; i += kSmallBS)
    sv[i] = i < n ? comp_make(col.keys[i], col.counts[i]) : ~0ull;  // padding sorts last
  __syncthreads();
  for (unsigned size = 2; size <= m; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      for (unsigned t = threadIdx.x; t < m / 2; t += kSmallBS) {
        const unsigned lo = 2 * t - (t & (stride - 1));
        const unsigned hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t a = sv[lo], c = sv[hi];
        if (up ? (c < a) : (a < c)) {
          sv[lo] = c;
          sv[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (unsigned i = threadIdx.x; i < n; i += kSmallBS) {
    const uint64_t v = sv[i];
    col.keys[i] = comp_key(v);
    col.counts[i] = comp_cnt(v);
  }
}

// launch A: workgroup = one chunk of one list; a thread per compare-exchange of a stage (the device
// is idle beside these few workgroups: what counts is the length of the 66 stages, not occupancy)
__global__ __launch_bounds__(kSmallBS) void sort_small_chunk_kernel(SmallBatch b) {
  __shared__ uint64_t sv[kSmallChunk];
  const int ci = small_col_of(b.chunk_start, b.ncols, blockIdx.x);
  const SmallCol col = b.c[ci];
  const unsigned first = (blockIdx.x - b.chunk_start[ci]) * kSmallChunk;
  const unsigned n = col.n - first < (unsigned)kSmallChunk ? col.n - first : (unsigned)kSmallChunk;
  unsigned m = 2;
  while (m < n) m <<= 1;
  for (unsigned i = threadIdx.x; i < m; i += kSmallBS)
    sv[i] = i < n ? comp_make(col.keys[first + i], col.counts[first + i]) : ~0ull;  // padding sorts last
  __syncthreads();
  // A stage of stride <= 64 pairs words inside blocks of 128, and thread t works in block t / 64:
  // every wave stays in its own 128 words, so such stages only wait for the wave's own LDS traffic.
  // A wider stage reads what other waves wrote: workgroup barriers around it.  (56 of the 66 stages
  // of a full chunk are narrow; a barrier of 16 waves per stage was most of this kernel's time.)
  for (unsigned size = 2; size <= m; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      const bool wide = stride > (unsigned)kWave;
      if (wide) __syncthreads();
      for (unsigned t = threadIdx.x; t < m / 2; t += kSmallBS) {
        const unsigned lo = 2 * t - (t & (stride - 1));
        const unsigned hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t a = sv[lo], c = sv[hi];
        if (up ? (c < a) : (a < c)) {
          sv[lo] = c;
          sv[hi] = a;
        }
      }
      if (wide) {
        __syncthreads();
      } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
  }
  __syncthreads();
  if (col.n > (unsigned)kSmallChunk) {
    for (unsigned i = threadIdx.x; i < n; i += kSmallBS) col.tmp[first + i] = sv[i];
    return;
  }
  for (unsigned i = threadIdx.x; i < n; i += kSmallBS) {
    const uint64_t v = sv[i];
    col.keys[i] = comp_key(v);
    col.counts[i] = comp_cnt(v);
  }
}

// launch B: thread = one element of a list of several chunks.  The searches in the other chunks
// do not depend on one another: they advance in step, one load each per round.
__global__ __launch_bounds__(kSmallRankBS) void sort_small_rank_kernel(SmallBatch b) {
  const int ci = small_col_of(b.rank_start, b.ncols, blockIdx.x);
  const SmallCol col = b.c[ci];
  const unsigned e = (blockIdx.x - b.rank_start[ci]) * kSmallRankBS + threadIdx.x;
  if (e >= col.n) return;
  const uint64_t *__restrict__ src = col.tmp;
  const uint64_t v = src[e];
  const unsigned own = e / kSmallChunk;
  const unsigned nchunks = (col.n + kSmallChunk - 1) / kSmallChunk;
  unsigned lo[kSmallMaxChunks], hi[kSmallMaxChunks];
#pragma unroll
  for (int q = 0; q < kSmallMaxChunks; ++q) {
    const unsigned at = (unsigned)q * kSmallChunk;
    lo[q] = 0;
    hi[q] = 0;
    if ((unsigned)q < nchunks && (unsigned)q != own)
      hi[q] = col.n - at < (unsigned)kSmallChunk ? col.n - at : (unsigned)kSmallChunk;
  }
  // entries of chunk q in front of v: words below it, and equal words of the chunks before its own.
  // All loads of a round are issued before any is looked at (a search that is over reads its own
  // element again): 12 load latencies per thread, not 12 per chunk.
  for (int step = 0; step < 12; ++step) {  // 2^12 > kSmallChunk + 1 outcomes
    unsigned mid[kSmallMaxChunks];
    uint64_t a[kSmallMaxChunks];
#pragma unroll
    for (int q = 0; q < kSmallMaxChunks; ++q) {
      mid[q] = (lo[q] + hi[q]) >> 1;
      a[q] = src[lo[q] < hi[q] ? (unsigned)q * kSmallChunk + mid[q] : e];
    }
#pragma unroll
    for (int q = 0; q < kSmallMaxChunks; ++q) {
      if (lo[q] < hi[q]) {
        if (a[q] < v || (a[q] == v && (unsigned)q < own))
          lo[q] = mid[q] + 1;
        else
          hi[q] = mid[q];
      }
    }
  }
  unsigned rank = e - own * kSmallChunk;
#pragma unroll
  for (int q = 0; q < kSmallMaxChunks; ++q) rank += lo[q];
  col.keys[rank] = comp_key(v);
  col.counts[rank] = comp_cnt(v);
}

// tmp layout of the packed path: compA[n] | compB[n] | tile_hist | chunk_tot
inline uint64_t sort2_tmp_bytes(uint64_t n) {
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile, hist_len = 256 * ntiles;
  return 2 * n * 8 + pad16(hist_len * 4) + scan_chunks(hist_len) * 8 + 64;
}

inline int vocab_sort_packed(int32_t *keys, int64_t *counts, uint64_t n, int64_t max_count,
                             void *tmp, hipStream_t stream) {
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile, hist_len = 256 * ntiles;
  char *p = reinterpret_cast<char *>(tmp);
  uint64_t *bufs[2];
  bufs[0] = reinterpret_cast<uint64_t *>(p);
  p += n * 8;
  bufs[1] = reinterpret_cast<uint64_t *>(p);
  p += n * 8;
  unsigned *tile_hist = reinterpret_cast<unsigned *>(p);
  p += pad16(hist_len * 4);
  unsigned long long *chunk_tot = reinterpret_cast<unsigned long long *>(p);
  int count_bytes = 0;
  for (uint64_t m = (uint64_t)max_count; m; m >>= 8) ++count_bytes;
  const int npass = 4 + count_bytes;  // 4 key bytes, then the live bytes of ~count
  const uint64_t *src = nullptr;
  int flip = 0;
  for (int pass = 0; pass < npass; ++pass) {
    const int shift = 8 * pass;
    const bool first = pass == 0, last = pass == npass - 1;
    if (first)
      sort2_hist_kernel<true><<<(unsigned)ntiles, kS2BS, 0, stream>>>(nullptr, keys, counts, n,
                                                                       shift, tile_hist, ntiles);
    else
      sort2_hist_kernel<false><<<(unsigned)ntiles, kS2BS, 0, stream>>>(src, nullptr, nullptr, n,
                                                                        shift, tile_hist, ntiles);
    NVT_CHECK_LAUNCH();
    const unsigned long long *cbase = nullptr;
    {
      int rc = exclusive_scan_u32_deferred(tile_hist, hist_len, chunk_tot, &cbase, stream);
      if (rc) return rc;
    }
    uint64_t *dst = bufs[flip];
    if (first)
      sort2_scatter_kernel<true, false><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          nullptr, keys, counts, n, shift, tile_hist, cbase, ntiles, dst, nullptr, nullptr);
    else if (last)
      sort2_scatter_kernel<false, true><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          src, nullptr, nullptr, n, shift, tile_hist, cbase, ntiles, nullptr, keys, counts);
    else
      sort2_scatter_kernel<false, false><<<(unsigned)ntiles, kS2BS, 0, stream>>>(
          src, nullptr, nullptr, n, shift, tile_hist, cbase, ntiles, dst, nullptr, nullptr);
    NVT_CHECK_LAUNCH();
    src = dst;
    flip ^= 1;
  }
  return NVT_OK;
}

template <typename K>
int vocab_sort(K *keys, int64_t *counts, uint64_t n, int64_t max_count, void *tmp,
               hipStream_t stream) {
  constexpr int NP = (int)sizeof(K) + 8;
  if (n <= 1) return NVT_OK;
  NVT_CHECK_ARG(n < (1ull << 32), "at most 2^32-1 vocabulary entries");
  if (n <= kSmallMax) {
    sort_small_kernel<K><<<1, kSmallBS, 0, stream>>>(keys, counts, (unsigned)n);
    NVT_CHECK_LAUNCH();
    return NVT_OK;
  }
  if constexpr (sizeof(K) == 4) {
    if (max_count > 0 && max_count < (1ll << 32) && n < (1ull << 30))
      return vocab_sort_onesweep(keys, counts, n, max_count, tmp, stream);
    if (max_count > 0 && max_count < (1ll << 32) && n < (1ull << 31))
      return vocab_sort_packed(keys, counts, n, max_count, tmp, stream);
  }
  const uint64_t ntiles = (n + kTileSort - 1) / kTileSort;
  // tmp layout: counts2 | keys2 | tile_hist | chunk_tot | pass_hist
  char *p = reinterpret_cast<char *>(tmp);
  int64_t *counts2 = reinterpret_cast<int64_t *>(p);
  p += n * sizeof(int64_t);
  K *keys2 = reinterpret_cast<K *>(p);
  p += pad16(n * sizeof(K));
  unsigned *tile_hist = reinterpret_cast<unsigned *>(p);
  const uint64_t hist_len = 256 * ntiles;
  p += pad16(hist_len * sizeof(unsigned));
  const uint64_t nchunks = (hist_len + kScanChunk - 1) / kScanChunk;
  unsigned long long *chunk_tot = reinterpret_cast<unsigned long long *>(p);
  p += nchunks * sizeof(unsigned long long);
  unsigned long long *pass_hist = reinterpret_cast<unsigned long long *>(p);

  bool run_pass[NP];
  if (max_count > 0) {
    // counts lie in [0, max_count]: the inverted-count bytes above its top byte are all 0xFF
    constexpr int KB = (int)sizeof(K);
    int count_bytes = 0;
    for (uint64_t m = (uint64_t)max_count; m; m >>= 8) ++count_bytes;
    for (int p = 0; p < NP; ++p) run_pass[p] = p < KB || (p - KB) < count_bytes;
  } else {
    NVT_CHECK_HIP(hipMemsetAsync(pass_hist, 0, NP * 256 * sizeof(unsigned long long), stream));
    sort_pass_hist_kernel<K><<<stream_grid(n, kBlock * 8, 4), kBlock, 0, stream>>>(keys, counts, n,
                                                                                     pass_hist);
    NVT_CHECK_LAUNCH();
    unsigned long long host_hist[NP * 256];
    NVT_CHECK_HIP(hipMemcpyAsync(host_hist, pass_hist, sizeof(host_hist), hipMemcpyDeviceToHost,
                                 stream));
    NVT_CHECK_HIP(hipStreamSynchronize(stream));
    for (int p = 0; p < NP; ++p) {
      run_pass[p] = true;
      for (int d = 0; d < 256; ++d)
        if (host_hist[p * 256 + d] == n) run_pass[p] = false;
    }
  }

  K *src_k = keys, *dst_k = keys2;
  int64_t *src_c = counts, *dst_c = counts2;
  for (int pass = 0; pass < NP; ++pass) {
    if (!run_pass[pass]) continue;
    sort_tile_hist_kernel<K><<<(unsigned)ntiles, kBlock, 0, stream>>>(src_k, src_c, n, pass,
                                                                      tile_hist, ntiles);
    NVT_CHECK_LAUNCH();
    {
      int rc = exclusive_scan_u32(tile_hist, hist_len, chunk_tot, stream);
      if (rc) return rc;
    }
    sort_scatter_kernel<K><<<(unsigned)ntiles, kBlock, 0, stream>>>(src_k, src_c, n, pass,
                                                                    tile_hist, ntiles, dst_k, dst_c);
    NVT_CHECK_LAUNCH();
    K *tk = src_k;
    src_k = dst_k;
    dst_k = tk;
    int64_t *tc = src_c;
    src_c = dst_c;
    dst_c = tc;
  }
  if (src_k != keys) {
    NVT_CHECK_HIP(hipMemcpyAsync(keys, src_k, n * sizeof(K), hipMemcpyDeviceToDevice, stream));
    NVT_CHECK_HIP(
        hipMemcpyAsync(counts, src_c, n * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  }
  return NVT_OK;
}

int vocab_sort_any(int key_bytes, void *keys, int64_t *counts, uint64_t n, int64_t max_count,
                   void *tmp, hipStream_t s) {
  NVT_PROF("vocab_sort", 0, s);
  if (key_bytes == 4) return vocab_sort<int32_t>((int32_t *)keys, counts, n, max_count, tmp, s);
  return vocab_sort<int64_t>((int64_t *)keys, counts, n, max_count, tmp, s);
}

bool vocab_sort_small_eligible(int key_bytes, uint64_t n, int64_t max_count) {
  return key_bytes == 4 && n >= 2 && n <= (uint64_t)kSmallPackedMax && max_count > 0 &&
         max_count < (1ll << 32);
}

int vocab_sort_small_batch(const SmallSortDesc *cols, int ncols, hipStream_t s) {
  for (int c0 = 0; c0 < ncols; c0 += kSmallBatch) {
    const int nc = ncols - c0 < kSmallBatch ? ncols - c0 : kSmallBatch;
    SmallBatch b, whole;  // whole: lists of several chunks without scratch, one workgroup each
    memset(&b, 0, sizeof(b));
    memset(&whole, 0, sizeof(whole));
    int nb = 0, nw = 0;
    for (int i = 0; i < nc; ++i) {
      const SmallSortDesc &d = cols[c0 + i];
      if (d.n > (unsigned)kSmallChunk && d.tmp == nullptr) {
        whole.c[nw++] = {d.keys, d.counts, nullptr, d.n};
        continue;
      }
      b.c[nb] = {d.keys, d.counts, reinterpret_cast<uint64_t *>(d.tmp), d.n};
      const unsigned chunks = (d.n + kSmallChunk - 1) / kSmallChunk;
      b.chunk_start[nb + 1] = b.chunk_start[nb] + chunks;
      b.rank_start[nb + 1] = b.rank_start[nb] + (chunks > 1 ? (d.n + kSmallRankBS - 1) / kSmallRankBS : 0u);
      ++nb;
    }
    b.ncols = nb;
    NVT_PROF("vocab_sort_small", 0, s);
    if (b.chunk_start[nb]) {
      sort_small_chunk_kernel<<<b.chunk_start[nb], kSmallBS, 0, s>>>(b);
      NVT_CHECK_LAUNCH();
    }
    if (b.rank_start[nb]) {
      sort_small_rank_kernel<<<b.rank_start[nb], kSmallRankBS, 0, s>>>(b);
      NVT_CHECK_LAUNCH();
    }
    if (nw) {
      sort_small_packed_many_kernel<<<nw, kSmallBS, 0, s>>>(whole);
      NVT_CHECK_LAUNCH();
    }
  }
  return NVT_OK;
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_vocab_sort_tmp_bytes(int key_bytes, uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes && (key_bytes == 4 || key_bytes == 8), "key_bytes must be 4 or 8");
  const uint64_t ntiles = (n + kTileSort - 1) / kTileSort;
  const uint64_t hist_len = 256 * ntiles;
  const uint64_t nchunks = (hist_len + kScanChunk - 1) / kScanChunk;
  *bytes = n * 8 + pad16(n * key_bytes) + pad16(hist_len * 4) + nchunks * 8 +
           (uint64_t)(key_bytes + 8) * 256 * 8 + 64;
  if (key_bytes == 4 && sort2_tmp_bytes(n) > *bytes) *bytes = sort2_tmp_bytes(n);
  if (key_bytes == 4 && os_tmp_bytes(n) > *bytes) *bytes = os_tmp_bytes(n);
  return NVT_OK;
}
int nvt_vocab_sort_i32(int32_t *keys, int64_t *counts, uint64_t n, int64_t max_count, void *tmp,
                       void *stream) {
  NVT_CHECK_ARG(n <= 1 || (keys && counts && tmp), "null pointer");
  return vocab_sort_any(4, keys, counts, n, max_count, tmp, (hipStream_t)stream);
}
int nvt_vocab_sort_i64(int64_t *keys, int64_t *counts, uint64_t n, int64_t max_count, void *tmp,
                       void *stream) {
  NVT_CHECK_ARG(n <= 1 || (keys && counts && tmp), "null pointer");
  return vocab_sort_any(8, keys, counts, n, max_count, tmp, (hipStream_t)stream);
}

}  // extern "C"
