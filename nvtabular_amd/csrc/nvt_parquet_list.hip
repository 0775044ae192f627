// Repetition / definition level streams of parquet list columns (Dataset.to_parquet, the PLAIN
// writer of parquet_plain.py): a list column is written as the standard three-level list, maximum
// repetition level 1 and maximum definition level 3.  This engine has no null lists, so a row of L
// leaves occupies max(L, 1) SLOTS: an empty row one slot (rep 0, def 1), leaf i of a row rep 0 / 1
// (first leaf of its row or not) and def 3 / 2 (valid or null).
//
// Plan (nvt_pqlist_plan), for the n rows behind `offsets`:
//   1. slot_len_kernel / scan_totals_kernel (nvt_scan.hpp) / slot_add_kernel: S[r] = the exclusive
//      prefix sum of max(len_r, 1), S[n] = the number of slots; 64 bits wide, tiles of 2048 rows.
//   2. pages_kernel, ONE workgroup (pages are few): nominal page p starts at the first row r with
//      S[r] >= p * page_slots (one search per page); a page that gets no row -- one row spans several
//      multiples -- is dropped.  The kept pages are numbered and their byte offsets in the packed
//      level buffers and their first pack tile are scanned in the same loop.  A page is never cut
//      inside a row.
// Pack (nvt_pqlist_pack_many): one launch over (page, slot) in tiles of 2048 slots of ONE page, so
//   a page's packing restarts at bit 0.  The row of a slot is a search in S: two lanes find the
//   first and the last row of the tile, S and the offsets of the rows between them are staged in
//   LDS and every lane searches there; a tile that spans more than kStage rows (long runs of empty
//   or one-leaf rows) searches global memory between the two bounds instead.  The repetition bits
//   of a wave's 64 slots are one __ballot word; the definition levels (2 bits) are two ballot words
//   interleaved into 16 bytes.  Every store is a whole 64-bit word: a page's rep / def region is
//   padded to 8 / 16 bytes and the bits behind its last slot are 0.  Row and leaf are found once per
//   slot and used for every column of the batch (columns that share the offsets); the non-null
//   leaves of a column and page are counted with integer atomics (deterministic).
#include "nvt_common.hpp"
#include "nvt_list_tile.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr uint64_t kTile = kListTile;  // rows (plan) or slots of one page (pack) per tile
constexpr int kStage = 1024 + 2;       // rows of one pack tile whose S / offsets are held in LDS
constexpr int kMaxCols = NVT_PQLIST_MAX_COLS;
constexpr int kHdr = NVT_PQLIST_HEADER_WORDS;
constexpr int kPg = NVT_PQLIST_PAGE_WORDS;

__host__ __device__ inline uint64_t ntiles_of(uint64_t n) { return list_ntiles(n); }
__device__ __forceinline__ uint64_t slots_of(int64_t len) { return len > 1 ? (uint64_t)len : 1; }
__host__ __device__ inline uint64_t rep_bytes_of(uint64_t slots) { return (slots + 7) / 8; }

// ---- plan: S ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void slot_len_kernel(const int64_t *__restrict__ off, uint64_t n,
                                                          uint64_t *__restrict__ S,
                                                          unsigned long long *__restrict__ tile_tot) {
  __shared__ uint64_t wsum[kBlock / kWave];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  const uint64_t nt = ntiles_of(n);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r0 = t * kTile + (uint64_t)threadIdx.x * 8;  // 8 consecutive rows per lane
    uint64_t len[8], tot = 0;
    int64_t prev = r0 < n ? off[r0] : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      len[j] = 0;
      if (r0 + j < n) {
        const int64_t next = off[r0 + j + 1];
        len[j] = slots_of(next - prev);
        prev = next;
      }
      tot += len[j];
    }
    const uint64_t inc = wave_incl_scan(tot);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t run = inc - tot;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (r0 + j < n) S[r0 + j] = run;
      run += len[j];
    }
    if (threadIdx.x == kBlock - 1) tile_tot[t] = run;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void slot_add_kernel(uint64_t *__restrict__ S, uint64_t n,
                                                          const unsigned long long *__restrict__ tile_base,
                                                          const int64_t *__restrict__ off) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint64_t v = S[i] + tile_base[i / kTile];
    S[i] = v;
    if (i == n - 1) S[n] = v + slots_of(off[n] - off[n - 1]);
  }
}

// ---- plan: page table ---------------------------------------------------------------------------
// the first r in [0, n] with S[r] >= x (S is strictly increasing; S[n] is the slot total)
__device__ __forceinline__ uint64_t first_row_at(const uint64_t *S, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (S[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void pages_kernel(const int64_t *__restrict__ off,
                                                       const int64_t *__restrict__ origin,
                                                       const uint64_t *__restrict__ S, uint64_t n,
                                                       uint64_t page_slots, uint64_t max_pages, uint64_t rep_cap,
                                                       uint64_t def_cap, uint64_t *__restrict__ table) {
  __shared__ uint64_t srow[kBlock + 1];
  __shared__ uint64_t wsum[4][kBlock / kWave];
  __shared__ uint64_t carry[4];  // kept pages, rep bytes, def bytes, pack tiles before this round
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  const uint64_t total = S[n];
  const uint64_t pnom = (total + page_slots - 1) / page_slots;
  uint64_t *pages = table + kHdr;
  if (pnom > max_pages) {  // (more slots than the caller sized the buffers for: nothing is laid out)
    if (threadIdx.x < (unsigned)kHdr) table[threadIdx.x] = threadIdx.x == 0 ? pnom : threadIdx.x == 7 ? 1 : 0;
    return;
  }
  if (threadIdx.x < 4) carry[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t b = 0; b < pnom; b += kBlock) {
    for (unsigned k = threadIdx.x; k <= (unsigned)kBlock; k += kBlock) {
      const uint64_t p = b + k;
      srow[k] = p >= pnom ? n : first_row_at(S, n, p * page_slots);
    }
    __syncthreads();
    const uint64_t row0 = srow[threadIdx.x], row1 = srow[threadIdx.x + 1];
    const bool live = b + threadIdx.x < pnom && row1 > row0;
    const uint64_t slot0 = live ? S[row0] : 0;
    const uint64_t slots = live ? S[row1] - slot0 : 0;
    uint64_t v[4], ex[4];
    v[0] = live ? 1 : 0;
    v[1] = (rep_bytes_of(slots) + 7) & ~7ull;         // a page's rep region: whole 64-bit words
    v[2] = (2 * rep_bytes_of(slots) + 15) & ~15ull;   // its def region: whole 128-bit pairs
    v[3] = ntiles_of(slots);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t inc = wave_incl_scan(v[q]);
      if (lane == 63) wsum[q][w] = inc;
      ex[q] = inc - v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ex[q] += carry[q];
      for (unsigned k = 0; k < w; ++k) ex[q] += wsum[q][k];
    }
    if (live && ex[0] < max_pages) {
      uint64_t *e = pages + ex[0] * kPg;
      e[0] = row0;
      e[1] = row1 - row0;
      e[2] = slot0;
      e[3] = slots;
      e[4] = ex[1];
      e[5] = ex[2];
      e[6] = ex[3];
      e[7] = (uint64_t)(off[row1] - off[row0]);
    }
    __syncthreads();
    if (threadIdx.x == kBlock - 1)
      for (int q = 0; q < 4; ++q) carry[q] = ex[q] + v[q];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    table[0] = carry[0];
    table[1] = total;
    table[2] = carry[1];
    table[3] = carry[2];
    table[4] = carry[3];
    table[5] = (uint64_t)(off[0] - origin[0]);  // the leaves of the rows, counted from the column's first
    table[6] = (uint64_t)(off[n] - origin[0]);
    table[7] = (carry[0] > max_pages || carry[1] > rep_cap || carry[2] > def_cap) ? 1 : 0;
  }
}

// ---- pack ---------------------------------------------------------------------------------------
struct PCol {
  const uint8_t *valid;
  uint64_t bit0, nbits;
  uint64_t *def_out;
  unsigned long long *nonnull;
};
struct PBatch {
  PCol c[kMaxCols];
  int ncols;
};

// the row r in [lo, hi] with a[r] <= p < a[r + 1] (it exists: a[lo] <= p < a[hi + 1])
__device__ __forceinline__ uint64_t slot_row(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t p) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (a[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// bit i of x -> bit 2 i
__device__ __forceinline__ uint64_t spread_bits(uint32_t x) {
  uint64_t v = x;
  v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
  v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

__global__ __launch_bounds__(kBlock) void pack_kernel(PBatch b, const int64_t *__restrict__ off,
                                                      const int64_t *__restrict__ origin,
                                                      const uint64_t *__restrict__ S,
                                                      const uint64_t *__restrict__ table,
                                                      uint64_t *__restrict__ rep_out) {
  __shared__ uint64_t sS[kStage];
  __shared__ int64_t sO[kStage];
  __shared__ uint64_t sbound[2];
  __shared__ unsigned long long scount[kMaxCols];
  if (table[7] != 0) return;  // (the plan did not fit the buffers: the host raises after its read-back)
  const uint64_t npages = table[0], ntiles = table[4];
  const uint64_t *pages = table + kHdr;
  const int64_t o0 = origin[0];
  const unsigned lane = lane_id();
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t pi = 0, phi = npages - 1;  // the page of tile t: the last one whose first tile is <= t
    while (pi < phi) {
      const uint64_t mid = (pi + phi + 1) >> 1;
      if (pages[mid * kPg + 6] <= t) pi = mid;
      else phi = mid - 1;
    }
    const uint64_t *pg = pages + pi * kPg;
    const uint64_t row0 = pg[0], nrows = pg[1], slot0 = pg[2], nslots = pg[3];
    uint64_t *rep_pg = rep_out != nullptr ? rep_out + (pg[4] >> 3) : nullptr;
    const uint64_t def_word0 = pg[5] >> 3;
    const uint64_t q0 = (t - pg[6]) * kTile;  // (slots of the page; q0 is a multiple of 64)
    const uint64_t q1 = q0 + kTile < nslots ? q0 + kTile : nslots;
    if (threadIdx.x < 2)
      sbound[threadIdx.x] = slot_row(S, row0, row0 + nrows - 1, slot0 + (threadIdx.x == 0 ? q0 : q1 - 1));
    if (threadIdx.x < (unsigned)kMaxCols) scount[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t rlo = sbound[0], rhi = sbound[1];
    const bool staged = rhi - rlo + 2 <= (uint64_t)kStage;  // (block-uniform)
    if (staged)
      for (uint64_t k = threadIdx.x; k < rhi - rlo + 2; k += kBlock) {
        sS[k] = S[rlo + k];
        sO[k] = off[rlo + k];
      }
    __syncthreads();
    for (uint64_t q = q0 + threadIdx.x; q < q0 + kTile; q += kBlock) {  // (q - lane is a multiple of 64)
      const bool live = q < q1;
      bool leaf = false;
      uint64_t k = 0;
      int64_t at = 0;
      if (live) {
        const uint64_t g = slot0 + q;
        int64_t a, len;
        if (staged) {
          const uint64_t j = slot_row(sS, 0, rhi - rlo, g);
          k = g - sS[j];
          a = sO[j];
          len = sO[j + 1] - a;
        } else {
          const uint64_t r = slot_row(S, rlo, rhi, g);
          k = g - S[r];
          a = off[r];
          len = off[r + 1] - a;
        }
        leaf = len >= 1;  // (an empty row is one slot that holds no leaf)
        at = a + (int64_t)k;
      }
      const uint64_t w64 = q >> 6;
      const bool store = lane == 0 && live;  // (lane 0 holds the first slot of the word)
      const uint64_t rep = __ballot(live && k > 0);
      if (store && rep_pg != nullptr) rep_pg[w64] = rep;
      const uint64_t is_leaf = __ballot(leaf);
      for (int ci = 0; ci < b.ncols; ++ci) {
        const PCol &c = b.c[ci];
        bool ok = leaf;
        if (ok && c.valid != nullptr) {
          const uint64_t bit = c.bit0 + (uint64_t)(at - o0);
          ok = bit < c.nbits && ((c.valid[bit >> 3] >> (bit & 7)) & 1);
        }
        const uint64_t okw = __ballot(ok);
        const uint64_t low = __ballot(live && (!leaf || ok));  // def 1 (empty row) and def 3 (valid leaf)
        if (store) {
          uint64_t *d = c.def_out + def_word0 + 2 * w64;
          d[0] = spread_bits((uint32_t)low) | (spread_bits((uint32_t)is_leaf) << 1);
          d[1] = spread_bits((uint32_t)(low >> 32)) | (spread_bits((uint32_t)(is_leaf >> 32)) << 1);
          if (okw != 0) atomicAdd(&scount[ci], (unsigned long long)__popcll(okw));
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)b.ncols && scount[threadIdx.x] != 0)
      atomicAdd(&b.c[threadIdx.x].nonnull[pi], scount[threadIdx.x]);
    __syncthreads();
  }
}

// ---- unpack: staged level streams -> offsets + leaf bitmap (the parquet reader) ------------------
// The streams of nvt_pq_decode_list_chunk: rep 1 bit per slot, def W bits per slot, LSB first.  A slot
// is a row start when rep == 0, a leaf when def >= leaf_level, a non-null leaf when def == max_def.
//   count: one wave per tile of 2048 slots, popcounts of whole words -> row starts and leaves per
//          tile; two exclusive scans (nvt_scan.hpp) give every tile its first row and first leaf.
//   emit:  one wave per tile walks its 32 groups of 64 slots, one slot per lane: three ballot words
//          (start, leaf, valid); a lane's row / leaf rank = the wave's running base + the popcount of
//          the lower lanes.  A start lane stores offsets[row] = leaf rank.  Leaves take one validity
//          bit each and the other slots none, so a tile's bits start anywhere in a word: the wave
//          builds them in LDS (atomicOr at rank - first word of the tile), stores the words that lie
//          wholly inside the tile's leaves and merges the at most two it shares with its neighbours
//          into the zeroed bitmap with a 64-bit atomicOr (commutative: the result is deterministic).
constexpr int kUnpackWaves = kBlock / kWave;
constexpr int kUnpackWords = (int)(kTile / 64) + 2;   // bit string of one tile: 2048 bits at any bit offset

__device__ __forceinline__ uint64_t live_mask(uint64_t slot0, uint64_t n_slots) {
  return slot0 >= n_slots ? 0ull : (n_slots - slot0 >= 64 ? ~0ull : ((1ull << (n_slots - slot0)) - 1ull));
}
// 32 definition levels at 2 bits -> bit 2 i set when level i >= leaf_level (1 or 2)
__device__ __forceinline__ uint64_t leaf_pairs(uint64_t d, int leaf_level) {
  return (leaf_level == 1 ? (d | (d >> 1)) : (d >> 1)) & 0x5555555555555555ull;
}

__global__ __launch_bounds__(kBlock) void unpack_count_kernel(const uint64_t *__restrict__ rep,
                                                               const uint64_t *__restrict__ def, int width,
                                                               uint64_t n_slots, int leaf_level, uint64_t ntiles,
                                                               unsigned *__restrict__ tile_rows,
                                                               unsigned *__restrict__ tile_leaves) {
  const unsigned lane = lane_id();
  const uint64_t t = (uint64_t)blockIdx.x * kUnpackWaves + threadIdx.x / kWave;
  if (t >= ntiles) return;
  unsigned starts = 0, leaves = 0;
  const uint64_t g = t * (kTile / 64) + lane;   // lanes 0 .. 31: one group of 64 slots each
  const uint64_t live = lane < kTile / 64 ? live_mask(g * 64, n_slots) : 0ull;
  if (live) {
    starts = (unsigned)__popcll(~rep[g] & live);
    if (width == 1) {
      leaves = (unsigned)__popcll(def[g] & live);
    } else {
      leaves = (unsigned)__popcll(leaf_pairs(def[2 * g], leaf_level) & spread_bits((uint32_t)live));
      if (live >> 32)
        leaves += (unsigned)__popcll(leaf_pairs(def[2 * g + 1], leaf_level) & spread_bits((uint32_t)(live >> 32)));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    starts += __shfl_down(starts, off, 64);
    leaves += __shfl_down(leaves, off, 64);
  }
  if (lane == 0) {
    tile_rows[t] = starts;
    tile_leaves[t] = leaves;
  }
}

__global__ __launch_bounds__(kBlock) void unpack_emit_kernel(const uint64_t *__restrict__ rep,
                                                              const uint64_t *__restrict__ def, int width,
                                                              uint64_t n_slots, int leaf_level, int max_def,
                                                              uint64_t rows, uint64_t leaves, uint64_t ntiles,
                                                              const unsigned *__restrict__ tile_rows,
                                                              const unsigned *__restrict__ tile_leaves,
                                                              int64_t *__restrict__ offsets,
                                                              unsigned long long *__restrict__ leaf_valid) {
  __shared__ unsigned long long sbits[kUnpackWaves][kUnpackWords];
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  const uint64_t t = (uint64_t)blockIdx.x * kUnpackWaves + w;
  const bool tile_live = t < ntiles;   // (wave-uniform; every wave of the block reaches the barriers)
  if (blockIdx.x == 0 && threadIdx.x == 0) offsets[rows] = (int64_t)leaves;
  for (unsigned k = lane; k < (unsigned)kUnpackWords; k += kWave) sbits[w][k] = 0ull;
  __syncthreads();
  uint64_t row_at = tile_live ? tile_rows[t] : 0, leaf_at = tile_live ? tile_leaves[t] : 0;
  const uint64_t leaf0 = leaf_at, word0 = leaf0 >> 6;
  const uint64_t lower = (1ull << lane) - 1ull;
  if (tile_live) {
    for (unsigned gi = 0; gi < kTile / 64; ++gi) {
      const uint64_t s0 = t * kTile + (uint64_t)gi * 64;
      if (s0 >= n_slots) break;   // (uniform)
      const uint64_t slot = s0 + lane;
      const bool live = slot < n_slots;
      unsigned d = 0;
      bool cont = false;
      if (live) {
        cont = (rep[slot >> 6] >> lane) & 1ull;
        d = width == 1 ? (unsigned)((def[slot >> 6] >> lane) & 1ull)
                       : (unsigned)((def[slot >> 5] >> ((slot & 31) * 2)) & 3ull);
      }
      const bool leaf = live && d >= (unsigned)leaf_level;
      const uint64_t startw = __ballot(live && !cont);
      const uint64_t leafw = __ballot(leaf);
      const uint64_t validw = __ballot(leaf && d == (unsigned)max_def);
      const uint64_t lrank = leaf_at + (uint64_t)__popcll(leafw & lower);
      if (live && !cont) {
        const uint64_t row = row_at + (uint64_t)__popcll(startw & lower);
        if (row < rows) offsets[row] = (int64_t)lrank;
      }
      if (leaf_valid != nullptr && ((validw >> lane) & 1ull) && lrank < leaves) {
        const uint64_t k = (lrank >> 6) - word0;   // < kUnpackWords: lrank - leaf0 < kTile
        if (k < (uint64_t)kUnpackWords) atomicOr(&sbits[w][k], 1ull << (lrank & 63));
      }
      row_at += (uint64_t)__popcll(startw);
      leaf_at += (uint64_t)__popcll(leafw);
    }
  }
  __syncthreads();
  if (tile_live && leaf_valid != nullptr) {
    const uint64_t nwords = (leaves + 63) / 64;
    const uint64_t leaf1 = leaf_at < leaves ? leaf_at : leaves;   // the tile's leaves: [leaf0, leaf1)
    for (unsigned k = lane; k < (unsigned)kUnpackWords; k += kWave) {
      const uint64_t wi = word0 + k;
      const unsigned long long v = sbits[w][k];
      if (wi >= nwords || wi * 64 >= leaf1) continue;
      if (wi * 64 >= leaf0 && (wi + 1) * 64 <= leaf1) leaf_valid[wi] = v;   // no other tile has a bit here
      else if (v != 0ull) atomicOr(&leaf_valid[wi], v);                      // shared with a neighbour tile
    }
  }
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pqlist_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  *bytes = (ntiles_of(n) + 1) * 8;
  return NVT_OK;
}

int nvt_pqlist_plan(const int64_t *offsets, const int64_t *origin, uint64_t n, uint64_t page_slots, uint64_t max_pages, uint64_t rep_cap,
                    uint64_t def_cap, uint64_t *slot_start, uint64_t *table, void *ws, uint64_t ws_bytes,
                    void *stream) {
  NVT_CHECK_ARG(offsets && origin && slot_start && table, "null pointer");
  NVT_CHECK_ARG(n > 0, "n must be positive");
  NVT_CHECK_ARG(page_slots > 0, "page_slots must be positive");
  NVT_CHECK_ARG(max_pages > 0, "max_pages must be positive");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace must be 8-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (ntiles_of(n) + 1) * 8, "workspace smaller than nvt_pqlist_ws_bytes(n)");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t nt = ntiles_of(n);
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(ws);
  NVT_PROF("pqlist_plan", (n + 1) * 32, s);
  slot_len_kernel<<<stream_grid(nt, 1), kBlock, 0, s>>>(offsets, n, slot_start, tot);
  NVT_CHECK_LAUNCH();
  scan_totals_kernel<<<1, kBlock, 0, s>>>(tot, nt);
  NVT_CHECK_LAUNCH();
  slot_add_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(slot_start, n, tot, offsets);
  NVT_CHECK_LAUNCH();
  pages_kernel<<<1, kBlock, 0, s>>>(offsets, origin, slot_start, n, page_slots, max_pages, rep_cap, def_cap, table);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_pqlist_pack_many(const nvt_pqlist_col *cols, int ncols, const int64_t *offsets, const int64_t *origin,
                         uint64_t n, const uint64_t *slot_start, const uint64_t *table, uint64_t max_pages,
                         uint64_t max_slots, uint8_t *rep_out, void *stream) {
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(ncols > 0, "ncols must be positive");
  NVT_CHECK_ARG(offsets && origin && slot_start && table && rep_out, "null pointer");
  NVT_CHECK_ARG(n > 0, "n must be positive");
  NVT_CHECK_ARG(max_pages > 0, "max_pages must be positive");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(rep_out) & 7) == 0, "rep_out must be 8-byte aligned");
  for (int i = 0; i < ncols; ++i) {
    NVT_CHECK_ARG(cols[i].def_out && cols[i].nonnull, "null pointer");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(cols[i].def_out) & 7) == 0, "def_out must be 8-byte aligned");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(cols[i].nonnull) & 7) == 0, "nonnull must be 8-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  // every tile lies inside one page: at most one partly filled tile per page
  const unsigned grid = stream_grid(ntiles_of(max_slots) + max_pages, 1);
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    PBatch b;
    memset(&b, 0, sizeof(b));
    b.ncols = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
    uint64_t bytes = (n + 1) * 16 + max_slots / 8;
    for (int j = 0; j < b.ncols; ++j) {
      const nvt_pqlist_col &c = cols[i0 + j];
      b.c[j] = PCol{c.leaf_valid, c.bit0, c.nbits, reinterpret_cast<uint64_t *>(c.def_out),
                    reinterpret_cast<unsigned long long *>(c.nonnull)};
      bytes += max_slots / 4 + (c.leaf_valid ? max_slots / 8 : 0);
      NVT_CHECK_HIP(hipMemsetAsync(c.nonnull, 0, max_pages * 8, s));
    }
    NVT_PROF("pqlist_pack_many", bytes, s);
    // (the repetition stream is the same for every column: the first batch writes it)
    pack_kernel<<<grid, kBlock, 0, s>>>(b, offsets, origin, slot_start, table,
                                        i0 == 0 ? reinterpret_cast<uint64_t *>(rep_out) : nullptr);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

static uint64_t unpack_tile_bytes(uint64_t ntiles) { return (ntiles * 4 + 255) & ~255ull; }

int nvt_pqlist_unpack_ws_bytes(uint64_t n_slots, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  const uint64_t nt = ntiles_of(n_slots);
  *bytes = 2 * unpack_tile_bytes(nt) + scan_chunks(nt) * 8 + 256;
  return NVT_OK;
}

int nvt_pqlist_unpack(const uint8_t *rep, const uint8_t *def, int def_width, uint64_t n_slots, int leaf_level,
                      int max_def, uint64_t rows, uint64_t leaves, int64_t *offsets, uint8_t *leaf_valid,
                      void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(offsets, "null offsets");
  NVT_CHECK_ARG(def_width == 1 || def_width == 2, "def_width is 1 or 2");
  NVT_CHECK_ARG(leaf_level == 1 || leaf_level == 2, "leaf_level is 1 or 2");
  NVT_CHECK_ARG(max_def == leaf_level || max_def == leaf_level + 1, "max_def is leaf_level (+ 1 for optional leaves)");
  NVT_CHECK_ARG((max_def == 1) == (def_width == 1), "def_width 1 goes with max_def 1");
  NVT_CHECK_ARG(n_slots < (1ull << 32), "fewer than 2^32 slots");
  NVT_CHECK_ARG(rows <= n_slots && leaves <= n_slots, "more rows or leaves than slots");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(offsets) & 7) == 0 && (reinterpret_cast<uintptr_t>(leaf_valid) & 7) == 0,
                "offsets / leaf_valid must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (leaf_valid != nullptr && leaves > 0) NVT_CHECK_HIP(hipMemsetAsync(leaf_valid, 0, ((leaves + 63) / 64) * 8, s));
  if (n_slots == 0) {   // no slots: every row (there should be none) is empty
    NVT_CHECK_HIP(hipMemsetAsync(offsets, 0, (rows + 1) * 8, s));
    return NVT_OK;
  }
  NVT_CHECK_ARG(rep && def && ws, "null pointer");
  NVT_CHECK_ARG(((reinterpret_cast<uintptr_t>(rep) | reinterpret_cast<uintptr_t>(def) |
                  reinterpret_cast<uintptr_t>(ws)) & 7) == 0, "rep / def / ws must be 8-byte aligned");
  const uint64_t nt = ntiles_of(n_slots);
  NVT_CHECK_ARG(ws_bytes >= 2 * unpack_tile_bytes(nt) + scan_chunks(nt) * 8 + 256,
                "workspace smaller than nvt_pqlist_unpack_ws_bytes(n_slots)");
  unsigned *tile_rows = reinterpret_cast<unsigned *>(ws);
  unsigned *tile_leaves = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(ws) + unpack_tile_bytes(nt));
  unsigned long long *chunk_tot =
      reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ws) + 2 * unpack_tile_bytes(nt));
  const uint64_t *r64 = reinterpret_cast<const uint64_t *>(rep), *d64 = reinterpret_cast<const uint64_t *>(def);
  NVT_PROF("pqlist_unpack", n_slots * (1 + def_width) / 8 + (rows + 1) * 8 + leaves / 8, s);
  const unsigned grid = (unsigned)((nt + kUnpackWaves - 1) / kUnpackWaves);
  unpack_count_kernel<<<grid, kBlock, 0, s>>>(r64, d64, def_width, n_slots, leaf_level, nt, tile_rows, tile_leaves);
  NVT_CHECK_LAUNCH();
  int rc = exclusive_scan_u32(tile_rows, nt, chunk_tot, s);
  if (rc) return rc;
  rc = exclusive_scan_u32(tile_leaves, nt, chunk_tot, s);
  if (rc) return rc;
  unpack_emit_kernel<<<grid, kBlock, 0, s>>>(r64, d64, def_width, n_slots, leaf_level, max_def, rows, leaves, nt,
                                             tile_rows, tile_leaves, offsets,
                                             reinterpret_cast<unsigned long long *>(leaf_valid));
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
