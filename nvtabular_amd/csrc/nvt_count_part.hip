// Path P of nvt_dense_count_* (paths 1 / 2 / 3): hash-partitioned counting for columns whose
// distinct keys do not fit one LDS table (int64 keys and weighted merges of any size; int32 keys
// take the range / sort paths first).
//   P0  per-workgroup LDS histogram of the top hash bits  -> bucket sizes
//   P0b scan -> exact bucket starts (no over-allocation, no overflow)
//   P1  scatter rows to 64 / 256 coarse buckets  (LDS-staged, 512 B contiguous runs)
//   P2  paths 2 / 3: scatter each coarse bucket to 64 / 256 fine buckets
//   P3  one workgroup per fine bucket (per chunk of a bucket a hot key inflated): LDS table count
//       -> staged results, copied out without atomics; P4 merges the chunks of split buckets
//   All occurrences of a key land in one fine bucket, so counts are exact and the only atomics
//   left are LDS ones plus one reservation per workgroup of P4.
//   HBM traffic: 6 x 4 B per row (3 reads + 2 writes + hist read) against 4 B algorithmic.
// With NVT_PATH_HOT (int32 keys, unweighted) the histogram pass also counts the rows of a sampled
// set of hot keys (nvt_hot_sample.hip) and switches them off for everything downstream.
#include <type_traits>

#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_lds_table.hpp"
#include "nvt_scan.hpp"

#ifndef NVT_SMALL_DIV
#define NVT_SMALL_DIV 4
#endif

namespace nvt {

// ---------------------------------------------------------------------------
// Path P
// ---------------------------------------------------------------------------
constexpr int kTile = 8192;        // rows per scatter tile (32 rows per thread)
constexpr int kChunk = 65536;      // rows one P3 workgroup counts
#ifndef NVT_COUNT_BS
#define NVT_COUNT_BS 512
#endif
constexpr int kCountBS = NVT_COUNT_BS;      // P3 workgroup size
constexpr int kMaxFine = 1 << 14;  // up to 6 + 8 hash bits
constexpr int kHistBlocks = 512;

template <typename K>
__device__ __forceinline__ uint32_t part_hash(K key) {
  // independent of the LDS-table hash (which uses bits >= 17 of slot_hash)
  return fmix32((uint32_t)slot_hash(key) * 0x9E3779B1u + 0x7F4A7C15u);
}

// P0, tile by tile (same kTile-row tiles as the P1 scatter).  Per tile: the histogram over
// the COARSE bucket (top b1 hash bits) goes to tile_hist[bucket * ntiles + tile]; after a
// device-wide exclusive scan of that bucket-major array every (tile, bucket) pair knows
// exactly where it writes, so P1 needs no cursor atomics (they cost half its time: 5.5 k
// tiles bumping the same 64-256 words) and the partition is deterministic.  Per workgroup:
// the histogram over the FINE bucket (top b1+b2 bits) for the bucket boundaries.
template <typename K>
__global__ __launch_bounds__(1024) void part_hist_kernel(const K *__restrict__ keys,
                                                           const uint8_t *__restrict__ valid,
                                                           const int64_t *__restrict__ weights,
                                                           uint64_t n, int b1, int bits,
                                                           unsigned *block_hist, unsigned *tile_hist,
                                                           uint64_t ntiles, uint64_t *state) {
  __shared__ unsigned h[kMaxFine];
  __shared__ unsigned ht[256];
  __shared__ unsigned long long s_nulls;
  const int nb = 1 << bits, nc = 1 << b1;
  for (int i = threadIdx.x; i < nb; i += 1024) h[i] = 0;
  if (threadIdx.x == 0) s_nulls = 0;
  unsigned long long nulls = 0;
  constexpr int VEC = DKey<K>::vec;
  constexpr int NV = kTile / VEC / 1024;  // 16-byte vectors per thread per tile (2 or 4)
  using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (threadIdx.x < 256) ht[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t row0 = tile * kTile;
    VecT pack[NV];
    unsigned vb[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row0 + ((uint64_t)u * 1024 + threadIdx.x) * VEC;
      vb[u] = 0x10000;  // not a full in-range vector
      if (i0 + VEC <= n) {
        pack[u] = *reinterpret_cast<const VecT *>(keys + i0);
        vb[u] = valid ? (unsigned)valid[i0 >> 3] : 0xFFu;  // raw bitmap byte, shifted later
      }
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row0 + ((uint64_t)u * 1024 + threadIdx.x) * VEC;
      K kv[VEC];
      unsigned bits_ok = 0, in_range = 0;
      if (!(vb[u] & 0x10000)) {
        if constexpr (sizeof(K) == 4) {
          kv[0] = pack[u].x;
          kv[1] = pack[u].y;
          kv[2] = pack[u].z;
          kv[3] = pack[u].w;
        } else {
          kv[0] = pack[u].x;
          kv[1] = pack[u].y;
        }
        bits_ok = (vb[u] >> (i0 & 7)) & ((1u << VEC) - 1u);
        in_range = (1u << VEC) - 1u;
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          kv[j] = 0;
          if (i0 + j < n) {
            in_range |= 1u << j;
            if (bit_valid(valid, i0 + j)) {
              kv[j] = keys[i0 + j];
              bits_ok |= 1u << j;
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if ((bits_ok >> j) & 1) {
          const unsigned fine = part_hash<K>(kv[j]) >> (32 - bits);
          atomicAdd(&ht[fine >> (bits - b1)], 1u);
          if (bits > b1) atomicAdd(&h[fine], 1u);
        }
      }
      const unsigned nmask = in_range & ~bits_ok;
      if (weights == nullptr) {
        nulls += __popc(nmask);
      } else if (nmask) {
        for (int j = 0; j < VEC; ++j)
          if ((nmask >> j) & 1) nulls += (unsigned long long)weights[i0 + j];
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
      const unsigned c = ht[threadIdx.x];
      tile_hist[(uint64_t)threadIdx.x * ntiles + tile] = c;
      if (bits == b1) h[threadIdx.x] += c;  // one level: fine == coarse
    }
    __syncthreads();
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 1024) block_hist[(uint64_t)blockIdx.x * nb + i] = h[i];
  // one device atomic per WORKGROUP (an atomic per wave on this single word serialised at the
  // memory side: +85 us on every column that has nulls)
  if (nulls) atomicAdd(&s_nulls, nulls);
  __syncthreads();
  if (threadIdx.x == 0 && s_nulls) atomicAdd((unsigned long long *)&state[DS_NULLS], s_nulls);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd((unsigned long long *)&state[DS_ROWS], (unsigned long long)n);
}

// ---- hot filter in front of paths 1 / 2 / 3 (int32 keys, unweighted) ----------------------------
// A power-law column sends 60-95 % of its rows to a few thousand keys (Criteo C1: 65 % of the
// rows carry one of the 14 k most frequent of 6.2 M keys).  Partitioning those rows is wasted
// work: they only need counters.  So the histogram pass also looks every key up in a read-only
// LDS table of "hot" keys; a hit is ONE LDS atomic and the row is switched off in the bitmap
// that the scatter / count stages see (they already skip null rows), a miss goes through the
// partition as before.  Everything downstream of the histogram then handles only the cold
// rows (measured with an ideal hot set, tools/coldfrac_probe.py: C1 595 -> 368 us, C11
// 495 -> 240 us incl. the plain histogram pass).
//   hot_sample_kernel   (nvt_hot_sample.hip) one workgroup picks the hot set from up to 64 blocks of 1024 rows
//                       spread over the column: keys seen twice first, then first come while
//                       there is room.  The table image is written once, so that every
//                       workgroup of the histogram pass holds the SAME slot layout and the
//                       per-workgroup counters can be summed slot by slot (no hash merge).
//                       A sample that the table would serve badly (< 1/8 of its rows) empties
//                       the image: the column then behaves exactly as without the filter.
//   part_hist_hot_kernel  part_hist_kernel + lookup + cold bitmap + per-workgroup hot counters
//   hot_reduce_kernel   column sums of the counters -> (key, count) entries appended to the
//                       output list behind the partition's entries
// The hot set is a heuristic; the result is exact for ANY hot set because a key is either in
// the image (all of its rows are counted by the counters) or not (all of them are partitioned).
// The table's geometry (kHotSlots, kHotWidth, NVT_HOT_WIDTH) is in nvt_lds_table.hpp.
constexpr int kHotBlocks = 256;         // histogram workgroups (one per CU: 130 KiB of LDS each)

// slot of `key` in its bucket (already loaded), or -1
__device__ __forceinline__ int hot_find(const int2 &b, int32_t key, uint32_t base) {
  int slot = -1;
  slot = b.x == key ? (int)base : slot;
  slot = b.y == key ? (int)base + 1 : slot;
  return slot;
}
__device__ __forceinline__ int hot_find(const int4 &b, int32_t key, uint32_t base) {
  int slot = -1;
  slot = b.x == key ? (int)base : slot;
  slot = b.y == key ? (int)base + 1 : slot;
  slot = b.z == key ? (int)base + 2 : slot;
  slot = b.w == key ? (int)base + 3 : slot;
  return slot;
}

// part_hist_kernel for int32 keys without weights, with the hot-key lookup (see above).
// cold[] is an Arrow bitmap over whole tiles: bit = row valid AND key not hot.
__global__ __launch_bounds__(1024) void part_hist_hot_kernel(
    const int32_t *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n, int b1,
    int bits, const int32_t *__restrict__ image, unsigned *block_hist, unsigned *tile_hist,
    uint64_t ntiles, uint8_t *cold, unsigned *hot_cnt, uint64_t *state) {
  using K = int32_t;
  constexpr K EMPTY = DKey<K>::empty;
  __shared__ unsigned h[kMaxFine];
  using BucketT = std::conditional<kHotWidth == 4, int4, int2>::type;
  __shared__ BucketT tk[kHotBuckets];
  __shared__ unsigned tc[kHotSlots];
  __shared__ unsigned ht[256];
  __shared__ unsigned long long s_nulls;
  const int nb = 1 << bits, nc = 1 << b1;
  for (int i = threadIdx.x; i < nb; i += 1024) h[i] = 0;
  for (int i = threadIdx.x; i < kHotBuckets; i += 1024)
    tk[i] = reinterpret_cast<const BucketT *>(image)[i];
  for (int i = threadIdx.x; i < kHotSlots; i += 1024) tc[i] = 0;
  if (threadIdx.x == 0) s_nulls = 0;
  unsigned long long nulls = 0;
  constexpr int VEC = 4;
  constexpr int NV = kTile / VEC / 1024;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if (threadIdx.x < 256) ht[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t row0 = tile * kTile;
    int4 pack[NV];
    unsigned vb[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row0 + ((uint64_t)u * 1024 + threadIdx.x) * VEC;
      vb[u] = 0x10000;  // not a full in-range vector
      if (i0 + VEC <= n) {
        pack[u] = *reinterpret_cast<const int4 *>(keys + i0);
        vb[u] = valid ? (unsigned)valid[i0 >> 3] : 0xFFu;
      }
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row0 + ((uint64_t)u * 1024 + threadIdx.x) * VEC;
      K kv[VEC];
      unsigned bits_ok = 0, in_range = 0;
      if (!(vb[u] & 0x10000)) {
        kv[0] = pack[u].x;
        kv[1] = pack[u].y;
        kv[2] = pack[u].z;
        kv[3] = pack[u].w;
        bits_ok = (vb[u] >> (i0 & 7)) & 0xFu;
        in_range = 0xFu;
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          kv[j] = 0;
          if (i0 + j < n) {
            in_range |= 1u << j;
            if (bit_valid(valid, i0 + j)) {
              kv[j] = keys[i0 + j];
              bits_ok |= 1u << j;
            }
          }
        }
      }
      // the buckets of all keys of the vector are requested before any of them is used
      BucketT bk[VEC];
      uint32_t sa[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        sa[j] = hot_bucket(kv[j]);
        bk[j] = tk[sa[j]];
      }
      unsigned cold_bits = 0;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if ((bits_ok >> j) & 1) {
          const K key = kv[j];
          const int slot = hot_find(bk[j], key, kHotWidth * sa[j]);
          if (slot >= 0 && key != EMPTY) {
            atomicAdd(&tc[slot], 1u);
          } else {
            cold_bits |= 1u << j;
            const unsigned fine = part_hash<K>(key) >> (32 - bits);
            atomicAdd(&ht[fine >> (bits - b1)], 1u);
            if (bits > b1) atomicAdd(&h[fine], 1u);
          }
        }
      }
      nulls += __popc(in_range & ~bits_ok);
      // one bitmap byte = the vectors of two neighbouring lanes (i0 is a multiple of 4)
      const unsigned other = __shfl_xor(cold_bits, 1, 64);
      if ((threadIdx.x & 1) == 0) cold[i0 >> 3] = (uint8_t)(cold_bits | (other << 4));
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
      const unsigned c = ht[threadIdx.x];
      tile_hist[(uint64_t)threadIdx.x * ntiles + tile] = c;
      if (bits == b1) h[threadIdx.x] += c;
    }
    __syncthreads();
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 1024) block_hist[(uint64_t)blockIdx.x * nb + i] = h[i];
  for (int i = threadIdx.x; i < kHotSlots; i += 1024)
    hot_cnt[(uint64_t)blockIdx.x * kHotSlots + i] = tc[i];
  if (nulls) atomicAdd(&s_nulls, nulls);
  __syncthreads();
  if (threadIdx.x == 0 && s_nulls) atomicAdd((unsigned long long *)&state[DS_NULLS], s_nulls);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd((unsigned long long *)&state[DS_ROWS], (unsigned long long)n);
}

// column sums of the per-workgroup hot counters -> entries appended to the output list.
// 64 slots per workgroup x 16 groups of counter rows: every thread sums nblocks / 16 values
// with all loads in flight (one thread per slot walking 256 rows took 100 us).
constexpr int kHotRedGroups = 16;
__global__ __launch_bounds__(64 * kHotRedGroups) void hot_reduce_kernel(
    const int32_t *__restrict__ image, const unsigned *__restrict__ hot_cnt, int nblocks,
    int32_t *out_keys, int64_t *out_cnt, uint64_t out_cap, uint64_t *state) {
  constexpr int32_t EMPTY = DKey<int32_t>::empty;
  __shared__ unsigned long long part[kHotRedGroups][64];
  const unsigned l = threadIdx.x & 63, g = threadIdx.x >> 6;
  const unsigned slot = blockIdx.x * 64 + l;
  unsigned long long t = 0;
#pragma unroll 16
  for (int b = (int)g; b < nblocks; b += kHotRedGroups) t += hot_cnt[(uint64_t)b * kHotSlots + slot];
  part[g][l] = t;
  __syncthreads();
  if (g != 0) return;  // one wave finishes the 64 slots
  unsigned long long tot = 0;
#pragma unroll
  for (int q = 0; q < kHotRedGroups; ++q) tot += part[q][l];
  const int32_t key = image[slot];
  if (key == EMPTY) tot = 0;
  const unsigned long long peers = __ballot(tot > 0);
  const unsigned total = (unsigned)__popcll(peers);
  if (total == 0) return;
  unsigned long long b0 = 0;
  if (l == 0) b0 = atomicAdd((unsigned long long *)&state[DS_OUT], (unsigned long long)total);
  const unsigned long long base = __shfl(b0, 0, 64);
  if (base + total > out_cap) {
    if (l == 0) atomicOr((unsigned long long *)&state[DS_OVF], 2ull);
    return;
  }
  if (tot > 0) {
    const uint64_t pos = base + (unsigned)__popcll(peers & ((1ull << l) - 1ull));
    out_keys[pos] = key;
    out_cnt[pos] = (int64_t)tot;
  }
  unsigned long long mx = tot;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_down(mx, off, 64);
    mx = o > mx ? o : mx;
  }
  if (l == 0 && mx > 0) {
    unsigned long long *gm = reinterpret_cast<unsigned long long *>(&state[NVT_ST_MAXCOUNT]);
    if (mx > __hip_atomic_load(gm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(gm, mx);
  }
}

// P0b-1: bucket totals = column sums of the per-block histograms.  64 bins x 16 row groups
// per workgroup; loads are coalesced across bins, 16 in flight per lane, 2 batches per lane
// (with 4 row groups the 128-deep per-lane chain made this 31 us for 512 KB of input).
constexpr int kReduceGroups = 16;
__global__ __launch_bounds__(64 * kReduceGroups) void part_reduce_kernel(
    const unsigned *__restrict__ block_hist, int nblocks, int nb, unsigned long long *totals) {
  __shared__ unsigned long long part[kReduceGroups][64];
  const int f = blockIdx.x * 64 + (threadIdx.x & 63);
  const int g = threadIdx.x >> 6;
  unsigned long long t = 0;
  if (f < nb) {
#pragma unroll 16
    for (int b = g; b < nblocks; b += kReduceGroups) t += block_hist[(uint64_t)b * nb + f];
  }
  part[g][threadIdx.x & 63] = t;
  __syncthreads();
  if (g == 0 && f < nb) {
    unsigned long long tot = 0;
#pragma unroll
    for (int k = 0; k < kReduceGroups; ++k) tot += part[k][threadIdx.x];
    totals[f] = tot;
  }
}

// P0b-2: exclusive scan -> exact bucket starts, cursors, per-coarse tile starts. One block.
__global__ __launch_bounds__(1024) void part_scan_kernel(const unsigned long long *__restrict__ totals,
                                                         int bits, int b1,
                                                         unsigned long long *fine_start,
                                                         unsigned long long *fine_cursor,
                                                         unsigned long long *coarse_cursor,
                                                         unsigned *tile_start,
                                                         unsigned *chunk_start,
                                                         unsigned *pchunk_start,
                                                         unsigned long long chunk_rows,
                                                         unsigned long long small_rows) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry;
  const int nb = 1 << bits;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    int f = base + threadIdx.x;
    unsigned long long v = f < nb ? totals[f] : 0, inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned long long o = __shfl_up(inc, off, 64);
      if (lane_id() >= (unsigned)off) inc += o;
    }
    const unsigned w = threadIdx.x / kWave;
    if (lane_id() == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long wb = carry;
    for (unsigned k = 0; k < w; ++k) wb += wsum[k];
    if (f < nb) {
      fine_start[f] = wb + inc - v;
      fine_cursor[f] = wb + inc - v;
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry = wb + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) fine_start[nb] = carry;
  __syncthreads();
  const int nc = 1 << b1, sub = nb >> b1;
  if ((int)threadIdx.x < nc) coarse_cursor[threadIdx.x] = fine_start[threadIdx.x * sub];
  {  // per-coarse-bucket tile counts -> exclusive scan (nc <= 256: one value per thread; a
     // serial loop over dependent global loads here cost 25 us per column)
    __shared__ unsigned tcnt[256];
    if ((int)threadIdx.x < nc) {
      const unsigned long long sz =
          fine_start[(threadIdx.x + 1) * sub] - fine_start[threadIdx.x * sub];
      tcnt[threadIdx.x] = (unsigned)((sz + kTile - 1) / kTile);
    }
    __syncthreads();
    if (threadIdx.x < kWave) {  // one wave scans the <= 256 counts, 4 per lane
      unsigned v[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (int)threadIdx.x * 4 + j;
        v[j] = c < nc ? tcnt[c] : 0;
        tot += v[j];
      }
      unsigned inc = tot;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        unsigned o = __shfl_up(inc, off, 64);
        if (lane_id() >= (unsigned)off) inc += o;
      }
      unsigned run = inc - tot;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (int)threadIdx.x * 4 + j;
        if (c < nc) tile_start[c] = run;
        run += v[j];
      }
      if (threadIdx.x == kWave - 1) tile_start[nc] = inc;
    }
  }
  // P3 work list: a fine bucket is processed as one primary chunk of chunk_rows plus, when a
  // hot key drags its whole bucket (skew), excess chunks of small_rows; such "split" buckets
  // get one partial-list region per chunk, merged per bucket by P4.  Two more block scans.
  __syncthreads();
  __shared__ unsigned long long wsum2[16][2];
  __shared__ unsigned long long carry2[2];
  if (threadIdx.x == 0) carry2[0] = carry2[1] = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    int f = base + threadIdx.x;
    unsigned long long sz = f < nb ? fine_start[f + 1] - fine_start[f] : 0;
    // primary chunk of chunk_rows, the excess (skew) in chunks of small_rows
    unsigned long long k = sz <= chunk_rows ? (sz > 0)
                                            : 1 + (sz - chunk_rows + small_rows - 1) / small_rows;
    unsigned long long v0 = k, v1 = (k > 1) ? k : 0, i0 = v0, i1 = v1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned long long o0 = __shfl_up(i0, off, 64), o1 = __shfl_up(i1, off, 64);
      if (lane_id() >= (unsigned)off) {
        i0 += o0;
        i1 += o1;
      }
    }
    const unsigned w = threadIdx.x / kWave;
    if (lane_id() == 63) {
      wsum2[w][0] = i0;
      wsum2[w][1] = i1;
    }
    __syncthreads();
    unsigned long long b0 = carry2[0], b1c = carry2[1];
    for (unsigned q = 0; q < w; ++q) {
      b0 += wsum2[q][0];
      b1c += wsum2[q][1];
    }
    if (f < nb) {
      chunk_start[f] = (unsigned)(b0 + i0 - v0);
      pchunk_start[f] = (unsigned)(b1c + i1 - v1);
    }
    __syncthreads();
    if (threadIdx.x == 1023) {
      carry2[0] = b0 + i0;
      carry2[1] = b1c + i1;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    chunk_start[nb] = (unsigned)carry2[0];
    pchunk_start[nb] = (unsigned)carry2[1];
  }
}

// P1 / P2: LDS-staged scatter of one tile of rows into 2^nbits buckets.
//   LEVEL 1: tile t covers input rows [t*kTile, ...); bucket = top b1 bits of the hash.
//   LEVEL 2: tiles are laid out per coarse bucket (tile_start); bucket = the next nbits.
template <typename K, int LEVEL, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void part_scatter_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid,
    const int64_t *__restrict__ weights, uint64_t n, int b1, int nbits,
    const unsigned long long *__restrict__ fine_start, unsigned long long *cursor,
    const unsigned *__restrict__ tile_start, const unsigned *__restrict__ tile_off,
    const unsigned long long *__restrict__ tile_off_base, K *__restrict__ out_keys,
    int64_t *__restrict__ out_w) {
  constexpr int ROWS = kTile / kBlock;
  __shared__ K stage[kTile];
  __shared__ unsigned lcnt[256], loff[256];
  __shared__ unsigned long long gbase[256];
  __shared__ uint64_t seg_lo, seg_hi;
  __shared__ int coarse_s;
  const int nbk = 1 << nbits;
  if (LEVEL == 1) {
    if (threadIdx.x == 0) {
      seg_lo = (uint64_t)blockIdx.x * kTile;
      seg_hi = seg_lo + kTile < n ? seg_lo + kTile : n;
      coarse_s = 0;
    }
  } else {
    if (threadIdx.x == 0) {
      const int nc = 1 << b1;
      int c = -1;
      if (blockIdx.x < tile_start[nc]) {
        int lo = 0, hi = nc - 1;  // last c with tile_start[c] <= blockIdx.x
        while (lo < hi) {
          int mid = (lo + hi + 1) >> 1;
          if (tile_start[mid] <= blockIdx.x) lo = mid; else hi = mid - 1;
        }
        c = lo;
      }
      coarse_s = c;
      if (c >= 0) {
        const int sub = nbk;
        uint64_t cs = fine_start[(uint64_t)c * sub], ce = fine_start[(uint64_t)(c + 1) * sub];
        seg_lo = cs + (uint64_t)(blockIdx.x - tile_start[c]) * kTile;
        seg_hi = seg_lo + kTile < ce ? seg_lo + kTile : ce;
      }
    }
  }
  if (threadIdx.x < 256) lcnt[threadIdx.x] = 0;
  __syncthreads();
  if (LEVEL == 2 && coarse_s < 0) return;
  const uint64_t lo = seg_lo, hi = seg_hi;
  const int shift = (LEVEL == 1) ? (32 - b1) : (32 - b1 - nbits);
  const uint32_t mask = (uint32_t)nbk - 1;

  constexpr int RSLOTS = ROWS + (LEVEL == 2 ? 1 : 0);  // LEVEL 2: + one row of the overhang
  K k[RSLOTS];
  unsigned pos[RSLOTS];
  unsigned short bk[RSLOTS];
  // row handled by register slot r.  LEVEL 1 reads the (16-byte aligned) input column with
  // one 16-byte load per lane and takes the VEC validity bits from a single bitmap byte;
  // LEVEL 2 segments start anywhere, so they are read element-wise.
  constexpr int VEC = DKey<K>::vec;
  // LEVEL 2 segments start anywhere: they are read with 16-byte loads from the aligned
  // address below `lo` (rows outside [lo, hi) masked off); the up to VEC - 1 rows this pushes
  // past the last full vector are the "overhang", one per thread 0 .. VEC-2, in slot ROWS.
  // (Element-wise loads issued 4x the load instructions: 174 us against 94 us for LEVEL 1.)
  const uint64_t a0 = LEVEL == 1 ? lo : (lo & ~(uint64_t)(VEC - 1));
  auto row_of = [&](int r) -> uint64_t {
    if (r == ROWS) return a0 + (uint64_t)kTile + threadIdx.x;  // overhang (LEVEL 2 only)
    return a0 + ((uint64_t)(r / VEC) * kBlock + threadIdx.x) * VEC + (r % VEC);
  };
  if (LEVEL == 1) {
    using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
    constexpr int NV = ROWS / VEC;
    VecT pack[NV];
    unsigned vraw[NV];
    // phase 1: issue every load of the tile (keys + raw bitmap bytes), no dependent math
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row_of(u * VEC);
      vraw[u] = 0x10000;  // not a full in-range vector
      if (i0 + VEC <= hi) {
        pack[u] = *reinterpret_cast<const VecT *>(keys + i0);
        vraw[u] = valid ? (unsigned)valid[i0 >> 3] : 0xFFu;
      }
    }
    // phase 2: bucket + rank
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row_of(u * VEC);
      unsigned vb = 0;
      K kv[VEC];
      if (!(vraw[u] & 0x10000)) {
        if constexpr (sizeof(K) == 4) {
          kv[0] = pack[u].x;
          kv[1] = pack[u].y;
          kv[2] = pack[u].z;
          kv[3] = pack[u].w;
        } else {
          kv[0] = pack[u].x;
          kv[1] = pack[u].y;
        }
        vb = (vraw[u] >> (i0 & 7)) & ((1u << VEC) - 1u);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          kv[j] = 0;
          if (i0 + j < hi && bit_valid(valid, i0 + j)) {
            kv[j] = keys[i0 + j];
            vb |= 1u << j;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int r = u * VEC + j;
        bk[r] = 0xFFFF;
        k[r] = kv[j];
        if ((vb >> j) & 1) {
          unsigned b = (part_hash<K>(kv[j]) >> shift) & mask;
          bk[r] = (unsigned short)b;
          pos[r] = atomicAdd(&lcnt[b], 1u);
        }
      }
    }
  } else {
    using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
    constexpr int NV = ROWS / VEC;
    VecT pack[NV];
    bool full[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row_of(u * VEC);
      full[u] = i0 < hi && i0 + VEC <= n;  // the 16 bytes exist (n = length of the buffer)
      if (full[u]) pack[u] = *reinterpret_cast<const VecT *>(keys + i0);
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const uint64_t i0 = row_of(u * VEC);
      K kv[VEC];
      if (full[u]) {
        if constexpr (sizeof(K) == 4) {
          kv[0] = pack[u].x;
          kv[1] = pack[u].y;
          kv[2] = pack[u].z;
          kv[3] = pack[u].w;
        } else {
          kv[0] = pack[u].x;
          kv[1] = pack[u].y;
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) kv[j] = (i0 + j >= lo && i0 + j < hi) ? keys[i0 + j] : (K)0;
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int r = u * VEC + j;
        bk[r] = 0xFFFF;
        k[r] = kv[j];
        if (i0 + j >= lo && i0 + j < hi) {
          unsigned b = (part_hash<K>(kv[j]) >> shift) & mask;
          bk[r] = (unsigned short)b;
          pos[r] = atomicAdd(&lcnt[b], 1u);
        }
      }
    }
    {  // overhang rows a0 + kTile .. a0 + kTile + VEC - 2
      const uint64_t i = row_of(ROWS);
      bk[ROWS] = 0xFFFF;
      k[ROWS] = (K)0;
      if (threadIdx.x < VEC - 1 && i >= lo && i < hi) {
        k[ROWS] = keys[i];
        unsigned b = (part_hash<K>(k[ROWS]) >> shift) & mask;
        bk[ROWS] = (unsigned short)b;
        pos[ROWS] = atomicAdd(&lcnt[b], 1u);
      }
    }
  }
  __syncthreads();
  // exclusive scan of lcnt over the block (kBlock == 256 >= buckets) + global reservation
  {
    __shared__ unsigned ws4[kBlock / kWave];
    const unsigned v = (int)threadIdx.x < nbk ? lcnt[threadIdx.x] : 0;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o = __shfl_up(inc, off, 64);
      if (lane_id() >= (unsigned)off) inc += o;
    }
    const unsigned w = threadIdx.x / kWave;
    if (lane_id() == 63) ws4[w] = inc;
    __syncthreads();
    unsigned add = 0;
    for (unsigned q = 0; q < w; ++q) add += ws4[q];
    loff[threadIdx.x] = add + inc - v;
    if ((int)threadIdx.x < nbk && v) {
      if (LEVEL == 1) {
        // exact offset of this (tile, bucket) from the scanned per-tile histograms
        gbase[threadIdx.x] =
            scan_lookup(tile_off, tile_off_base, (uint64_t)threadIdx.x * gridDim.x + blockIdx.x);
      } else {
        unsigned long long *cur = cursor + (uint64_t)coarse_s * nbk;
        gbase[threadIdx.x] = atomicAdd(&cur[threadIdx.x], (unsigned long long)v);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RSLOTS; ++r)
    if (bk[r] != 0xFFFF) stage[loff[bk[r]] + pos[r]] = k[r];
  __syncthreads();
  const unsigned total = loff[nbk - 1] + lcnt[nbk - 1];
  for (unsigned i = threadIdx.x; i < total; i += kBlock) {
    K key = stage[i];
    unsigned b = (part_hash<K>(key) >> shift) & mask;
    out_keys[gbase[b] + (i - loff[b])] = key;
  }
  if (WEIGHTED) {
    // weights ride along: same destination, recomputed from (bucket, pos)
#pragma unroll
    for (int r = 0; r < RSLOTS; ++r) {
      if (bk[r] != 0xFFFF) out_w[gbase[bk[r]] + pos[r]] = weights[row_of(r)];
    }
  }
}

// P3: one workgroup per (fine bucket, chunk of kChunk rows).  Single-chunk buckets go
// straight to the output list; chunks of split buckets write partial lists for P4.
template <typename K, bool WEIGHTED, int SLOTS, int BS>
__global__ __launch_bounds__(BS) void part_count_kernel(
    const K *__restrict__ keys, const int64_t *__restrict__ weights,
    const unsigned long long *__restrict__ fine_start, const unsigned *__restrict__ chunk_start,
    const unsigned *__restrict__ pchunk_start, int nb, uint64_t chunk_rows, uint64_t small_rows,
    K *part_keys, int64_t *part_cnt, unsigned *part_len, K *tmp_keys, int64_t *tmp_cnt, unsigned *blk_cnt,
    unsigned long long *blk_lo, uint64_t *state) {
  constexpr K EMPTY = DKey<K>::empty;
  using C = typename std::conditional<WEIGHTED, unsigned long long, unsigned>::type;
  __shared__ K lkeys[SLOTS];
  __shared__ C lcnt[SLOTS];
  __shared__ unsigned lfill, lovf;
  __shared__ unsigned long long s_sent;
  __shared__ int s_f;
  __shared__ unsigned s_j;
  // Unit order = dispatch order: the nb primary chunks first (one per bucket), then the small
  // excess chunks of split buckets, which fill the tail.  (With equal-size chunks a hot
  // bucket's ~30 extra units started a whole second round on the 256 CUs: +130 us per column.)
  if (threadIdx.x == 0) {
    int f = -1;
    unsigned j = 0;
    if ((int)blockIdx.x < nb) {
      if (chunk_start[blockIdx.x + 1] > chunk_start[blockIdx.x]) f = (int)blockIdx.x;
    } else {
      const unsigned p = blockIdx.x - (unsigned)nb;  // index into the split buckets' regions
      if (p < pchunk_start[nb]) {
        int lo = 0, hi = nb - 1;  // last f with pchunk_start[f] <= p (skips unsplit buckets)
        while (lo < hi) {
          int mid = (lo + hi + 1) >> 1;
          if (pchunk_start[mid] <= p) lo = mid; else hi = mid - 1;
        }
        j = p - pchunk_start[lo];
        if (j > 0) f = lo;  // j == 0 is the primary chunk, already a unit of its own
      }
    }
    s_f = f;
    s_j = j;
    lfill = 0;
    lovf = 0;
    s_sent = 0;
  }
  __syncthreads();
  const int f = s_f;
  if (f < 0) {
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = 0;
    return;
  }
  for (int i = threadIdx.x; i < SLOTS; i += BS) {
    lkeys[i] = EMPTY;
    lcnt[i] = 0;
  }
  __syncthreads();
  const unsigned j = s_j;
  const unsigned nchunks = chunk_start[f + 1] - chunk_start[f];
  const uint64_t end = fine_start[f + 1];
  const uint64_t lo = fine_start[f] + (j == 0 ? 0 : chunk_rows + (uint64_t)(j - 1) * small_rows);
  const uint64_t span = j == 0 ? chunk_rows : small_rows;
  const uint64_t hi = lo + span < end ? lo + span : end;
  bool failed = false;
  unsigned long long my_sent = 0;
  // Split buckets exist because of a hot key, and in their chunks most lanes of every wave
  // would add to the SAME LDS word (a 64-way same-address conflict serialises the atomic:
  // such chunks ran ~4x slower per row).  Sample 64 rows of the chunk; a key holding >= 25 %
  // of the sample is counted in a per-lane register instead and added once per wave.
  __shared__ K s_hk;
  __shared__ int s_has_hk;
  K hk = EMPTY;
  bool has_hk = false;
  if (nchunks > 1) {  // workgroup-uniform
    if (threadIdx.x < kWave) {
      const K smp = keys[lo + ((hi - lo) * threadIdx.x) / kWave];
      K best = EMPTY;
      int bestc = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const K cand = __shfl(smp, c * 16 + 5, 64);
        const int m = __popcll(__ballot(smp == cand));
        if (m > bestc) {
          bestc = m;
          best = cand;
        }
      }
      if (threadIdx.x == 0) {
        s_has_hk = (bestc >= 16 && best != EMPTY) ? 1 : 0;
        s_hk = best;
      }
    }
    __syncthreads();
    has_hk = s_has_hk != 0;
    hk = s_hk;
  }
  unsigned long long my_hot = 0;
  auto add_one = [&](K key, unsigned long long w) {
    if (key == EMPTY) {
      my_sent += w;
      return;
    }
    if (has_hk && key == hk) {
      my_hot += w;
      return;
    }
    if (!lds_add<K, C, SLOTS>(lkeys, lcnt, &lfill, key, (C)w, part_hash<K>(key))) failed = true;
  };
  if constexpr (!WEIGHTED) {
    // bucket segments start anywhere: peel to a 16-byte boundary, then 16-byte loads (the
    // element-wise version issued 4x the load instructions and ran at half the speed of the
    // stage-1 kernel on the same number of rows per CU)
    constexpr int VEC = DKey<K>::vec;
    using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
    const uint64_t head = (lo + VEC - 1) / VEC * VEC < hi ? (lo + VEC - 1) / VEC * VEC : hi;
    const uint64_t body_end = head + (hi - head) / VEC * VEC;
    for (uint64_t i = lo + threadIdx.x; i < head; i += BS) add_one(keys[i], 1ull);
    for (uint64_t i = body_end + threadIdx.x; i < hi; i += BS) add_one(keys[i], 1ull);
    const VecT *vk = reinterpret_cast<const VecT *>(keys + head);
    const uint64_t nvec = (body_end - head) / VEC;
    constexpr int U = 4;
    for (uint64_t v0 = threadIdx.x; v0 < nvec; v0 += (uint64_t)BS * U) {
      if (lfill > (unsigned)max_fill(SLOTS)) break;
      VecT pack[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t v = v0 + (uint64_t)u * BS;
        if (v < nvec) pack[u] = vk[v];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (v0 + (uint64_t)u * BS >= nvec) continue;
        if constexpr (sizeof(K) == 4) {
          add_one(pack[u].x, 1ull);
          add_one(pack[u].y, 1ull);
          add_one(pack[u].z, 1ull);
          add_one(pack[u].w, 1ull);
        } else {
          add_one(pack[u].x, 1ull);
          add_one(pack[u].y, 1ull);
        }
      }
    }
  } else {
    constexpr int U = 8;
    for (uint64_t i0 = lo + threadIdx.x; i0 < hi; i0 += (uint64_t)BS * U) {
      if (lfill > (unsigned)max_fill(SLOTS)) break;
      K kk[U];
      unsigned long long ww[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint64_t i = i0 + (uint64_t)u * BS;
        ww[u] = 0;
        if (i < hi) {
          kk[u] = keys[i];
          ww[u] = (unsigned long long)weights[i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + (uint64_t)u * BS < hi) add_one(kk[u], ww[u]);
    }
  }
  if (has_hk) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) my_hot += __shfl_down(my_hot, off, 64);
    if (lane_id() == 0 && my_hot > 0 &&
        !lds_add<K, C, SLOTS>(lkeys, lcnt, &lfill, hk, (C)my_hot, part_hash<K>(hk)))
      failed = true;
  }
  if (failed) atomicOr(&lovf, 1u);
  if (my_sent) atomicAdd(&s_sent, my_sent);
  __syncthreads();
  if (lovf || lfill > (unsigned)max_fill(SLOTS)) {
    if (threadIdx.x == 0) {
      atomicOr((unsigned long long *)&state[DS_OVF], 1ull);
      blk_cnt[blockIdx.x] = 0;
    }
    return;
  }
  if (threadIdx.x == 0 && s_sent) atomicAdd((unsigned long long *)&state[DS_SENT], s_sent);
  if (nchunks == 1) {
    // No output cursor here: thousands of workgroups bumping one word serialise at the
    // memory side and made this kernel 2x slower.  The distinct keys of rows [lo, hi) fit in
    // tmp[lo, hi); part_offsets_kernel / part_copy_kernel pack the pieces afterwards.
    if (threadIdx.x == 0) blk_lo[blockIdx.x] = lo;
    lds_flush_region<K, C, BS, SLOTS>(lkeys, lcnt, tmp_keys + lo, tmp_cnt + lo,
                                      &blk_cnt[blockIdx.x], state);
  } else {
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = 0;
    const uint64_t region = (uint64_t)(pchunk_start[f] + j);
    lds_flush_region<K, C, BS, SLOTS>(lkeys, lcnt, part_keys + region * max_fill(SLOTS),
                                      part_cnt + region * max_fill(SLOTS), &part_len[region]);
  }
}

// P3b: exclusive scan of the per-workgroup result counts -> packed offsets; the total seeds
// the output cursor that P4 continues from.  One workgroup.
__global__ __launch_bounds__(1024) void part_offsets_kernel(const unsigned *__restrict__ blk_cnt,
                                                            unsigned nblk,
                                                            unsigned long long *blk_off,
                                                            uint64_t out_cap, uint64_t *state) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (unsigned base = 0; base < nblk; base += 1024) {
    unsigned i = base + threadIdx.x;
    unsigned long long v = i < nblk ? blk_cnt[i] : 0, inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned long long o = __shfl_up(inc, off, 64);
      if (lane_id() >= (unsigned)off) inc += o;
    }
    const unsigned w = threadIdx.x / kWave;
    if (lane_id() == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long wb = carry;
    for (unsigned k = 0; k < w; ++k) wb += wsum[k];
    if (i < nblk) blk_off[i] = wb + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = wb + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (carry > out_cap) atomicOr((unsigned long long *)&state[DS_OVF], 2ull);
    state[DS_OUT] = carry > out_cap ? 0 : carry;
  }
}

// P3c: pack every workgroup's staged result into the output list (coalesced copies)
template <typename K>
__global__ __launch_bounds__(kBlock) void part_copy_kernel(
    const K *__restrict__ tmp_keys, const int64_t *__restrict__ tmp_cnt,
    const unsigned *__restrict__ blk_cnt, const unsigned long long *__restrict__ blk_off,
    const unsigned long long *__restrict__ blk_lo, K *out_keys, int64_t *out_cnt,
    const uint64_t *__restrict__ state) {
  const unsigned cnt = blk_cnt[blockIdx.x];
  if (cnt == 0 || (state[DS_OVF] & 2)) return;
  const unsigned long long src = blk_lo[blockIdx.x], dst = blk_off[blockIdx.x];
  for (unsigned i = threadIdx.x; i < cnt; i += kBlock) {
    out_keys[dst + i] = tmp_keys[src + i];
    out_cnt[dst + i] = tmp_cnt[src + i];
  }
}

// P4: one workgroup per split bucket merges that bucket's per-chunk partial lists (same
// table geometry as P3, so whatever fitted there fits here).
template <typename K, typename C, int SLOTS>
__global__ __launch_bounds__(kStageBS) void part_merge_kernel(
    const unsigned *__restrict__ chunk_start, const unsigned *__restrict__ pchunk_start,
    const K *__restrict__ part_keys, const int64_t *__restrict__ part_cnt,
    const unsigned *__restrict__ part_len, K *out_keys, int64_t *out_cnt, uint64_t out_cap,
    unsigned long long *cursor, uint64_t *state) {
  constexpr K EMPTY = DKey<K>::empty;
  const int f = blockIdx.x;
  const unsigned nchunks = chunk_start[f + 1] - chunk_start[f];
  if (nchunks <= 1) return;
  // an earlier kernel of this call already overflowed: the result is discarded anyway
  // (and a full table would make every insert below walk kLdsProbe slots: 8 ms per launch)
  __shared__ K lkeys[SLOTS];
  __shared__ C lcnt[SLOTS];
  __shared__ unsigned lfill, lovf;
  __shared__ int s_skip;
  if (threadIdx.x == 0) {
    lfill = 0;
    lovf = 0;
    s_skip = (int)(__hip_atomic_load(&state[DS_OVF], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1);
  }
  __syncthreads();
  if (s_skip) return;  // workgroup-uniform
  for (int i = threadIdx.x; i < SLOTS; i += kStageBS) {
    lkeys[i] = EMPTY;
    lcnt[i] = 0;
  }
  __syncthreads();
  bool failed = false;
  // a wave per region, 4 independent loads in flight per lane: a hot bucket has ~200 short
  // regions, and walking them one after the other with the whole workgroup was a chain of
  // ~400 dependent global-load latencies (140 us)
  const unsigned lane = lane_id(), wv = threadIdx.x / kWave;
  constexpr int UM = 4;
  for (unsigned j = wv; j < nchunks; j += kStageBS / kWave) {
    const uint64_t region = (uint64_t)(pchunk_start[f] + j);
    const unsigned len = part_len[region];
    const K *pk = part_keys + region * max_fill(SLOTS);
    const int64_t *pc = part_cnt + region * max_fill(SLOTS);
    for (unsigned i0 = lane; i0 < len; i0 += kWave * UM) {
      if (lfill > (unsigned)max_fill(SLOTS)) break;  // filling up: the call fails below
      K kk[UM];
      int64_t cc[UM];
#pragma unroll
      for (int u = 0; u < UM; ++u) {
        const unsigned i = i0 + u * kWave;
        if (i < len) {
          kk[u] = pk[i];
          cc[u] = pc[i];
        }
      }
#pragma unroll
      for (int u = 0; u < UM; ++u)
        if (i0 + u * kWave < len &&
            !lds_add<K, C, SLOTS>(lkeys, lcnt, &lfill, kk[u], (C)cc[u], part_hash<K>(kk[u])))
          failed = true;
    }
  }
  if (failed) atomicOr(&lovf, 1u);
  __syncthreads();
  if (lovf || lfill > (unsigned)max_fill(SLOTS)) {
    if (threadIdx.x == 0) atomicOr((unsigned long long *)&state[DS_OVF], 1ull);
    return;
  }
  lds_flush<K, C, kStageBS, SLOTS>(lkeys, lcnt, out_keys, out_cnt, out_cap, cursor, state);
}

// ---- host side ------------------------------------------------------------------------------------
// Partitioned paths:
//   1: ONE level, 256 buckets, 16384-slot tables (int32 keys, unweighted; 8192 otherwise):
//      up to ~2.5 M distinct keys with a single scatter pass;
//   2: 64 x 64 buckets, 4096-slot tables (8192 when weighted)      up to ~9 M distinct;
//   3: 64 x 256 buckets, 8192-slot tables                          up to ~32 M distinct.
struct PathCfg {
  int b1, b2, slots;
  uint64_t chunk_rows;  // primary chunk of a bucket
  uint64_t small_rows;  // chunk size for a bucket's excess rows (skew)
};
// upper bounds on the partial-list regions of split buckets and on P3 work units
inline uint64_t max_regions_of(const PathCfg &c, uint64_t n) {
  return n / c.small_rows + n / c.chunk_rows + 2;  // excess chunks + one primary per split bucket
}
inline uint64_t max_units_of(const PathCfg &c, uint64_t n, int nb) {
  return (uint64_t)nb + max_regions_of(c, n);
}
inline PathCfg path_cfg(int path, int key_bytes, int weighted, uint64_t n) {
  const bool small = weighted || key_bytes == 8;
  if (path == 1) {
    // one workgroup per bucket in the common case: chunk = average bucket + 15 %, so only
    // buckets inflated by a hot key are split (and merged by P4)
    uint64_t chunk = (n / 256) + (n / 256) / 7 + 1;
    chunk = chunk < 65536 ? 65536 : (chunk > (1ull << 20) ? (1ull << 20) : chunk);
    // the excess of a bucket inflated by a hot key is cut into eighths, dispatched after all
    // primary chunks, so it fills the tail instead of starting a second round
    uint64_t small_rows = chunk / NVT_SMALL_DIV < 16384 ? 16384 : chunk / NVT_SMALL_DIV;
    return {8, 0, small ? kLdsSlots : kLdsSlotsBig, chunk, small_rows};
  }
  if (path == 2) return {6, 6, weighted ? kLdsSlots : 4096, (uint64_t)kChunk, (uint64_t)kChunk};
  return {6, 8, kLdsSlots, (uint64_t)kChunk, (uint64_t)kChunk};
}

// The workspace: one walk yields the size (base == nullptr) and the pointers.
struct PartCountWs {
  char *bufA, *bufB;
  int64_t *wA, *wB;
  unsigned *block_hist, *tile_start, *tile_hist;
  unsigned long long *scan_tot;
  unsigned long long *fine_start, *fine_cursor, *coarse_cursor, *totals;
  unsigned *chunk_start, *pchunk_start, *part_len;
  char *part_keys;
  int64_t *part_cnt;
  uint64_t max_regions;
  char *tmp_keys;      // [n] staged P3 results (row-range addressed)
  int64_t *tmp_cnt;    // [n]
  unsigned *blk_cnt;   // [t3 max]
  unsigned long long *blk_off, *blk_lo;
  // hot filter
  int32_t *hot_image;   // [kHotSlots] table image of the hot keys
  unsigned *hot_cnt;    // [kHotBlocks][kHotSlots] per-workgroup counters
  uint8_t *cold_bits;   // [ntiles * kTile / 8] valid AND not hot
};
static uint64_t part_count_ws_layout(int kind, bool hot, int key_bytes, bool weighted, uint64_t n,
                                     char *base, PartCountWs *ws) {
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    char *p = base ? base + off : nullptr;
    off += pad16(bytes);
    return p;
  };
  PartCountWs w;
  memset(&w, 0, sizeof(w));
  w.bufA = take(n * key_bytes);
  w.bufB = take(n * key_bytes);
  if (weighted) {
    w.wA = (int64_t *)take(n * 8);
    w.wB = (int64_t *)take(n * 8);
  }
  w.block_hist = (unsigned *)take((uint64_t)kHistBlocks * kMaxFine * 4);
  w.tile_start = (unsigned *)take(260 * 4);
  {
    const uint64_t ntiles = (n + kTile - 1) / kTile, len = 256 * ntiles;
    w.tile_hist = (unsigned *)take(len * 4);
    w.scan_tot = (unsigned long long *)take(scan_chunks(len) * 8 + 8);
  }
  w.fine_start = (unsigned long long *)take((kMaxFine + 1) * 8);
  w.fine_cursor = (unsigned long long *)take((kMaxFine + 1) * 8);
  w.coarse_cursor = (unsigned long long *)take(256 * 8);
  w.totals = (unsigned long long *)take((uint64_t)kMaxFine * 8);
  w.chunk_start = (unsigned *)take((kMaxFine + 1) * 4);
  w.pchunk_start = (unsigned *)take((kMaxFine + 1) * 4);
  const PathCfg cfg = path_cfg(kind, key_bytes, weighted, n);
  w.max_regions = max_regions_of(cfg, n);
  w.part_len = (unsigned *)take(w.max_regions * 4);
  w.part_keys = take(w.max_regions * max_fill(cfg.slots) * key_bytes);
  w.part_cnt = (int64_t *)take(w.max_regions * max_fill(cfg.slots) * 8);
  const uint64_t t3max = max_units_of(cfg, n, kMaxFine) + 1;
  w.tmp_keys = take(n * key_bytes);
  w.tmp_cnt = (int64_t *)take(n * 8);
  w.blk_cnt = (unsigned *)take(t3max * 4);
  w.blk_off = (unsigned long long *)take(t3max * 8);
  w.blk_lo = (unsigned long long *)take(t3max * 8);
  if (hot) {
    w.hot_image = (int32_t *)take(kHotSlots * 4);
    w.hot_cnt = (unsigned *)take((uint64_t)kHotBlocks * kHotSlots * 4);
    w.cold_bits = (uint8_t *)take((n + kTile - 1) / kTile * (kTile / 8));
  }
  *ws = w;
  return off;
}
uint64_t part_count_ws_bytes(int kind, bool hot, int key_bytes, bool weighted, uint64_t n) {
  PartCountWs w;
  return part_count_ws_layout(kind, hot, key_bytes, weighted, n, nullptr, &w);
}

// P1 and, with b2 > 0, P2: rows (`valid`: the column's bitmap, or the cold rows behind the hot
// filter) -> fine buckets.  *fine_keys / *fine_w: what P3 reads.
template <typename K, bool WEIGHTED>
static int part_scatter(const nvt_count_col &c, const uint8_t *valid, int b1, int b2, unsigned t1,
                        const unsigned long long *tile_base, const PartCountWs &w,
                        const K **fine_keys, const int64_t **fine_w, hipStream_t s) {
  part_scatter_kernel<K, 1, WEIGHTED><<<t1, kBlock, 0, s>>>(
      (const K *)c.keys, valid, c.weights, c.n, b1, b1, w.fine_start, w.coarse_cursor, w.tile_start,
      w.tile_hist, tile_base, (K *)w.bufA, w.wA);
  NVT_CHECK_LAUNCH();
  *fine_keys = (const K *)w.bufA;
  *fine_w = w.wA;
  if (b2) {
    const unsigned t2 = t1 + (1u << b1);  // upper bound: every coarse bucket rounds up once
    part_scatter_kernel<K, 2, WEIGHTED><<<t2, kBlock, 0, s>>>(
        (const K *)w.bufA, nullptr, w.wA, c.n, b1, b2, w.fine_start, w.fine_cursor, w.tile_start,
        nullptr, nullptr, (K *)w.bufB, w.wB);
    NVT_CHECK_LAUNCH();
    *fine_keys = (const K *)w.bufB;
    *fine_w = w.wB;
  }
  return NVT_OK;
}

// P3 (count per work unit), the atomic-free copy of its results and P4 (merge of split buckets)
// for tables of SLOTS slots with counts of type C, t3 = upper bound on the P3 units
template <typename K, bool WEIGHTED, typename C, int SLOTS, int BS>
static int part_count_merge(const nvt_count_col &c, const K *fine_keys, const int64_t *fine_w,
                            const PartCountWs &w, int bits, const PathCfg &cfg, unsigned t3,
                            hipStream_t s) {
  K *out_keys = (K *)c.out_keys;
  part_count_kernel<K, WEIGHTED, SLOTS, BS><<<t3, BS, 0, s>>>(
      fine_keys, fine_w, w.fine_start, w.chunk_start, w.pchunk_start, 1 << bits, cfg.chunk_rows,
      cfg.small_rows, (K *)w.part_keys, w.part_cnt, w.part_len, (K *)w.tmp_keys, w.tmp_cnt,
      w.blk_cnt, w.blk_lo, c.state);
  NVT_CHECK_LAUNCH();
  part_offsets_kernel<<<1, 1024, 0, s>>>(w.blk_cnt, t3, w.blk_off, c.out_capacity, c.state);
  NVT_CHECK_LAUNCH();
  part_copy_kernel<K><<<t3, kBlock, 0, s>>>((const K *)w.tmp_keys, w.tmp_cnt, w.blk_cnt, w.blk_off,
                                            w.blk_lo, out_keys, c.out_counts, c.state);
  NVT_CHECK_LAUNCH();
  part_merge_kernel<K, C, SLOTS><<<1u << bits, kStageBS, 0, s>>>(
      w.chunk_start, w.pchunk_start, (const K *)w.part_keys, w.part_cnt, w.part_len, out_keys,
      c.out_counts, c.out_capacity, reinterpret_cast<unsigned long long *>(c.state) + DS_OUT,
      c.state);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

template <typename K>
int part_count(const nvt_count_col &c, int kind, bool hot, hipStream_t s) {
  const K *keys = (const K *)c.keys;
  const uint8_t *valid = c.valid;
  const uint64_t n = c.n;
  const bool weighted = c.weights != nullptr;
  PartCountWs w;
  part_count_ws_layout(kind, hot, (int)sizeof(K), weighted, n, (char *)c.ws, &w);
  const PathCfg cfg = path_cfg(kind, (int)sizeof(K), weighted, n);
  const int b1 = cfg.b1, b2 = cfg.b2, bits = b1 + b2;
  const unsigned t1 = (unsigned)((n + kTile - 1) / kTile);
  const unsigned t3 = (unsigned)max_units_of(cfg, n, 1 << bits);  // upper bound on P3 units
  int hist_blocks = kHistBlocks;
  if (hot) {
    if constexpr (sizeof(K) == 4) {
      if (c.hot_image) {
        w.hot_image = c.hot_image;  // sampled by nvt_dense_count_many ahead of the pipelines
      } else {
        HotSampleBatch hb;
        hb.c[0] = {keys, valid, n, w.hot_image, 0, 0};
        int rc = hot_sample_launch(hb, 1, s);
        if (rc) return rc;
      }
      hist_blocks = kHotBlocks;
      part_hist_hot_kernel<<<kHotBlocks, 1024, 0, s>>>(keys, valid, n, b1, bits, w.hot_image,
                                                       w.block_hist, w.tile_hist, t1, w.cold_bits,
                                                       w.hot_cnt, c.state);
      NVT_CHECK_LAUNCH();
      valid = w.cold_bits;  // the scatter sees the cold rows only
    }
  } else {
    part_hist_kernel<K><<<kHistBlocks, 1024, 0, s>>>(keys, valid, c.weights, n, b1, bits,
                                                       w.block_hist, w.tile_hist, t1, c.state);
    NVT_CHECK_LAUNCH();
  }
  const unsigned long long *tile_base = nullptr;  // last scan step is done by the P1 scatter
  int rc = exclusive_scan_u32_deferred(w.tile_hist, ((uint64_t)1 << b1) * t1, w.scan_tot,
                                       &tile_base, s);
  if (rc) return rc;
  part_reduce_kernel<<<((1 << bits) + 63) / 64, 64 * kReduceGroups, 0, s>>>(
      w.block_hist, hist_blocks, 1 << bits, w.totals);
  NVT_CHECK_LAUNCH();
  part_scan_kernel<<<1, 1024, 0, s>>>(w.totals, bits, b1, w.fine_start, w.fine_cursor,
                                      w.coarse_cursor, w.tile_start, w.chunk_start,
                                      w.pchunk_start, cfg.chunk_rows, cfg.small_rows);
  NVT_CHECK_LAUNCH();
  const K *fine_keys = nullptr;
  const int64_t *fine_w = nullptr;
  rc = weighted ? part_scatter<K, true>(c, valid, b1, b2, t1, tile_base, w, &fine_keys, &fine_w, s)
                : part_scatter<K, false>(c, valid, b1, b2, t1, tile_base, w, &fine_keys, &fine_w, s);
  if (rc) return rc;
  if (weighted) {
    rc = part_count_merge<K, true, unsigned long long, kLdsSlots, kCountBS>(c, fine_keys, fine_w, w,
                                                                            bits, cfg, t3, s);
  } else if (cfg.slots == kLdsSlotsBig) {
    if constexpr (sizeof(K) == 4)
      rc = part_count_merge<K, false, unsigned, kLdsSlotsBig, 1024>(c, fine_keys, fine_w, w, bits,
                                                                    cfg, t3, s);
  } else if (cfg.slots == 4096) {
    rc = part_count_merge<K, false, unsigned, 4096, kCountBS>(c, fine_keys, fine_w, w, bits, cfg, t3, s);
  } else {
    rc = part_count_merge<K, false, unsigned, kLdsSlots, kCountBS>(c, fine_keys, fine_w, w, bits,
                                                                   cfg, t3, s);
  }
  if (rc) return rc;
  if (hot) {
    if constexpr (sizeof(K) == 4) {
      hot_reduce_kernel<<<kHotSlots / 64, 64 * kHotRedGroups, 0, s>>>(
          w.hot_image, w.hot_cnt, kHotBlocks, (int32_t *)c.out_keys, c.out_counts, c.out_capacity,
          c.state);
      NVT_CHECK_LAUNCH();
    }
  }
  return NVT_OK;
}
template int part_count<int32_t>(const nvt_count_col &, int, bool, hipStream_t);
template int part_count<int64_t>(const nvt_count_col &, int, bool, hipStream_t);

}  // namespace nvt
