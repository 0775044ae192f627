// Vocabulary order from a KEY-SORTED (key, count) list: ONE stable counting pass.
// The range path of the counting stage (nvt_range_count.hip) emits its list in key order and a
// histogram of cls = min(count, 255).  "count descending, key ascending" (categorify.py:1300,
// 1316) is then: class 255 (count >= 255; a few thousand entries of a 45 M-row power-law
// column, never more than rows / 255) in front, then classes 254 .. 1, every class in the key
// order it already has.  One stable scatter by class does that for all but the first class,
// whose entries are sorted afterwards by the (small) generic sort; the encode table is filled
// by the same scatter, where every entry learns its label.  Against the 7-pass radix sort +
// separate table build: 12 B read + 12 B written per entry instead of ~120, 4 launches
// instead of 11.
// Same tile geometry, ballot ranking and decoupled look-back as os_scatter_kernel of nvt_sort.hip
// (nvt_sort_tile.hpp holds what the two share).
//
// The parts, in the order of this file:
//  * class scatter (cls_scatter_body: cls_scatter_kernel for one vocabulary, cls_scatter_many_kernel
//    for the OrdBatch of a fit, label_shard_kernel for a shard of a list that several ranks own):
//    ordered (key, count) arrays, label_of[] = label of the entry at every position of the
//    key-sorted list, the entries of class 255 in front and still unlabelled (-1).
//  * the encode table of the vocabulary, one of three kinds:
//      hashed -- the scatter inserts every entry of the classes below 255 itself;
//      dumped -- the counting pass left {key, position} slots in key order.  Where it also recorded
//                the slot of every entry (src_slots), the scatter stores each label into that slot
//                and label_of[] is not written; otherwise (C-ABI callers without slots) range_patch*
//                stream over the table and replace the positions by label_of[position];
//      flat   -- laid out from the sorted keys by a prefix maximum (flat_params* + flat_build*,
//                also the groupby index of nvt_flat_index_build; read by nvt_flat_lookup.hip).
//  * the class-255 tail: sorted by nvt_sort.hip (one batched small sort for all vocabularies of a
//    call, vocab_order_tail_batch; a longer tail on its own), then range_fix_prefix* write the
//    labels first_label + j of the sorted entries into a dumped or flat table (encode_insert_any
//    into a hashed one).
//  * lists that arrive labelled (multi-GPU, vocab_from_labels): one scatter by label, then the
//    same table builds.
// All of it runs inside ONE workspace per vocabulary, described once by order_ws().
#include <vector>

#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"
#include "nvt_range.hpp"
#include "nvt_sort_tile.hpp"

namespace nvt {

__device__ __forceinline__ unsigned cls_digit(uint64_t comp) {
  const uint32_t cnt = ~(uint32_t)(comp >> 32);
  return 255u - (cnt < 255u ? cnt : 255u);
}

__device__ __forceinline__ void cls_scatter_body(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ cnts, uint64_t n,
    const unsigned *__restrict__ cls_hist, unsigned *status, unsigned *ticket, int32_t *out_keys,
    int64_t *out_cnts, unsigned long long *table, uint64_t mask, int64_t first_label,
    int64_t *sentinel_label, int32_t *label_of, int32_t *big_src = nullptr,
    const uint32_t *__restrict__ src_slots = nullptr, unsigned long long *slot_table = nullptr,
    uint64_t nslots = 0) {
  // src_slots set (a dumped range table whose counting pass recorded the slot of every entry): the
  // label goes straight into the high word of slot_table[src_slots[i]], label_of[] is not written
  // big_src set (a SHARD of a list that several ranks own, nvt_vocab_label_shard): only the
  // entries of class 255 are written out (compacted in key order at the front of out_*, with
  // their positions in the shard), every other entry only gets its label
  constexpr int NW = kS2BS / kWave;
  __shared__ unsigned wcnt[NW][256];
  __shared__ unsigned goff[256];
  __shared__ unsigned wtot[NW], btot[NW];
  __shared__ unsigned s_tile;
  __shared__ uint64_t stage[kS2Tile];
  const unsigned w = threadIdx.x / kWave, l = lane_id();
  if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u);
#pragma unroll
  for (int q = 0; q < NW; ++q) wcnt[q][threadIdx.x] = 0;
  // class bases: digit d = 255 - cls, base[d] = entries of the classes in front of it
  unsigned cbase;
  {
    const unsigned v = cls_hist[255 - threadIdx.x];
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o = __shfl_up(inc, off, 64);
      if (l >= (unsigned)off) inc += o;
    }
    if (l == 63) btot[w] = inc;
    __syncthreads();
    unsigned wb = 0;
    for (unsigned q = 0; q < w; ++q) wb += btot[q];
    cbase = wb + inc - v;
  }
  const unsigned tile = s_tile;
  uint64_t c[kS2Rows];
  unsigned short local[kS2Rows];
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = s2_elem(tile, w, r, l);
    c[r] = ~0ull;
    if (i < n) {
      // the packed word keeps 32 count bits: a count beyond them (class 255 whatever its low word
      // says) is packed as the largest one, and written out from the source list further down
      const int64_t cn = cnts[i];
      c[r] = comp_make(keys[i], cn > 0xFFFFFFFFll ? 0xFFFFFFFFll : cn);
    }
  }
  const uint64_t tile_base = (uint64_t)tile * kS2Tile;
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const bool act = s2_elem(tile, w, r, l) < n;
    const unsigned d = cls_digit(c[r]);
    const unsigned long long peers = match_digit(d, act);
    const unsigned rank = __popcll(peers & ((1ull << l) - 1ull));
    const unsigned before = act ? wcnt[w][d] : 0;
    __builtin_amdgcn_wave_barrier();
    if (act && rank == 0) wcnt[w][d] = before + (unsigned)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    local[r] = (unsigned short)(before + rank);
  }
  __syncthreads();
  {
    const unsigned d = threadIdx.x;
    unsigned t[NW], tot = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      t[q] = wcnt[q][d];
      tot += t[q];
    }
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
        --tb;
      }
      __hip_atomic_store(my, kOsPrefix | (excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    goff[d] = cbase + excl - dstart;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = s2_elem(tile, w, r, l);
    if (i < n) {
      const unsigned d = cls_digit(c[r]);
      const unsigned sidx = wcnt[w][d] + local[r];
      stage[sidx] = c[r];
      // range table: label of the entry at position i of the key-ordered list (class 255 is
      // labelled after its own sort: -1 here)
      const int32_t lab = d != 0 ? (int32_t)(first_label + goff[d] + sidx) : -1;
      if (src_slots != nullptr) {
        // (the smallest int32 owns no slot: 0xFFFFFFFF, past the end of every table)
        const uint32_t sl = src_slots[i];
        if (sl < nslots) reinterpret_cast<uint32_t *>(slot_table + sl)[1] = (uint32_t)lab;
      } else if (label_of != nullptr) {
        label_of[i] = lab;
      }
      if (big_src != nullptr && d == 0) big_src[goff[0] + sidx] = (int32_t)i;
      if (d == 0) out_cnts[goff[0] + sidx] = cnts[i];  // class 255: the count itself, all 64 bits
    }
  }
  __syncthreads();
  const unsigned tile_n = (unsigned)(n - tile_base < (uint64_t)kS2Tile ? n - tile_base : kS2Tile);
#pragma unroll 4
  for (int j = 0; j < kS2Rows; ++j) {
    const unsigned idx = j * kS2BS + threadIdx.x;
    if (idx < tile_n) {
      const uint64_t v = stage[idx];
      const unsigned d = cls_digit(v);
      if (big_src != nullptr && d != 0) continue;
      const unsigned dst = goff[d] + idx;
      const int32_t key = comp_key(v);
      out_keys[dst] = key;
      if (d != 0) out_cnts[dst] = comp_cnt(v);
      if (key == INT32_MIN && d != 0 && sentinel_label != nullptr) {
        *sentinel_label = first_label + (int64_t)dst;
      } else if (table != nullptr && d != 0) {  // class 255 gets its labels after its own sort
        const int64_t label = first_label + (int64_t)dst;
        {
          const unsigned long long want = ((unsigned long long)(uint32_t)label << 32) | (uint32_t)key;
          uint64_t slot = (uint64_t)slot_hash(key) & mask;
          while (atomicCAS(&table[slot], kEncEmptySlot, want) != kEncEmptySlot) slot = (slot + 1) & mask;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kS2BS) void cls_scatter_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ cnts, uint64_t n,
    const unsigned *__restrict__ cls_hist, unsigned *status, unsigned *ticket, int32_t *out_keys,
    int64_t *out_cnts, unsigned long long *table, uint64_t mask, int64_t first_label,
    int64_t *sentinel_label, int32_t *label_of, const uint32_t *__restrict__ src_slots,
    unsigned long long *slot_table, uint64_t nslots) {
  cls_scatter_body(keys, cnts, n, cls_hist, status, ticket, out_keys, out_cnts, table, mask,
                   first_label, sentinel_label, label_of, nullptr, src_slots, slot_table, nslots);
}

// ---- the same ordering for SEVERAL vocabularies per launch --------------------------------
// A Criteo fit orders 13 key-sorted vocabularies; one launch chain per vocabulary (memsets,
// scatter, patch / build: ~10 launches each) kept the HOST busy for as long as the kernels ran
// (~130 launches, 1.0 ms of a 12 ms step).  Here every stage is ONE launch for all vocabularies
// of the call: the tiles of all lists form one grid (a block finds its vocabulary in a prefix
// table of 16 entries), streaming stages use blockIdx.y = vocabulary.
constexpr int kOrdBatch = 16;
struct OrdJob {
  const int32_t *keys;
  const int64_t *cnts;
  const unsigned *cls_hist;
  unsigned *status, *ticket;
  int32_t *out_keys;
  int64_t *out_cnts;
  int32_t *label_of;
  const uint32_t *src_slots;  // dumped table: labels go through these, no patch pass
  unsigned long long *table;
  int64_t *sentinel_label;
  int32_t *aux;
  unsigned long long *fb_status;
  unsigned long long n, capacity, nslots, flat_slots, first_label, status_words, fb_words;
};
struct OrdBatch {
  OrdJob j[kOrdBatch];
  unsigned tile_start[kOrdBatch + 1];
  unsigned flat_start[kOrdBatch + 1];
  int njobs;
};
__device__ __forceinline__ int ord_job_of(const unsigned *start, int n, unsigned b) {
  int c = 0;
  while (c + 1 < n && b >= start[c + 1]) ++c;
  return c;
}

__global__ __launch_bounds__(kBlock) void ord_prep_kernel(OrdBatch b) {
  const OrdJob &j = b.j[blockIdx.y];
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint64_t t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  for (uint64_t i = t0; i < j.status_words; i += stride) j.status[i] = 0;   // + the ticket word
  for (uint64_t i = t0; i < j.fb_words; i += stride) j.fb_status[i] = 0;
  if (j.flat_slots) {  // flat table: every slot empty before the build
    for (uint64_t i = t0; i < j.capacity; i += stride) j.table[i] = kEncEmptySlot;
  }
  if (t0 == 0) *j.sentinel_label = -1;
}

__global__ __launch_bounds__(kS2BS) void cls_scatter_many_kernel(OrdBatch b) {
  const int ji = ord_job_of(b.tile_start, b.njobs, blockIdx.x);
  const OrdJob &j = b.j[ji];
  cls_scatter_body(j.keys, j.cnts, j.n, j.cls_hist, j.status, j.ticket, j.out_keys, j.out_cnts,
                   nullptr, 0, (int64_t)j.first_label, j.sentinel_label, j.label_of, nullptr,
                   j.src_slots, j.table, j.nslots);
}

// Range table (dumped by the counting pass: slot = {key, position in the key-ordered list}):
// positions -> labels.  One streaming pass: the slots are in key order, so label_of[] is read
// front to back as well.
__device__ __forceinline__ void range_patch_body(unsigned long long *table, uint64_t nslots,
                                                 const int32_t *__restrict__ label_of) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock * 2;
  for (uint64_t s0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 2; s0 < nslots; s0 += stride) {
    ulonglong2 e = *reinterpret_cast<ulonglong2 *>(table + s0);  // nslots is even, 16-byte aligned
    bool dirty = false;
    if ((int32_t)(uint32_t)e.x != INT32_MIN) {
      e.x = ((unsigned long long)(uint32_t)label_of[(uint32_t)(e.x >> 32)] << 32) | (uint32_t)e.x;
      dirty = true;
    }
    if ((int32_t)(uint32_t)e.y != INT32_MIN) {
      e.y = ((unsigned long long)(uint32_t)label_of[(uint32_t)(e.y >> 32)] << 32) | (uint32_t)e.y;
      dirty = true;
    }
    if (dirty) *reinterpret_cast<ulonglong2 *>(table + s0) = e;
  }
}
__global__ __launch_bounds__(kBlock) void range_patch_kernel(unsigned long long *table,
                                                             uint64_t nslots,
                                                             const int32_t *__restrict__ label_of) {
  range_patch_body(table, nslots, label_of);
}

// labels of the (few) entries of class 255 after their own sort: vocab[j] -> first_label + j
// (repeated in range_fix_prefix_many_kernel on purpose: one shared body compiles to other machine code)
__global__ __launch_bounds__(kBlock) void range_fix_prefix_kernel(
    unsigned long long *table, const int32_t *__restrict__ aux, const int32_t *__restrict__ vocab,
    uint64_t n_big, int64_t first_label, int64_t *sentinel_label, uint64_t table_slots) {
  const RangeMap map = load_map(aux);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n_big; j += stride) {
    const int32_t key = vocab[j];
    const int64_t label = first_label + (int64_t)j;
    if (key == INT32_MIN) {
      *sentinel_label = label;
      continue;
    }
    uint64_t s = map.table_slot(key);
    if (map.flat) {  // runs in key order: bounded search (keys that cluster in their range)
      s = flat_find_from(table, table_slots, s, key, table[s]);
      if (s != ~0ull) table[s] = ((unsigned long long)(uint32_t)label << 32) | (uint32_t)key;
      continue;
    }
    while (true) {
      const unsigned long long e = table[s];
      if ((int32_t)(uint32_t)e == key) {
        table[s] = ((unsigned long long)(uint32_t)label << 32) | (uint32_t)key;
        break;
      }
      if ((int32_t)(uint32_t)e == INT32_MIN) break;  // cannot happen for a key of the vocabulary
      ++s;
    }
  }
}

__global__ __launch_bounds__(kBlock) void range_patch_many_kernel(OrdBatch b) {
  const OrdJob &j = b.j[blockIdx.y];
  if (j.flat_slots || j.nslots == 0 || j.src_slots != nullptr) return;
  range_patch_body(j.table, j.nslots, j.label_of);
}

struct FixJob {
  unsigned long long *table;
  const int32_t *aux, *vocab;
  int64_t *sentinel_label;
  unsigned long long n_big, first_label, table_slots;
};
struct FixBatch {
  FixJob j[kOrdBatch];
};
__global__ __launch_bounds__(kBlock) void range_fix_prefix_many_kernel(FixBatch b) {
  const FixJob &f = b.j[blockIdx.y];
  const RangeMap map = load_map(f.aux);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < f.n_big; j += stride) {
    const int32_t key = f.vocab[j];
    const int64_t label = (int64_t)f.first_label + (int64_t)j;
    if (key == INT32_MIN) {
      *f.sentinel_label = label;
      continue;
    }
    uint64_t s = map.table_slot(key);
    if (map.flat) {
      s = flat_find_from(f.table, f.table_slots, s, key, f.table[s]);
      if (s != ~0ull) f.table[s] = ((unsigned long long)(uint32_t)label << 32) | (uint32_t)key;
      continue;
    }
    while (true) {
      const unsigned long long e = f.table[s];
      if ((int32_t)(uint32_t)e == key) {
        f.table[s] = ((unsigned long long)(uint32_t)label << 32) | (uint32_t)key;
        break;
      }
      if ((int32_t)(uint32_t)e == INT32_MIN) break;
      ++s;
    }
  }
}

// histogram of min(count, 255) of a (key, count) list that did not come from the range path (the
// multi-GPU merge gathers key-sorted owner shards): what cls_scatter_kernel needs
__global__ __launch_bounds__(kBlock) void class_hist_kernel(const int64_t *__restrict__ cnts,
                                                            uint64_t n, unsigned *hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  unsigned ones = 0;  // class 1 is most of a power-law vocabulary: counted in a register
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t c = cnts[i];
    if (c == 1)
      ++ones;
    else
      atomicAdd(&h[c < 255 ? (c < 0 ? 0 : (unsigned)c) : 255u], 1u);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ones += __shfl_down(ones, off, 64);
  if (lane_id() == 0 && ones) atomicAdd(&h[1], ones);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// ---- flat range table from a KEY-SORTED list: no atomics, no random inserts ---------------------
// A vocabulary table with linear probing and a MONOTONE slot function can be laid out directly
// from the sorted keys: home slots h_i = f(K_i) are non-decreasing in i, so the position of entry
// i is p_i = max(h_i, p_{i-1} + 1) = i + max_{j <= i}(h_j - j) -- a prefix MAXIMUM over the list
// (decoupled look-back over the tiles), after which every entry is written once, positions
// increasing.  Against 36 M random 8-byte CAS inserts (the sort path's vocabularies, or the
// union a multi-GPU merge gathers): one streaming pass.  Lookups probe forward from f(key) to
// the key or an empty slot, exactly like the dumped tables of the range path (RangeMap.flat).
// The largest displacement p_i - h_i goes to aux[NVT_FLAT_AUX_MAXDISP]: keys that cluster in
// their range make long runs, the caller then builds an ordinary hashed table instead.
__device__ __forceinline__ void flat_params_body(const int32_t *__restrict__ keys, uint64_t n,
                                                 uint64_t slots, int32_t *aux) {
  // span of the (sorted) keys, the sentinel key (smallest int32, not in the table) left out
  const uint64_t first = (n > 1 && keys[0] == INT32_MIN) ? 1 : 0;
  const uint64_t lo = ukey(keys[first]), hi = ukey(keys[n - 1]);
  const uint64_t span = hi - lo, F = slots;  // any slot count < 2^32 (no power of two needed)
  uint32_t mul;
  int sh;
  range_map_params(span, F, &mul, &sh);
  aux[NVT_RANGE_AUX_LO] = (int32_t)(uint32_t)lo;
  aux[NVT_RANGE_AUX_LO + 1] = (int32_t)(uint32_t)span;
  aux[NVT_RANGE_AUX_LO + 2] = (int32_t)mul;
  aux[NVT_RANGE_AUX_LO + 3] = 0;
  aux[NVT_RANGE_AUX_LO + 4] = sh;
  aux[NVT_RANGE_AUX_LO + 5] = 1;  // flat layout
  aux[NVT_RANGE_AUX_LO + 6] = keys[0] == INT32_MIN ? 1 : 0;  // position 0 holds the smallest int32 (not in the table)
  aux[NVT_FLAT_AUX_MAXDISP] = 0;
}
__global__ void flat_params_kernel(const int32_t *__restrict__ keys, uint64_t n, uint64_t slots,
                                   int32_t *aux) {
  flat_params_body(keys, n, slots, aux);
}

constexpr unsigned long long kFbAgg = 1ull << 62, kFbPrefix = 2ull << 62, kFbMask = (1ull << 62) - 1ull;
constexpr long long kFbBias = 1ll << 40;  // h - i is > -2^30: biased to an unsigned value

__device__ __forceinline__ void flat_build_body(
    const int32_t *__restrict__ keys, const int32_t *__restrict__ label_of, uint64_t n,
    int32_t *aux, unsigned long long *status, unsigned *ticket, unsigned long long *table,
    uint64_t table_slots) {
  constexpr int NW = kS2BS / kWave;
  __shared__ unsigned long long wmax[NW];
  __shared__ unsigned long long s_carry;
  __shared__ unsigned s_tile;
  if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u);
  __syncthreads();
  const unsigned tile = s_tile, w = threadIdx.x / kWave, l = lane_id();
  const RangeMap map = load_map(aux);
  // element (wave w, row r, lane l): waves own contiguous 1024-entry runs (s2_elem)
  int32_t k[kS2Rows];
  unsigned long long d[kS2Rows];  // biased h - i, 0 = no entry
  unsigned long long run = 0;     // running maximum over this wave's rows so far
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = s2_elem(tile, w, r, l);
    k[r] = i < n ? keys[i] : INT32_MIN;
    d[r] = 0;
    if (i < n && k[r] != INT32_MIN) d[r] = (unsigned long long)((long long)map.fine(k[r]) - (long long)i + kFbBias);
  }
  // inclusive prefix maximum inside the wave's run: lanes of a row, then the rows in order
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    unsigned long long v = d[r];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long o = __shfl_up(v, off, 64);
      if (l >= (unsigned)off) v = o > v ? o : v;
    }
    v = run > v ? run : v;
    d[r] = v;
    run = __shfl(v, 63, 64);
  }
  if (l == 63) wmax[w] = run;
  __syncthreads();
  unsigned long long wprev = 0, tmax = 0;
  for (int q = 0; q < NW; ++q) {
    if (q < (int)w) wprev = wmax[q] > wprev ? wmax[q] : wprev;
    tmax = wmax[q] > tmax ? wmax[q] : tmax;
  }
  if (threadIdx.x == 0) {
    unsigned long long *my = status + tile;
    __hip_atomic_store(my, (tile == 0 ? kFbPrefix : kFbAgg) | tmax, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long carry = 0;
    if (tile > 0) {
      unsigned tb = tile - 1;
      while (true) {
        const unsigned long long v = __hip_atomic_load(status + tb, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
        const unsigned f = (unsigned)(v >> 62);
        if (f == 0) {
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        const unsigned long long val = v & kFbMask;
        carry = val > carry ? val : carry;
        if (f == 2) break;
        --tb;
      }
      const unsigned long long incl = carry > tmax ? carry : tmax;
      __hip_atomic_store(my, kFbPrefix | incl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_carry = carry;
  }
  __syncthreads();
  const unsigned long long before = s_carry > wprev ? s_carry : wprev;
  unsigned maxdisp = 0;
#pragma unroll
  for (int r = 0; r < kS2Rows; ++r) {
    const uint64_t i = s2_elem(tile, w, r, l);
    if (i >= n || k[r] == INT32_MIN) continue;
    const unsigned long long m = d[r] > before ? d[r] : before;
    const uint64_t p = (uint64_t)((long long)i + ((long long)m - kFbBias));
    const uint64_t h = map.fine(k[r]);
    const unsigned disp = (unsigned)(p - h < 0xFFFFFFFFull ? p - h : 0xFFFFFFFFull);
    maxdisp = disp > maxdisp ? disp : maxdisp;
    if (p < table_slots)
      table[p] = ((unsigned long long)(uint32_t)(label_of ? label_of[i] : (int32_t)i) << 32) | (uint32_t)k[r];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_down(maxdisp, off, 64);
    maxdisp = o > maxdisp ? o : maxdisp;
  }
  if (l == 0 && maxdisp > 0) atomicMax(reinterpret_cast<unsigned *>(aux + NVT_FLAT_AUX_MAXDISP), maxdisp);
}
__global__ __launch_bounds__(kS2BS) void flat_build_kernel(
    const int32_t *__restrict__ keys, const int32_t *__restrict__ label_of, uint64_t n,
    int32_t *aux, unsigned long long *status, unsigned *ticket, unsigned long long *table,
    uint64_t table_slots) {
  flat_build_body(keys, label_of, n, aux, status, ticket, table, table_slots);
}
__global__ void flat_params_many_kernel(OrdBatch b) {
  const OrdJob &j = b.j[blockIdx.x];
  if (j.flat_slots) flat_params_body(j.keys, j.n, j.flat_slots, j.aux);
}
__global__ __launch_bounds__(kS2BS) void flat_build_many_kernel(OrdBatch b) {
  const int ji = ord_job_of(b.flat_start, b.njobs, blockIdx.x);
  const OrdJob &j = b.j[ji];
  const uint64_t ntiles = (j.n + kS2Tile - 1) / kS2Tile;
  flat_build_body(j.keys, j.label_of, j.n, j.aux, j.fb_status,
                  reinterpret_cast<unsigned *>(j.fb_status + ntiles), j.table, j.capacity);
}

// ---- vocabulary order of a list that is SHARDED over the ranks of a multi-GPU fit -------------
// Every rank owns a key range of the merged (key, count) list.  The order "count descending, key
// ascending" of the union is: class 255 (count >= 255, sorted exactly once all ranks' few such
// entries are gathered), then classes 254 .. 1, each in key order = owner by owner, every owner's
// entries in the order they have.  The label of an entry of class c < 255 is therefore
//   (entries of the classes in front of c, all owners) + (entries of class c on the owners in
//   front of this one) + (its rank among this shard's entries of class c)
// -- the last term is what the class scatter computes; the first two come in as class bases
// (`cls_hist` here is the caller's difference array of those bases: the kernel's exclusive prefix
// over the digits reproduces them modulo 2^32).  Every rank orders 1 / G of the union instead of
// all of it.
__global__ __launch_bounds__(kS2BS) void label_shard_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ cnts, uint64_t n,
    const unsigned *__restrict__ cls_hist, unsigned *status, unsigned *ticket, int32_t *big_keys,
    int64_t *big_cnts, int32_t *label_of, int32_t *big_src) {
  cls_scatter_body(keys, cnts, n, cls_hist, status, ticket, big_keys, big_cnts, nullptr, 0, 0, nullptr,
                   label_of, big_src);
}

// vocabulary + table from a key-sorted list whose entries carry their position in the vocabulary
// order (labels[i], 0-based): ordered arrays by ONE scatter, absolute labels for the table build
__global__ __launch_bounds__(kBlock) void label_scatter_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ cnts, const int32_t *__restrict__ labels,
    uint64_t n, int64_t first_label, int32_t *__restrict__ out_keys, int64_t *__restrict__ out_cnts,
    int32_t *__restrict__ abs_label, int64_t *sentinel_label) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int32_t k = keys[i];
    const uint32_t l = (uint32_t)labels[i];
    out_keys[l] = k;
    out_cnts[l] = cnts[i];
    abs_label[i] = (int32_t)(first_label + (int64_t)l);
    if (k == INT32_MIN && sentinel_label != nullptr) *sentinel_label = first_label + (int64_t)l;
  }
}

// ---- the ordering workspace of ONE vocabulary (n entries, n_big of them in class 255) ----------
//   status words of the class scatter + ticket | sort scratch | label_of[n] | flat-build status + ticket
// (tmp == nullptr: only `bytes` means anything; status_bytes / fb_bytes: what is zeroed before a run)
struct OrderWs {
  unsigned *status, *ticket, *fb_ticket;
  char *sort_tmp;
  int32_t *label_of;
  unsigned long long *fb_status;
  uint64_t ntiles, status_bytes, fb_bytes, bytes;
};
static OrderWs order_ws(void *tmp, uint64_t n, uint64_t n_big) {
  OrderWs w;
  w.ntiles = (n + kS2Tile - 1) / kS2Tile;
  w.status_bytes = w.ntiles * 256 * 4 + 64;
  w.fb_bytes = w.ntiles * 8 + 64;
  uint64_t sort_bytes = 0;
  if (n_big > 1) (void)nvt_vocab_sort_tmp_bytes(4, n_big, &sort_bytes);
  const uint64_t sort_at = pad16(w.status_bytes), label_at = sort_at + pad16(sort_bytes),
                 fb_at = label_at + pad16(n * 4);
  const uintptr_t base = reinterpret_cast<uintptr_t>(tmp);
  w.status = reinterpret_cast<unsigned *>(base);
  w.ticket = w.status + w.ntiles * 256;
  w.sort_tmp = reinterpret_cast<char *>(base + sort_at);
  w.label_of = reinterpret_cast<int32_t *>(base + label_at);
  w.fb_status = reinterpret_cast<unsigned long long *>(base + fb_at);
  w.fb_ticket = reinterpret_cast<unsigned *>(w.fb_status + w.ntiles);
  w.bytes = fb_at + pad16(w.fb_bytes) + 64;
  return w;
}

int vocab_from_labels(const int32_t *src_keys, const int64_t *src_cnts, const int32_t *labels, uint64_t n,
                      int32_t *out_keys, int64_t *out_cnts, void *tmp, int64_t first_label, void *table,
                      uint64_t capacity, int64_t *sentinel_label, const int32_t *range_aux,
                      uint64_t flat_slots, hipStream_t s) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(n < (1ull << 30), "at most 2^30-1 vocabulary entries");
  const OrderWs w = order_ws(tmp, n, 0);  // (no class scatter, no tail: label_of and the flat build)
  int32_t *abs_label = w.label_of;
  const bool flat = table != nullptr && range_aux != nullptr && flat_slots > 0;
  if (table != nullptr) {
    if (flat) {
      NVT_CHECK_ARG(flat_slots >= 64 && flat_slots < (1ull << 32), "flat table: 64 .. 2^32-1 slots");
      NVT_CHECK_ARG(capacity >= flat_slots + n + 64, "flat table: slots + n + 64");
    }
    int rc = encode_clear_any(4, table, capacity, sentinel_label, s);  // (also: no sentinel key yet)
    if (rc) return rc;
  }
  NVT_PROF("vocab_order", 0, s);
  label_scatter_kernel<<<stream_grid(n, kBlock, 8), kBlock, 0, s>>>(src_keys, src_cnts, labels, n, first_label,
                                                                    out_keys, out_cnts, abs_label,
                                                                    table != nullptr ? sentinel_label : nullptr);
  NVT_CHECK_LAUNCH();
  if (flat) {
    int32_t *aux = const_cast<int32_t *>(range_aux);
    flat_params_kernel<<<1, 1, 0, s>>>(src_keys, n, flat_slots, aux);
    NVT_CHECK_LAUNCH();
    NVT_CHECK_HIP(hipMemsetAsync(w.fb_status, 0, w.fb_bytes, s));
    flat_build_kernel<<<(unsigned)w.ntiles, kS2BS, 0, s>>>(src_keys, abs_label, n, aux, w.fb_status,
                                                          w.fb_ticket, (unsigned long long *)table,
                                                          capacity);
    NVT_CHECK_LAUNCH();
  } else if (table != nullptr) {
    // an ordinary hashed table: the ordered keys carry the labels first_label + position
    int rc = encode_insert_any(4, out_keys, n, first_label, table, capacity, sentinel_label, s);
    if (rc) return rc;
  }
  return NVT_OK;
}

uint64_t vocab_order_tmp_bytes(uint64_t n, uint64_t n_big) { return order_ws(nullptr, n, n_big).bytes; }

int vocab_order_from_sorted(const int32_t *src_keys, const int64_t *src_cnts, uint64_t n,
                            const unsigned *cls_hist, uint64_t n_big, int64_t max_count,
                            int32_t *out_keys, int64_t *out_cnts, void *tmp, int64_t first_label,
                            void *table, uint64_t capacity, int64_t *sentinel_label,
                            const int32_t *range_aux, int range_nb_log2, hipStream_t s,
                            bool *tail_deferred, uint64_t flat_slots, const uint32_t *src_slots) {
  *tail_deferred = false;
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(n < (1ull << 30), "at most 2^30-1 vocabulary entries");
  NVT_CHECK_ARG(n_big <= n, "n_big > n");
  const OrderWs w = order_ws(tmp, n, n_big);
  // range table (range_aux set): `table` holds {key, position} slots already (dumped by the
  // counting pass) and only needs its positions replaced by labels -- no clear, no inserts.
  // flat (flat_slots > 0, range_aux = the block that RECEIVES the map): the table is laid
  // out from the sorted keys by a prefix maximum, see flat_build_kernel.
  const bool flat = table != nullptr && range_aux != nullptr && flat_slots > 0;
  const bool ranged = table != nullptr && range_aux != nullptr;
  // dumped table + the slots the counting pass recorded: the scatter labels the slots itself
  const bool slotted = ranged && !flat && src_slots != nullptr;
  const uint64_t nslots = ((uint64_t)1 << range_nb_log2) * kRpRegion + kRpGuard;
  if (flat) {
    NVT_CHECK_ARG(flat_slots >= 64 && flat_slots < (1ull << 32), "flat table: 64 .. 2^32-1 slots");
    NVT_CHECK_ARG(capacity >= flat_slots + n + 64, "flat table: slots + n + 64");
    int rc = encode_clear_any(4, table, capacity, sentinel_label, s);
    if (rc) return rc;
  } else if (table && !ranged) {
    int rc = encode_clear_any(4, table, capacity, sentinel_label, s);
    if (rc) return rc;
  } else if (ranged) {
    NVT_CHECK_HIP(hipMemsetAsync(sentinel_label, 0xFF, 8, s));  // -1: no sentinel key
  }
  {
    NVT_PROF("vocab_order", 0, s);
    NVT_CHECK_HIP(hipMemsetAsync(w.status, 0, w.status_bytes, s));
    cls_scatter_kernel<<<(unsigned)w.ntiles, kS2BS, 0, s>>>(
        src_keys, src_cnts, n, cls_hist, w.status, w.ticket, out_keys, out_cnts,
        ranged ? nullptr : (unsigned long long *)table, capacity - 1, first_label, sentinel_label,
        ranged ? w.label_of : nullptr, slotted ? src_slots : nullptr,
        slotted ? (unsigned long long *)table : nullptr, slotted ? nslots : 0);
    NVT_CHECK_LAUNCH();
    if (flat) {
      int32_t *aux = const_cast<int32_t *>(range_aux);
      flat_params_kernel<<<1, 1, 0, s>>>(src_keys, n, flat_slots, aux);
      NVT_CHECK_LAUNCH();
      NVT_CHECK_HIP(hipMemsetAsync(w.fb_status, 0, w.fb_bytes, s));
      flat_build_kernel<<<(unsigned)w.ntiles, kS2BS, 0, s>>>(
          src_keys, w.label_of, n, aux, w.fb_status, w.fb_ticket, (unsigned long long *)table, capacity);
      NVT_CHECK_LAUNCH();
    } else if (ranged && !slotted) {
      range_patch_kernel<<<stream_grid(nslots / 2, kBlock, 8), kBlock, 0, s>>>(
          (unsigned long long *)table, nslots, w.label_of);
      NVT_CHECK_LAUNCH();
    }
  }
  // the sort of class 255 and the labels of its entries: left to ONE batched launch for all the
  // vocabularies of the call (vocab_order_tail_batch)
  if (vocab_sort_small_eligible(4, n_big, max_count)) {
    *tail_deferred = true;
    return NVT_OK;
  }
  if (n_big > 1) {
    int rc = vocab_sort_any(4, out_keys, out_cnts, n_big, max_count, w.sort_tmp, s);
    if (rc) return rc;
  }
  if (table && n_big > 0) {
    if (ranged) {
      NVT_PROF("encode_build", 0, s);
      range_fix_prefix_kernel<<<stream_grid(n_big, kBlock), kBlock, 0, s>>>(
          (unsigned long long *)table, range_aux, out_keys, n_big, first_label, sentinel_label,
          capacity);
      NVT_CHECK_LAUNCH();
    } else {
      int rc = encode_insert_any(4, out_keys, n_big, first_label, table, capacity, sentinel_label, s);
      if (rc) return rc;
    }
  }
  return NVT_OK;
}

// vocab_order_from_sorted for several vocabularies that own a range table (dumped or flat): every
// stage one launch (ord_prep / cls_scatter_many / flat_params_many + flat_build_many /
// range_patch_many, the last only when a dumped table came without slots), then the class-255 tails (one batched small sort + one label launch; a tail
// too long for the small sort is sorted on its own).
int vocab_order_sorted_batch(const OrderSortedJob *jobs, int njobs, hipStream_t s) {
  for (int j0 = 0; j0 < njobs; j0 += kOrdBatch) {
    const int nj = njobs - j0 < kOrdBatch ? njobs - j0 : kOrdBatch;
    OrdBatch b;
    memset(&b, 0, sizeof(b));
    std::vector<OrderTail> tails;
    OrderWs ws[kOrdBatch];
    bool any_flat = false, any_patch = false;  // any_patch: a dumped table without slots
    for (int i = 0; i < nj; ++i) {
      const OrderSortedJob &q = jobs[j0 + i];
      NVT_CHECK_ARG(q.n > 0 && q.n < (1ull << 30), "1 .. 2^30-1 vocabulary entries");
      NVT_CHECK_ARG(q.n_big <= q.n, "n_big > n");
      NVT_CHECK_ARG(q.table && q.range_aux && q.tmp && q.sentinel_label, "range table jobs only");
      const OrderWs &w = ws[i] = order_ws(q.tmp, q.n, q.n_big);
      OrdJob &o = b.j[i];
      o.keys = q.src_keys;
      o.cnts = q.src_cnts;
      o.cls_hist = q.cls_hist;
      o.status = w.status;
      o.ticket = w.ticket;
      o.out_keys = q.out_keys;
      o.out_cnts = q.out_cnts;
      o.label_of = w.label_of;
      o.src_slots = q.flat_slots ? nullptr : q.src_slots;
      o.table = reinterpret_cast<unsigned long long *>(q.table);
      o.sentinel_label = q.sentinel_label;
      o.aux = const_cast<int32_t *>(q.range_aux);
      o.fb_status = w.fb_status;  // (flat_build_many_kernel finds the ticket behind the tiles' words itself)
      o.n = q.n;
      o.capacity = q.capacity;
      o.flat_slots = q.flat_slots;
      o.nslots = q.flat_slots ? 0 : ((uint64_t)1 << q.range_nb_log2) * kRpRegion + kRpGuard;
      o.first_label = (unsigned long long)q.first_label;
      o.status_words = w.status_bytes / 4;
      o.fb_words = q.flat_slots ? w.fb_bytes / 8 : 0;
      if (q.flat_slots) {
        NVT_CHECK_ARG(q.flat_slots >= 64 && q.flat_slots < (1ull << 32), "flat table: 64 .. 2^32-1 slots");
        NVT_CHECK_ARG(q.capacity >= q.flat_slots + q.n + 64, "flat table: slots + n + 64");
        any_flat = true;
      } else if (q.src_slots == nullptr) {
        any_patch = true;
      }
      b.tile_start[i + 1] = b.tile_start[i] + (unsigned)w.ntiles;
      b.flat_start[i + 1] = b.flat_start[i] + (q.flat_slots ? (unsigned)w.ntiles : 0u);
    }
    b.njobs = nj;
    {
      NVT_PROF("vocab_order", 0, s);
      ord_prep_kernel<<<dim3(any_flat ? 2048 : 64, nj), kBlock, 0, s>>>(b);
      NVT_CHECK_LAUNCH();
      cls_scatter_many_kernel<<<b.tile_start[nj], kS2BS, 0, s>>>(b);
      NVT_CHECK_LAUNCH();
      if (any_flat) {
        flat_params_many_kernel<<<nj, 1, 0, s>>>(b);
        NVT_CHECK_LAUNCH();
        flat_build_many_kernel<<<b.flat_start[nj], kS2BS, 0, s>>>(b);
        NVT_CHECK_LAUNCH();
      }
      if (any_patch) {
        range_patch_many_kernel<<<dim3(1024, nj), kBlock, 0, s>>>(b);
        NVT_CHECK_LAUNCH();
      }
    }
    for (int i = 0; i < nj; ++i) {
      const OrderSortedJob &q = jobs[j0 + i];
      if (q.n_big == 0) continue;
      if (vocab_sort_small_eligible(4, q.n_big, q.max_count)) {
        tails.push_back({q.out_keys, q.out_cnts, q.n_big, q.first_label, q.table, q.capacity,
                         q.sentinel_label, q.range_aux, q.tmp, q.n});
        continue;
      }
      // a class 255 beyond the one-workgroup sort (merged multi-partition vocabularies), or of
      // one entry (nothing to sort)
      if (q.n_big > 1) {
        int rc = vocab_sort_any(4, q.out_keys, q.out_cnts, q.n_big, q.max_count, ws[i].sort_tmp, s);
        if (rc) return rc;
      }
      NVT_PROF("encode_build", 0, s);
      range_fix_prefix_kernel<<<stream_grid(q.n_big, kBlock), kBlock, 0, s>>>(
          (unsigned long long *)q.table, q.range_aux, q.out_keys, q.n_big, q.first_label,
          q.sentinel_label, q.capacity);
      NVT_CHECK_LAUNCH();
    }
    if (!tails.empty()) {
      int rc = vocab_order_tail_batch(tails.data(), (int)tails.size(), s);
      if (rc) return rc;
    }
  }
  return NVT_OK;
}

// class 255 of several vocabularies (vocab_order_from_sorted with tail_deferred): ONE batched
// sort launch (a workgroup per vocabulary) instead of a one-workgroup launch per vocabulary,
// then the labels of the sorted entries
int vocab_order_tail_batch(const OrderTail *t, int nt, hipStream_t s) {
  if (nt == 0) return NVT_OK;
  std::vector<SmallSortDesc> d(nt);
  for (int i = 0; i < nt; ++i) {
    d[i].keys = t[i].keys;
    d[i].counts = t[i].counts;
    d[i].n = (unsigned)t[i].n_big;
    d[i].tmp = t[i].tmp ? order_ws(t[i].tmp, t[i].n, t[i].n_big).sort_tmp : nullptr;
  }
  int rc = vocab_sort_small_batch(d.data(), nt, s);
  if (rc) return rc;
  NVT_PROF("encode_build", 0, s);
  // range tables (dumped or flat): the labels of all vocabularies in one launch
  for (int i0 = 0; i0 < nt;) {
    FixBatch fb;
    memset(&fb, 0, sizeof(fb));
    int nf = 0;
    uint64_t longest = 0;
    for (; i0 < nt && nf < kOrdBatch; ++i0) {
      if (!t[i0].table || !t[i0].range_aux) continue;
      fb.j[nf++] = {(unsigned long long *)t[i0].table, t[i0].range_aux, t[i0].keys,
                    t[i0].sentinel_label, t[i0].n_big, (unsigned long long)t[i0].first_label,
                    t[i0].capacity};
      longest = t[i0].n_big > longest ? t[i0].n_big : longest;
    }
    if (nf) {
      range_fix_prefix_many_kernel<<<dim3(stream_grid(longest, kBlock), nf), kBlock, 0, s>>>(fb);
      NVT_CHECK_LAUNCH();
    }
  }
  for (int i = 0; i < nt; ++i) {
    if (!t[i].table) continue;
    if (t[i].range_aux) {
      continue;  // (labelled above)
    } else {
      rc = encode_insert_any(4, t[i].keys, t[i].n_big, t[i].first_label, t[i].table, t[i].capacity,
                             t[i].sentinel_label, s);
      if (rc) return rc;
    }
  }
  return NVT_OK;
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_class_hist(const int64_t *counts, uint64_t n, uint32_t *hist, void *stream) {
  NVT_CHECK_ARG(hist && (n == 0 || counts), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_CHECK_HIP(hipMemsetAsync(hist, 0, 256 * 4, s));
  if (n == 0) return NVT_OK;
  class_hist_kernel<<<stream_grid(n, kBlock * 8, 4), kBlock, 0, s>>>(counts, n, hist);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}
int nvt_vocab_label_shard(const int32_t *keys, const int64_t *counts, uint64_t n, const uint32_t *class_base_diff,
                          void *tmp, int32_t *label_of, int32_t *big_keys, int64_t *big_counts,
                          int32_t *big_src, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(keys && counts && class_base_diff && tmp && label_of && big_keys && big_counts && big_src,
                "null pointer");
  NVT_CHECK_ARG(n < (1ull << 30), "at most 2^30-1 entries");
  hipStream_t s = (hipStream_t)stream;
  const OrderWs w = order_ws(tmp, n, 0);
  NVT_PROF("vocab_order", 0, s);
  NVT_CHECK_HIP(hipMemsetAsync(w.status, 0, w.status_bytes, s));
  label_shard_kernel<<<(unsigned)w.ntiles, kS2BS, 0, s>>>(keys, counts, n, class_base_diff, w.status,
                                                         w.ticket, big_keys, big_counts, label_of, big_src);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_vocab_order_tmp_bytes(uint64_t n, uint64_t n_big, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out pointer");
  *bytes = vocab_order_tmp_bytes(n, n_big);
  return NVT_OK;
}

int nvt_flat_index_tmp_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile;
  *bytes = pad16(ntiles * 8 + 64) + 64;
  return NVT_OK;
}

int nvt_flat_index_build(const int32_t *keys, uint64_t n, uint64_t slots, int32_t *aux, void *table,
                         uint64_t capacity, void *tmp, void *stream) {
  NVT_CHECK_ARG(keys && aux && table && tmp, "null pointer");
  NVT_CHECK_ARG(n >= 1 && n < (1ull << 30), "1 .. 2^30-1 keys");
  NVT_CHECK_ARG(slots >= 64 && slots < (1ull << 32), "slots must be 64 .. 2^32-1");
  NVT_CHECK_ARG(capacity >= slots + n + 64, "flat table: slots + n + 64");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_index", 0, s);
  const uint64_t ntiles = (n + kS2Tile - 1) / kS2Tile;
  unsigned long long *status = reinterpret_cast<unsigned long long *>(tmp);
  // the sentinel label of an encode table has no meaning here: it lands in the status block and
  // is wiped with it
  int rc = encode_clear_any(4, table, capacity, reinterpret_cast<int64_t *>(status), s);
  if (rc) return rc;
  NVT_CHECK_HIP(hipMemsetAsync(status, 0, ntiles * 8 + 64, s));
  flat_params_kernel<<<1, 1, 0, s>>>(keys, n, slots, aux);
  NVT_CHECK_LAUNCH();
  flat_build_kernel<<<(unsigned)ntiles, kS2BS, 0, s>>>(
      keys, nullptr, n, aux, status, reinterpret_cast<unsigned *>(status + ntiles),
      (unsigned long long *)table, capacity);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
