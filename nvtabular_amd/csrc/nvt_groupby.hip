// Multi-key groupby-aggregate tables: JoinGroupby / TargetEncoding fit and
// "combo" Categorify (categorify.py:955-1137 with agg columns), plus the
// row -> group lookup their transforms need (join_groupby.py:198-203,
// target_encoding.py:350-371: a left merge on the key columns followed by a
// re-sort; here a read-only probe that keeps row order).
//
// Slot protocol (keys are 1..3 int64 words + a null mask, too wide for one CAS):
//   state word 0 = empty, 1 = being written, 2 = ready.
//   writer: CAS 0->1, write-through (sc1) stores of the key words, drain
//           (s_waitcnt vmcnt(0)), write-through store of state = 2;
//   reader: L1-bypassing (sc1) load of state, then of the key words.
// Per-CU L1s are never refreshed by other CUs' stores and the per-XCD L2s are
// not coherent, so every protocol word goes through agent-scope atomics;
// accumulators are only ever touched by atomic RMWs, which execute at the
// memory side.  (MI355X_MICROARCH.md, "Workgroup dispatch ... visibility".)
//
// The rest of the family (nvt_groupby.hpp): nvt_segreduce.hip, nvt_order_rows.hip,
// nvt_sorted_groupby.hip.
#include <cstdlib>
#include <limits>

#include "nvt_groupby.hpp"
#include "nvt_prof.hpp"

// One 16-byte header per slot: a probe of a single-key table (the common JoinGroupby /
// TargetEncoding group) touches ONE 64-byte sector instead of four arrays (state, null mask,
// key, group id: gb_lookup 1.78 -> ms per 20 M rows, profiles/r02_notes.md).
struct nvt_gb_head {
  long long key0;
  unsigned meta;   // bits 0-7 slot state, bits 8-15 null mask of the key tuple
  unsigned index;  // slot -> compact group id (lookup tables), 0xFFFFFFFF = none
};

struct nvt_gb_table {
  int nkeys;
  int nvals;
  int flags;
  uint64_t capacity;
  struct nvt_gb_head *head;    // [cap] {first key component, state | null mask, group id}
  long long *keys;             // [nkeys - 1][cap] the further key components
  unsigned long long *size;    // [cap]
  unsigned long long *count;   // [cap]
  double *sum;                 // [nvals][cap]
  double *sumsq;               // [nvals][cap] or null
  double *vmin;                // [nvals][cap] or null
  double *vmax;                // [nvals][cap] or null
  uint64_t *state;             // [NVT_STATE_WORDS]
  void *block;                 // the arrays' block when it is ours (nvt_gb_create), else null
  void *scratch;               // sort workspace of nvt_gb_update (grown on demand)
  uint64_t scratch_bytes;
  int external;                // arrays live in caller-provided memory (nvt_gb_create_in)
  int external_scratch;        // scratch set by nvt_gb_set_workspace
};

namespace nvt {

constexpr unsigned ST_EMPTY = 0, ST_LOCKED = 1, ST_READY = 2;
constexpr int kGbMaxProbe = 1024;

struct GbMergeArgs {
  const int64_t *keys[kMaxKeys];
  const uint8_t *null_mask;
  const int64_t *size, *count;
  const double *sum[kMaxVals], *sumsq[kMaxVals], *vmin[kMaxVals], *vmax[kMaxVals];
};

struct GbOutArgs {
  int64_t *keys[kMaxKeys];
  uint8_t *null_mask;
  int64_t *size, *count;
  double *sum[kMaxVals], *sumsq[kMaxVals], *vmin[kMaxVals], *vmax[kMaxVals];
};

__device__ __forceinline__ uint64_t tuple_hash(const long long (&k)[kMaxKeys], unsigned nm,
                                               int nkeys) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ nm;
  for (int j = 0; j < nkeys; ++j) h = fmix64(h ^ (uint64_t)k[j]) + 0x9E3779B97F4A7C15ull * (j + 1);
  return fmix64(h);
}

// Find (or, when `insert`, create) the slot of a key tuple.  Returns the slot
// index or -1 (absent / overflow).
__device__ __forceinline__ int64_t find_slot(const GbView &t, const long long (&k)[kMaxKeys],
                                             unsigned nm, bool insert, unsigned *n_new,
                                             unsigned *ovf) {
  uint64_t slot = tuple_hash(k, nm, t.nkeys) & t.mask;
  int probe = 0;
  unsigned spins = 0;  // bounded wait on a LOCKED slot: report overflow rather than hang the GPU
  while (probe < kGbMaxProbe) {
    nvt_gb_head *hd = &t.head[slot];
    unsigned st = __hip_atomic_load(&hd->meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st == ST_EMPTY) {
      if (!insert) return -1;
      unsigned prev = atomicCAS(&hd->meta, ST_EMPTY, ST_LOCKED);
      if (prev == ST_EMPTY) {
        __hip_atomic_store(&hd->key0, k[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int j = 1; j < t.nkeys; ++j)
          __hip_atomic_store(&t.keys[(uint64_t)(j - 1) * t.cap + slot], k[j], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&hd->meta, ST_READY | (nm << 8), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        *n_new += 1;
        return (int64_t)slot;
      }
      st = prev;  // somebody else got it: fall through with its state
    }
    if (st == ST_LOCKED) {  // writer is a few instructions from READY: re-read
      if (++spins < (1u << 22)) continue;
      *ovf = 1;
      return -1;
    }
    // READY: compare (the null mask travels with the state word)
    bool same = (st >> 8) == nm &&
                __hip_atomic_load(&hd->key0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k[0];
    for (int j = 1; same && j < t.nkeys; ++j)
      same = __hip_atomic_load(&t.keys[(uint64_t)(j - 1) * t.cap + slot], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) == k[j];
    if (same) return (int64_t)slot;
    slot = (slot + 1) & t.mask;
    ++probe;
  }
  *ovf = 1;
  return -1;
}

__global__ __launch_bounds__(kBlock) void gb_clear_kernel(GbView t) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const double inf = std::numeric_limits<double>::infinity();
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < t.cap; i += stride) {
    nvt_gb_head e;
    e.key0 = 0;
    e.meta = ST_EMPTY;
    e.index = 0xFFFFFFFFu;
    t.head[i] = e;
    t.size[i] = 0;
    t.count[i] = 0;
    for (int j = 1; j < t.nkeys; ++j) t.keys[(uint64_t)(j - 1) * t.cap + i] = 0;
    for (int j = 0; j < t.nvals; ++j) {
      t.sum[(uint64_t)j * t.cap + i] = 0.0;
      if (t.sumsq) t.sumsq[(uint64_t)j * t.cap + i] = 0.0;
      if (t.vmin) {
        t.vmin[(uint64_t)j * t.cap + i] = inf;
        t.vmax[(uint64_t)j * t.cap + i] = -inf;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < NVT_STATE_WORDS) t.state[threadIdx.x] = 0;
}

__device__ __forceinline__ unsigned read_tuple(const GbRowArgs &a, int nkeys, uint64_t i,
                                               long long (&k)[kMaxKeys]) {
  unsigned nm = 0;
  for (int j = 0; j < kMaxKeys; ++j) k[j] = 0;
  for (int j = 0; j < nkeys; ++j) {
    if (bit_valid(a.key_valid[j], i))
      k[j] = a.keys[j][i];
    else
      nm |= 1u << j;
  }
  return nm;
}

__global__ __launch_bounds__(kBlock) void gb_update_kernel(GbView t, GbRowArgs a, uint64_t n) {
  unsigned n_new = 0, ovf = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    long long k[kMaxKeys];
    unsigned nm = read_tuple(a, t.nkeys, i, k);
    int64_t slot = find_slot(t, k, nm, true, &n_new, &ovf);
    if (slot < 0) continue;
    atomicAdd(&t.size[slot], 1ull);
    if (!(nm & 1u)) atomicAdd(&t.count[slot], 1ull);
    for (int j = 0; j < t.nvals; ++j) {
      double v;
      bool ok = load_val(a.vals[j], a.vdtype[j], i, &v) && bit_valid(a.val_valid[j], i);
      if (!ok) continue;
      uint64_t o = (uint64_t)j * t.cap + slot;
      atomicAdd(&t.sum[o], v);
      if (t.sumsq) atomicAdd(&t.sumsq[o], v * v);
      if (t.vmin) {
        atomic_min_f64(&t.vmin[o], v);
        atomic_max_f64(&t.vmax[o], v);
      }
    }
  }
  if (n_new) atomicAdd((unsigned long long *)&t.state[NVT_ST_OCCUPIED], (unsigned long long)n_new);
  if (ovf) atomicOr((unsigned long long *)&t.state[NVT_ST_OVERFLOW], 1ull);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd((unsigned long long *)&t.state[NVT_ST_ROWS], (unsigned long long)n);
}

// ---- update without per-row accumulator atomics (JoinGroupby / TargetEncoding fit) -----------
// The kernel above does up to 2 + 4 * nvals device atomics per row on the row's group; with the
// skewed keys these operators see, thousands of rows hit the same few slots and serialise at
// the memory side (20 M rows, 5 M keys, one float target: 5.5 s per fit + transform).  Instead:
//   gb_assign_kernel     row -> slot (find-or-insert: reads only once a key exists), written as
//                        the packed word (slot << 32 | row)
//   sort_words_bits      onesweep LSD radix on the slot bits: every group's rows become ONE run,
//                        in row order (stable)
//   gb_segreduce_kernel  wave-level segmented reduction over the sorted words (values gathered
//                        by row, nvt_segreduce.hip); one add per (wave, run) into the group's
//                        accumulators -- a hot group of a million rows costs 16 k adds instead of
//                        a million, and runs of cold groups touch distinct addresses.
__global__ __launch_bounds__(kBlock) void gb_assign_kernel(GbView t, GbRowArgs a, uint64_t n,
                                                           uint64_t *__restrict__ words) {
  unsigned n_new = 0, ovf = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    long long k[kMaxKeys];
    unsigned nm = read_tuple(a, t.nkeys, i, k);
    int64_t slot = find_slot(t, k, nm, true, &n_new, &ovf);
    // rows that found no slot (overflow: the call fails) sort behind everything else
    words[i] = ((uint64_t)(slot < 0 ? t.cap : (uint64_t)slot) << 32) | (uint64_t)(uint32_t)i;
  }
  if (n_new) atomicAdd((unsigned long long *)&t.state[NVT_ST_OCCUPIED], (unsigned long long)n_new);
  if (ovf) atomicOr((unsigned long long *)&t.state[NVT_ST_OVERFLOW], 1ull);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd((unsigned long long *)&t.state[NVT_ST_ROWS], (unsigned long long)n);
}

__global__ __launch_bounds__(kBlock) void gb_merge_kernel(GbView t, GbMergeArgs a, uint64_t n) {
  unsigned n_new = 0, ovf = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    long long k[kMaxKeys] = {0, 0, 0};
    unsigned nm = a.null_mask ? a.null_mask[i] : 0;
    for (int j = 0; j < t.nkeys; ++j) k[j] = ((nm >> j) & 1) ? 0 : a.keys[j][i];
    int64_t slot = find_slot(t, k, nm, true, &n_new, &ovf);
    if (slot < 0) continue;
    if (a.size) atomicAdd(&t.size[slot], (unsigned long long)a.size[i]);
    if (a.count) atomicAdd(&t.count[slot], (unsigned long long)a.count[i]);
    for (int j = 0; j < t.nvals; ++j) {
      uint64_t o = (uint64_t)j * t.cap + slot;
      if (a.sum[j]) atomicAdd(&t.sum[o], a.sum[j][i]);
      if (t.sumsq && a.sumsq[j]) atomicAdd(&t.sumsq[o], a.sumsq[j][i]);
      if (t.vmin && a.vmin[j]) {
        double lo = a.vmin[j][i], hi = a.vmax[j][i];
        if (lo == lo) atomic_min_f64(&t.vmin[o], lo);
        if (hi == hi) atomic_max_f64(&t.vmax[o], hi);
      }
    }
  }
  if (n_new) atomicAdd((unsigned long long *)&t.state[NVT_ST_OCCUPIED], (unsigned long long)n_new);
  if (ovf) atomicOr((unsigned long long *)&t.state[NVT_ST_OVERFLOW], 1ull);
}

// table -> dense group arrays, arbitrary order.  Each workgroup takes tiles of kBlock *
// kGbCompactItems consecutive slots, ranks the READY ones with a wave scan + LDS and reserves
// its output range with ONE atomic per tile (an atomic per wave on the single cursor
// serialises at the memory side: 4.5 ms for a 16 M-slot table, 39 % of the cfg4 step).
constexpr int kGbCompactItems = 8;
__global__ __launch_bounds__(kBlock) void gb_compact_kernel(GbView t, GbOutArgs o,
                                                            uint64_t *out_n) {
  constexpr uint64_t TILE = (uint64_t)kBlock * kGbCompactItems;
  __shared__ unsigned wsum[kBlock / kWave];
  __shared__ unsigned long long tile_base;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  const uint64_t ntiles = (t.cap + TILE - 1) / TILE;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // item q of the tile's round r is slot tile * TILE + r * kBlock + threadIdx.x (coalesced)
    unsigned occ = 0, mine = 0;
#pragma unroll
    for (int r = 0; r < kGbCompactItems; ++r) {
      const uint64_t i = tile * TILE + (uint64_t)r * kBlock + threadIdx.x;
      if (i < t.cap && (t.head[i].meta & 0xFFu) == ST_READY) {
        occ |= 1u << r;
        ++mine;
      }
    }
    unsigned inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned o2 = __shfl_up(inc, off, 64);
      if (lane >= (unsigned)off) inc += o2;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned wbase = 0, total = 0;
    for (unsigned q = 0; q < kBlock / kWave; ++q) {
      if (q < w) wbase += wsum[q];
      total += wsum[q];
    }
    if (threadIdx.x == 0)
      tile_base = total ? atomicAdd((unsigned long long *)out_n, (unsigned long long)total) : 0;
    __syncthreads();
    uint64_t g = tile_base + wbase + inc - mine;
#pragma unroll
    for (int r = 0; r < kGbCompactItems; ++r) {
      if (!((occ >> r) & 1)) continue;
      const uint64_t i = tile * TILE + (uint64_t)r * kBlock + threadIdx.x;
      const nvt_gb_head hd = t.head[i];
      // the table now also maps its keys to the compact group ids (nvt_gb_lookup works on it
      // without a second table built by nvt_gb_index_build)
      t.head[i].index = (unsigned)g;
      if (o.keys[0]) o.keys[0][g] = hd.key0;
      for (int j = 1; j < t.nkeys; ++j)
        if (o.keys[j]) o.keys[j][g] = t.keys[(uint64_t)(j - 1) * t.cap + i];
      if (o.null_mask) o.null_mask[g] = (uint8_t)(hd.meta >> 8);
      if (o.size) o.size[g] = (int64_t)t.size[i];
      if (o.count) o.count[g] = (int64_t)t.count[i];
      for (int j = 0; j < t.nvals; ++j) {
        uint64_t s = (uint64_t)j * t.cap + i;
        if (o.sum[j]) o.sum[j][g] = t.sum[s];
        if (o.sumsq[j]) o.sumsq[j][g] = t.sumsq ? t.sumsq[s] : qnan;
        if (o.vmin[j]) {
          double v = t.vmin ? t.vmin[s] : qnan;
          o.vmin[j][g] = (v == std::numeric_limits<double>::infinity()) ? qnan : v;
        }
        if (o.vmax[j]) {
          double v = t.vmax ? t.vmax[s] : qnan;
          o.vmax[j][g] = (v == -std::numeric_limits<double>::infinity()) ? qnan : v;
        }
      }
      ++g;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void gb_index_build_kernel(GbView t, GbMergeArgs a,
                                                                uint64_t n) {
  unsigned n_new = 0, ovf = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    long long k[kMaxKeys] = {0, 0, 0};
    unsigned nm = a.null_mask ? a.null_mask[i] : 0;
    for (int j = 0; j < t.nkeys; ++j) k[j] = ((nm >> j) & 1) ? 0 : a.keys[j][i];
    int64_t slot = find_slot(t, k, nm, true, &n_new, &ovf);
    if (slot >= 0) t.head[slot].index = (unsigned)i;
  }
  if (n_new) atomicAdd((unsigned long long *)&t.state[NVT_ST_OCCUPIED], (unsigned long long)n_new);
  if (ovf) atomicOr((unsigned long long *)&t.state[NVT_ST_OVERFLOW], 1ull);
}

__global__ __launch_bounds__(kBlock) void gb_lookup_kernel(GbView t, GbRowArgs a, uint64_t n,
                                                           int64_t *__restrict__ out) {
  unsigned n_new = 0, ovf = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    long long k[kMaxKeys];
    unsigned nm = read_tuple(a, t.nkeys, i, k);
    int64_t slot = find_slot(t, k, nm, false, &n_new, &ovf);
    unsigned g = 0xFFFFFFFFu;
    if (slot >= 0) g = t.head[slot].index;
    out[i] = g == 0xFFFFFFFFu ? -1 : (int64_t)g;
  }
}

inline GbView view_of(nvt_gb_table *t) {
  GbView v;
  v.nkeys = t->nkeys;
  v.nvals = t->nvals;
  v.flags = t->flags;
  v.cap = t->capacity;
  v.mask = t->capacity - 1;
  v.head = t->head;
  v.keys = t->keys;
  v.size = t->size;
  v.count = t->count;
  v.sum = t->sum;
  v.sumsq = t->sumsq;
  v.vmin = t->vmin;
  v.vmax = t->vmax;
  v.state = t->state;
  v.vcount = nullptr;
  return v;
}

static int gb_check_shape(const char *who, int nkeys, int nvals, uint64_t capacity) {
  if (!(nkeys >= 1 && nkeys <= kMaxKeys)) return bad_arg(who, "nkeys must be 1..3");
  if (!(nvals >= 0 && nvals <= kMaxVals)) return bad_arg(who, "nvals must be 0..8");
  if (!(capacity >= 64 && (capacity & (capacity - 1)) == 0))
    return bad_arg(who, "capacity must be 2^k >= 64");
  return NVT_OK;
}

// Where the arrays of a table of a (checked) shape lie in its block, as offsets from the
// block's first 256-byte boundary, and the block's size.  Arrays the shape does not have
// (further key components, values, sumsq, min / max) get kNoArray.
constexpr uint64_t kNoArray = ~0ull;
struct GbLayout {
  uint64_t head, keys, size, count, sum, state, sumsq, vmin, vmax;
  uint64_t bytes;  // all of them + 256 to align the block's start
};
static GbLayout gb_layout(int nkeys, int nvals, int flags, uint64_t capacity) {
  uint64_t off = 0;
  auto take = [&](bool have, uint64_t b) {
    if (!have) return kNoArray;
    const uint64_t r = off;
    off += pad256(b);
    return r;
  };
  GbLayout l;
  l.head = take(true, capacity * 16);
  l.keys = take(nkeys > 1, capacity * 8 * (nkeys - 1));
  l.size = take(true, capacity * 8);
  l.count = take(true, capacity * 8);
  l.sum = take(nvals > 0, capacity * 8 * nvals);
  l.state = take(true, NVT_STATE_WORDS * 8);
  l.sumsq = take(nvals && (flags & NVT_GB_SUMSQ), capacity * 8 * nvals);
  l.vmin = take(nvals && (flags & NVT_GB_MINMAX), capacity * 8 * nvals);
  l.vmax = take(nvals && (flags & NVT_GB_MINMAX), capacity * 8 * nvals);
  l.bytes = off + 256;
  return l;
}

// a table (of a checked shape) over a block of gb_layout(...).bytes bytes
static nvt_gb_table *gb_table_over(int nkeys, int nvals, int flags, uint64_t capacity, void *memory) {
  const GbLayout l = gb_layout(nkeys, nvals, flags, capacity);
  nvt_gb_table *t = new nvt_gb_table();
  memset(t, 0, sizeof(*t));
  t->nkeys = nkeys;
  t->nvals = nvals;
  t->flags = flags;
  t->capacity = capacity;
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(memory) + 255) & ~(uintptr_t)255);
  auto at = [&](uint64_t off) { return off == kNoArray ? nullptr : (void *)(base + off); };
  t->head = (nvt_gb_head *)at(l.head);
  t->keys = (long long *)at(l.keys);
  t->size = (unsigned long long *)at(l.size);
  t->count = (unsigned long long *)at(l.count);
  t->sum = (double *)at(l.sum);
  t->state = (uint64_t *)at(l.state);
  t->sumsq = (double *)at(l.sumsq);
  t->vmin = (double *)at(l.vmin);
  t->vmax = (double *)at(l.vmax);
  return t;
}

}  // namespace nvt

using namespace nvt;

extern "C" {

void nvt_gb_destroy(nvt_gb_table *t) {
  if (!t) return;
  if (!t->external && t->block) (void)hipFree(t->block);
  if (t->scratch && !t->external_scratch) (void)hipFree(t->scratch);
  delete t;
}

int nvt_gb_table_bytes(int nkeys, int nvals, int flags, uint64_t capacity, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  int rc = gb_check_shape(__func__, nkeys, nvals, capacity);
  if (rc) return rc;
  *bytes = gb_layout(nkeys, nvals, flags, capacity).bytes;
  return NVT_OK;
}

// Table whose arrays live in caller-provided device memory (nvt_gb_table_bytes() bytes, 256-byte
// aligned): no hipMalloc / hipFree -- both synchronise the device -- on the fit path.
int nvt_gb_create_in(int nkeys, int nvals, int flags, uint64_t capacity, void *memory,
                     uint64_t bytes, nvt_gb_table **out) {
  NVT_CHECK_ARG(out && memory, "null out/memory");
  int rc = gb_check_shape(__func__, nkeys, nvals, capacity);
  if (rc) return rc;
  NVT_CHECK_ARG(bytes >= gb_layout(nkeys, nvals, flags, capacity).bytes,
                "memory block too small (nvt_gb_table_bytes)");
  nvt_gb_table *t = gb_table_over(nkeys, nvals, flags, capacity, memory);
  t->external = 1;
  *out = t;
  return NVT_OK;
}

// The same over one block of its own, freed by nvt_gb_destroy
int nvt_gb_create(int nkeys, int nvals, int flags, uint64_t capacity, nvt_gb_table **out) {
  NVT_CHECK_ARG(out, "null out");
  int rc = gb_check_shape(__func__, nkeys, nvals, capacity);
  if (rc) return rc;
  void *block = nullptr;
  if (hipMalloc(&block, gb_layout(nkeys, nvals, flags, capacity).bytes) != hipSuccess) {
    set_error("nvt_gb_create: hipMalloc failed for capacity %llu", (unsigned long long)capacity);
    return NVT_ENOMEM;
  }
  nvt_gb_table *t = gb_table_over(nkeys, nvals, flags, capacity, block);
  t->block = block;
  *out = t;
  return NVT_OK;
}

// device address of the table's uint64[NVT_STATE_WORDS] state block (for nvt_mailbox_post)
uint64_t *nvt_gb_state_ptr(nvt_gb_table *t) { return t ? t->state : nullptr; }

int nvt_gb_update_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  *bytes = WordsWs(nullptr, n).bytes;
  return NVT_OK;
}
// caller-owned scratch for nvt_gb_update (nvt_gb_update_ws_bytes(n)); NULL returns to the
// table-owned, grown-on-demand buffer
int nvt_gb_set_workspace(nvt_gb_table *t, void *ws, uint64_t bytes) {
  NVT_CHECK_ARG(t, "null table");
  if (t->scratch && !t->external_scratch) (void)hipFree(t->scratch);
  t->scratch = ws;
  t->scratch_bytes = ws ? bytes : 0;
  t->external_scratch = ws ? 1 : 0;
  return NVT_OK;
}

int nvt_gb_clear(nvt_gb_table *t, void *stream) {
  NVT_CHECK_ARG(t, "null table");
  NVT_PROF("groupby_clear", 0, (hipStream_t)stream);
  gb_clear_kernel<<<stream_grid(t->capacity, kBlock * 2), kBlock, 0, (hipStream_t)stream>>>(
      view_of(t));
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_gb_update(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *const *key_valid,
                  const void *const *vals, const int *vdtypes, const uint8_t *const *val_valid,
                  uint64_t n, void *stream) {
  NVT_CHECK_ARG(t && keys, "null table/keys");
  NVT_CHECK_ARG(t->nvals == 0 || (vals && vdtypes), "null vals");
  if (n == 0) return NVT_OK;
  GbRowArgs a;
  int rc = row_args(a, __func__, t->nkeys, keys, key_valid, t->nvals, vals, vdtypes, val_valid);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_update", 0, s);
  if (n < (1ull << 15) || n >= (1ull << 30) || t->capacity > (1ull << 31)) {
    // tiny inputs (the sort would be launch latency) and > 2^30 rows per call: per-row atomics
    gb_update_kernel<<<stream_grid(n, kBlock * 2), kBlock, 0, s>>>(view_of(t), a, n);
    NVT_CHECK_LAUNCH();
    return NVT_OK;
  }
  const uint64_t need = WordsWs(nullptr, n).bytes;
  if (t->scratch_bytes < need) {
    NVT_CHECK_ARG(!t->external_scratch, "workspace set by nvt_gb_set_workspace is too small");
    if (t->scratch) {
      NVT_CHECK_HIP(hipStreamSynchronize(s));
      NVT_CHECK_HIP(hipFree(t->scratch));
      t->scratch = nullptr;
      t->scratch_bytes = 0;
    }
    const uint64_t grow = need + need / 4;
    if (hipMalloc(&t->scratch, grow) != hipSuccess) {
      set_error("nvt_gb_update: hipMalloc of %llu scratch bytes failed", (unsigned long long)grow);
      return NVT_ENOMEM;
    }
    t->scratch_bytes = grow;
  }
  const WordsWs ws(t->scratch, n);
  gb_assign_kernel<<<stream_grid(n, kBlock * 2), kBlock, 0, s>>>(view_of(t), a, n, ws.words);
  NVT_CHECK_LAUNCH();
  int cap_bits = 1;  // slots are < capacity; the overflow marker `capacity` needs one more bit
  while ((1ull << cap_bits) <= t->capacity) ++cap_bits;
  uint64_t *sorted = nullptr;
  rc = sort_words_bits(ws.words, n, 32, 32 + cap_bits, ws.sort_tmp, &sorted, s);
  if (rc) return rc;
  segreduce_launch(view_of(t), a, n, sorted, 1u, false, s);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

static int fill_merge_args(nvt_gb_table *t, GbMergeArgs &a, const int64_t *const *keys,
                           const uint8_t *null_mask, const int64_t *size, const int64_t *count,
                           const double *const *sum, const double *const *sumsq,
                           const double *const *vmin, const double *const *vmax) {
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < t->nkeys; ++j) {
    NVT_CHECK_ARG(keys && keys[j], "null key column");
    a.keys[j] = keys[j];
  }
  a.null_mask = null_mask;
  a.size = size;
  a.count = count;
  for (int j = 0; j < t->nvals; ++j) {
    a.sum[j] = sum ? sum[j] : nullptr;
    a.sumsq[j] = sumsq ? sumsq[j] : nullptr;
    a.vmin[j] = vmin ? vmin[j] : nullptr;
    a.vmax[j] = vmax ? vmax[j] : nullptr;
    NVT_CHECK_ARG((a.vmin[j] == nullptr) == (a.vmax[j] == nullptr), "min/max come in pairs");
  }
  return NVT_OK;
}

int nvt_gb_merge(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *key_null_mask,
                 const int64_t *size, const int64_t *count, const double *const *sum,
                 const double *const *sumsq, const double *const *vmin,
                 const double *const *vmax, uint64_t n, void *stream) {
  NVT_CHECK_ARG(t, "null table");
  if (n == 0) return NVT_OK;
  GbMergeArgs a;
  int rc = fill_merge_args(t, a, keys, key_null_mask, size, count, sum, sumsq, vmin, vmax);
  if (rc) return rc;
  gb_merge_kernel<<<stream_grid(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(view_of(t), a, n);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_gb_state(nvt_gb_table *t, uint64_t *host_state, void *stream) {
  NVT_CHECK_ARG(t && host_state, "null pointer");
  NVT_CHECK_HIP(hipMemcpyAsync(host_state, t->state, NVT_STATE_WORDS * 8, hipMemcpyDeviceToHost,
                               (hipStream_t)stream));
  NVT_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  return NVT_OK;
}

int nvt_gb_compact(nvt_gb_table *t, int64_t *const *out_keys, uint8_t *out_null_mask,
                   int64_t *out_size, int64_t *out_count, double *const *out_sum,
                   double *const *out_sumsq, double *const *out_min, double *const *out_max,
                   uint64_t *out_n, void *stream) {
  NVT_CHECK_ARG(t && out_n, "null pointer");
  GbOutArgs o;
  memset(&o, 0, sizeof(o));
  for (int j = 0; j < t->nkeys; ++j) o.keys[j] = out_keys ? out_keys[j] : nullptr;
  o.null_mask = out_null_mask;
  o.size = out_size;
  o.count = out_count;
  for (int j = 0; j < t->nvals; ++j) {
    o.sum[j] = out_sum ? out_sum[j] : nullptr;
    o.sumsq[j] = out_sumsq ? out_sumsq[j] : nullptr;
    o.vmin[j] = out_min ? out_min[j] : nullptr;
    o.vmax[j] = out_max ? out_max[j] : nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_compact", 0, s);
  NVT_CHECK_HIP(hipMemsetAsync(out_n, 0, sizeof(uint64_t), s));
  gb_compact_kernel<<<stream_grid(t->capacity, kBlock * kGbCompactItems), kBlock, 0, s>>>(view_of(t), o, out_n);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_gb_index_build(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *key_null_mask,
                       uint64_t n_groups, void *stream) {
  NVT_CHECK_ARG(t, "null table");
  NVT_CHECK_ARG(n_groups < t->capacity, "capacity must exceed the number of groups");
  int rc = nvt_gb_clear(t, stream);
  if (rc) return rc;
  if (n_groups == 0) return NVT_OK;
  GbMergeArgs a;
  rc = fill_merge_args(t, a, keys, key_null_mask, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr);
  if (rc) return rc;
  gb_index_build_kernel<<<stream_grid(n_groups, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      view_of(t), a, n_groups);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_gb_lookup(nvt_gb_table *t, const int64_t *const *keys, const uint8_t *const *key_valid,
                  uint64_t n, int64_t *out_group, void *stream) {
  NVT_CHECK_ARG(t && keys && out_group, "null pointer");
  if (n == 0) return NVT_OK;
  GbRowArgs a;
  int rc = row_args(a, __func__, t->nkeys, keys, key_valid, 0, nullptr, nullptr, nullptr);
  if (rc) return rc;
  NVT_PROF("groupby_lookup", n * 8ull * (uint64_t)t->nkeys, (hipStream_t)stream);
  gb_lookup_kernel<<<stream_grid(n, kBlock * 2), kBlock, 0, (hipStream_t)stream>>>(view_of(t), a,
                                                                                    n, out_group);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
