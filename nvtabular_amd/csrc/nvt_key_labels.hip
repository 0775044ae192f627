// Dense labels of a low-cardinality key (Dataset.to_parquet(partition_on=...)).
//
//   nvt_key_labels   label[i] = rank of row i's key among the distinct keys, ordered by first row
//
// The keys are the tags of nvt_join_hash.  At most NVT_LABEL_MAX of them are distinct, so the whole
// key set fits in LDS and the rows are read twice, at stream rate, with no table traffic to HBM.
//
// Four launches, so nothing depends on how workgroups are scheduled:
//   init    the global table (2 * NVT_LABEL_MAX tag slots + the two keys that have no tag slot)
//           and the status words
//   dedup   G <= 256 workgroups each own a contiguous run of whole tiles (NVT_LABEL_TILE rows) and
//           insert their rows into a workgroup-private LDS table: 64-bit CAS on the tag, atomicMin
//           on the first row.  At the end the workgroup merges its distinct keys into the global
//           table the same way (CAS on the tag, atomicMin on the first row); a global fill count
//           raises status 1.  A minimum does not depend on the order it is taken in.
//   rank    one workgroup lists the occupied slots as (first row, slot), sorts the at most 4096
//           words in LDS (bitonic) and writes the label of every slot, first_row and state[0].
//           First rows are distinct -- a row has one key -- so the order is total.
//   label   workgroups copy the tags and the slots' labels into LDS and label every row from there.
//           With 2+ key components a row's words and null bits are compared with those of its
//           key's first row (few rows, resident in L2): a difference is status 2.
//
// Two keys have no tag slot.  The tag 2^63 marks an empty slot, so rows with that tag share the
// entry kSlotEmptyTag; with ONE key component the rows with a null bit are one key whatever their
// tag, the entry kSlotNullKey.
//
// LDS.  dedup: 8192 tags (64 KiB) + 8194 first rows (32 KiB) = 96 KiB; label: 8192 tags + 8194
// 16-bit labels = 80 KiB.  Both run 1024 threads: one workgroup and 16 waves per CU.  (Two label
// workgroups of 512 threads would need 2 x 80 KiB, all 160 KiB of a CU to the byte; the same 16
// waves in one workgroup copy the table once per CU instead of twice.)  The local table is never
// more than three quarters full: a workgroup that has seen more than NVT_LABEL_MAX keys stops at
// the next tile boundary, and a tile adds at most NVT_LABEL_TILE = 2048 to the 4096 before it.
#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr int kLabBS = 1024;
constexpr int kLabSteps = NVT_LABEL_TILE / kLabBS;
constexpr unsigned kLabSlots = 2 * NVT_LABEL_MAX;
constexpr unsigned kSlotEmptyTag = kLabSlots, kSlotNullKey = kLabSlots + 1, kLabEntries = kLabSlots + 2;
constexpr unsigned long long kLabEmpty = 0x8000000000000000ull;
constexpr unsigned kNoRow = 0xFFFFFFFFu;
static_assert(NVT_LABEL_TILE % kLabBS == 0, "a tile is whole steps of the workgroup");
static_assert(NVT_LABEL_MAX + NVT_LABEL_TILE < kLabSlots, "the local table keeps a free slot");
static_assert(NVT_LABEL_MAX <= 65536, "labels are staged as 16 bits");

// workspace: tags | first rows | labels | fill count, every block on a 16-byte boundary
struct LabelWs {
  unsigned long long *tag;  // [kLabSlots]
  unsigned *first;          // [kLabEntries]
  uint16_t *label;          // [kLabEntries]
  unsigned *fill;           // distinct tags in `tag`
};
constexpr uint64_t kWsTag = 0;
constexpr uint64_t kWsFirst = kWsTag + (uint64_t)kLabSlots * 8;
constexpr uint64_t kWsLabel = kWsFirst + (((uint64_t)kLabEntries * 4 + 15) & ~15ull);
constexpr uint64_t kWsFill = kWsLabel + (((uint64_t)kLabEntries * 2 + 15) & ~15ull);
constexpr uint64_t kWsBytes = kWsFill + 16;

LabelWs label_ws(void *ws) {
  char *p = (char *)ws;
  return LabelWs{(unsigned long long *)(p + kWsTag), (unsigned *)(p + kWsFirst), (uint16_t *)(p + kWsLabel),
                 (unsigned *)(p + kWsFill)};
}

struct LabelShape {
  unsigned groups;
  uint64_t rows_per_grp;  // a multiple of the tile
};
LabelShape label_shape(uint64_t n) {
  LabelShape s;
  const uint64_t ntiles = (n + NVT_LABEL_TILE - 1) / NVT_LABEL_TILE;
  const uint64_t per = (ntiles + kCUs - 1) / kCUs;
  s.rows_per_grp = (per ? per : 1) * NVT_LABEL_TILE;
  s.groups = (unsigned)((n + s.rows_per_grp - 1) / s.rows_per_grp);
  if (s.groups == 0) s.groups = 1;
  return s;
}

// home slot: the tag of a single component is the raw value (consecutive integers, k << 13 ...)
__device__ __forceinline__ unsigned label_home(unsigned long long tag) {
  return (unsigned)(fmix64(tag) >> 32) & (kLabSlots - 1);
}

__global__ __launch_bounds__(kBlock) void label_init_kernel(LabelWs w, uint64_t *__restrict__ state) {
  for (unsigned s = blockIdx.x * kBlock + threadIdx.x; s < kLabEntries; s += gridDim.x * kBlock) {
    if (s < kLabSlots) w.tag[s] = kLabEmpty;
    w.first[s] = kNoRow;
    w.label[s] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *w.fill = 0;
    state[0] = 0;
    state[1] = 0;
  }
}

__global__ __launch_bounds__(kLabBS) void label_dedup_kernel(const uint64_t *__restrict__ tags,
                                                             const uint8_t *__restrict__ nulls, int nkeys,
                                                             uint64_t n, uint64_t rows_per_grp, LabelWs w,
                                                             uint64_t *__restrict__ state) {
  __shared__ unsigned long long ltag[kLabSlots];
  __shared__ unsigned lfirst[kLabEntries];
  __shared__ unsigned lfill;
  for (unsigned s = threadIdx.x; s < kLabEntries; s += kLabBS) {
    if (s < kLabSlots) ltag[s] = kLabEmpty;
    lfirst[s] = kNoRow;
  }
  if (threadIdx.x == 0) lfill = 0;
  __syncthreads();
  const uint64_t lo = (uint64_t)blockIdx.x * rows_per_grp;
  const uint64_t hi = lo + rows_per_grp < n ? lo + rows_per_grp : n;
  bool full = false;
  for (uint64_t t = lo; t < hi && !full; t += NVT_LABEL_TILE) {
    int over = 0;
#pragma unroll
    for (int r = 0; r < kLabSteps; ++r) {
      const uint64_t i = t + (uint64_t)r * kLabBS + threadIdx.x;
      if (i >= hi) continue;
      const unsigned long long tag = tags[i];
      const bool null_key = nkeys == 1 && nulls[i] != 0;
      if (null_key || tag == kLabEmpty) {
        atomicMin(&lfirst[null_key ? kSlotNullKey : kSlotEmptyTag], (unsigned)i);
        continue;
      }
      const unsigned h = label_home(tag);
      for (unsigned p = 0; p < kLabSlots; ++p) {
        const unsigned s = (h + p) & (kLabSlots - 1);
        unsigned long long cur = ltag[s];
        if (cur == kLabEmpty) {
          cur = atomicCAS(&ltag[s], kLabEmpty, tag);
          if (cur == kLabEmpty) {
            cur = tag;
            if (atomicAdd(&lfill, 1u) >= NVT_LABEL_MAX) over = 1;
          }
        }
        if (cur == tag) {
          atomicMin(&lfirst[s], (unsigned)i);
          break;
        }
      }
    }
    full = __syncthreads_or(over) != 0;  // (the same in every thread: the loop ends for all or none)
  }
  if (full) {
    if (threadIdx.x == 0) atomicMax((unsigned long long *)&state[1], 1ull);
    return;
  }
  for (unsigned s = threadIdx.x; s < kLabEntries; s += kLabBS) {
    const unsigned fr = lfirst[s];
    if (fr == kNoRow) continue;
    if (s >= kLabSlots) {
      atomicMin(&w.first[s], fr);
      continue;
    }
    if (__hip_atomic_load(w.fill, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > NVT_LABEL_MAX) {
      atomicMax((unsigned long long *)&state[1], 1ull);  // (already too many: leave the table alone)
      continue;
    }
    const unsigned long long tag = ltag[s];
    const unsigned h = label_home(tag);
    for (unsigned p = 0; p < kLabSlots; ++p) {
      const unsigned g = (h + p) & (kLabSlots - 1);
      unsigned long long cur = __hip_atomic_load(&w.tag[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kLabEmpty) {
        cur = atomicCAS(&w.tag[g], kLabEmpty, tag);
        if (cur == kLabEmpty) {
          cur = tag;
          if (atomicAdd(w.fill, 1u) >= NVT_LABEL_MAX) atomicMax((unsigned long long *)&state[1], 1ull);
        }
      }
      if (cur == tag) {
        atomicMin(&w.first[g], fr);
        break;
      }
    }
  }
}

__global__ __launch_bounds__(kLabBS) void label_rank_kernel(LabelWs w, uint32_t *__restrict__ first_row,
                                                            uint64_t *__restrict__ state) {
  __shared__ unsigned long long ent[NVT_LABEL_MAX];  // (first row << 32) | slot
  __shared__ unsigned cnt, status;
  for (unsigned q = threadIdx.x; q < NVT_LABEL_MAX; q += kLabBS) ent[q] = ~0ull;
  if (threadIdx.x == 0) {
    cnt = 0;
    status = (unsigned)state[1];
  }
  __syncthreads();
  if (status != 0) return;
  for (unsigned s = threadIdx.x; s < kLabEntries; s += kLabBS) {
    const unsigned fr = w.first[s];
    if (fr == kNoRow) continue;
    const unsigned pos = atomicAdd(&cnt, 1u);  // (any order: the list is sorted next)
    if (pos < NVT_LABEL_MAX) ent[pos] = ((unsigned long long)fr << 32) | s;
  }
  __syncthreads();
  const unsigned D = cnt;
  if (D > NVT_LABEL_MAX) {
    if (threadIdx.x == 0) state[1] = 1;
    return;
  }
  unsigned P = 2;
  while (P < D) P <<= 1;
  for (unsigned k = 2; k <= P; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned i = threadIdx.x; i < P; i += kLabBS) {
        const unsigned l = i ^ j;
        if (l > i) {
          const unsigned long long a = ent[i], b = ent[l];
          if (((i & k) == 0) == (a > b)) {
            ent[i] = b;
            ent[l] = a;
          }
        }
      }
      __syncthreads();
    }
  for (unsigned r = threadIdx.x; r < D; r += kLabBS) {
    const unsigned long long v = ent[r];
    w.label[(unsigned)v] = (uint16_t)r;
    first_row[r] = (uint32_t)(v >> 32);
  }
  if (threadIdx.x == 0) state[0] = D;
}

__global__ __launch_bounds__(kLabBS) void label_rows_kernel(const uint64_t *__restrict__ tags,
                                                            const uint8_t *__restrict__ nulls,
                                                            const uint64_t *__restrict__ words, int nkeys,
                                                            uint64_t n, LabelWs w,
                                                            const uint32_t *__restrict__ first_row,
                                                            uint32_t *__restrict__ label,
                                                            uint64_t *__restrict__ state) {
  __shared__ unsigned long long ltag[kLabSlots];
  __shared__ uint16_t llabel[kLabEntries];
  __shared__ unsigned status;
  if (threadIdx.x == 0) status = (unsigned)__hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (unsigned s = threadIdx.x; s < kLabEntries; s += kLabBS) {
    if (s < kLabSlots) ltag[s] = w.tag[s];
    llabel[s] = w.label[s];
  }
  __syncthreads();
  if (status == 1) return;  // (too many keys: no labels; a collision seen elsewhere does not stop the rest)
  for (uint64_t i = (uint64_t)blockIdx.x * kLabBS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kLabBS) {
    const unsigned long long tag = tags[i];
    const uint8_t nl = nulls[i];
    unsigned lab = 0;
    if (nkeys == 1 && nl != 0) {
      lab = llabel[kSlotNullKey];
    } else if (tag == kLabEmpty) {
      lab = llabel[kSlotEmptyTag];
    } else {
      const unsigned h = label_home(tag);
      for (unsigned p = 0; p < kLabSlots; ++p) {
        const unsigned s = (h + p) & (kLabSlots - 1);
        const unsigned long long cur = ltag[s];
        if (cur == tag) {
          lab = llabel[s];
          break;
        }
        if (cur == kLabEmpty) break;
      }
    }
    label[i] = lab;
    if (nkeys >= 2) {
      const uint64_t fr = first_row[lab];  // (lab < D and first_row[lab] < n whenever status is 0)
      bool differs = nulls[fr] != nl;
      for (int j = 0; j < nkeys; ++j) differs |= words[(uint64_t)j * n + fr] != words[(uint64_t)j * n + i];
      if (differs) atomicMax((unsigned long long *)&state[1], 2ull);
    }
  }
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_key_labels_tile_rows(void) { return NVT_LABEL_TILE; }

int nvt_key_labels_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  NVT_CHECK_ARG(n < (1ull << 32), "rows must be below 2^32");
  *bytes = kWsBytes;
  return NVT_OK;
}

int nvt_key_labels(const uint64_t *tags, const uint8_t *nulls, const uint64_t *words, int nkeys, uint64_t n,
                   uint32_t *label, uint32_t *first_row, uint64_t *state, void *ws, uint64_t ws_bytes,
                   void *stream) {
  NVT_CHECK_ARG(nkeys >= 1 && nkeys <= NVT_JOIN_MAX_KEYS, "nkeys must be 1 to 4");
  NVT_CHECK_ARG(n < (1ull << 32), "rows must be below 2^32");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(tags && nulls && label && first_row && state, "null pointer");
  NVT_CHECK_ARG(nkeys == 1 || words, "null words with two or more key components");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "workspace must be 16-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= kWsBytes, "workspace smaller than nvt_key_labels_ws_bytes(n)");
  const LabelWs w = label_ws(ws);
  const LabelShape sh = label_shape(n);
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("key_labels", n * 22, s);
  label_init_kernel<<<(kLabEntries + kBlock - 1) / kBlock, kBlock, 0, s>>>(w, state);
  NVT_CHECK_LAUNCH();
  label_dedup_kernel<<<sh.groups, kLabBS, 0, s>>>(tags, nulls, nkeys, n, sh.rows_per_grp, w, state);
  NVT_CHECK_LAUNCH();
  label_rank_kernel<<<1, kLabBS, 0, s>>>(w, first_row, state);
  NVT_CHECK_LAUNCH();
  label_rows_kernel<<<stream_grid(n, kLabBS, 1), kLabBS, 0, s>>>(tags, nulls, words, nkeys, n, w, first_row, label,
                                                                   state);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
