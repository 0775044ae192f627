// Hash partitioning of rows by key (Dataset.shuffle_by_keys).
//
//   nvt_partition_ids          partition id of every row from its 64-bit key tag (nvt_join_hash)
//   nvt_partition_plan         stable counting sort of the row indices by partition id
//   nvt_partition_gather_many  one output partition from slices of the input partitions' plans
//
// Plan.  G workgroups each own a contiguous run of whole tiles (NVT_PARTITION_TILE rows).  Three
// steps, each its own launch, so nothing depends on how workgroups are scheduled:
//   hist     per-workgroup histogram in LDS -> hist[p * G + g]       (integer LDS atomics: the
//            counts do not depend on their order)
//   scan     exclusive scan of hist in that (partition, workgroup) order (nvt_scan.hpp): the first
//            output position of the rows of partition p inside workgroup g
//   scatter  the workgroup walks its tiles in row order with a cursor per partition in LDS.  Inside
//            a tile wave w owns rows [128 w, 128 w + 128) in two steps of 64.  A row's rank among
//            the tile's rows of its partition is
//              (rows of earlier waves) + (rows of this wave's earlier step) + (lower lanes)
//            lower lanes: a ballot per bit of the id gives the lanes with the same id; the lowest of
//            them adds the wave's count into byte w of a packed word per partition (a wave holds at
//            most 128 rows of a tile, so a byte never carries), and the value that add returns has
//            in byte w what this wave's earlier step counted -- only wave w ever changes byte w, in
//            program order.  After a barrier the bytes below w are the earlier waves.
//          Every position is a function of the input alone: two runs give the same perm.
//
// Gather.  A wave owns 64 consecutive output rows; a row finds its segment by bisection over the
// segment starts staged in LDS, reads its source row from that segment's slice of a plan, and the
// validity word of the 64 rows is one ballot stored by lane 0 -- also where a segment boundary
// falls inside the word, which is why the gather runs per output partition.
#include "nvt_common.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr int kPSteps = NVT_PARTITION_TILE / kBlock;  // 64-row steps of one wave per tile
constexpr uint32_t kPMaxGroups = 1024;                // workgroups of a plan
static_assert(NVT_PARTITION_TILE % kBlock == 0 && kPSteps * kWave <= 255, "a wave's rows of a tile fit a byte");
static_assert(kBlock / kWave == 4, "four byte counters per packed word");

// the fixed finaliser of nvt_hip.h (splitmix64's)
__host__ __device__ __forceinline__ uint64_t partition_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__global__ __launch_bounds__(kBlock) void pid_kernel(const uint64_t *__restrict__ tags, uint64_t n, uint32_t P,
                                                     uint32_t *__restrict__ pid) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    pid[i] = (uint32_t)(((partition_mix(tags[i]) >> 32) * (uint64_t)P) >> 32);
}

struct PlanShape {
  uint32_t groups;        // workgroups
  uint64_t rows_per_grp;  // a multiple of the tile
  int nbits;              // 2^nbits >= P
};

PlanShape plan_shape(uint64_t n, uint32_t P) {
  PlanShape s;
  const uint64_t ntiles = (n + NVT_PARTITION_TILE - 1) / NVT_PARTITION_TILE;
  const uint64_t per = (ntiles + kPMaxGroups - 1) / kPMaxGroups;
  s.rows_per_grp = (per ? per : 1) * NVT_PARTITION_TILE;
  s.groups = (uint32_t)((n + s.rows_per_grp - 1) / s.rows_per_grp);
  if (s.groups == 0) s.groups = 1;
  s.nbits = 0;
  while ((1u << s.nbits) < P) ++s.nbits;
  return s;
}

uint64_t plan_hist_bytes(const PlanShape &s, uint32_t P) { return ((uint64_t)P * s.groups * 4 + 15) & ~15ull; }

// the active lanes whose id equals this lane's (garbage in an inactive lane)
__device__ __forceinline__ uint64_t same_id_lanes(unsigned id, bool act, int nbits) {
  uint64_t peers = __ballot(act);
  for (int b = 0; b < nbits; ++b) {
    const bool set = (id >> b) & 1u;
    const uint64_t m = __ballot(act && set);
    peers &= set ? m : ~m;
  }
  return peers;
}

__global__ __launch_bounds__(kBlock) void plan_hist_kernel(const uint32_t *__restrict__ pid, uint64_t n, uint32_t P,
                                                           int nbits, uint64_t rows_per_grp,
                                                           uint32_t *__restrict__ hist) {
  extern __shared__ unsigned plan_lds[];  // P counters
  for (uint32_t q = threadIdx.x; q < P; q += kBlock) plan_lds[q] = 0;
  __syncthreads();
  const uint64_t lo = (uint64_t)blockIdx.x * rows_per_grp;
  const uint64_t hi = lo + rows_per_grp < n ? lo + rows_per_grp : n;
  const unsigned lane = lane_id();
  for (uint64_t t = lo; t < hi; t += kBlock) {
    const uint64_t i = t + threadIdx.x;
    const bool act = i < hi;
    unsigned p = act ? pid[i] : 0u;
    p = p < P ? p : P - 1;  // (an id outside [0, P) never leaves the counters)
    const uint64_t peers = same_id_lanes(p, act, nbits);
    if (act && (unsigned)__ffsll((long long)peers) - 1u == lane) atomicAdd(&plan_lds[p], (unsigned)__popcll(peers));
  }
  __syncthreads();
  for (uint32_t q = threadIdx.x; q < P; q += kBlock) hist[(uint64_t)q * gridDim.x + blockIdx.x] = plan_lds[q];
}

__global__ __launch_bounds__(kBlock) void plan_counts_kernel(const uint32_t *__restrict__ first, uint32_t P,
                                                             uint32_t groups, uint64_t n,
                                                             uint64_t *__restrict__ counts) {
  for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < P; q += gridDim.x * kBlock) {
    const uint64_t a = first[(uint64_t)q * groups];
    const uint64_t b = q + 1 < P ? (uint64_t)first[(uint64_t)(q + 1) * groups] : n;
    counts[q] = b - a;
  }
}

__device__ __forceinline__ unsigned bytes_below(unsigned v, unsigned w) {
  unsigned s = 0;
#pragma unroll
  for (unsigned k = 0; k < kBlock / kWave; ++k)
    if (k < w) s += (v >> (8 * k)) & 0xFFu;
  return s;
}

__global__ __launch_bounds__(kBlock) void plan_scatter_kernel(const uint32_t *__restrict__ pid, uint64_t n,
                                                              uint32_t P, int nbits, uint64_t rows_per_grp,
                                                              const uint32_t *__restrict__ first,
                                                              int64_t *__restrict__ perm) {
  extern __shared__ unsigned plan_lds[];  // P cursors, then P packed per-wave counts of the tile
  unsigned *cursor = plan_lds, *wave_cnt = plan_lds + P;
  for (uint32_t q = threadIdx.x; q < P; q += kBlock) {
    cursor[q] = first[(uint64_t)q * gridDim.x + blockIdx.x];
    wave_cnt[q] = 0;
  }
  __syncthreads();
  const uint64_t lo = (uint64_t)blockIdx.x * rows_per_grp;
  const uint64_t hi = lo + rows_per_grp < n ? lo + rows_per_grp : n;
  const unsigned lane = lane_id(), w = threadIdx.x / kWave, shift = 8 * w;
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t t = lo; t < hi; t += NVT_PARTITION_TILE) {
    uint64_t row[kPSteps];
    unsigned p[kPSteps], rank[kPSteps];
    bool act[kPSteps], opens[kPSteps];
#pragma unroll
    for (int r = 0; r < kPSteps; ++r) {
      row[r] = t + (uint64_t)w * (kPSteps * kWave) + (uint64_t)r * kWave + lane;
      act[r] = row[r] < hi;
      const unsigned v = act[r] ? pid[row[r]] : 0u;
      p[r] = v < P ? v : P - 1;
    }
#pragma unroll
    for (int r = 0; r < kPSteps; ++r) {
      const uint64_t peers = same_id_lanes(p[r], act[r], nbits);
      const unsigned leader = (unsigned)__ffsll((long long)peers) - 1u;
      unsigned old = 0;
      if (act[r] && leader == lane) old = atomicAdd(&wave_cnt[p[r]], (unsigned)__popcll(peers) << shift);
      old = (__shfl(old, (int)(leader & 63u), 64) >> shift) & 0xFFu;  // this wave's earlier steps
      rank[r] = old + (unsigned)__popcll(peers & below);
      opens[r] = act[r] && leader == lane && old == 0;  // first rows of the id in this wave
    }
    __syncthreads();
    unsigned packed[kPSteps];
#pragma unroll
    for (int r = 0; r < kPSteps; ++r) {
      packed[r] = 0;
      if (act[r]) {
        packed[r] = wave_cnt[p[r]];
        const unsigned before = bytes_below(packed[r], w);
        perm[(uint64_t)cursor[p[r]] + before + rank[r]] = (int64_t)row[r];
        opens[r] = opens[r] && before == 0;  // ... and in the tile: one lane per id present
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPSteps; ++r)
      if (opens[r]) {
        cursor[p[r]] += bytes_below(packed[r], kBlock / kWave);
        wave_cnt[p[r]] = 0;
      }
    __syncthreads();
  }
}

struct PCol {
  const void *const *src;
  const uint8_t *const *src_valid;
  void *dst;
  uint64_t *dst_valid;
  int width;
};
struct PBatch {
  PCol c[NVT_PARTITION_MAX_COLS];
  int ncols;
};

__global__ __launch_bounds__(kBlock) void pgather_kernel(PBatch b, const nvt_partition_seg *__restrict__ segs,
                                                         int nsegs, uint64_t m) {
  __shared__ uint64_t seg_start[NVT_PARTITION_MAX_SEGS];
  __shared__ const int64_t *seg_idx[NVT_PARTITION_MAX_SEGS];
  for (int q = threadIdx.x; q < nsegs; q += kBlock) {
    seg_start[q] = segs[q].start;
    seg_idx[q] = segs[q].idx;
  }
  __syncthreads();
  const uint64_t nchunks = (m + 63) / 64;
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / kWave);
  const unsigned lane = lane_id();
  for (uint64_t c = wave; c < nchunks; c += nwaves) {
    const uint64_t row = c * 64 + lane;
    const bool in = row < m;
    int s = 0;
    uint64_t f = 0;
    if (in) {
      int hi = nsegs;  // the last segment with start <= row (empty segments are passed over)
      while (hi - s > 1) {
        const int mid = (s + hi) >> 1;
        if (seg_start[mid] <= row) s = mid;
        else hi = mid;
      }
      f = (uint64_t)seg_idx[s][row - seg_start[s]];
    }
    for (int j = 0; j < b.ncols; ++j) {
      const PCol &g = b.c[j];
      if (in) {
        const void *src = g.src[s];
        if (g.width == 8) ((uint64_t *)g.dst)[row] = ((const uint64_t *)src)[f];
        else if (g.width == 4) ((uint32_t *)g.dst)[row] = ((const uint32_t *)src)[f];
        else if (g.width == 2) ((uint16_t *)g.dst)[row] = ((const uint16_t *)src)[f];
        else ((uint8_t *)g.dst)[row] = ((const uint8_t *)src)[f];
      }
      if (g.dst_valid != nullptr) {
        const uint64_t word = __ballot(in && bit_valid(g.src_valid[s], f));  // (no bitmap: all valid)
        if (lane == 0) g.dst_valid[c] = word;
      }
    }
  }
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_partition_tile_rows(void) { return NVT_PARTITION_TILE; }

int nvt_partition_ids(const uint64_t *tags, uint64_t n, uint32_t P, uint32_t *pid, void *stream) {
  NVT_CHECK_ARG(P >= 1 && P <= NVT_PARTITION_MAX, "P must be 1 to 4096");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(tags && pid, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("partition_ids", n * 12, s);
  pid_kernel<<<stream_grid(n, kBlock * 4), kBlock, 0, s>>>(tags, n, P, pid);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_partition_plan_ws_bytes(uint64_t n, uint32_t P, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  NVT_CHECK_ARG(P >= 1 && P <= NVT_PARTITION_MAX, "P must be 1 to 4096");
  NVT_CHECK_ARG(n < (1ull << 32), "rows must be below 2^32");
  const PlanShape sh = plan_shape(n, P);
  *bytes = plan_hist_bytes(sh, P) + scan_chunks((uint64_t)P * sh.groups) * 8;
  return NVT_OK;
}

int nvt_partition_plan(const uint32_t *pid, uint64_t n, uint32_t P, int64_t *perm, uint64_t *counts, void *ws,
                       uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(P >= 1 && P <= NVT_PARTITION_MAX, "P must be 1 to 4096");
  NVT_CHECK_ARG(n < (1ull << 32), "rows must be below 2^32");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(pid && perm && counts, "null pointer");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "workspace must be 16-byte aligned");
  const PlanShape sh = plan_shape(n, P);
  const uint64_t hist_bytes = plan_hist_bytes(sh, P);
  const uint64_t len = (uint64_t)P * sh.groups;
  NVT_CHECK_ARG(ws_bytes >= hist_bytes + scan_chunks(len) * 8, "workspace smaller than nvt_partition_plan_ws_bytes(n, P)");
  uint32_t *hist = (uint32_t *)ws;
  unsigned long long *chunk_tot = (unsigned long long *)((char *)ws + hist_bytes);
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("partition_plan", n * 16 + len * 16, s);
  plan_hist_kernel<<<sh.groups, kBlock, (size_t)P * 4, s>>>(pid, n, P, sh.nbits, sh.rows_per_grp, hist);
  NVT_CHECK_LAUNCH();
  const int rc = exclusive_scan_u32(hist, len, chunk_tot, s);
  if (rc) return rc;
  plan_counts_kernel<<<(P + kBlock - 1) / kBlock, kBlock, 0, s>>>(hist, P, sh.groups, n, counts);
  NVT_CHECK_LAUNCH();
  plan_scatter_kernel<<<sh.groups, kBlock, (size_t)P * 8, s>>>(pid, n, P, sh.nbits, sh.rows_per_grp, hist, perm);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_partition_gather_many(const nvt_partition_col *cols, int ncols, const nvt_partition_seg *segs, int nsegs,
                              uint64_t m, void *stream) {
  NVT_CHECK_ARG(cols, "null column descriptors");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= NVT_PARTITION_MAX_COLS, "ncols must be 1 to 16");
  PBatch b;
  memset(&b, 0, sizeof(b));
  b.ncols = ncols;
  uint64_t per_row = 8;
  for (int j = 0; j < ncols; ++j) {
    const nvt_partition_col &c = cols[j];
    NVT_CHECK_ARG(c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8, "width must be 1, 2, 4 or 8 bytes");
    NVT_CHECK_ARG((c.src && c.dst) || m == 0, "null column");
    NVT_CHECK_ARG((c.src_valid != nullptr) == (c.dst_valid != nullptr), "src_valid and dst_valid go together");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.dst_valid) & 7) == 0, "dst_valid must be 8-byte aligned");
    b.c[j] = PCol{c.src, c.src_valid, c.dst, reinterpret_cast<uint64_t *>(c.dst_valid), c.width};
    per_row += 2 * (uint64_t)c.width + (c.dst_valid ? 1 : 0);
  }
  if (m == 0) return NVT_OK;
  NVT_CHECK_ARG(segs, "null segments");
  NVT_CHECK_ARG(nsegs >= 1 && nsegs <= NVT_PARTITION_MAX_SEGS, "nsegs must be 1 to 1024");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("partition_gather", m * per_row, s);
  pgather_kernel<<<stream_grid((m + 63) / 64, kBlock / kWave), kBlock, 0, s>>>(b, segs, nsegs, m);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
