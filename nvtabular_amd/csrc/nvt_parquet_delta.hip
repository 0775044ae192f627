// Parquet in, DELTA_BINARY_PACKED data pages of flat INT32 / INT64 columns: the device half (DESIGN.md,
// "DELTA_BINARY_PACKED in the parquet reader").  The host (nvt_pq_decode_chunk_delta, nvt_parquet.hip)
// has walked the block headers of every page and staged the pages' bytes with one record per page and
// one per needed miniblock; nothing is decoded there.  Here
//
//   value k = first_value + sum_{j < k} (min_delta of j's block + the w-bit number j of its miniblock)
//
// is a bit-unpack and a prefix sum over the page, wrapping in the column's width.
//
//   tile     a run of floor(2048 / vpm) consecutive miniblocks of ONE page (vpm = values per miniblock,
//            a multiple of 32), i.e. up to 2048 deltas, taken by one workgroup of 256 lanes: lane t owns
//            the 8 consecutive deltas 8 t .. 8 t + 7, which lie in one miniblock and, at w bits each,
//            start at a BYTE of it.
//   staging  miniblocks start at any byte of the staged bytes (headers have odd lengths).  Every
//            miniblock of the tile gets a slot of 8 vpm + 32 bytes of LDS; the workgroup fills the
//            slots with aligned 16-byte global loads from the 16-byte boundary in front of the
//            miniblock on (the slot keeps the byte offset: at & 15), so that no global load is
//            unaligned or narrower than 16 bytes.  A value is then two (w <= 32) or three 32-bit LDS
//            reads and a funnel shift; w = 0 reads nothing, w = 64 is never shifted by 64.
//            (Slots per miniblock, not the tile's byte span: the span holds the block headers between
//            its miniblocks, which a page may make as long as it likes; the slots bound the LDS at
//            18 KiB whatever the page says.)
//   scan     three launches and no waiting between workgroups: pass 1 reduces every tile to its
//            wrapping sum, a wave per page turns the sums into the value in front of every tile, pass
//            2 unpacks again, scans (lane, wave, workgroup), adds the carry and passes the values
//            through LDS -- the slots are free by then -- so that the stores into the page's hole are
//            consecutive over the lanes.  Unpacking twice reads the 1 - 2 bytes per value twice;
//            storing deltas and fixing them up would read and write 8.
//
// Everything is computed in the column's width (uint32_t / uint64_t: unsigned arithmetic wraps).
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr unsigned kTile = NVT_PQ_DELTA_TILE;
constexpr unsigned kPer = kTile / kBlock;                 // deltas per lane
constexpr unsigned kMaxMbs = kTile / 32;                  // miniblocks per tile at the smallest vpm
constexpr unsigned kLdsBytes = kTile * 8 + kMaxMbs * 32;  // floor(2048 / vpm) slots of 8 vpm + 32 bytes
static_assert(kPer == 8 && kBlock / kWave == 4, "a lane owns one byte-aligned group of 8 deltas");
// the way out of pass 2: value e of the tile sits at element e + e / 8 (a lane writes its 8 values
// behind each other: the skew spreads the lanes over the banks); 2048 + 255 elements of 8 bytes
static_assert((kTile + kTile / 8) * 8 <= kLdsBytes, "the transposed values fit the slots");

// kernels_parquet_delta.fill_holes writes these records as 6 words of 8 bytes
static_assert(sizeof(nvt_pq_delta_page) == 48 && offsetof(nvt_pq_delta_page, mbs) == 8 &&
                  offsetof(nvt_pq_delta_page, dst) == 16 && offsetof(nvt_pq_delta_page, first_value) == 24 &&
                  offsetof(nvt_pq_delta_page, count) == 32 && offsetof(nvt_pq_delta_page, vpm) == 36 &&
                  offsetof(nvt_pq_delta_page, width) == 40 && offsetof(nvt_pq_delta_page, first_tile) == 44,
              "nvt_pq_delta_page: {bytes, mbs, dst, first_value, count | vpm << 32, width | first_tile << 32}");

struct MbRec {
  uint64_t at_w;      // byte position in the staged bytes | bit width << 56
  int64_t min_delta;
};

struct TileGeom {
  const MbRec *mb;    // the tile's first miniblock record
  unsigned vpm, nmb;  // values per miniblock; miniblocks of this tile
  unsigned valid;     // deltas of this tile that are values of the page
  uint64_t d0;        // the tile's first delta among the page's
};

__host__ __device__ inline uint64_t page_tiles(uint32_t count, uint32_t vpm) {
  const uint64_t per = (uint64_t)(kTile / vpm) * vpm;
  return ((uint64_t)count - 1 + per - 1) / per;
}

__device__ __forceinline__ TileGeom tile_geom(const nvt_pq_delta_page &pg, uint64_t tile) {
  TileGeom g;
  g.vpm = pg.vpm;
  const unsigned mpt = kTile / g.vpm, per = mpt * g.vpm;
  const uint64_t k = tile - pg.first_tile;
  g.d0 = k * per;
  const uint64_t left = (uint64_t)pg.count - 1 - g.d0;
  g.valid = left < per ? (unsigned)left : per;
  g.nmb = (g.valid + g.vpm - 1) / g.vpm;
  g.mb = reinterpret_cast<const MbRec *>(pg.mbs) + k * mpt;
  return g;
}

// the tile's miniblocks -> their slots; ends with a barrier
__device__ __forceinline__ void stage_tile(uint4 *lds16, const uint4 *__restrict__ bytes16, const TileGeom &g) {
  const unsigned cpm = g.vpm / 2 + 2;   // 16-byte chunks per slot
  for (unsigned i = threadIdx.x; i < g.nmb * cpm; i += kBlock) {
    const unsigned m = i / cpm, c = i - m * cpm;
    const uint64_t aw = g.mb[m].at_w;
    const unsigned w = (unsigned)(aw >> 56);
    const uint64_t at = aw & ((1ull << 56) - 1ull);
    // w = 0: nothing to read; else the chunks that hold bytes [at, at + vpm w / 8): at most vpm / 2 + 1
    const unsigned nch = w ? (unsigned)(((at & 15) + (uint64_t)g.vpm * w / 8 + 15) >> 4) : 0u;
    if (c < nch) lds16[m * cpm + c] = bytes16[(at >> 4) + c];
  }
  __syncthreads();
}

// v[j] = delta 8 t + j of the tile with its block's min_delta added, 0 behind the page's last delta
template <typename T>
__device__ __forceinline__ void unpack8(const uint32_t *lds, const TileGeom &g, T v[kPer]) {
  const unsigned d = threadIdx.x * kPer;
#pragma unroll
  for (unsigned j = 0; j < kPer; ++j) v[j] = 0;
  if (d >= g.valid) return;
  const unsigned m = d / g.vpm, i0 = d - m * g.vpm;
  const MbRec rec = g.mb[m];
  const unsigned w = (unsigned)(rec.at_w >> 56);
  const T md = (T)rec.min_delta;
  const uint32_t *slot = lds + m * (g.vpm * 2 + 8);   // (8 vpm + 32 bytes in words)
  const uint64_t mask = w >= 64 ? ~0ull : ((1ull << w) - 1ull);
  unsigned b = ((unsigned)(rec.at_w & 15) << 3) + i0 * w;   // bit position in the slot
#pragma unroll
  for (unsigned j = 0; j < kPer; ++j, b += w) {
    uint64_t x = 0;
    if (w) {
      const unsigned word = b >> 5, s = b & 31;
      x = ((uint64_t)slot[word + 1] << 32 | slot[word]) >> s;
      if (sizeof(T) == 8 && w > 32 && s) x |= (uint64_t)slot[word + 2] << (64 - s);
      x &= mask;
    }
    if (d + j < g.valid) v[j] = (T)x + md;
  }
}

template <typename T>
__device__ __forceinline__ void sum_body(uint4 *lds16, uint64_t *wsum, const nvt_pq_delta_page &pg,
                                         uint64_t *__restrict__ tile_sums) {
  const TileGeom g = tile_geom(pg, blockIdx.x);
  stage_tile(lds16, reinterpret_cast<const uint4 *>(pg.bytes), g);
  T v[kPer];
  unpack8<T>(reinterpret_cast<const uint32_t *>(lds16), g, v);
  T s = 0;
#pragma unroll
  for (unsigned j = 0; j < kPer; ++j) s += v[j];
  unsigned long long t = (unsigned long long)s;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if (lane_id() == 0) wsum[threadIdx.x / kWave] = t;
  __syncthreads();
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = (uint64_t)(T)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(kBlock) void delta_sum_kernel(const nvt_pq_delta_page *__restrict__ pages,
                                                           const uint32_t *__restrict__ tile_page,
                                                           uint64_t *__restrict__ tile_sums) {
  __shared__ uint4 lds16[kLdsBytes / 16];
  __shared__ uint64_t wsum[kBlock / kWave];
  const nvt_pq_delta_page pg = pages[tile_page[blockIdx.x]];
  if (pg.width == 4)
    sum_body<uint32_t>(lds16, wsum, pg, tile_sums);
  else
    sum_body<uint64_t>(lds16, wsum, pg, tile_sums);
}

// a wave per page: tile_sums[t] <- first_value + the sums of the page's tiles in front of t; value 0
__global__ __launch_bounds__(kBlock) void delta_carry_kernel(const nvt_pq_delta_page *__restrict__ pages,
                                                             uint64_t npages, uint64_t *__restrict__ tile_sums) {
  const uint64_t p = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (p >= npages) return;   // (uniform per wave)
  const unsigned lane = lane_id();
  const nvt_pq_delta_page pg = pages[p];
  unsigned long long carry = (unsigned long long)pg.first_value;
  if (lane == 0) {
    if (pg.width == 4)
      *reinterpret_cast<uint32_t *>(pg.dst) = (uint32_t)carry;
    else
      *reinterpret_cast<uint64_t *>(pg.dst) = carry;
  }
  const uint64_t nt = page_tiles(pg.count, pg.vpm);
  uint64_t *sums = tile_sums + pg.first_tile;
  for (uint64_t base = 0; base < nt; base += kWave) {   // (uniform)
    const uint64_t i = base + lane;
    const unsigned long long x = i < nt ? sums[i] : 0ull;
    unsigned long long inc = x;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const unsigned long long o = __shfl_up(inc, off, 64);
      if (lane >= (unsigned)off) inc += o;
    }
    if (i < nt) sums[i] = carry + inc - x;
    carry += __shfl(inc, kWave - 1, 64);
  }
}

template <typename T>
__device__ __forceinline__ void scan_body(uint4 *lds16, uint64_t *wsum, const nvt_pq_delta_page &pg,
                                          const uint64_t *__restrict__ tile_sums) {
  const TileGeom g = tile_geom(pg, blockIdx.x);
  stage_tile(lds16, reinterpret_cast<const uint4 *>(pg.bytes), g);
  T v[kPer];
  unpack8<T>(reinterpret_cast<const uint32_t *>(lds16), g, v);
#pragma unroll
  for (unsigned j = 1; j < kPer; ++j) v[j] += v[j - 1];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  unsigned long long inc = (unsigned long long)v[kPer - 1];
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long o = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += o;
  }
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();   // (every lane has read its slot: the slots become the way out)
  unsigned long long base = tile_sums[blockIdx.x] + inc - (unsigned long long)v[kPer - 1];
  for (unsigned q = 0; q < wave; ++q) base += wsum[q];
  T *out = reinterpret_cast<T *>(lds16);
  const unsigned d = threadIdx.x * kPer;
#pragma unroll
  for (unsigned j = 0; j < kPer; ++j)
    if (d + j < g.valid) out[d + j + threadIdx.x] = (T)base + v[j];   // element e at e + e / 8
  __syncthreads();
  // delta e of the tile is delta d0 + e of the page and gives the page's value d0 + e + 1
  T *__restrict__ dst = reinterpret_cast<T *>(pg.dst) + g.d0 + 1;
  for (unsigned e = threadIdx.x; e < g.valid; e += kBlock) dst[e] = out[e + (e >> 3)];
}

__global__ __launch_bounds__(kBlock) void delta_scan_kernel(const nvt_pq_delta_page *__restrict__ pages,
                                                            const uint32_t *__restrict__ tile_page,
                                                            const uint64_t *__restrict__ tile_sums) {
  __shared__ uint4 lds16[kLdsBytes / 16];
  __shared__ uint64_t wsum[kBlock / kWave];
  const nvt_pq_delta_page pg = pages[tile_page[blockIdx.x]];
  if (pg.width == 4)
    scan_body<uint32_t>(lds16, wsum, pg, tile_sums);
  else
    scan_body<uint64_t>(lds16, wsum, pg, tile_sums);
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_delta_decode(const nvt_pq_delta_page *pages, uint64_t npages, const uint32_t *tile_page, uint64_t ntiles,
                        uint64_t *tile_sums, void *stream) {
  if (npages == 0) return NVT_OK;
  NVT_CHECK_ARG(pages, "null page table");
  NVT_CHECK_ARG(ntiles == 0 || (tile_page && tile_sums), "null tile table / workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(pages) & 7) == 0 && (reinterpret_cast<uintptr_t>(tile_sums) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(tile_page) & 3) == 0,
                "tables must be aligned to their words");
  NVT_CHECK_ARG(npages < (1ull << 32) && ntiles < (1ull << 31), "fewer than 2^32 pages and 2^31 tiles");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_delta_decode", ntiles * (uint64_t)kTile * 8, s);
  if (ntiles) {
    delta_sum_kernel<<<(unsigned)ntiles, kBlock, 0, s>>>(pages, tile_page, tile_sums);
    NVT_CHECK_LAUNCH();
  }
  const unsigned per = kBlock / kWave;
  delta_carry_kernel<<<(unsigned)((npages + per - 1) / per), kBlock, 0, s>>>(pages, npages, tile_sums);
  NVT_CHECK_LAUNCH();
  if (ntiles) {
    delta_scan_kernel<<<(unsigned)ntiles, kBlock, 0, s>>>(pages, tile_page, tile_sums);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
