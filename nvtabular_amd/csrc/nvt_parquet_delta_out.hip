// DELTA_BINARY_PACKED pages of the PLAIN parquet writer: the non-null values of one flat INT32 /
// INT64 column chunk as self-contained delta pages, block size 128, 4 miniblocks of 32.
// include/nvt_hip.h, "parquet out: DELTA_BINARY_PACKED pages", states the contract; DESIGN.md,
// "DELTA_BINARY_PACKED in the PLAIN parquet writer", the reasons.
//
// A page of nv values holds nv - 1 deltas (taken modulo 2^bits); delta j of the page is
// v[j + 1] - v[j], so the first delta of a block reads one value across the block boundary and no
// delta crosses a page boundary (a page's first value is in its header).
//
// Work split: ONE WAVE owns ONE BLOCK of 128 deltas.  Lane l holds deltas l and l + 64: miniblocks
// 0 / 1 are the two 32-lane halves of the first register, miniblocks 2 / 3 of the second.
// min_delta is a wave min-reduction over both registers (cross-lane shuffles, no LDS); a
// miniblock's width is the bit length of the OR of its 32 relative deltas, an OR-reduction over a
// half-wave (the OR has the bit length of the maximum).  Lanes behind the page's last delta hold
// the relative delta 0: they pad the last used miniblock with zero bits and touch neither min nor OR.
//
// nvt_pq_delta_out_size, on the caller's stream:
//   1. pdo_size_kernel    grid (x, page): the waves of a page's x-blocks stride over its blocks and
//                         write every block's byte count -- varint length of zigzag(min_delta), 4
//                         width bytes, 4 * width bytes per used miniblock -- to `cnt`; page p's
//                         counts start at cnt[page_start[p] / 128 + p] (the ranges of two pages
//                         never overlap: ceil((nv - 1) / 128) <= nv / 128 + 1).
//   2. pdo_scan_kernel    one workgroup per page: exclusive scan of the page's counts in LDS, tiles
//                         of 8192 with a carry that starts at the page header's length; cnt becomes
//                         the byte offset of every block inside its page's region, len[p] the
//                         region's length.
//   3. pdo_pages_kernel   one wave: at[p] = 16-byte aligned start of every region in `out`,
//                         state = {sum of len, pays, error, bytes of out in use}; error: a page
//                         table that is negative, descending or past n.  THE CHUNK RULE
//                         RUNS HERE: pays = n > 0, no error, sum(len) < n * itemsize.
// nvt_pq_delta_out_pack:
//   4. pdo_pack_kernel    returns at once unless `pays`.  A wave recomputes its block and assembles
//                         the block image in LDS: the relative deltas go to LDS, the header bytes
//                         are placed so that they END at byte 16 of the image buffer, and the
//                         miniblock dwords follow from byte 16 on, aligned in LDS -- lane t builds
//                         dword t of the block from the values that overlap its 32 bits.  The first
//                         wave of a page's first x-block also writes the page header.
//
// Stores to `out`: a block image starts at ANY byte of `out`, so the dword that holds its first or
// last bytes may also hold bytes of the neighbouring block (or of the page header), written by
// another wave or workgroup.  NOBODY OWNS A SHARED DWORD AND NOBODY READ-MODIFY-WRITES ONE: a wave
// stores the bytes in front of the image's first 4-byte boundary and behind its last one as single
// bytes, and only the aligned dwords that lie ENTIRELY inside its image as dwords (coalesced; the
// source is read from LDS at the image's byte phase with a funnel shift).  Page headers (at most
// 23 bytes) go out as single bytes.  All stores are ordinary vector stores.  The bytes between a
// region's end and the next 16-byte boundary are never written.
#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr int kPdoBlock = NVT_PQ_DELTA_OUT_BLOCK;   // deltas per block
constexpr int kPdoMini = 32;                        // deltas per miniblock
constexpr int kPdoWaves = kBlock / kWave;           // blocks a workgroup assembles at a time
constexpr int kPdoImgWords = 264;                   // 16 header bytes | 1024 body bytes | funnel slack
constexpr int kPdoScanTile = 8192;                  // counts a scan tile holds in LDS (32 per thread)
constexpr uint64_t kPdoMaxValues = 1ull << 28;      // (every byte offset of a chunk fits 32 bits)

template <typename T>
struct PdoU;
template <>
struct PdoU<int32_t> { typedef uint32_t type; };
template <>
struct PdoU<int64_t> { typedef uint64_t type; };

__device__ __forceinline__ unsigned pdo_bitlen(uint64_t x) { return x ? 64u - (unsigned)__clzll((long long)x) : 0u; }
__device__ __forceinline__ unsigned pdo_varint_len(uint64_t z) {
  const unsigned b = pdo_bitlen(z);
  return b ? (b + 6u) / 7u : 1u;
}
__device__ __forceinline__ uint64_t pdo_zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
// byte i of the varint of z (i < pdo_varint_len(z))
__device__ __forceinline__ uint8_t pdo_varint_byte(uint64_t z, unsigned i, unsigned len) {
  return (uint8_t)(((z >> (7u * i)) & 0x7Full) | (i + 1u < len ? 0x80u : 0u));
}

// page p of the table, clamped so that nothing is ever read outside [0, n)
__device__ __forceinline__ void pdo_page(const int64_t *__restrict__ page_start, uint64_t p, uint64_t n, uint64_t &lo,
                                         uint64_t &nv) {
  int64_t a = page_start[p], b = page_start[p + 1];
  a = a < 0 ? 0 : (a > (int64_t)n ? (int64_t)n : a);
  b = b < a ? a : (b > (int64_t)n ? (int64_t)n : b);
  lo = (uint64_t)a;
  nv = (uint64_t)(b - a);
}
__device__ __forceinline__ uint64_t pdo_cnt_base(uint64_t lo, uint64_t p) { return lo / kPdoBlock + p; }

// Block b of the page whose values start at v: this lane's two relative deltas, the block's
// min_delta (sign-extended) and the widths of its 4 miniblocks (0 for the ones that hold no delta).
template <typename T>
__device__ __forceinline__ void pdo_block(const T *__restrict__ v, uint64_t nd, uint64_t b, unsigned lane,
                                          typename PdoU<T>::type &r0, typename PdoU<T>::type &r1, int64_t &min_delta,
                                          unsigned w[4]) {
  typedef typename PdoU<T>::type U;
  const uint64_t j0 = b * kPdoBlock + lane, j1 = j0 + 64;
  const bool ok0 = j0 < nd, ok1 = j1 < nd;   // (delta j reads v[j] and v[j + 1], j + 1 <= nd = nv - 1)
  const T d0 = ok0 ? (T)((U)v[j0 + 1] - (U)v[j0]) : (T)0;
  const T d1 = ok1 ? (T)((U)v[j1 + 1] - (U)v[j1]) : (T)0;
  T m = ok1 ? (d1 < d0 ? d1 : d0) : d0;
  const T m_lane0 = __shfl(m, 0, 64);   // (the block's delta 0 is always valid: a lane without deltas votes with it)
  if (!ok0) m = m_lane0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(m, off, 64);
    m = o < m ? o : m;
  }
  r0 = ok0 ? (U)((U)d0 - (U)m) : (U)0;
  r1 = ok1 ? (U)((U)d1 - (U)m) : (U)0;
  U o0 = r0, o1 = r1;
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {   // (xor offsets below 32 stay inside a half-wave)
    o0 |= __shfl_xor(o0, off, 64);
    o1 |= __shfl_xor(o1, off, 64);
  }
  w[0] = pdo_bitlen((uint64_t)__shfl(o0, 0, 64));
  w[1] = pdo_bitlen((uint64_t)__shfl(o0, 32, 64));
  w[2] = pdo_bitlen((uint64_t)__shfl(o1, 0, 64));
  w[3] = pdo_bitlen((uint64_t)__shfl(o1, 32, 64));
  min_delta = (int64_t)m;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pdo_size_kernel(const T *__restrict__ values, uint64_t n,
                                                          const int64_t *__restrict__ page_start, uint64_t npages,
                                                          uint32_t *__restrict__ cnt) {
  typedef typename PdoU<T>::type U;
  const unsigned lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * kPdoWaves + threadIdx.x / kWave;
  const uint64_t nwaves = (uint64_t)gridDim.x * kPdoWaves;
  for (uint64_t p = blockIdx.y; p < npages; p += gridDim.y) {
    uint64_t lo, nv;
    pdo_page(page_start, p, n, lo, nv);
    const uint64_t nd = nv ? nv - 1 : 0, nb = (nd + kPdoBlock - 1) / kPdoBlock;
    const uint64_t base = pdo_cnt_base(lo, p);
    for (uint64_t b = wave; b < nb; b += nwaves) {   // (uniform per wave)
      U r0, r1;
      int64_t md;
      unsigned w[4];
      pdo_block<T>(values + lo, nd, b, lane, r0, r1, md, w);
      if (lane == 0) cnt[base + b] = pdo_varint_len(pdo_zigzag(md)) + 4u + 4u * (w[0] + w[1] + w[2] + w[3]);
    }
  }
}

// header of a page: varint 128 (2 bytes) | varint 4 | varint nv | zigzag first value
template <typename T>
__device__ __forceinline__ unsigned pdo_header_len(const T *__restrict__ values, uint64_t lo, uint64_t nv,
                                                   uint64_t &zfirst) {
  zfirst = nv ? pdo_zigzag((int64_t)values[lo]) : 0ull;
  return 3u + pdo_varint_len(nv) + pdo_varint_len(zfirst);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pdo_scan_kernel(const T *__restrict__ values, uint64_t n,
                                                          const int64_t *__restrict__ page_start, uint64_t npages,
                                                          uint32_t *__restrict__ cnt, int64_t *__restrict__ len) {
  // entry i of a tile lives at i + i / 32: a thread walks its 32 consecutive entries without every
  // thread of the wave hitting the same bank
  __shared__ uint32_t tile[kPdoScanTile + kPdoScanTile / 32];
  __shared__ uint32_t wave_tot[kPdoWaves];
  const unsigned tid = threadIdx.x, lane = lane_id(), wv = tid / kWave;
  constexpr unsigned per = kPdoScanTile / kBlock;
  for (uint64_t p = blockIdx.x; p < npages; p += gridDim.x) {
    uint64_t lo, nv, zfirst;
    pdo_page(page_start, p, n, lo, nv);
    const uint64_t nd = nv ? nv - 1 : 0, nb = (nd + kPdoBlock - 1) / kPdoBlock;
    uint32_t *c = cnt + pdo_cnt_base(lo, p);
    uint32_t carry = pdo_header_len<T>(values, lo, nv, zfirst);
    for (uint64_t t0 = 0; t0 < nb; t0 += kPdoScanTile) {   // (uniform)
      const unsigned m = (unsigned)(nb - t0 < (uint64_t)kPdoScanTile ? nb - t0 : (uint64_t)kPdoScanTile);
      for (unsigned i = tid; i < (unsigned)kPdoScanTile; i += kBlock) tile[i + i / 32] = i < m ? c[t0 + i] : 0u;
      __syncthreads();
      uint32_t sum = 0;
      for (unsigned k = 0; k < per; ++k) {   // (per == 32: thread t's entries are one padded row)
        const unsigned i = tid * per + k;
        const uint32_t x = tile[i + i / 32];
        tile[i + i / 32] = sum;
        sum += x;
      }
      uint32_t inc = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= (unsigned)off) inc += o;
      }
      if (lane == 63) wave_tot[wv] = inc;
      __syncthreads();
      uint32_t before = carry + inc - sum, total = 0;
      for (unsigned k = 0; k < (unsigned)kPdoWaves; ++k) {
        if (k < wv) before += wave_tot[k];
        total += wave_tot[k];
      }
      for (unsigned k = 0; k < per; ++k) {
        const unsigned i = tid * per + k;
        tile[i + i / 32] += before;
      }
      __syncthreads();
      for (unsigned i = tid; i < m; i += kBlock) c[t0 + i] = tile[i + i / 32];
      carry += total;
      __syncthreads();
    }
    if (tid == 0) len[p] = (int64_t)carry;
  }
}

// one wave: at[], the state record, the table's and out_cap's checks, and the chunk rule
__global__ __launch_bounds__(kWave) void pdo_pages_kernel(const int64_t *__restrict__ page_start, uint64_t npages,
                                                          uint64_t n, uint64_t itemsize,
                                                          int64_t *__restrict__ state, int64_t *__restrict__ at,
                                                          const int64_t *__restrict__ len) {
  const unsigned lane = lane_id();
  uint64_t carry = 0, total = 0;
  bool bad = false;
  for (uint64_t p0 = 0; p0 < npages; p0 += 64) {
    const uint64_t p = p0 + lane;
    const bool in = p < npages;
    const uint64_t l = in ? (uint64_t)len[p] : 0ull;
    if (in) {
      const int64_t a = page_start[p], b = page_start[p + 1];
      bad |= a < 0 || b < a || b > (int64_t)n;
    }
    const uint64_t padded = (l + 15) & ~15ull;
    uint64_t inc = padded, sum = l;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint64_t o = __shfl_up(inc, off, 64);
      if (lane >= (unsigned)off) inc += o;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (in) at[p] = (int64_t)(carry + inc - padded);
    carry += __shfl(inc, 63, 64);
    total += sum;
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
    // (pays => used <= total + 15 * npages < n * itemsize + 16 * npages, the out_cap the pack insists on)
    const uint64_t used = carry;
    const bool err = any_bad;
    state[0] = (int64_t)total;
    state[1] = (n > 0 && !err && total < n * itemsize) ? 1 : 0;
    state[2] = err ? 1 : 0;
    state[3] = (int64_t)used;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pdo_pack_kernel(const T *__restrict__ values, uint64_t n,
                                                          const int64_t *__restrict__ page_start, uint64_t npages,
                                                          const uint32_t *__restrict__ cnt,
                                                          const int64_t *__restrict__ state,
                                                          const int64_t *__restrict__ at, uint8_t *__restrict__ out) {
  typedef typename PdoU<T>::type U;
  if (state[1] == 0) return;   // the chunk stays PLAIN: no pack work (uniform over the grid)
  __shared__ U rel[kPdoWaves][kPdoBlock];
  __shared__ uint32_t img[kPdoWaves][kPdoImgWords];
  const unsigned lane = lane_id(), wv = threadIdx.x / kWave;
  U *my_rel = rel[wv];
  uint32_t *my_img = img[wv];
  uint8_t *my_img8 = reinterpret_cast<uint8_t *>(my_img);
  for (uint64_t p = blockIdx.y; p < npages; p += gridDim.y) {
    uint64_t lo, nv;
    pdo_page(page_start, p, n, lo, nv);
    const uint64_t nd = nv ? nv - 1 : 0, nb = (nd + kPdoBlock - 1) / kPdoBlock;
    const uint32_t *c = cnt + pdo_cnt_base(lo, p);
    uint8_t *region = out + at[p];
    if (blockIdx.x == 0 && wv == 0) {   // the page header, byte by byte
      uint64_t zfirst;
      const unsigned hl = pdo_header_len<T>(values, lo, nv, zfirst);
      const unsigned ln = pdo_varint_len(nv), lz = hl - 3u - ln;
      if (lane < hl) {
        uint8_t byte;
        if (lane < 3)
          byte = lane == 0 ? 0x80 : lane == 1 ? 0x01 : 0x04;
        else if (lane < 3 + ln)
          byte = pdo_varint_byte(nv, lane - 3, ln);
        else
          byte = pdo_varint_byte(zfirst, lane - 3 - ln, lz);
        region[lane] = byte;
      }
    }
    // every wave of the workgroup makes the same number of trips: the barriers below are uniform
    for (uint64_t g = blockIdx.x; g * kPdoWaves < nb; g += gridDim.x) {
      const uint64_t b = g * kPdoWaves + wv;
      const bool live = b < nb;   // (uniform per wave)
      unsigned w[4] = {0, 0, 0, 0};
      unsigned hl = 0;
      if (live) {
        U r0, r1;
        int64_t md;
        pdo_block<T>(values + lo, nd, b, lane, r0, r1, md, w);
        my_rel[lane] = r0;
        my_rel[lane + 64] = r1;
        const uint64_t z = pdo_zigzag(md);
        const unsigned lz = pdo_varint_len(z);
        hl = lz + 4u;
        if (lane < lz) my_img8[16 - hl + lane] = pdo_varint_byte(z, lane, lz);
        if (lane < 4) my_img8[12 + lane] = (uint8_t)((w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24)) >> (8u * lane));
      }
      __syncthreads();
      const unsigned D = w[0] + w[1] + w[2] + w[3];   // the body's dwords: a miniblock at width w is w dwords
      const uint32_t wp = w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24);
      if (live) {
        for (unsigned t = lane; t < D; t += kWave) {
          unsigned mb = 0, j = t, wd = wp & 0xFFu;
          while (j >= wd) {   // (t < D: ends with mb <= 3)
            j -= wd;
            ++mb;
            wd = (wp >> (8u * mb)) & 0xFFu;
          }
          const unsigned bit0 = 32u * j;
          uint32_t dw = 0;
          for (unsigned k = bit0 / wd; k < (unsigned)kPdoMini && k * wd < bit0 + 32u; ++k) {
            const uint64_t x = (uint64_t)my_rel[mb * kPdoMini + k];
            const int sh = (int)(k * wd) - (int)bit0;
            dw |= sh >= 0 ? (uint32_t)(x << sh) : (uint32_t)(x >> (-sh));
          }
          my_img[4 + t] = dw;
        }
      }
      __syncthreads();
      if (live) {
        const unsigned L = hl + 4u * D, s0 = 16u - hl;   // the image: bytes [s0, s0 + L) of my_img8
        uint8_t *dst = region + c[b];
        unsigned head = (unsigned)((4u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
        head = head < L ? head : L;
        const unsigned nbody = (L - head) / 4u, tail0 = head + 4u * nbody;
        if (lane < head) dst[lane] = my_img8[s0 + lane];
        uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst + head);
        for (unsigned i = lane; i < nbody; i += kWave) {
          const unsigned s = s0 + head + 4u * i, sh = 8u * (s & 3u);
          const uint32_t a = my_img[s >> 2], hi = my_img[(s >> 2) + 1];
          dst32[i] = sh ? (a >> sh) | (hi << (32u - sh)) : a;
        }
        if (lane < L - tail0) dst[tail0 + lane] = my_img8[s0 + tail0 + lane];
      }
      __syncthreads();   // (the next trip overwrites rel and img)
    }
  }
}

inline int pdo_itemsize(int dtype) { return dtype == NVT_I32 ? 4 : dtype == NVT_I64 ? 8 : 0; }
inline uint64_t pdo_cnt_slots(uint64_t n, uint64_t npages) { return n / kPdoBlock + npages + 1; }
// grid of the per-block kernels: x covers the blocks a page can have (4 per workgroup), y the pages
inline dim3 pdo_grid(uint64_t n, uint64_t npages) {
  const uint64_t per_page = (n / kPdoBlock + 1 + kPdoWaves - 1) / kPdoWaves;
  const uint64_t gy = npages < 1024 ? npages : 1024;
  uint64_t gx = per_page < 2048 ? per_page : 2048;
  if (gx * gy > (uint64_t)kCUs * 64) gx = ((uint64_t)kCUs * 64 + gy - 1) / gy;   // (many small pages: fewer x-blocks each)
  return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_delta_out_ws_bytes(uint64_t n, uint64_t npages, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null bytes");
  NVT_CHECK_ARG(n < kPdoMaxValues && npages < (1ull << 31), "fewer than 2^28 values and 2^31 pages");
  *bytes = pad16(pdo_cnt_slots(n, npages) * 4);
  return NVT_OK;
}

int nvt_pq_delta_out_size(const void *values, int dtype, uint64_t n, const int64_t *page_start, uint64_t npages,
                          int64_t *table, void *ws, uint64_t ws_bytes, void *stream) {
  NVT_CHECK_ARG(pdo_itemsize(dtype), "dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(n < kPdoMaxValues && npages < (1ull << 31), "fewer than 2^28 values and 2^31 pages");
  NVT_CHECK_ARG(npages >= 1, "at least one page");
  NVT_CHECK_ARG((values || n == 0) && page_start && table && ws, "null pointer");
  NVT_CHECK_ARG(ws_bytes >= pad16(pdo_cnt_slots(n, npages) * 4), "workspace too small");
  NVT_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)table % 8 == 0 && (uintptr_t)page_start % 8 == 0 &&
                    (uintptr_t)values % (uintptr_t)pdo_itemsize(dtype) == 0,
                "ws 16-byte, tables 8-byte aligned, values to their size");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_delta_out_size", n * (uint64_t)pdo_itemsize(dtype), s);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(ws);
  int64_t *at = table + NVT_PQ_DELTA_OUT_STATE_WORDS, *len = at + npages;
  const dim3 grid = pdo_grid(n, npages);
  const unsigned scan_grid = (unsigned)(npages < 65535 ? npages : 65535);
  if (dtype == NVT_I32) {
    pdo_size_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)values, n, page_start, npages, cnt);
    NVT_CHECK_LAUNCH();
    pdo_scan_kernel<int32_t><<<scan_grid, kBlock, 0, s>>>((const int32_t *)values, n, page_start, npages, cnt, len);
  } else {
    pdo_size_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)values, n, page_start, npages, cnt);
    NVT_CHECK_LAUNCH();
    pdo_scan_kernel<int64_t><<<scan_grid, kBlock, 0, s>>>((const int64_t *)values, n, page_start, npages, cnt, len);
  }
  NVT_CHECK_LAUNCH();
  pdo_pages_kernel<<<1, kWave, 0, s>>>(page_start, npages, n, (uint64_t)pdo_itemsize(dtype), table, at, len);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_pq_delta_out_pack(const void *values, int dtype, uint64_t n, const int64_t *page_start, uint64_t npages,
                          const int64_t *table, uint8_t *out, uint64_t out_cap, const void *ws, uint64_t ws_bytes,
                          void *stream) {
  NVT_CHECK_ARG(pdo_itemsize(dtype), "dtype must be NVT_I32 or NVT_I64");
  NVT_CHECK_ARG(n < kPdoMaxValues && npages < (1ull << 31), "fewer than 2^28 values and 2^31 pages");
  NVT_CHECK_ARG(npages >= 1, "at least one page");
  if (n == 0) return NVT_OK;   // (a chunk without values never pays)
  NVT_CHECK_ARG(values && page_start && table && ws && out, "null pointer");
  NVT_CHECK_ARG(ws_bytes >= pad16(pdo_cnt_slots(n, npages) * 4), "workspace too small");
  NVT_CHECK_ARG(out_cap >= n * (uint64_t)pdo_itemsize(dtype) + 16 * npages, "out_cap below n * itemsize + 16 * npages");
  NVT_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)table % 8 == 0,
                "ws / out 16-byte, table 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_delta_out_pack", n * (uint64_t)pdo_itemsize(dtype), s);
  const uint32_t *cnt = reinterpret_cast<const uint32_t *>(ws);
  const int64_t *at = table + NVT_PQ_DELTA_OUT_STATE_WORDS;
  const dim3 grid = pdo_grid(n, npages);
  if (dtype == NVT_I32)
    pdo_pack_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)values, n, page_start, npages, cnt, table, at, out);
  else
    pdo_pack_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)values, n, page_start, npages, cnt, table, at, out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
