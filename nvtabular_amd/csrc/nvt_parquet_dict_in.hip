// Parquet in, dictionary-encoded data pages of flat 4- / 8-byte number columns: the device half
// ("Dictionary pages of number columns in the parquet reader").  The host
// (nvt_pq_decode_chunk_dict, nvt_parquet.hip) has walked the pages and the run headers of their index
// streams and staged, per column of a partition, the chunks' dictionaries, a run table and the bytes
// of the bit-packed runs as the file holds them (include/nvt_hip.h, nvt_pq_dict_stage).  Here every
// packed (non-null) value that a dictionary page owes is written into its place:
//
//   value q = dict[a + index of q]   (REPEAT: the entry a itself; KEEP: the host's value stays)
//
//   grid     one workgroup per entry of the host's group table {column, first tile}: it takes
//            kTilesPerWg consecutive tiles of kTile = 4096 values of ONE column, so that a partition of
//            39 columns is one launch and the per-workgroup setup below is paid once per 16 Ki values.
//   dict     a column whose staged dictionaries (all chunks of the partition, heads included) fit
//            kDictLdsBytes is copied to LDS once per workgroup with 16-byte loads and gathered there;
//            a larger one is gathered from global memory (pyarrow keeps a dictionary under 1 MiB: L2).
//            The LDS of a workgroup is 60 KiB with it, so two workgroups share a CU's 160 KiB.
//   runs     thread 0 finds the tile's first run by binary search over the table in global memory.
//            From there the tile's runs pass through LDS in WINDOWS of kWin records (starts apart, so
//            the search reads consecutive words): a tile of 4096 values may hold 4096 runs (8 windows)
//            or lie inside one run (1 window of 1 record).  A lane owns kPer = 16 values in groups of
//            16 bytes (group g of step s: values (s * 256 + lane) * G ..., G = 4 or 2); per group it
//            searches the window's starts once and walks on from there, so short runs cost a compare
//            each and long ones nothing.  Entry ids stay in registers across the windows.
//   unpack   per window two LDS atomics give the first and last word of `packed` that its PACKED runs
//            need inside the tile; that span (up to 4096 + 64 words: 4096 values at 32 bits and the
//            runs' alignment) goes to LDS with 16-byte loads.  Index k of a run is two LDS words and a
//            funnel shift (v_alignbit_b32).  A word outside the staged span -- only a table that lies
//            about its runs gets there -- is an aligned 32-bit global load, bounded by packed_bytes.
//   check    a packed index is compared with the entries in its chunk's head (one broadcast LDS / L2
//            read per value) and a + index with ndict; a miss writes 0 and is counted per lane, a wave
//            adds its count with one atomic at the end.
//   stores   a group whose G values are all filled is one 16-byte store, consecutive over the lanes;
//            a group that holds a KEEP position or the column's end stores its filled values one by
//            one.  Nothing else is written.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr unsigned kTile = NVT_PQ_DICT_TILE;
constexpr unsigned kTilesPerWg = NVT_PQ_DICT_TILES_PER_WG;
constexpr unsigned kDictLdsBytes = NVT_PQ_DICT_LDS_BYTES;
constexpr unsigned kPer = kTile / kBlock;      // values per lane and tile
constexpr unsigned kWin = 512;                 // run records per LDS window
constexpr unsigned kSpanWords = kTile + 64;    // words of `packed` per window held in LDS
constexpr uint32_t kKeep = 0xFFFFFFFFu;        // "leave this position alone"
constexpr uint32_t kBad = 0xFFFFFFFEu;         // "write 0 and count" (entry positions stay below 2^31)
static_assert(kPer == 16 && kSpanWords % 4 == 0 && kDictLdsBytes % 16 == 0, "16 values per lane, 16-byte LDS rows");
static_assert(kDictLdsBytes + kSpanWords * 4 + kWin * 16 + (kWin + 1) * 4 + 64 <= 64 * 1024,
              "a workgroup's LDS stays under 64 KiB: two of them per CU");

// kernels_parquet_dict_in.fill_holes writes these descriptors as 9 words of 8 bytes
static_assert(sizeof(nvt_pq_dict_col) == 72 && offsetof(nvt_pq_dict_col, nruns) == 8 &&
                  offsetof(nvt_pq_dict_col, packed) == 16 && offsetof(nvt_pq_dict_col, packed_bytes) == 24 &&
                  offsetof(nvt_pq_dict_col, dict) == 32 && offsetof(nvt_pq_dict_col, ndict) == 40 &&
                  offsetof(nvt_pq_dict_col, type_size) == 48 && offsetof(nvt_pq_dict_col, values) == 56 &&
                  offsetof(nvt_pq_dict_col, nvalues) == 64,
              "nvt_pq_dict_col: {runs, nruns, packed, packed_bytes, dict, ndict, type_size, values, nvalues}");

struct Lds {
  uint4 dict[kDictLdsBytes / 16];
  uint4 span[kSpanWords / 4];
  uint4 rec[kWin];
  uint32_t start[kWin + 1];
  uint32_t first_run;
  uint32_t span_lo, span_hi;   // first word / the word behind the last that the window's packed runs need
};

// the largest r in [lo, hi] with get(r) <= q when the starts ascend; some r of [lo, hi] whatever they hold
template <typename G>
__device__ __forceinline__ uint64_t run_of(G get, uint64_t lo, uint64_t hi, uint32_t q) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (get(mid) <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <typename T>
__device__ __forceinline__ void fill_tiles(const nvt_pq_dict_col &c, uint32_t first_tile, Lds &l, unsigned &nbad) {
  constexpr unsigned G = 16 / sizeof(T);   // values per 16-byte group
  constexpr unsigned S = kPer / G;         // groups per lane and tile
  const unsigned tid = threadIdx.x;
  const uint32_t *__restrict__ runs = c.runs;
  const uint4 *__restrict__ runs16 = reinterpret_cast<const uint4 *>(c.runs);
  const uint32_t *__restrict__ packed = reinterpret_cast<const uint32_t *>(c.packed);
  const uint4 *__restrict__ packed16 = reinterpret_cast<const uint4 *>(c.packed);
  const T *__restrict__ dict = reinterpret_cast<const T *>(c.dict);
  const uint32_t *__restrict__ dict32 = reinterpret_cast<const uint32_t *>(c.dict);
  T *__restrict__ values = reinterpret_cast<T *>(c.values);
  const uint64_t nruns = c.nruns, nvalues = c.nvalues, ndict = c.ndict;
  const uint64_t packed_words = c.packed_bytes / 4, packed_quads = c.packed_bytes / 16;
  const uint64_t ntiles = (nvalues + kTile - 1) / kTile;
  if (nruns == 0 || first_tile >= ntiles) return;   // (uniform)

  // the column's dictionaries -> LDS, once for all tiles of this workgroup
  const bool in_lds = ndict * sizeof(T) <= kDictLdsBytes;   // (uniform)
  const T *sdict = reinterpret_cast<const T *>(l.dict);
  const uint32_t *sdict32 = reinterpret_cast<const uint32_t *>(l.dict);
  if (in_lds) {
    const unsigned words = (unsigned)(ndict * sizeof(T) / 4), quads = words / 4;
    const uint4 *dict16 = reinterpret_cast<const uint4 *>(c.dict);
    for (unsigned i = tid; i < quads; i += kBlock) l.dict[i] = dict16[i];
    uint32_t *tail = reinterpret_cast<uint32_t *>(l.dict);
    for (unsigned i = quads * 4 + tid; i < words; i += kBlock) tail[i] = dict32[i];
  }
  const uint32_t *sspan = reinterpret_cast<const uint32_t *>(l.span);

  const uint64_t tile_end = (uint64_t)first_tile + kTilesPerWg < ntiles ? (uint64_t)first_tile + kTilesPerWg : ntiles;
  for (uint64_t tile = first_tile; tile < tile_end; ++tile) {
    const uint32_t p0 = (uint32_t)(tile * kTile);
    const uint32_t p1 = (uint64_t)p0 + kTile < nvalues ? p0 + kTile : (uint32_t)nvalues;
    uint32_t id[kPer];
#pragma unroll
    for (unsigned e = 0; e < kPer; ++e) id[e] = kKeep;
    if (tid == 0) l.first_run = (uint32_t)run_of([&](uint64_t r) { return runs[4 * r]; }, 0, nruns - 1, p0);
    __syncthreads();   // (also: the dictionary is staged; the last tile's windows are done with)
    uint64_t rw = l.first_run;
    for (;;) {   // windows of the tile's runs
      const unsigned nwin = nruns - rw < kWin ? (unsigned)(nruns - rw) : kWin;
      for (unsigned k = tid; k <= nwin; k += kBlock) l.start[k] = runs[4 * (rw + k)];   // (rw + nwin <= nruns: the closing record)
      for (unsigned k = tid; k < nwin; k += kBlock) l.rec[k] = runs16[rw + k];
      if (tid == 0) {
        l.span_lo = 0xFFFFFFFFu;
        l.span_hi = 0;
      }
      __syncthreads();
      const uint32_t wend = l.start[nwin];
      const uint32_t wlo = l.start[0] > p0 ? l.start[0] : p0, whi = wend < p1 ? wend : p1;
      // the words of `packed` this window's runs need for positions [wlo, whi)
      for (unsigned k = tid; k < nwin; k += kBlock) {
        const uint4 rec = l.rec[k];
        const unsigned width = (rec.y >> 8) & 0xFFu;
        if ((rec.y & 0xFFu) != NVT_PQ_RUN_PACKED || width < 1 || width > 32) continue;
        const uint32_t s0 = rec.x > wlo ? rec.x : wlo, s1 = l.start[k + 1] < whi ? l.start[k + 1] : whi;
        if (s0 >= s1) continue;
        const uint64_t wa = (uint64_t)rec.w + (((uint64_t)(s0 - rec.x) * width) >> 5);
        const uint64_t wb = (uint64_t)rec.w + (((uint64_t)(s1 - rec.x) * width + 31) >> 5) + 1;   // (+ the funnel's high word)
        atomicMin(&l.span_lo, wa < 0xFFFFFFFFull ? (uint32_t)wa : 0xFFFFFFFFu);
        atomicMax(&l.span_hi, wb < 0xFFFFFFFFull ? (uint32_t)wb : 0xFFFFFFFFu);
      }
      __syncthreads();
      uint64_t span0 = 0, span1 = 0;   // words [span0, span1) of `packed` are in LDS
      if (l.span_lo != 0xFFFFFFFFu) {
        const uint64_t q0 = l.span_lo / 4;
        uint64_t q1 = ((uint64_t)l.span_hi + 3) / 4;
        if (q1 > packed_quads) q1 = packed_quads;
        if (q1 > q0 + kSpanWords / 4) q1 = q0 + kSpanWords / 4;
        if (q1 > q0) {
          for (uint64_t i = tid; i < q1 - q0; i += kBlock) l.span[i] = packed16[q0 + i];
          span0 = q0 * 4;
          span1 = q1 * 4;
        }
      }
      __syncthreads();
      auto word = [&](uint64_t w) -> uint32_t {   // w < packed_words
        return (w >= span0 && w < span1) ? sspan[w - span0] : packed[w];
      };
#pragma unroll
      for (unsigned s = 0; s < S; ++s) {
        const uint32_t qg = p0 + (s * kBlock + tid) * G;
        if (qg + G <= wlo || qg >= whi) continue;
        unsigned r = (unsigned)run_of([&](uint64_t k) { return l.start[k]; }, 0, nwin - 1, qg > wlo ? qg : wlo);
#pragma unroll
        for (unsigned j = 0; j < G; ++j) {
          const uint32_t q = qg + j;
          if (q < wlo || q >= whi) continue;
          while (r + 1 < nwin && q >= l.start[r + 1]) ++r;
          const uint4 rec = l.rec[r];   // {start, kind | width << 8, a, b}
          const unsigned kind = rec.y & 0xFFu, width = (rec.y >> 8) & 0xFFu;
          uint32_t e = kBad;
          if (kind == NVT_PQ_RUN_KEEP) {
            e = kKeep;
          } else if (q < rec.x) {
            // (a table whose starts do not ascend: counted)
          } else if (kind == NVT_PQ_RUN_REPEAT) {
            if (rec.z < ndict) e = rec.z;
          } else if (kind == NVT_PQ_RUN_PACKED && width >= 1 && width <= 32) {
            const uint64_t bit = (uint64_t)(q - rec.x) * width;
            const uint64_t w = (uint64_t)rec.w + (bit >> 5);
            const uint64_t head = (uint64_t)rec.z * sizeof(T);   // the chunk's head lies in front of entry a
            if (w < packed_words && head >= NVT_PQ_DICT_HEAD_BYTES && rec.z <= ndict) {
              const uint32_t lo = word(w), hi = w + 1 < packed_words ? word(w + 1) : 0u;
              uint32_t v = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(bit & 31));
              if (width < 32) v &= (1u << width) - 1u;
              const uint64_t hw = (head - NVT_PQ_DICT_HEAD_BYTES) / 4;
              const uint32_t lim = in_lds ? sdict32[hw] : dict32[hw];
              if (v < lim && (uint64_t)rec.z + v < ndict) e = rec.z + v;
            }
          }
          id[s * G + j] = e;
        }
      }
      __syncthreads();   // (every lane is done with this window's LDS)
      if (rw + nwin >= nruns || wend >= p1) break;   // (uniform)
      rw += nwin;
    }
    // gather and store
#pragma unroll
    for (unsigned s = 0; s < S; ++s) {
      const uint32_t qg = p0 + (s * kBlock + tid) * G;
      T v[G];
      bool whole = true;
#pragma unroll
      for (unsigned j = 0; j < G; ++j) {
        const uint32_t e = id[s * G + j];
        v[j] = 0;
        if (e == kKeep) whole = false;
        else if (e == kBad) ++nbad;
        else v[j] = in_lds ? sdict[e] : dict[e];
      }
      if (whole) {
        uint4 o;
        if (sizeof(T) == 4) {
          o = make_uint4((uint32_t)v[0], (uint32_t)v[1 % G], (uint32_t)v[2 % G], (uint32_t)v[3 % G]);
        } else {
          const uint64_t a = (uint64_t)v[0], b = (uint64_t)v[1 % G];
          o = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
        }
        *reinterpret_cast<uint4 *>(values + qg) = o;
      } else {
#pragma unroll
        for (unsigned j = 0; j < G; ++j)
          if (id[s * G + j] != kKeep) values[qg + j] = v[j];
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void pq_dict_fill_kernel(const nvt_pq_dict_col *__restrict__ cols, unsigned ncols,
                                                              const uint32_t *__restrict__ groups,
                                                              uint32_t *__restrict__ bad) {
  __shared__ Lds l;
  const uint32_t col = groups[2 * (uint64_t)blockIdx.x], first_tile = groups[2 * (uint64_t)blockIdx.x + 1];
  if (col >= ncols) return;   // (uniform)
  const nvt_pq_dict_col c = cols[col];
  unsigned nbad = 0;
  if (c.type_size == 4)
    fill_tiles<uint32_t>(c, first_tile, l, nbad);
  else if (c.type_size == 8)
    fill_tiles<uint64_t>(c, first_tile, l, nbad);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nbad += __shfl_down(nbad, off, 64);
  if (lane_id() == 0 && nbad) atomicAdd(bad, nbad);
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_dict_fill_many(const nvt_pq_dict_col *cols, int ncols, const uint32_t *groups, uint64_t ngroups,
                          uint32_t *bad, void *stream) {
  if (ngroups == 0) return NVT_OK;
  NVT_CHECK_ARG(cols && groups && bad, "null pointer");
  NVT_CHECK_ARG(ncols >= 1, "groups without a column");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(cols) & 7) == 0 && (reinterpret_cast<uintptr_t>(groups) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(bad) & 3) == 0,
                "tables must be aligned to their words");
  NVT_CHECK_ARG(ngroups < (1ull << 31), "fewer than 2^31 tile groups");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_dict_fill", ngroups * (uint64_t)(kTilesPerWg * kTile) * 8, s);
  pq_dict_fill_kernel<<<(unsigned)ngroups, kBlock, 0, s>>>(cols, (unsigned)ncols, groups, bad);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
