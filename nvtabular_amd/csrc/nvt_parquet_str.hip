// Parquet in, string columns: the dictionary-index streams of a partition are expanded on the device.
// The host decoder (nvt_pq_decode_str_chunk, nvt_parquet.hip) leaves a run table and the bytes of
// the bit-packed runs as the file holds them (include/nvt_hip.h, "parquet in: string columns");
// nvt_pq_expand_runs turns them into one entry id per non-null value:
//
//   * the output values are spread over the grid in tiles of 2048, one value per lane and step, so
//     the stores are coalesced whatever the runs look like (as slice_move_kernel spreads leaves);
//   * the run of a tile's first and last value is a binary search over the table in global memory
//     (two lanes); the starts of the tile's runs -- at most 2049, no run is empty -- are staged in
//     LDS and every lane finds its run there.  A table that breaks that promise is searched in
//     global memory instead: it costs time, never a read outside the table;
//   * a packed value is two aligned 32-bit loads and a funnel shift (v_alignbit_b32): value k of a
//     run lies at bit k * width of the run's words, and runs start on a word;
//   * an id outside [0, entries) becomes -1 and is counted per lane; a wave adds its count with one
//     atomic at the end.
#include <hip/hip_runtime.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr uint64_t kRunTile = 2048;      // output values per tile
constexpr unsigned kRunStage = 2048 + 2; // run starts of one tile held in LDS

// the record r in [lo, hi] with start(r) <= q < start(r + 1) when the starts ascend; some record of
// [lo, hi] whatever they hold.  get(r) = start of record r
template <typename G>
__device__ __forceinline__ uint64_t run_of(G get, uint64_t lo, uint64_t hi, uint32_t q) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (get(mid) <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void pq_expand_runs_kernel(const uint4 *__restrict__ runs, uint64_t nruns,
                                                                const uint32_t *__restrict__ packed,
                                                                uint64_t packed_words, uint64_t entries,
                                                                uint64_t nvalues, int32_t *__restrict__ out,
                                                                uint32_t *__restrict__ bad) {
  __shared__ uint32_t sstart[kRunStage];
  __shared__ uint64_t sbound[2];
  const uint32_t *starts = reinterpret_cast<const uint32_t *>(runs);   // start of record r = starts[4 * r]
  auto global_start = [&](uint64_t r) { return starts[4 * r]; };
  auto lds_start = [&](uint64_t r) { return sstart[r]; };
  const uint64_t nt = (nvalues + kRunTile - 1) / kRunTile;
  unsigned nbad = 0;
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t p0 = t * kRunTile;
    const uint64_t p1 = p0 + kRunTile < nvalues ? p0 + kRunTile : nvalues;
    if (threadIdx.x < 2)
      sbound[threadIdx.x] = run_of(global_start, 0, nruns - 1, (uint32_t)(threadIdx.x == 0 ? p0 : p1 - 1));
    __syncthreads();
    const uint64_t rlo = sbound[0];
    const uint64_t rhi = sbound[1] >= rlo ? sbound[1] : rlo;
    const bool staged = rhi - rlo + 1 <= (uint64_t)kRunStage;   // (block-uniform)
    if (staged)
      for (uint64_t k = threadIdx.x; k < rhi - rlo + 1; k += kBlock) sstart[k] = starts[4 * (rlo + k)];
    __syncthreads();
    for (uint64_t q = p0 + threadIdx.x; q < p1; q += kBlock) {
      const uint64_t r = staged ? rlo + run_of(lds_start, 0, rhi - rlo, (uint32_t)q)
                                : run_of(global_start, rlo, rhi, (uint32_t)q);
      const uint4 rec = runs[r];   // {start, kind | width << 8, a, b}: the lanes of a run load one address
      const unsigned kind = rec.y & 0xFFu, width = (rec.y >> 8) & 0xFFu;
      uint64_t id = ~0ull;
      if (q >= rec.x) {
        const uint64_t k = q - rec.x;
        if (kind == NVT_PQ_RUN_REPEAT) {
          id = rec.z;
        } else if (kind == NVT_PQ_RUN_SEQUENCE) {
          id = (uint64_t)rec.z + k;
        } else if (kind == NVT_PQ_RUN_PACKED && width >= 1 && width <= 32) {
          const uint64_t bit = k * width;
          const uint64_t w = (uint64_t)rec.w + (bit >> 5);
          if (w + 1 < packed_words) {
            const uint32_t lo = packed[w], hi = packed[w + 1];
            uint32_t v = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(bit & 31));
            if (width < 32) v &= (1u << width) - 1u;
            id = (uint64_t)rec.z + v;
          }
        }
      }
      const bool ok = id < entries;
      out[q] = ok ? (int32_t)id : -1;
      nbad += ok ? 0u : 1u;
    }
    __syncthreads();
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nbad += __shfl_down(nbad, off, 64);
  if (lane_id() == 0 && nbad) atomicAdd(bad, nbad);
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_expand_runs(const uint32_t *runs, uint64_t nruns, const uint32_t *closing, const uint8_t *packed,
                       uint64_t packed_bytes, uint64_t entries, uint64_t nvalues, int32_t *out, uint32_t *bad,
                       void *stream) {
  NVT_CHECK_ARG(closing, "null closing record");
  NVT_CHECK_ARG(closing[0] == nvalues && (closing[1] & 0xFFu) == NVT_PQ_RUN_END,
                "the run table's closing record does not say nvalues");
  if (nvalues == 0) return NVT_OK;
  NVT_CHECK_ARG(runs && packed && out && bad, "null pointer");
  NVT_CHECK_ARG(nruns >= 1, "values without a run");
  NVT_CHECK_ARG(nvalues < (1ull << 32) - kRunTile && entries < (1ull << 31), "fewer than 2^32 - 2048 values, 2^31 entries");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(runs) & 15) == 0 && (reinterpret_cast<uintptr_t>(packed) & 3) == 0,
                "runs must be 16-byte, packed 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("pq_expand_runs", packed_bytes + nvalues * 4, s);
  const uint64_t nt = (nvalues + kRunTile - 1) / kRunTile;
  const unsigned grid = (unsigned)(nt < (uint64_t)kCUs * 8 ? nt : (uint64_t)kCUs * 8);
  pq_expand_runs_kernel<<<grid, kBlock, 0, s>>>(reinterpret_cast<const uint4 *>(runs), nruns,
                                                reinterpret_cast<const uint32_t *>(packed), packed_bytes / 4, entries,
                                                nvalues, out, bad);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
