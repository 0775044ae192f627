// The sample in front of a counting pipeline: one workgroup per column picks the hot keys of the
// hot filter (nvt_count_part.hip, path | NVT_PATH_HOT) from up to 64 blocks of 1024 rows and writes
// the table image every histogram workgroup loads.  For a column of the range path
// (nvt_range_count.hip, nb_log2 > 0) the same pass also derives the key range, rescues frequent
// keys that lost their bucket and decides on the piecewise map (image[NVT_RANGE_AUX_*]).
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_lds_table.hpp"
#include "nvt_range.hpp"

namespace nvt {

constexpr int kHotSampleBlocks = 64;    // x 1024 rows

// one workgroup per column (the LDS work of a sample is ~80 us on one CU: the columns of a
// call are sampled side by side, ahead of their pipelines)
__global__ __launch_bounds__(1024) void hot_sample_kernel(const HotSampleBatch batch) {
  constexpr int32_t EMPTY = DKey<int32_t>::empty;
  const int32_t *__restrict__ keys = batch.c[blockIdx.x].keys;
  const uint8_t *__restrict__ valid = batch.c[blockIdx.x].valid;
  const uint64_t n = batch.c[blockIdx.x].n;
  int32_t *image = batch.c[blockIdx.x].image;
  __shared__ int32_t tk[kHotSlots];
  __shared__ unsigned seen[2048];  // 64 K-bit "seen once" filter
  __shared__ unsigned s_hits, s_rows, s_umin, s_umax;
  // range path only: how often the sample shows every image slot's key, and a one-row sketch of
  // the keys that found their bucket full -- a FREQUENT key that lost the race for its bucket
  // would flood one region of the partition pass (see the rescue below)
  __shared__ unsigned tcnt[kHotSlots];
  __shared__ unsigned msk[2048];
  __shared__ int32_t mk[256];
  __shared__ unsigned mc[256];
  __shared__ unsigned s_missed;
  const bool rescue = batch.c[blockIdx.x].nb_log2 > 0;
  __shared__ uint64_t s_map[5];
  unsigned pmb[kHotSlots / 1024], pmr[kHotSlots / 1024];
  bool pieces_done = false;
  for (int i = threadIdx.x; i < kHotSlots; i += 1024) tk[i] = EMPTY;
  for (int i = threadIdx.x; i < 2048; i += 1024) seen[i] = 0;
  if (rescue) {
    for (int i = threadIdx.x; i < kHotSlots; i += 1024) tcnt[i] = 0;
    for (int i = threadIdx.x; i < 2048; i += 1024) msk[i] = 0;
    if (threadIdx.x < 256) {
      mk[threadIdx.x] = EMPTY;
      mc[threadIdx.x] = 0;
    }
  }
  if (threadIdx.x == 0) {
    s_missed = 0;
    s_hits = s_rows = 0;
    s_umin = 0xFFFFFFFFu;
    s_umax = 0u;
  }
  unsigned umin = 0xFFFFFFFFu, umax = 0u;  // order-preserving unsigned images of the sampled keys
  __syncthreads();
  const uint64_t nblk = (n + 1023) / 1024;
  const unsigned S = (unsigned)(nblk < (uint64_t)kHotSampleBlocks ? nblk : kHotSampleBlocks);
  const uint64_t step = (S ? nblk / S : 1) * 1024;  // rows between the starts of sampled blocks
  auto insert = [&](int32_t key, uint32_t) -> bool {
    const uint32_t b = hot_bucket(key) * kHotWidth;
#pragma unroll
    for (int c = 0; c < kHotWidth; ++c) {
      const int32_t prev = atomicCAS(&tk[b + c], EMPTY, key);
      if (prev == EMPTY || prev == key) return true;
    }
    return false;
  };
  // the sample is read in batches of kBatch rows per thread, every load of a batch in flight
  // before the first is used (one workgroup: a dependent load per row would pay the memory
  // latency 2 x 64 times -- 200 us; holding all 64 rows per thread in registers spills)
  constexpr int kBatch = 16;
  int32_t kreg[kBatch];
  auto load_batch = [&](unsigned it0) {
#pragma unroll
    for (int q = 0; q < kBatch; ++q) {
      const unsigned it = it0 + q;
      const uint64_t i = (uint64_t)it * step + threadIdx.x;
      kreg[q] = (it < S && i < n) ? keys[i] : EMPTY;
    }
    if (valid) {  // null rows are skipped like the sentinel key
      unsigned vm = 0;
#pragma unroll
      for (int q = 0; q < kBatch; ++q) {
        const unsigned it = it0 + q;
        const uint64_t i = (uint64_t)it * step + threadIdx.x;
        const unsigned byte = (it < S && i < n) ? valid[i >> 3] : 0u;
        vm |= ((byte >> (i & 7)) & 1u) << q;
      }
#pragma unroll
      for (int q = 0; q < kBatch; ++q)
        if (!((vm >> q) & 1u)) kreg[q] = EMPTY;
    }
  };
  // sweep 1: a key enters the table when the sample shows it for the second time
  for (unsigned it0 = 0; it0 < S; it0 += kBatch) {
    load_batch(it0);
#pragma unroll
    for (int q = 0; q < kBatch; ++q) {
      const int32_t key = kreg[q];
      if (key != EMPTY) {
        const uint32_t h = slot_hash(key);
        const uint32_t bit = (h * 0x9E3779B1u) >> 16;
        const unsigned m = 1u << (bit & 31);
        if (atomicOr(&seen[bit >> 5], m) & m) insert(key, h);
      }
    }
  }
  __syncthreads();
  // sweep 2: the remaining keys, first come, while their buckets have room; the share of
  // sampled rows that find their key estimates what the table will absorb
  unsigned hits = 0, rows = 0;
  for (unsigned it0 = 0; it0 < S; it0 += kBatch) {
    load_batch(it0);
#pragma unroll
    for (int q = 0; q < kBatch; ++q) {
      const int32_t key = kreg[q];
      if (key != EMPTY) {
        const uint32_t h = slot_hash(key);  // (the sketch of the rescue below)
        const uint32_t b = hot_bucket(key) * kHotWidth;
        bool found = false;
#pragma unroll
        for (int c = 0; c < kHotWidth; ++c) found = found || tk[b + c] == key;
        bool in = found;
        if (!found) in = insert(key, h);
        if (rescue) {
          if (in) {
#pragma unroll
            for (int c = 0; c < kHotWidth; ++c)
              if (tk[b + c] == key) atomicAdd(&tcnt[b + c], 1u);
          } else {
            atomicAdd(&msk[(h * 0x85EBCA6Bu) >> 21], 1u);
            atomicAdd(&s_missed, 1u);
          }
        }
        hits += found;
        rows += 1;
        const unsigned u = (unsigned)key ^ 0x80000000u;
        umin = u < umin ? u : umin;
        umax = u > umax ? u : umax;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    hits += __shfl_down(hits, off, 64);
    rows += __shfl_down(rows, off, 64);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned a = __shfl_down(umin, off, 64), b = __shfl_down(umax, off, 64);
    umin = a < umin ? a : umin;
    umax = b > umax ? b : umax;
  }
  if (lane_id() == 0) {
    atomicAdd(&s_hits, hits);
    atomicAdd(&s_rows, rows);
    atomicMin(&s_umin, umin);
    atomicMax(&s_umax, umax);
  }
  __syncthreads();
  if (rescue) {
    // Rescue of frequent keys that are NOT in the image.  The image takes keys first come, so a
    // key as frequent as 1 % of the rows occasionally finds both slots of its bucket taken by
    // two rarer keys; all its rows then go through ONE bin of the partition pass and overflow a
    // (bucket, workgroup) region (2 x the average rows + 64): about one 45 M-row Criteo partition
    // in a hundred had to be recounted on the sort path for that.  A key whose sample count
    // reaches rows / (2 * buckets) replaces the rarer occupant of its bucket.  The sketch makes
    // the common case (nothing to rescue) free: a third sweep of the sample runs only when some
    // sketch counter stands out from the noise of the one-off keys.
    const unsigned nbk = 1u << batch.c[blockIdx.x].nb_log2;
    const unsigned T = max(16u, s_rows / (2u * nbk));
    const unsigned thr = T + 2u * (s_missed / 2048u);
    const int any = __syncthreads_or(msk[threadIdx.x] >= thr || msk[threadIdx.x + 1024] >= thr);
    if (any) {
      for (unsigned it0 = 0; it0 < S; it0 += kBatch) {
        load_batch(it0);
#pragma unroll
        for (int q = 0; q < kBatch; ++q) {
          const int32_t key = kreg[q];
          if (key == EMPTY) continue;
          const uint32_t h = slot_hash(key);
          if (msk[(h * 0x85EBCA6Bu) >> 21] < thr) continue;
          const uint32_t b = hot_bucket(key) * kHotWidth;
          bool found = false;
#pragma unroll
          for (int c = 0; c < kHotWidth; ++c) found = found || tk[b + c] == key;
          if (found) continue;
          uint32_t m = (h >> 3) & 255u;
          for (int step = 0; step < 256; ++step, m = (m + 1) & 255u) {  // exact count of the candidates
            const int32_t prev = atomicCAS(&mk[m], EMPTY, key);
            if (prev == EMPTY || prev == key) {
              atomicAdd(&mc[m], 1u);
              break;
            }
          }
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int m = 0; m < 256; ++m) {
          const int32_t key = mk[m];
          const unsigned c = mc[m];
          if (key == EMPTY || c < T) continue;
          const uint32_t b = hot_bucket(key) * kHotWidth;
          int worst = 0;
#pragma unroll
          for (int w = 1; w < kHotWidth; ++w)
            if (tcnt[b + w] < tcnt[b + worst]) worst = w;
          if (tcnt[b + worst] < c) {  // the rarer occupant leaves the image (and goes through the bins)
            tk[b + worst] = key;
            tcnt[b + worst] = c;
          }
        }
      }
      __syncthreads();
    }
  }
  const bool useful = (uint64_t)s_hits * 8 >= (uint64_t)s_rows && s_rows > 0;
  for (int i = threadIdx.x; i < kHotSlots; i += 1024) image[i] = useful ? tk[i] : EMPTY;
  const int nb_log2 = batch.c[blockIdx.x].nb_log2;
  if (nb_log2 > 0 && threadIdx.x == 0) {
    // range path: fine slot = (min(u - ulo, span) * mul) >> sh over the sampled span padded by
    // 1/64 on either side (keys outside land in the edge slots: monotone, just unbalanced);
    // see RangeMap in nvt_range_count.hip
    uint64_t lo = s_umin, hi = s_umax;
    if (s_rows == 0) {
      lo = 0;
      hi = 0xFFFFFFFFull;
    }
    const uint64_t pad = ((hi - lo) >> 6) + 1;
    lo = lo > pad ? lo - pad : 0;
    hi = hi + pad < 0xFFFFFFFFull ? hi + pad : 0xFFFFFFFFull;
    const uint64_t span = hi - lo, F = 1ull << (nb_log2 + 14);
    uint32_t mul;
    int sh;
    range_map_params(span, F, &mul, &sh);
    image[NVT_RANGE_AUX_LO] = (int32_t)(uint32_t)lo;
    image[NVT_RANGE_AUX_LO + 1] = (int32_t)(uint32_t)span;
    image[NVT_RANGE_AUX_LO + 2] = (int32_t)mul;
    image[NVT_RANGE_AUX_LO + 3] = 0;
    image[NVT_RANGE_AUX_LO + 4] = sh;
    image[NVT_RANGE_AUX_LO + 5] = 0;  // bucket-region table layout (nvt_range.hpp)
    image[NVT_RANGE_AUX_LO + 7] = 0;  // linear map (the piecewise form is decided below)
    s_map[0] = lo;
    s_map[1] = span;
    s_map[2] = mul;
    s_map[3] = (uint64_t)sh;
  }
  if (nb_log2 >= 6 && batch.c[blockIdx.x].pieces) {
    // ---- piecewise map: the caller put kRpPieces + 1 splitters (order-preserving u32 images,
    // strictly increasing) into the aux block -- taken from an EXACT key-ordered (key, count)
    // list of an earlier pass over this column (kernels.range_splitters: rows and distinct keys
    // blended, so that no piece holds more than ~2x the average of either).  A sample of a few
    // thousand rows cannot do this: nearly every cold key is a singleton in it, so it sees rows,
    // not distinct keys, and the tail pieces of a dense-id column came out with 3.5x the average
    // number of distinct keys (tools/pieces_probe.py).  Here: multipliers + the CSR of the hot keys.
    __shared__ uint32_t s_pw[2 * kRpPieces + 3];
    for (int p = threadIdx.x; p <= kRpPieces; p += 1024)
      s_pw[p] = (uint32_t)image[NVT_RANGE_AUX_PW + p];
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t S = 1u << (nb_log2 + 8);   // fine slots per piece = buckets / 64 x 16384
      bool ok = true;
      for (int p = 0; p < kRpPieces; ++p) ok = ok && s_pw[p + 1] > s_pw[p];
      if (ok) {
        uint32_t flags[2] = {0u, 0u};
        for (int p = 0; p < kRpPieces; ++p) {
          const uint32_t w = s_pw[p + 1] - s_pw[p];
          uint32_t mulp;
          if (w > S) {
            mulp = (uint32_t)((((uint64_t)S) << 32) / w);
            flags[p >> 5] |= 1u << (p & 31);
          } else {  // fewer keys than slots: 16-bit fixed point (an integer factor S / w would leave
                    // up to half of the piece's slots unused and its first buckets overfull)
            const uint64_t m16 = (((uint64_t)S) << 16) / w;
            mulp = (uint32_t)(m16 < 0xFFFFFFFFull ? m16 : 0xFFFFFFFFull);
          }
          s_pw[kRpPwMul + p] = mulp;
        }
        s_pw[kRpPwSh] = flags[0];
        s_pw[kRpPwSh + 1] = flags[1];
        s_map[4] = S;
      } else {
        s_map[4] = 0;   // (malformed splitters: the linear map)
      }
    }
    __syncthreads();
    if (s_map[4]) {
      for (int p = threadIdx.x; p < 2 * kRpPieces + 3; p += 1024) image[NVT_RANGE_AUX_PW + p] = (int32_t)s_pw[p];
      if (threadIdx.x == 0) image[NVT_RANGE_AUX_LO + 7] = (int32_t)s_map[4];
    }
    __syncthreads();
    // (the CSR below maps the hot keys with the map that was just decided)
    if (s_map[4]) {
      RangeMap pm;
      pm.ulo = 0; pm.span = 0; pm.mul = 0; pm.sh = 0; pm.flat = 0;
      pm.piece_slots = (uint32_t)s_map[4];
      pm.pw = s_pw;
      pm.lpw = (const __attribute__((address_space(3))) uint32_t *)s_pw;
      unsigned *bcnt = seen;
      for (int i = threadIdx.x; i < 1025; i += 1024) bcnt[i] = 0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kHotSlots / 1024; ++q) {
        const int i = q * 1024 + threadIdx.x;
        const int32_t key = useful ? tk[i] : EMPTY;
        pmb[q] = 0xFFFFFFFFu;
        if (key != EMPTY) {
          pmb[q] = pm.fine(key) >> 14;
          pmr[q] = atomicAdd(&bcnt[pmb[q]], 1u);
        }
      }
      pieces_done = true;
    }
  } else if (nb_log2 > 0 && threadIdx.x == 0) {
    s_map[4] = 0;
  }
  if (nb_log2 > 0) {
    // the image slots indexed by range bucket (counting sort): the per-bucket count workgroup
    // of the range path picks up its hot keys without scanning the whole image
    unsigned *bcnt = seen;  // 2048 words, free again
    unsigned myb[kHotSlots / 1024], myr[kHotSlots / 1024];
    if (!pieces_done) {
    for (int i = threadIdx.x; i < 1025; i += 1024) bcnt[i] = 0;
    __syncthreads();
    const uint64_t lo = s_map[0], span = s_map[1], mul = s_map[2];
    const int sh = (int)s_map[3];
#pragma unroll
    for (int q = 0; q < kHotSlots / 1024; ++q) {
      const int i = q * 1024 + threadIdx.x;
      const int32_t key = useful ? tk[i] : EMPTY;
      myb[q] = 0xFFFFFFFFu;
      if (key != EMPTY) {
        const uint64_t u = (uint32_t)key ^ 0x80000000u;
        uint64_t d = u > lo ? u - lo : 0;
        d = d < span ? d : span;
        myb[q] = (unsigned)((((d << sh) * mul) >> 32) >> 14);  // RangeMap::fine
        myr[q] = atomicAdd(&bcnt[myb[q]], 1u);
      }
    }
    } else {
#pragma unroll
      for (int q = 0; q < kHotSlots / 1024; ++q) {
        myb[q] = pmb[q];
        myr[q] = pmr[q];
      }
    }
    __syncthreads();
    // exclusive scan of the 1024 bucket counts (one per thread)
    __shared__ unsigned swt[16];
    const unsigned v = bcnt[threadIdx.x];
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned o = __shfl_up(inc, off, 64);
      if (lane_id() >= (unsigned)off) inc += o;
    }
    if (lane_id() == 63) swt[threadIdx.x / 64] = inc;
    __syncthreads();
    unsigned wb = 0;
    for (unsigned q = 0; q < threadIdx.x / 64; ++q) wb += swt[q];
    const unsigned start = wb + inc - v;
    __syncthreads();
    bcnt[threadIdx.x] = start;
    image[NVT_RANGE_AUX_HOTSTART + threadIdx.x] = (int32_t)start;
    if (threadIdx.x == 1023) image[NVT_RANGE_AUX_HOTSTART + 1024] = (int32_t)(start + v);
    __syncthreads();
    unsigned short *order = reinterpret_cast<unsigned short *>(image + NVT_RANGE_AUX_HOTORDER);
#pragma unroll
    for (int q = 0; q < kHotSlots / 1024; ++q)
      if (myb[q] != 0xFFFFFFFFu) order[bcnt[myb[q]] + myr[q]] = (unsigned short)(q * 1024 + threadIdx.x);
  }
}

int hot_sample_launch(const HotSampleBatch &batch, int ncols, hipStream_t s) {
  hot_sample_kernel<<<ncols, 1024, 0, s>>>(batch);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // namespace nvt
