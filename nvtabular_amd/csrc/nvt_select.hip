// Exact order statistics of a column without sorting it: MSD radix select (FillMedian.fit).
//
// Every value maps to an order-preserving unsigned key of its own width (float: flip all bits of
// a negative value, the sign bit of the others; int: flip the sign bit).  The two middle ranks
// k_lo = (m - 1) / 2 and k_hi = m / 2 of the m participating rows are found digit by digit, 11
// bits at a time from the top (3 passes for a 32-bit key, 6 for a 64-bit key): a pass histograms
// the current digit of the rows whose higher digits equal the prefix selected so far
// (nvt_select_hist_many: one streaming pass over one chunk of every column, per-workgroup LDS
// histograms, one global atomic per non-empty bin), then one small workgroup per column picks
// the bin that holds each rank (nvt_select_step).  The histograms of the chunks of a column, and
// of the ranks of a job, simply add.  Nothing is read back between the passes: a column that is
// resolved sets its `done` word and the remaining launches return at once for it.
//
// Candidate path: when the top-digit bins of the two ranks hold at most NVT_SELECT_CAND_CAP rows,
// pass 1 copies the keys of those rows into the column's candidate buffer instead of counting
// them, and nvt_select_finish resolves the remaining digits inside that buffer (one workgroup
// per column, the buffer stays in L2).  A column read twice instead of 3 / 6 times.
//
// Reference: nvtabular/ops/fill.py:83-146 (FillMedian), whose tests pin the fitted value to
// pandas' quantile(0.5, interpolation="linear") of the non-null rows.
#include <limits>
#include <type_traits>

#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {

constexpr int kSelBins = NVT_SELECT_BINS;
constexpr int kSelDigit = 11;
constexpr int kFinishBlock = 1024;
static_assert(kSelBins == 1 << kSelDigit, "one bin per digit value");

// ---- keys --------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t sel_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ uint64_t sel_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t sel_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ uint64_t sel_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }

// passes of a key of `bits` bits, and the digit pass p looks at: digits are cut from the TOP, so
// the last one is the short one (10 bits of a 32-bit key, 9 of a 64-bit key)
__host__ __device__ __forceinline__ int sel_passes(int bits) { return (bits + kSelDigit - 1) / kSelDigit; }
// bits below the digit of pass p
__host__ __device__ __forceinline__ int sel_shift(int bits, int p) {
  const int s = bits - kSelDigit * (p + 1);
  return s > 0 ? s : 0;
}
// bits below the digits of the passes BEFORE p (p >= 1): what the prefix comparison shifts out
__host__ __device__ __forceinline__ int sel_prefix_shift(int bits, int p) { return bits - kSelDigit * p; }
__device__ __forceinline__ unsigned sel_digit(uint64_t key, int bits, int p) {
  const int hb = sel_prefix_shift(bits, p);           // the digit lies below bit hb ...
  const int sh = sel_shift(bits, p);                  // ... and above bit sh
  return (unsigned)((key >> sh) & ((1ull << (hb - sh)) - 1ull));
}

// ---- LDS histogram add of a whole wave -----------------------------------------------------
// Every lane of the wave calls this together.  Rows of real columns crowd into a few bins (the top
// digit of a float is its sign and exponent; counts are zero-inflated), and lanes that add to
// one LDS address are served one after the other: twice, the lanes that hold the digit of the
// first remaining lane are counted with a ballot and added by that lane alone.
__device__ __forceinline__ void wave_hist_add(uint32_t *h, unsigned digit, bool on) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint64_t act = __ballot(on);
    if (!act) return;
    const int first = __ffsll((unsigned long long)act) - 1;
    const unsigned d0 = (unsigned)__shfl((int)digit, first, kWave);
    const bool mine = on && digit == d0;
    const uint64_t same = __ballot(mine);
    if (mine) {
      if ((int)lane_id() == first) atomicAdd(&h[d0], (uint32_t)__popcll(same));
      on = false;
    }
  }
  if (on) atomicAdd(&h[digit], 1u);
}

// ---- state ---------------------------------------------------------------------------------
struct SelCol {
  const void *x;
  const uint8_t *valid;
  uint64_t n;
  double fill_val;
  int dtype, has_fill;
  unsigned grid;
};
struct SelBatch {
  SelCol c[NVT_SELECT_MAX_COLS];
};

__device__ __forceinline__ uint64_t *sel_state(uint64_t *state, unsigned col) {
  return state + (uint64_t)col * NVT_SELECT_STATE_WORDS;
}

// what a pass needs of a column's state, read once per workgroup
struct SelView {
  uint64_t plo, phi;
  int bits, hb;       // key width; bits below the prefix (pass >= 1)
  bool same, gather;  // both ranks follow one prefix; this launch gathers candidates
};

// one chunk of one column
template <typename T>
__device__ __forceinline__ void select_hist_body(const SelCol &c, const SelView &v, int pass,
                                                 uint32_t *h0, uint32_t *h1, uint64_t *st) {
  constexpr int VEC = 16 / sizeof(T);
  const T *x = (const T *)c.x;
  const uint8_t *valid = c.valid;
  const uint64_t fill_key = c.has_fill ? sel_key((T)c.fill_val) : 0;
  const bool has_fill = c.has_fill;
  uint64_t *cand = st + NVT_SELECT_ST_CAND;
  unsigned long long *cand_n = (unsigned long long *)(st + NVT_SELECT_ST_NCAND);

  auto row = [&](T raw, bool ok, bool live) {
    // live = false: the lane has no row in this round (it still takes part in the wave's votes)
    bool on = live;
    uint64_t key = 0;
    if (live) {
      if (ok && !is_nan(raw)) key = sel_key(raw);
      else if (has_fill) key = fill_key;
      else on = false;
    }
    if (pass == 0) {
      wave_hist_add(h0, sel_digit(key, v.bits, 0), on);
      return;
    }
    const bool mlo = on && ((key ^ v.plo) >> v.hb) == 0;
    const bool mhi = on && !v.same && ((key ^ v.phi) >> v.hb) == 0;
    if (v.gather) {
      // the rows of the rank bins go to the candidate buffer: one counter add per wave
      const bool take = mlo || mhi;
      const uint64_t votes = __ballot(take);
      if (!votes) return;
      const int first = __ffsll((unsigned long long)votes) - 1;
      unsigned long long base = 0;
      if ((int)lane_id() == first) base = atomicAdd(cand_n, (unsigned long long)__popcll(votes));
      base = __shfl(base, first, kWave);
      if (take) {
        const uint64_t at = base + __popcll(votes & ((1ull << lane_id()) - 1ull));
        if (at < NVT_SELECT_CAND_CAP) cand[at] = key;   // (the step counted them: always true)
      }
      return;
    }
    const unsigned d = sel_digit(key, v.bits, pass);
    wave_hist_add(h0, d, mlo);
    if (!v.same) wave_hist_add(h1, d, mhi);
  };

  // every lane of a workgroup makes the same number of rounds (the votes above need whole waves)
  const uint64_t nvec = c.n / VEC;
  const uint64_t stride = (uint64_t)c.grid * kBlock;
  for (uint64_t b = (uint64_t)blockIdx.x * kBlock; b < nvec; b += stride) {
    const uint64_t i = b + threadIdx.x;
    const bool live = i < nvec;
    T val[VEC];
    unsigned vbits = 0xFFu;
    if (live) {
      typedef int v4i_ntl __attribute__((ext_vector_type(4)));
      const v4i_ntl raw = __builtin_nontemporal_load(reinterpret_cast<const v4i_ntl *>(x + i * VEC));
      memcpy(val, &raw, 16);
      if (valid != nullptr) vbits = (unsigned)valid[(i * VEC) >> 3] >> ((i * VEC) & 7);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) val[j] = T(0);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) row(val[j], (vbits >> j) & 1, live);
  }
  if (blockIdx.x == 0) {   // the rows behind the last whole vector: fewer than VEC
    const uint64_t i = nvec * VEC + threadIdx.x;
    const bool live = threadIdx.x < kWave ? i < c.n : false;
    if (threadIdx.x < kWave) row(live ? x[i] : T(0), live && bit_valid(valid, i), live);
  }
}

__global__ __launch_bounds__(kBlock) void select_hist_kernel(SelBatch b, int pass, uint64_t *state,
                                                             unsigned col0) {
  const SelCol &c = b.c[blockIdx.y];
  if (blockIdx.x >= c.grid) return;
  uint64_t *st = sel_state(state, col0 + blockIdx.y);
  if (st[NVT_SELECT_ST_DONE]) return;
  SelView v;
  v.bits = (int)st[NVT_SELECT_ST_BITS];
  if (pass >= sel_passes(v.bits)) return;
  v.plo = st[NVT_SELECT_ST_KEY_LO];
  v.phi = st[NVT_SELECT_ST_KEY_HI];
  v.same = pass == 0 || v.plo == v.phi;
  v.hb = pass == 0 ? 0 : sel_prefix_shift(v.bits, pass);
  const bool cand = st[NVT_SELECT_ST_USE_CAND] != 0;
  if (cand && pass > 1) return;   // (nvt_select_finish sets `done` behind pass 1)
  v.gather = cand && pass == 1;

  __shared__ uint32_t h[2][kSelBins];
  for (int i = threadIdx.x; i < 2 * kSelBins; i += kBlock) (&h[0][0])[i] = 0;
  __syncthreads();
  switch (c.dtype) {
    case NVT_F32: select_hist_body<float>(c, v, pass, h[0], h[1], st); break;
    case NVT_F64: select_hist_body<double>(c, v, pass, h[0], h[1], st); break;
    case NVT_I32: select_hist_body<int32_t>(c, v, pass, h[0], h[1], st); break;
    default: select_hist_body<int64_t>(c, v, pass, h[0], h[1], st); break;
  }
  if (v.gather) return;
  __syncthreads();
  unsigned long long *g = (unsigned long long *)(st + NVT_SELECT_ST_HIST);
  const int nh = v.same ? kSelBins : 2 * kSelBins;
  for (int i = threadIdx.x; i < nh; i += kBlock) {
    const uint32_t k = (&h[0][0])[i];
    if (k) atomicAdd(g + i, (unsigned long long)k);
  }
}

// ---- picking the bins ------------------------------------------------------------------------
// The ranks and prefixes of one column while a workgroup works on them (LDS).
struct SelRanks {
  uint64_t plo, phi;   // digits selected so far, in place (the bits below are 0)
  uint64_t klo, khi;   // ranks inside the rows that share the prefix
  uint64_t clo, chi;   // rows in the bins just picked
  unsigned dlo, dhi;   // the bins just picked
};

// Every thread of the workgroup calls this.  h0 / h1: kSelBins counts of the rows that share the
// prefix of the low / high rank (h1 == h0 while the ranks share a prefix).  Picks the bin of each
// rank, appends it to the prefix and makes the rank relative to the bin.  `sums`: LDS, one word
// per thread.
template <typename H>
__device__ __forceinline__ void select_pick(const H *h0, const H *h1, int sh, SelRanks *r, uint64_t *sums) {
  const int per = kSelBins / blockDim.x;
  for (int which = 0; which < 2; ++which) {
    const H *h = which ? h1 : h0;
    uint64_t s = 0;
    for (int j = 0; j < per; ++j) s += (uint64_t)h[threadIdx.x * per + j];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {   // exclusive prefix over the threads' sums
      uint64_t run = 0;
      for (unsigned t = 0; t < blockDim.x; ++t) {
        const uint64_t v = sums[t];
        sums[t] = run;
        run += v;
      }
    }
    __syncthreads();
    const uint64_t k = which ? r->khi : r->klo;
    uint64_t below = sums[threadIdx.x];
    __syncthreads();
    if (k >= below && k < below + s) {   // exactly one thread: the bin lies in its range
      for (int j = 0; j < per; ++j) {
        const uint64_t cnt = (uint64_t)h[threadIdx.x * per + j];
        if (k < below + cnt) {
          const unsigned d = threadIdx.x * per + j;
          if (which) {
            r->phi |= (uint64_t)d << sh;
            r->khi = k - below;
            r->chi = cnt;
            r->dhi = d;
          } else {
            r->plo |= (uint64_t)d << sh;
            r->klo = k - below;
            r->clo = cnt;
            r->dlo = d;
          }
          break;
        }
        below += cnt;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void select_step_kernel(uint64_t *state, int pass) {
  uint64_t *st = sel_state(state, blockIdx.x);
  if (st[NVT_SELECT_ST_DONE]) return;
  const int bits = (int)st[NVT_SELECT_ST_BITS];
  const int npass = sel_passes(bits);
  if (pass >= npass) return;
  if (pass == 1 && st[NVT_SELECT_ST_USE_CAND]) return;   // (nothing was counted: the rows were gathered)
  uint64_t *hist = st + NVT_SELECT_ST_HIST;

  __shared__ SelRanks r;
  __shared__ uint64_t sums[kBlock];
  __shared__ uint64_t total;
  if (pass == 0) {
    // m = the rows counted = the sum of the bins
    uint64_t s = 0;
    for (int i = threadIdx.x; i < kSelBins; i += kBlock) s += hist[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t m = 0;
      for (int t = 0; t < kBlock; ++t) m += sums[t];
      total = m;
      r.plo = r.phi = 0;
      r.klo = m ? (m - 1) / 2 : 0;
      r.khi = m / 2;
    }
    __syncthreads();
    if (total == 0) {
      if (threadIdx.x == 0) {
        st[NVT_SELECT_ST_M] = 0;
        st[NVT_SELECT_ST_DONE] = 1;
      }
      return;   // (every bin is 0 already)
    }
  } else {
    if (threadIdx.x == 0) {
      r.plo = st[NVT_SELECT_ST_KEY_LO];
      r.phi = st[NVT_SELECT_ST_KEY_HI];
      r.klo = st[NVT_SELECT_ST_RANK_LO];
      r.khi = st[NVT_SELECT_ST_RANK_HI];
    }
    __syncthreads();
  }
  const bool same = pass == 0 || r.plo == r.phi;
  __syncthreads();
  select_pick<uint64_t>(hist, same ? hist : hist + kSelBins, sel_shift(bits, pass), &r, sums);
  for (int i = threadIdx.x; i < 2 * kSelBins; i += kBlock) hist[i] = 0;
  if (threadIdx.x == 0) {
    st[NVT_SELECT_ST_KEY_LO] = r.plo;
    st[NVT_SELECT_ST_KEY_HI] = r.phi;
    st[NVT_SELECT_ST_RANK_LO] = r.klo;
    st[NVT_SELECT_ST_RANK_HI] = r.khi;
    if (pass == 0) {
      st[NVT_SELECT_ST_M] = total;
      const uint64_t rows = r.clo + (r.dhi != r.dlo ? r.chi : 0);
      const bool cand = st[NVT_SELECT_ST_ALLOW_CAND] != 0 && npass > 1 && rows <= NVT_SELECT_CAND_CAP;
      st[NVT_SELECT_ST_USE_CAND] = cand ? 1 : 0;
      st[NVT_SELECT_ST_PATH] = cand ? NVT_SELECT_PATH_CAND : NVT_SELECT_PATH_FULL;
      st[NVT_SELECT_ST_NCAND] = 0;
    }
    if (pass == npass - 1) st[NVT_SELECT_ST_DONE] = 1;
  }
}

// The remaining digits of a candidate column, inside its buffer.
__global__ __launch_bounds__(kFinishBlock) void select_finish_kernel(uint64_t *state) {
  uint64_t *st = sel_state(state, blockIdx.x);
  if (st[NVT_SELECT_ST_DONE] || !st[NVT_SELECT_ST_USE_CAND]) return;
  const int bits = (int)st[NVT_SELECT_ST_BITS];
  const int npass = sel_passes(bits);
  uint64_t ncand = st[NVT_SELECT_ST_NCAND];
  if (ncand > NVT_SELECT_CAND_CAP) ncand = NVT_SELECT_CAND_CAP;
  const uint64_t *cand = st + NVT_SELECT_ST_CAND;

  __shared__ SelRanks r;
  __shared__ uint64_t sums[kFinishBlock];
  __shared__ uint32_t h[2][kSelBins];
  if (threadIdx.x == 0) {
    r.plo = st[NVT_SELECT_ST_KEY_LO];
    r.phi = st[NVT_SELECT_ST_KEY_HI];
    r.klo = st[NVT_SELECT_ST_RANK_LO];
    r.khi = st[NVT_SELECT_ST_RANK_HI];
  }
  __syncthreads();
  for (int pass = 1; pass < npass; ++pass) {
    for (int i = threadIdx.x; i < 2 * kSelBins; i += kFinishBlock) (&h[0][0])[i] = 0;
    __syncthreads();
    const uint64_t plo = r.plo, phi = r.phi;
    const bool same = plo == phi;
    const int hb = sel_prefix_shift(bits, pass);
    constexpr int U = 4;   // independent loads in flight: one workgroup has little else to hide them
    for (uint64_t i0 = threadIdx.x; i0 < ncand; i0 += (uint64_t)kFinishBlock * U) {
      uint64_t key[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t i = i0 + (uint64_t)u * kFinishBlock;
        key[u] = i < ncand ? cand[i] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + (uint64_t)u * kFinishBlock >= ncand) break;
        const unsigned d = sel_digit(key[u], bits, pass);
        if (((key[u] ^ plo) >> hb) == 0) atomicAdd(&h[0][d], 1u);
        if (!same && ((key[u] ^ phi) >> hb) == 0) atomicAdd(&h[1][d], 1u);
      }
    }
    __syncthreads();
    select_pick<uint32_t>(h[0], same ? h[0] : h[1], sel_shift(bits, pass), &r, sums);
  }
  if (threadIdx.x == 0) {
    st[NVT_SELECT_ST_KEY_LO] = r.plo;
    st[NVT_SELECT_ST_KEY_HI] = r.phi;
    st[NVT_SELECT_ST_RANK_LO] = r.klo;
    st[NVT_SELECT_ST_RANK_HI] = r.khi;
    st[NVT_SELECT_ST_DONE] = 1;
  }
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_select_hist_many(const nvt_select_col *cols, int ncols, int pass, void *state, void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must be >= 0");
  NVT_CHECK_ARG(pass >= 0 && pass < NVT_SELECT_MAX_PASSES, "pass must be 0 .. 5");
  if (ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(cols, "null descriptors");
  NVT_CHECK_ARG(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be non-null and 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < ncols; ++i) {
    const nvt_select_col &c = cols[i];
    NVT_CHECK_ARG(c.dtype == NVT_F32 || c.dtype == NVT_F64 || c.dtype == NVT_I32 || c.dtype == NVT_I64,
                  "unsupported dtype");
    NVT_CHECK_ARG(c.n == 0 || (c.x && (reinterpret_cast<uintptr_t>(c.x) & 15) == 0),
                  "x must be non-null and 16-byte aligned");
  }
  for (int c0 = 0; c0 < ncols; c0 += NVT_SELECT_MAX_COLS) {
    const int nc = ncols - c0 < NVT_SELECT_MAX_COLS ? ncols - c0 : NVT_SELECT_MAX_COLS;
    SelBatch b;
    memset(&b, 0, sizeof(b));
    unsigned grid = 0;
    uint64_t bytes = 0;
    for (int i = 0; i < nc; ++i) {
      const nvt_select_col &c = cols[c0 + i];
      SelCol &d = b.c[i];
      d.x = c.x;
      d.valid = c.valid;
      d.n = c.n;
      d.fill_val = c.fill_val;
      d.dtype = c.dtype;
      d.has_fill = c.has_fill;
      const int width = c.dtype == NVT_F32 || c.dtype == NVT_I32 ? 4 : 8;
      // (a column without rows in this chunk launches no workgroup that does anything)
      d.grid = c.n ? stream_grid(c.n / (16 / width) + 1, kBlock * 8, 2) : 0;
      grid = d.grid > grid ? d.grid : grid;
      bytes += c.n * width;
    }
    if (!grid) continue;
    NVT_PROF("select_hist", bytes, s);
    select_hist_kernel<<<dim3(grid, nc), kBlock, 0, s>>>(b, pass, reinterpret_cast<uint64_t *>(state),
                                                         (unsigned)c0);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_select_step(void *state, int ncols, int pass, void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must be >= 0");
  NVT_CHECK_ARG(pass >= 0 && pass < NVT_SELECT_MAX_PASSES, "pass must be 0 .. 5");
  if (ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be non-null and 8-byte aligned");
  select_step_kernel<<<ncols, kBlock, 0, (hipStream_t)stream>>>(reinterpret_cast<uint64_t *>(state), pass);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_select_finish(void *state, int ncols, void *stream) {
  NVT_CHECK_ARG(ncols >= 0, "ncols must be >= 0");
  if (ncols == 0) return NVT_OK;
  NVT_CHECK_ARG(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be non-null and 8-byte aligned");
  select_finish_kernel<<<ncols, kFinishBlock, 0, (hipStream_t)stream>>>(reinterpret_cast<uint64_t *>(state));
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
