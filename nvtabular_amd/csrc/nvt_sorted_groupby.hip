// ---- one int32 key column: groupby by SORTING (JoinGroupby / TargetEncoding fit) --------------
// The hash update of nvt_groupby.hip costs a random 16-byte probe per row (gb_assign 1.28 ms for
// 20 M rows), a sort of (slot, row) words, and a compaction of the sparse table afterwards.  With
// ONE key column of at most 32 bits none of the three is needed: the rows are sorted by the key
// itself,
//   sort_packed_keys     words = (key image << 32 | fold << rb | row), packed from the column by
//                        the histogram and the first scatter pass (never written out unsorted);
//                        onesweep LSD radix on bits [rb, 64): every key's rows are one run, the
//                        folds of a key (TargetEncoding's kfold) consecutive sub-runs
//   sgb_rle_kernel       run heads -> group index g (decoupled look-back over the tiles): the
//                        groups come out DENSE and ordered by key, the words are rewritten as
//                        ((g * kfold + fold) << 32 | row)
//   gb_segreduce_kernel  the same wave-level segmented reduction as the hash table's sort path
//                        (nvt_segreduce.hip), into dense arrays
//                        indexed g * kfold + fold (monotone in the sorted order: atomics of
//                        neighbouring waves fall into neighbouring sectors)
//   sgb_fold_total_kernel  per-key totals as the sum over the key's folds (TargetEncoding needs
//                        both tables, categorify.py:1344-1540 run twice in the reference)
// and the key -> group index for the transform side is a flat range table laid out from the
// sorted keys (flat_build_kernel, nvt_vocab_order.hip) instead of a second hash table.
#include <limits>

#include "nvt_groupby.hpp"
#include "nvt_prof.hpp"

namespace nvt {

#ifndef NVT_SGB_ROWS
#define NVT_SGB_ROWS 16
#endif
constexpr int kSgbRows = NVT_SGB_ROWS;
constexpr int kSgbTile = kBlock * kSgbRows;
constexpr unsigned long long kSgbAgg = 1ull << 62, kSgbPrefix = 2ull << 62,
                             kSgbMask = (1ull << 62) - 1ull;

// smallest / largest key of a column (int64 columns take the sort path when their keys span
// less than 2^32): out2 = {min, max}, initialised by the caller to {INT64_MAX, INT64_MIN}
template <typename K>
__global__ __launch_bounds__(kBlock) void key_minmax_kernel(const K *__restrict__ keys, uint64_t n,
                                                            long long *out2) {
  long long mn = INT64_MAX, mx = INT64_MIN;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const long long k = (long long)keys[i];
    mn = k < mn ? k : mn;
    mx = k > mx ? k : mx;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane_id() == 0) {
    atomicMin(&out2[0], mn);
    atomicMax(&out2[1], mx);
  }
}

// MERGE (owner-side merge of (key, count) rows, nvt_count_merge_sorted): the words are
// (column << (rb + 32) | key image << rb | row), a group is a (column, key) pair; out_keys
// receives the group's COLUMN, out_keys32 its key, the rewritten words carry slot = group.
template <bool MERGE>
__global__ __launch_bounds__(kBlock) void sgb_rle_kernel(
    const uint64_t *__restrict__ in, uint64_t n, int rb, unsigned kfold, uint64_t cap,
    unsigned long long *status, unsigned *ticket, int64_t *__restrict__ out_keys,
    int32_t *__restrict__ out_keys32, uint64_t *__restrict__ out_words, uint64_t *state,
    int64_t bias) {
  constexpr int NW = kBlock / kWave;
  __shared__ unsigned wtot[NW];
  __shared__ unsigned long long s_base;
  __shared__ unsigned s_tile;
  if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u);
  __syncthreads();
  const unsigned tile = s_tile, w = threadIdx.x / kWave, l = lane_id();
  const uint64_t wave0 = (uint64_t)tile * kSgbTile + (uint64_t)w * (kSgbRows * kWave);
  uint64_t W[kSgbRows];
  unsigned long long hb[kSgbRows];  // ballot of the run heads of every 64-word row
  // group field (key image; MERGE: column + key image) in front of this wave's run (one
  // address: a broadcast load)
  const int fsh = MERGE ? rb : 32;
  uint64_t prev_hi = (wave0 > 0 && wave0 < n) ? in[wave0 - 1] >> fsh : 0ull;
  unsigned wheads = 0;
#pragma unroll
  for (int r = 0; r < kSgbRows; ++r) {
    const uint64_t i = wave0 + (uint64_t)r * kWave + l;
    const bool act = i < n;
    W[r] = act ? in[i] : ~0ull;
    const uint64_t hi = W[r] >> fsh;
    uint64_t up = __shfl_up(hi, 1, 64);
    if (l == 0) up = prev_hi;
    const bool head = act && (i == 0 || hi != up);
    hb[r] = __ballot(head);
    prev_hi = __shfl(hi, 63, 64);
    wheads += (unsigned)__popcll(hb[r]);
  }
  if (l == 0) wtot[w] = wheads;
  __syncthreads();
  unsigned wbase = 0, ttot = 0;
  for (int q = 0; q < NW; ++q) {
    if (q < (int)w) wbase += wtot[q];
    ttot += wtot[q];
  }
  if (threadIdx.x == 0) {
    unsigned long long *my = status + tile;
    __hip_atomic_store(my, (tile == 0 ? kSgbPrefix : kSgbAgg) | (unsigned long long)ttot,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long carry = 0;
    if (tile > 0) {
      unsigned tb = tile - 1;
      while (true) {
        const unsigned long long v =
            __hip_atomic_load(status + tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned f = (unsigned)(v >> 62);
        if (f == 0) {
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        carry += v & kSgbMask;
        if (f == 2) break;
        --tb;
      }
      __hip_atomic_store(my, kSgbPrefix | (carry + ttot), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    s_base = carry;
    if ((uint64_t)(tile + 1) * kSgbTile >= n) {  // the tile that holds the last row
      const unsigned long long g = carry + ttot;
      state[NVT_ST_OCCUPIED] = g;
      state[NVT_ST_ROWS] = n;
      if (g > cap) state[NVT_ST_NEED] = g;
    }
  }
  __syncthreads();
  uint64_t g0 = s_base + wbase;  // run heads in front of this wave's rows
  const uint64_t rowmask = rb >= 32 ? 0xFFFFFFFFull : ((1ull << rb) - 1ull);
#pragma unroll
  for (int r = 0; r < kSgbRows; ++r) {
    const uint64_t i = wave0 + (uint64_t)r * kWave + l;
    const unsigned incl = (unsigned)__popcll(hb[r] & ((2ull << l) - 1ull));
    if (i < n) {
      const uint64_t g = g0 + incl - 1;  // >= 0: row 0 is a head
      const bool fits = g < cap;
      if constexpr (MERGE) {
        if (((hb[r] >> l) & 1ull) && fits) {
          out_keys[g] = (int64_t)(W[r] >> (rb + 32));                             // column
          out_keys32[g] = (int32_t)((uint32_t)(W[r] >> rb) ^ 0x80000000u);        // key
        }
        out_words[i] = ((fits ? g : 0xFFFFFFFFull) << 32) | (W[r] & rowmask);
      } else {
        const uint32_t hi = (uint32_t)(W[r] >> 32);
        if (((hb[r] >> l) & 1ull) && fits) {
          out_keys[g] = (int64_t)((uint64_t)hi + (uint64_t)bias);  // the key itself
          out_keys32[g] = (int32_t)(hi ^ 0x80000000u);              // key - bias - 2^31: the flat index's key
        }
        const uint64_t low = W[r] & 0xFFFFFFFFull;
        const uint64_t fold = (rb >= 32 || kfold == 1) ? 0ull : (low >> rb);
        const uint64_t slot = fits ? g * kfold + fold : 0xFFFFFFFFull;
        out_words[i] = (slot << 32) | (low & rowmask);
      }
    }
    g0 += (unsigned)__popcll(hb[r]);
  }
}

__global__ __launch_bounds__(kBlock) void sgb_fill_kernel(double *__restrict__ p, uint64_t n,
                                                          double v) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) p[i] = v;
}

// per-key totals over the folds (+ the one-probe records of the transform).  A workgroup takes
// kBlock consecutive groups: their kfold-entry runs of fsize / fsum are contiguous and are read
// coalesced, the records (2 * (kfold + 1) doubles per group) are assembled in LDS and leave as
// one contiguous block (a thread per group wrote 12 scattered 8-byte words: 462 us for 5 M groups).
constexpr int kSgbMaxFoldLds = 16;
__global__ __launch_bounds__(kBlock) void sgb_fold_total_kernel(
    const uint64_t *__restrict__ state, unsigned kfold, uint64_t cap, int nvals,
    const unsigned long long *__restrict__ fsize, const double *__restrict__ fsum,
    unsigned long long *__restrict__ tsize, double *__restrict__ tsum,
    double *__restrict__ records) {
  // (sized by the launch for THIS kfold: the 16-fold maximum as a static array held 70 KB, two
  // workgroups per CU; 25 KB for five folds lets six of them hide each other's loads)
  extern __shared__ double lrec[];  // [kBlock][2 * (kfold + 1)]
  uint64_t ng = state[NVT_ST_OCCUPIED];
  ng = ng < cap ? ng : cap;
  const unsigned rs = 2 * (kfold + 1);
  const uint64_t nblocks = (ng + kBlock - 1) / kBlock;
  for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const uint64_t g0 = b * kBlock;
    const unsigned cnt = (unsigned)((ng - g0) < (uint64_t)kBlock ? (ng - g0) : (uint64_t)kBlock);
    for (int j = 0; j < (nvals > 0 ? nvals : 1); ++j) {
      // stage {sum_f, count_f} of the block's groups: element e = (group, fold) in memory order
      for (unsigned e = threadIdx.x; e < cnt * kfold; e += kBlock) {
        const unsigned g = e / kfold, f = e - g * kfold;
        lrec[g * rs + 3 + 2 * f] = (double)fsize[g0 * kfold + e];
        if (nvals) lrec[g * rs + 2 + 2 * f] = fsum[(uint64_t)j * cap * kfold + g0 * kfold + e];
      }
      __syncthreads();
      if (threadIdx.x < cnt) {
        const unsigned g = threadIdx.x;
        double d = 0.0, c = 0.0;
        for (unsigned f = 0; f < kfold; ++f) {
          if (nvals) d += lrec[g * rs + 2 + 2 * f];
          c += lrec[g * rs + 3 + 2 * f];
        }
        lrec[g * rs] = d;
        lrec[g * rs + 1] = c;
        if (j == 0) tsize[g0 + g] = (unsigned long long)c;  // counts < 2^53: exact
        if (nvals) tsum[(uint64_t)j * cap + g0 + g] = d;
      }
      __syncthreads();
      if (records && nvals) {
        double *dst = records + ((uint64_t)j * cap + g0) * rs;
        for (unsigned e = threadIdx.x; e < cnt * rs; e += kBlock) dst[e] = lrec[e];
      }
      __syncthreads();
    }
  }
}

// owner-side merge of the (key, count) rows a rank receives in the multi-GPU exchange
// (categorify.py:1054-1070 _mid_level_groupby on the owner): rows = (count << 32 | key) words in
// `nseg` segments (source-major, column-minor: segment s belongs to column s % ncol).  The rows
// are tagged with their column and sorted by (column, key): equal keys of a column become one
// run whose counts are summed by the segmented reduction -- the merged lists come out ordered
// by key (what the vocabulary ordering wants) without a hash table and without a second sort.
constexpr int kMergeRowBits = 26;  // rows per call < 2^26; 32 key bits; 6 column bits
__global__ __launch_bounds__(kBlock) void merge_pack_kernel(const int64_t *__restrict__ rows,
                                                            uint64_t n,
                                                            const uint64_t *__restrict__ seg_off,
                                                            int nseg, int ncol,
                                                            uint64_t *__restrict__ words,
                                                            int32_t *__restrict__ cnt32) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    int lo = 0, hi = nseg;  // the segment with seg_off[s] <= i < seg_off[s + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    const uint64_t col = (uint64_t)(lo % ncol);
    const uint64_t w = (uint64_t)rows[i];
    const uint64_t img = (uint32_t)w ^ 0x80000000u;
    words[i] = (col << (kMergeRowBits + 32)) | (img << kMergeRowBits) | i;
    cnt32[i] = (int32_t)(w >> 32);
  }
}

// the look-back of sgb_rle_kernel over n words: a status word per tile and, behind them, the
// tile ticket; `bytes` of it are zero before the launch.  (Addresses are computed as integers:
// the _ws_bytes functions lay the workspace out from a null base.)
struct SgbStatus {
  uint64_t ntiles, bytes;
  unsigned long long *status;
  unsigned *ticket;
  SgbStatus(void *base, uint64_t n)
      : ntiles((n + kSgbTile - 1) / kSgbTile),
        bytes(ntiles * 8 + 64),
        status(reinterpret_cast<unsigned long long *>(base)),
        ticket(reinterpret_cast<unsigned *>(reinterpret_cast<uintptr_t>(base) + ntiles * 8)) {}
};

// nvt_count_merge_sorted: words[n] | sort scratch | cnt32[n] | regrouped[n] | status + ticket
struct MergeWs {
  uint64_t *words;
  void *sort_tmp;
  int32_t *cnt32;
  uint64_t *regrouped;
  void *status;
  uint64_t bytes;
  MergeWs(void *base, uint64_t n) {
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    auto take = [&](uint64_t b) {
      void *r = reinterpret_cast<void *>(p);
      p += pad256(b);
      return r;
    };
    words = reinterpret_cast<uint64_t *>(take(n * 8));
    sort_tmp = take(sort_words_tmp_bytes(n));
    cnt32 = reinterpret_cast<int32_t *>(take(n * 4));
    regrouped = reinterpret_cast<uint64_t *>(take(n * 8));
    status = take(SgbStatus(nullptr, n).bytes);
    bytes = (uint64_t)(p - reinterpret_cast<uintptr_t>(base)) + 512;
  }
};

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_sgb_sort_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  *bytes = pad256(n * 8) + pad256(sort_words_tmp_bytes(n)) + 512;
  return NVT_OK;
}

int nvt_key_minmax(const void *keys, int key_dtype, uint64_t n, int64_t *out2, void *stream) {
  NVT_CHECK_ARG(keys && out2, "null pointer");
  NVT_CHECK_ARG(key_dtype == NVT_I32 || key_dtype == NVT_I64, "key dtype must be int32 / int64");
  hipStream_t s = (hipStream_t)stream;
  const int64_t init[2] = {INT64_MAX, INT64_MIN};
  NVT_CHECK_HIP(hipMemcpyAsync(out2, init, sizeof(init), hipMemcpyHostToDevice, s));
  if (n == 0) return NVT_OK;
  NVT_PROF("groupby_sort", n * (key_dtype == NVT_I64 ? 8ull : 4ull), s);
  const unsigned grid = stream_grid(n, kBlock * 8);
  if (key_dtype == NVT_I32)
    key_minmax_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)keys, n, (long long *)out2);
  else
    key_minmax_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)keys, n, (long long *)out2);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_sgb_sort(const void *keys, int key_dtype, int64_t key_bias, const uint8_t *fold, int kfold,
                 uint64_t n, void *ws, uint64_t **sorted_out, int *row_bits_out, void *stream) {
  NVT_CHECK_ARG(keys && ws && sorted_out && row_bits_out, "null pointer");
  NVT_CHECK_ARG(key_dtype == NVT_I32 || key_dtype == NVT_I64, "key dtype must be int32 / int64");
  NVT_CHECK_ARG(kfold >= 1 && kfold <= 256, "kfold must be 1..256");
  NVT_CHECK_ARG((kfold > 1) == (fold != nullptr), "fold ids come with kfold > 1");
  int fb = 0;
  while ((1 << fb) < kfold) ++fb;
  const int rb = 32 - fb;
  NVT_CHECK_ARG(n >= 1 && n < (1ull << 30) && n <= (1ull << rb), "row index does not fit next to the fold");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_sort", n * (key_dtype == NVT_I64 ? 8ull : 4ull), s);
  // (the unsorted words are never written out: the histogram and the first scatter pass pack them
  // from the column -- sgb_pack_kernel's 8 bytes per row written + read twice are gone)
  void *sort_tmp = reinterpret_cast<char *>(ws) + pad256(n * 8);
  uint64_t *sorted = nullptr;
  int rc = sort_packed_keys(keys, key_dtype, key_bias, fold, rb, n, sort_tmp, &sorted, s);
  if (rc) return rc;
  *sorted_out = sorted;
  *row_bits_out = rb;
  return NVT_OK;
}

int nvt_sgb_regroup_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  *bytes = pad256(SgbStatus(nullptr, n).bytes) + 256;
  return NVT_OK;
}

int nvt_sgb_regroup(const uint64_t *sorted, int row_bits, int kfold, int64_t key_bias, uint64_t n,
                    uint64_t cap, int64_t *out_keys, int32_t *out_keys32, uint64_t *regrouped,
                    uint64_t *state, void *ws, void *stream) {
  NVT_CHECK_ARG(sorted && out_keys && out_keys32 && regrouped && state && ws, "null pointer");
  NVT_CHECK_ARG(regrouped != sorted, "regrouped must not alias the sorted words");
  NVT_CHECK_ARG(kfold >= 1 && kfold <= 256, "kfold must be 1..256");
  NVT_CHECK_ARG(row_bits >= 24 && row_bits <= 32, "row_bits must be 24..32");
  NVT_CHECK_ARG(kfold == 1 || (1 << (32 - row_bits)) >= kfold, "the sorted words carry fewer fold bits");
  NVT_CHECK_ARG(n >= 1 && n < (1ull << 30), "1 .. 2^30-1 rows");
  NVT_CHECK_ARG(cap >= 1 && cap * (uint64_t)kfold < 0xFFFFFFFFull, "capacity * kfold must be < 2^32 - 1");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_sorted", n * 4ull, s);
  const SgbStatus st(ws, n);
  NVT_CHECK_HIP(hipMemsetAsync(st.status, 0, st.bytes, s));
  NVT_CHECK_HIP(hipMemsetAsync(state, 0, NVT_STATE_WORDS * 8, s));
  sgb_rle_kernel<false><<<(unsigned)st.ntiles, kBlock, 0, s>>>(sorted, n, row_bits, (unsigned)kfold,
                                                               cap, st.status, st.ticket, out_keys,
                                                               out_keys32, regrouped, state, key_bias);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_sgb_reduce(const uint64_t *regrouped, int words_kfold, int kfold, const void *const *vals,
                   const int *vdtypes, const uint8_t *const *val_valid, int nvals, int flags,
                   uint64_t n, uint64_t cap, uint64_t *out_size, double *out_sum, double *out_sumsq,
                   double *out_min, double *out_max, uint64_t *tot_size, double *tot_sum,
                   double *te_records, const uint64_t *state, const void *const *sorted_in,
                   void *const *sorted_out, void *stream) {
  NVT_CHECK_ARG(regrouped && out_size && state, "null pointer");
  NVT_CHECK_ARG(nvals >= 0 && nvals <= kMaxVals, "nvals must be 0..8");
  NVT_CHECK_ARG(nvals == 0 || (vals && vdtypes && out_sum), "null vals / out_sum");
  NVT_CHECK_ARG(words_kfold >= 1 && words_kfold <= 256, "words_kfold must be 1..256");
  NVT_CHECK_ARG(kfold == words_kfold || kfold == 1, "kfold must be 1 or the words' kfold");
  NVT_CHECK_ARG(kfold == 1 || kfold <= kSgbMaxFoldLds, "at most 16 folds");
  NVT_CHECK_ARG(kfold == 1 || (tot_size && (nvals == 0 || tot_sum)), "null totals");
  NVT_CHECK_ARG(te_records == nullptr || (kfold > 1 && nvals > 0), "records come with folds and values");
  NVT_CHECK_ARG(((flags & NVT_GB_SUMSQ) != 0) == (out_sumsq != nullptr) || nvals == 0, "sumsq flag / array");
  NVT_CHECK_ARG(((flags & NVT_GB_MINMAX) != 0) == (out_min != nullptr && out_max != nullptr) || nvals == 0,
                "min/max flag / arrays");
  NVT_CHECK_ARG(n >= 1 && n < (1ull << 30), "1 .. 2^30-1 rows");
  NVT_CHECK_ARG(cap >= 1 && cap * (uint64_t)kfold < 0xFFFFFFFFull, "capacity * kfold must be < 2^32 - 1");
  GbRowArgs a;
  int rc = row_args(a, __func__, 0, nullptr, nullptr, nvals, vals, vdtypes, val_valid, sorted_in,
                    sorted_out);
  if (rc) return rc;
  for (int j = 0; j < nvals; ++j) {
    NVT_CHECK_ARG(!(a.sorted_in[j] && a.val_valid[j]), "sorted values come without a validity bitmap");
    NVT_CHECK_ARG(vdtypes[j] != NVT_I64 || (!a.sorted_in[j] && !a.sorted_out[j]),
                  "int64 values are not carried in sorted order (not exact in a double)");
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("groupby_sorted", n * 4ull, s);
  const uint64_t slots = cap * (uint64_t)kfold;
  NVT_CHECK_HIP(hipMemsetAsync(out_size, 0, slots * 8, s));
  if (nvals) NVT_CHECK_HIP(hipMemsetAsync(out_sum, 0, slots * 8 * nvals, s));
  if (nvals && out_sumsq) NVT_CHECK_HIP(hipMemsetAsync(out_sumsq, 0, slots * 8 * nvals, s));
  if (nvals && out_min) {
    const double inf = std::numeric_limits<double>::infinity();
    sgb_fill_kernel<<<stream_grid(slots * nvals, kBlock * 4), kBlock, 0, s>>>(out_min, slots * nvals, inf);
    sgb_fill_kernel<<<stream_grid(slots * nvals, kBlock * 4), kBlock, 0, s>>>(out_max, slots * nvals, -inf);
    NVT_CHECK_LAUNCH();
  }
  const GbView t = dense_view(slots, nvals, out_size, nullptr, nullptr, out_sum,
                              nvals ? out_sumsq : nullptr, nvals ? out_min : nullptr,
                              nvals ? out_max : nullptr);
  const uint32_t div = kfold == words_kfold ? 1u : (uint32_t)words_kfold;
  segreduce_launch(t, a, n, regrouped, div, true, s);
  NVT_CHECK_LAUNCH();
  if (kfold > 1) {
    const size_t lds = (size_t)kBlock * 2 * ((size_t)kfold + 1) * sizeof(double);
    if (lds > 48 * 1024)  // (13-16 folds: beyond the default dynamic limit)
      NVT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sgb_fold_total_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    sgb_fold_total_kernel<<<stream_grid(cap, kBlock, 8), kBlock, lds, s>>>(
        state, (unsigned)kfold, cap, nvals, reinterpret_cast<const unsigned long long *>(out_size),
        out_sum, reinterpret_cast<unsigned long long *>(tot_size), tot_sum, te_records);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_count_merge_sorted_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  *bytes = MergeWs(nullptr, n).bytes;
  return NVT_OK;
}

int nvt_count_merge_sorted(const int64_t *rows, uint64_t n, const uint64_t *seg_off, int nseg,
                           int ncol, int32_t *out_keys, int64_t *out_col, double *out_sum,
                           uint64_t *state, void *ws, void *stream) {
  NVT_CHECK_ARG(rows && seg_off && out_keys && out_col && out_sum && state && ws, "null pointer");
  NVT_CHECK_ARG(n >= 1 && n < (1ull << kMergeRowBits), "1 .. 2^26-1 rows per call");
  NVT_CHECK_ARG(nseg >= 1 && ncol >= 1 && ncol <= (1 << (64 - 32 - kMergeRowBits)) && nseg % ncol == 0,
                "1..64 columns, whole groups of segments");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("count_merge_sorted", n * 8ull, s);
  const MergeWs w(ws, n);
  const SgbStatus st(w.status, n);
  NVT_CHECK_HIP(hipMemsetAsync(st.status, 0, st.bytes, s));
  NVT_CHECK_HIP(hipMemsetAsync(state, 0, NVT_STATE_WORDS * 8, s));
  NVT_CHECK_HIP(hipMemsetAsync(out_sum, 0, n * 8, s));
  merge_pack_kernel<<<stream_grid(n, kBlock * 4), kBlock, 0, s>>>(rows, n, seg_off, nseg, ncol, w.words,
                                                                  w.cnt32);
  NVT_CHECK_LAUNCH();
  int cb = 1;
  while ((1 << cb) < ncol) ++cb;
  uint64_t *sorted = nullptr;
  int rc = sort_words_bits(w.words, n, kMergeRowBits, kMergeRowBits + 32 + cb, w.sort_tmp, &sorted, s);
  if (rc) return rc;
  sgb_rle_kernel<true><<<(unsigned)st.ntiles, kBlock, 0, s>>>(sorted, n, kMergeRowBits, 1u, n,
                                                              st.status, st.ticket, out_col, out_keys,
                                                              w.regrouped, state, 0);
  NVT_CHECK_LAUNCH();
  const GbView t = dense_view(n, 1, nullptr, nullptr, nullptr, out_sum, nullptr, nullptr, nullptr);
  GbRowArgs a;
  memset(&a, 0, sizeof(a));
  a.vals[0] = w.cnt32;
  a.vdtype[0] = NVT_I32;
  segreduce_launch(t, a, n, w.regrouped, 1u, true, s);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
