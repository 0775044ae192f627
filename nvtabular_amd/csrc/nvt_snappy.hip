// Snappy pages of the PLAIN parquet writer: the values regions of a row group's column chunks become
// snappy ELEMENT streams (literals and copies; the varint in front of a page body is the host's).
//
// Element streams made independently for consecutive pieces of the input may be concatenated as long
// as no copy reaches back past the start of its own piece.  So a values region is cut into FRAGMENTS
// of at most kFrag = 32 KiB that never straddle a page, every fragment is parsed by ONE wave into a
// slot of its own, and the streams of a page's fragments, moved together, are the page's elements.
//   1. plan_kernel (one workgroup per column): the page starts become fragment records {source byte
//      offset, length, page, column} in the batch's fragment table.  The host sizes the table from
//      the bound ceil(bytes / kFrag) + pages per column; a page table that would need more sets the
//      column's error word.
//   2. compress_kernel (one wave per fragment): a hash table of 4096 positions in LDS.  The wave looks
//      at a window of 64 consecutive positions; lane k hashes the 4 bytes at cursor + k and has two
//      candidates: the position one element size back (4 or 8 bytes -- matches nearer than the
//      window are invisible to the table) and the table entry, which holds only positions in front
//      of the window.  The lowest lane whose candidate really holds the same 4 bytes wins; the wave
//      extends the match 64 bytes at a time, emits the pending literal and the copy (pieces of at
//      most 64 bytes, 2-byte offsets), inserts the window positions up to the winner (LDS atomicMax
//      on position + 1: two lanes on one slot leave the same entry whatever their order) and goes on
//      behind the match.  No hit: all 64 positions are inserted and the cursor advances by 64.
//      Every iteration advances the cursor by at least 4 bytes and every loop is bounded by the
//      fragment length; no load touches a word that holds no byte of the fragment; before each
//      emit the room left in the slot is checked, and a slot that would overflow sets the column's
//      error word and ends the fragment with nothing reported.  A wave never waits for another.
//   3. gather: a 64-bit exclusive scan of the fragment sizes (tile scan, scan_totals_kernel of
//      nvt_scan.hpp, add: three launches, no look-back), then gather_kernel moves every fragment's
//      stream to its place in the column's dense buffer: the shift is byte-granular, the loads and
//      the stores inside a stream are aligned words (v_alignbyte_b32), the first and the last word
//      of a stream, which it shares with its neighbours, are stored byte by byte.
// The compressed bytes of a page are summed with integer atomics (the same whatever the order).
#include "nvt_common.hpp"
#include "nvt_list_tile.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr uint32_t kFrag = NVT_SNAPPY_FRAG;
constexpr int kMaxCols = NVT_SNAPPY_MAX_COLS;
constexpr int kHashBits = 12;
constexpr int kRec = NVT_SNAPPY_FRAG_WORDS;   // words of a fragment record
constexpr uint64_t kScanTile = kListTile;     // fragment sizes per tile of the scan (256 lanes x 8)

struct SCol {
  const uint8_t *src;
  const int64_t *page_start;
  uint64_t npages, nbytes, frag_base, max_frags, dense_cap;
  uint8_t *dense;
  unsigned long long *out;
  uint32_t unit, elem;
};
struct SBatch {
  SCol c[kMaxCols];
  int ncols, col0;   // (col0: the index of c[0] among the call's descriptors, as the records name it)
};

__host__ __device__ inline uint64_t frags_bound(uint64_t nbytes, uint64_t npages) {
  return (nbytes + kFrag - 1) / kFrag + npages;
}

// ---- plan ----------------------------------------------------------------------------------------
// byte position of page start x: x * unit clamped to [0, nbytes]
__device__ __forceinline__ uint64_t page_byte(int64_t x, uint32_t unit, uint64_t nbytes) {
  if (x <= 0) return 0;
  return (uint64_t)x > nbytes / unit ? nbytes : (uint64_t)x * unit;
}

__global__ __launch_bounds__(kBlock) void plan_kernel(SBatch b, uint64_t *__restrict__ table) {
  __shared__ uint64_t wsum[kBlock / kWave];
  const SCol &c = b.c[blockIdx.x];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  for (uint64_t i = threadIdx.x; i < c.npages + NVT_SNAPPY_OUT_WORDS; i += kBlock) c.out[i] = 0;
  uint64_t carry = 0;   // fragments of the pages in front of this round's (the same in every lane)
  for (uint64_t p0 = 0; p0 < c.npages; p0 += kBlock) {
    const uint64_t p = p0 + threadIdx.x;
    uint64_t lo = 0, hi = 0;
    if (p < c.npages) {
      lo = page_byte(c.page_start[p], c.unit, c.nbytes);
      hi = page_byte(c.page_start[p + 1], c.unit, c.nbytes);
      if (hi < lo) hi = lo;
    }
    const uint64_t nf = (hi - lo + kFrag - 1) / kFrag;
    const uint64_t inc = wave_incl_scan(nf);
    __syncthreads();   // (wsum of the round before has been read)
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t first = carry + inc - nf, all = 0;
    for (unsigned k = 0; k < kBlock / kWave; ++k) {
      if (k < w) first += wsum[k];
      all += wsum[k];
    }
    for (uint64_t k = 0; k < nf; ++k) {
      const uint64_t f = first + k;
      if (f >= c.max_frags) break;   // (never written outside the column's records)
      uint64_t *rec = table + (c.frag_base + f) * kRec;
      const uint64_t at = lo + k * kFrag;
      rec[0] = at;
      rec[1] = hi - at < kFrag ? hi - at : kFrag;
      rec[2] = p;
      rec[3] = (uint64_t)(b.col0 + (int)blockIdx.x);
    }
    carry += all;
  }
  __syncthreads();   // (behind the clearing of `out`)
  if (threadIdx.x == 0) {
    c.out[c.npages + NVT_SNAPPY_OUT_FRAGS] = carry < c.max_frags ? carry : c.max_frags;
    if (carry > c.max_frags) c.out[c.npages + NVT_SNAPPY_OUT_ERROR] = NVT_SNAPPY_ERR_PLAN;
  }
}

// ---- compress ------------------------------------------------------------------------------------
// the 4 bytes at s + p, from the aligned words that hold them (all of them bytes of the fragment)
__device__ __forceinline__ uint32_t load4(const uint8_t *s, uint32_t p) {
  const uint8_t *a = s + p;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
  const uint32_t *w = reinterpret_cast<const uint32_t *>(a - sh);
  const uint32_t lo = w[0];
  const uint32_t hi = sh ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

__device__ __forceinline__ uint32_t hash4(uint32_t w) { return (w * 0x1E35A7BDu) >> (32 - kHashBits); }

// bytes of a literal element of n bytes (n <= 65536)
__device__ __forceinline__ uint32_t literal_bytes(uint32_t n) {
  return n == 0 ? 0 : n + (n <= 60 ? 1 : (n <= 256 ? 2 : 3));
}

// the literal element of s[0, n) at o (the caller has checked the room); -> its bytes
__device__ __forceinline__ uint32_t emit_literal(uint8_t *o, const uint8_t *s, uint32_t n, unsigned lane) {
  if (n == 0) return 0;
  const uint32_t tag = n <= 60 ? 1 : (n <= 256 ? 2 : 3);
  if (lane == 0) {
    if (tag == 1) {
      o[0] = (uint8_t)((n - 1) << 2);
    } else if (tag == 2) {
      o[0] = (uint8_t)(60 << 2);
      o[1] = (uint8_t)(n - 1);
    } else {
      o[0] = (uint8_t)(61 << 2);
      o[1] = (uint8_t)((n - 1) & 0xFF);
      o[2] = (uint8_t)((n - 1) >> 8);
    }
  }
  for (uint32_t i = lane; i < n; i += kWave) o[tag + i] = s[i];
  return tag + n;
}

__global__ __launch_bounds__(kWave) void compress_kernel(SBatch b, const uint64_t *__restrict__ table,
                                                         unsigned long long *__restrict__ frag_size,
                                                         uint8_t *__restrict__ slots, uint64_t slot_cap,
                                                         uint64_t e0, uint64_t e1) {
  __shared__ uint32_t tab[1 << kHashBits];   // position + 1 of the last place a hash was seen; 0: none
  const unsigned lane = threadIdx.x;
  for (uint64_t e = e0 + blockIdx.x; e < e1; e += gridDim.x) {
    const uint64_t *rec = table + e * kRec;
    const uint64_t at = rec[0], len = rec[1], page = rec[2], col = rec[3] - (uint64_t)b.col0;
    if (len == 0 || len > kFrag || col >= (uint64_t)b.ncols) continue;   // (an unused record)
    const SCol &c = b.c[col];
    if (at > c.nbytes || c.nbytes - at < len || page >= c.npages) continue;
    const uint32_t L = (uint32_t)len, elem = c.elem;
    const uint8_t *s = c.src + at;
    uint8_t *o = slots + e * slot_cap;
    __syncthreads();   // (the fragment before is done with the table)
    for (uint32_t i = lane; i < (1u << kHashBits); i += kWave) tab[i] = 0;
    __syncthreads();
    uint32_t cur = 0, lit0 = 0;
    uint64_t out = 0;
    bool fail = false;
    // every pass moves the cursor by 64 or behind a match of 4 bytes or more: at most L / 4 + 1 passes
    for (uint32_t pass = 0; pass <= L / 4 && cur + 4 <= L; ++pass) {
      const uint32_t p = cur + lane;
      const bool ok = p + 4 <= L;
      uint32_t h = 0;
      int cand = -1;
      if (ok) {
        const uint32_t w = load4(s, p);
        h = hash4(w);
        if (p >= elem && load4(s, p - elem) == w) {
          cand = (int)(p - elem);
        } else {
          const uint32_t t = tab[h];
          if (t && load4(s, t - 1) == w) cand = (int)(t - 1);
        }
      }
      const unsigned long long hits = __ballot(cand >= 0);
      if (!hits) {
        if (ok) atomicMax(&tab[h], p + 1);
        __syncthreads();
        cur += kWave;
        continue;
      }
      const int k = __builtin_ctzll(hits);
      const uint32_t mp = cur + (uint32_t)k, mq = (uint32_t)__shfl(cand, k, kWave);
      if (ok && (int)lane <= k) atomicMax(&tab[h], p + 1);
      uint32_t m = 4;
      for (uint32_t g = 0; g <= L / kWave; ++g) {   // (mp + m reaches L after at most L / 64 + 1 rounds)
        const uint32_t i = m + lane;
        const bool eq = mp + i < L && s[mp + i] == s[mq + i];
        const unsigned long long ne = __ballot(!eq);
        if (ne) {
          m += (uint32_t)__builtin_ctzll(ne);
          break;
        }
        m += kWave;
      }
      const uint32_t n = mp - lit0, pieces = (m + 63) / 64, off = mp - mq;
      if (out + literal_bytes(n) + 3ull * pieces > slot_cap) {
        fail = true;
        break;
      }
      out += emit_literal(o + out, s + lit0, n, lane);
      for (uint32_t j = lane; j < pieces; j += kWave) {   // copies with a 2-byte offset, 1 .. 64 bytes each
        const uint32_t piece = m - 64 * j < 64 ? m - 64 * j : 64;
        uint8_t *q = o + out + 3 * j;
        q[0] = (uint8_t)(((piece - 1) << 2) | 2);
        q[1] = (uint8_t)(off & 0xFF);
        q[2] = (uint8_t)(off >> 8);
      }
      out += 3ull * pieces;
      cur = mp + m;
      lit0 = cur;
      __syncthreads();
    }
    if (!fail) {
      const uint32_t n = L - lit0;
      if (out + literal_bytes(n) > slot_cap) fail = true;
      else out += emit_literal(o + out, s + lit0, n, lane);
    }
    if (lane == 0) {
      if (fail) {
        c.out[c.npages + NVT_SNAPPY_OUT_ERROR] = NVT_SNAPPY_ERR_SLOT;
      } else {
        frag_size[e] = out;
        atomicAdd(&c.out[page], (unsigned long long)out);
        atomicAdd(&c.out[c.npages + NVT_SNAPPY_OUT_TOTAL], (unsigned long long)out);
      }
    }
  }
}

// ---- gather --------------------------------------------------------------------------------------
// pos[i] for i in [0, n]: tile-local exclusive prefix of size[0, n); tile_tot[t] the tile's total
__global__ __launch_bounds__(kBlock) void scan_tile_kernel(const unsigned long long *__restrict__ size, uint64_t n,
                                                           unsigned long long *__restrict__ pos,
                                                           unsigned long long *__restrict__ tile_tot) {
  __shared__ uint64_t wsum[kBlock / kWave];
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  const uint64_t nt = list_ntiles(n + 1);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t j0 = t * kScanTile + (uint64_t)threadIdx.x * 8;
    uint64_t v[8], tot = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      v[q] = j0 + q < n ? size[j0 + q] : 0;
      tot += v[q];
    }
    const uint64_t inc = wave_incl_scan(tot);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t run = inc - tot;
    for (unsigned k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (j0 + q <= n) pos[j0 + q] = run;
      run += v[q];
    }
    if (threadIdx.x == kBlock - 1) tile_tot[t] = run;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void scan_add_tiles_kernel(unsigned long long *__restrict__ pos, uint64_t n,
                                                                const unsigned long long *__restrict__ tile_base) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * kBlock)
    pos[j] += tile_base[j / kScanTile];
}

__global__ __launch_bounds__(kBlock) void gather_kernel(SBatch b, const uint64_t *__restrict__ table,
                                                        const unsigned long long *__restrict__ frag_size,
                                                        const unsigned long long *__restrict__ frag_pos,
                                                        const uint8_t *__restrict__ slots, uint64_t slot_cap,
                                                        uint64_t e0, uint64_t e1) {
  for (uint64_t e = e0 + blockIdx.x; e < e1; e += gridDim.x) {
    const uint64_t n = frag_size[e], col = table[e * kRec + 3] - (uint64_t)b.col0;
    if (n == 0 || n > slot_cap || col >= (uint64_t)b.ncols) continue;
    const SCol &c = b.c[col];
    if (e < c.frag_base || e >= c.frag_base + c.max_frags) continue;
    const uint64_t d0 = frag_pos[e] - frag_pos[c.frag_base];
    const uint64_t total = frag_pos[c.frag_base + c.max_frags] - frag_pos[c.frag_base];
    // a column whose streams do not fit its dense buffer is left out as a whole (the host sees the total)
    if (total > c.dense_cap || d0 > total || total - d0 < n) continue;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(slots + e * slot_cap);   // (4-byte aligned)
    const int64_t nwords = (int64_t)((n + 3) >> 2);   // words of the slot that hold a byte of the stream
    uint8_t *dst = c.dense + d0;
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t end = d + n;
    for (uintptr_t a = (d & ~(uintptr_t)3) + 4 * (uintptr_t)threadIdx.x; a < end; a += 4 * kBlock) {
      const int64_t r = (int64_t)a - (int64_t)d;   // stream bytes [r, r + 4) fall into this word (r >= -3)
      const int64_t qi = r >> 2;
      const uint32_t lo = (qi >= 0 && qi < nwords) ? w[qi] : 0u;
      const uint32_t hi = (qi + 1 >= 0 && qi + 1 < nwords) ? w[qi + 1] : 0u;
      const uint32_t val = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(r & 3));
      uint8_t *q = reinterpret_cast<uint8_t *>(a);
      if (r >= 0 && r + 4 <= (int64_t)n) {
        *reinterpret_cast<uint32_t *>(q) = val;
        continue;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (r + i >= 0 && r + i < (int64_t)n) q[i] = (uint8_t)(val >> (8 * i));
    }
  }
}

inline uint64_t scan_ws_bytes(uint64_t total_frags) { return pad16(list_ntiles(total_frags + 1) * 8) + 16; }

// Argument rules shared by the three entries; nothing is launched when one is broken.
int check_args(const char *who, const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch) {
#define SNAPPY_ARG(cond, msg)              \
  do {                                     \
    if (!(cond)) {                         \
      nvt::set_error("%s: %s", who, msg);  \
      return NVT_EINVAL;                   \
    }                                      \
  } while (0)
  SNAPPY_ARG(cols && batch, "null descriptors");
  SNAPPY_ARG(ncols > 0, "ncols must be positive");
  SNAPPY_ARG(batch->frag_table && batch->frag_size && batch->frag_pos && batch->slots && batch->ws, "null pointer");
  SNAPPY_ARG(batch->total_frags > 0 && batch->total_frags < (1ull << 40), "total_frags out of range");
  SNAPPY_ARG(batch->slot_cap >= 4 && batch->slot_cap % 4 == 0 && batch->slot_cap <= (1u << 20),
             "slot_cap must be a multiple of 4 in [4, 2^20]");
  SNAPPY_ARG(batch->ws_bytes >= scan_ws_bytes(batch->total_frags), "workspace smaller than nvt_snappy_ws_bytes");
  SNAPPY_ARG(((reinterpret_cast<uintptr_t>(batch->frag_table) | reinterpret_cast<uintptr_t>(batch->frag_size) |
               reinterpret_cast<uintptr_t>(batch->frag_pos) | reinterpret_cast<uintptr_t>(batch->ws)) & 7) == 0,
             "fragment arrays and ws must be 8-byte aligned");
  SNAPPY_ARG((reinterpret_cast<uintptr_t>(batch->slots) & 3) == 0, "slots must be 4-byte aligned");
  uint64_t next = 0;
  for (int i = 0; i < ncols; ++i) {
    const nvt_snappy_col &c = cols[i];
    SNAPPY_ARG(c.elem == 4 || c.elem == 8, "element size must be 4 or 8");
    SNAPPY_ARG(c.unit >= 1, "unit must be positive");
    SNAPPY_ARG(c.npages >= 1 && c.npages < (1ull << 32), "npages out of range");
    SNAPPY_ARG(c.nbytes < (1ull << 48), "nbytes out of range");
    SNAPPY_ARG(c.page_start && c.out && (c.src || c.nbytes == 0) && (c.dense || c.dense_cap == 0), "null pointer");
    SNAPPY_ARG((reinterpret_cast<uintptr_t>(c.out) & 7) == 0 && (reinterpret_cast<uintptr_t>(c.page_start) & 7) == 0,
               "out / page_start must be 8-byte aligned");
    SNAPPY_ARG((reinterpret_cast<uintptr_t>(c.dense) & 3) == 0, "dense must be 4-byte aligned");
    SNAPPY_ARG(c.frag_base == next, "fragment ranges must follow each other from 0");
    SNAPPY_ARG(c.max_frags >= frags_bound(c.nbytes, c.npages), "max_frags below ceil(nbytes / FRAG) + npages");
    SNAPPY_ARG(c.max_frags <= batch->total_frags - next, "fragment ranges pass total_frags");
    next += c.max_frags;
  }
  SNAPPY_ARG(next == batch->total_frags, "fragment ranges do not add up to total_frags");
#undef SNAPPY_ARG
  return NVT_OK;
}

// descriptors [i0, i0 + b.ncols) by value; -> their range of fragment records
void fill_batch(SBatch &b, const nvt_snappy_col *cols, int ncols, int i0, uint64_t *e0, uint64_t *e1) {
  memset(&b, 0, sizeof(b));
  b.ncols = ncols - i0 < kMaxCols ? ncols - i0 : kMaxCols;
  b.col0 = i0;
  for (int j = 0; j < b.ncols; ++j) {
    const nvt_snappy_col &c = cols[i0 + j];
    SCol &d = b.c[j];
    d.src = c.src;
    d.page_start = c.page_start;
    d.npages = c.npages;
    d.nbytes = c.nbytes;
    d.frag_base = c.frag_base;
    d.max_frags = c.max_frags;
    d.dense_cap = c.dense_cap;
    d.dense = c.dense;
    d.out = reinterpret_cast<unsigned long long *>(c.out);
    d.unit = c.unit;
    d.elem = c.elem;
  }
  *e0 = cols[i0].frag_base;
  *e1 = cols[i0 + b.ncols - 1].frag_base + cols[i0 + b.ncols - 1].max_frags;
}

inline unsigned frag_grid(uint64_t entries) { return (unsigned)(entries < (1u << 20) ? (entries ? entries : 1) : (1u << 20)); }

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_snappy_slot_bytes(uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null pointer");
  *bytes = NVT_SNAPPY_SLOT_BYTES;
  return NVT_OK;
}

int nvt_snappy_ws_bytes(uint64_t total_frags, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null pointer");
  *bytes = scan_ws_bytes(total_frags);
  return NVT_OK;
}

int nvt_snappy_plan_many(const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch, void *stream) {
  if (int rc = check_args(__func__, cols, ncols, batch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("snappy_plan", batch->total_frags * 8 * kRec, s);
  NVT_CHECK_HIP(hipMemsetAsync(batch->frag_table, 0, batch->total_frags * 8 * kRec, s));
  NVT_CHECK_HIP(hipMemsetAsync(batch->frag_size, 0, (batch->total_frags + 1) * 8, s));
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    SBatch b;
    uint64_t e0, e1;
    fill_batch(b, cols, ncols, i0, &e0, &e1);
    plan_kernel<<<b.ncols, kBlock, 0, s>>>(b, batch->frag_table);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_snappy_compress_many(const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch, void *stream) {
  if (int rc = check_args(__func__, cols, ncols, batch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint64_t bytes = 0;
  for (int i = 0; i < ncols; ++i) bytes += cols[i].nbytes;
  NVT_PROF("snappy_compress", bytes, s);
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    SBatch b;
    uint64_t e0, e1;
    fill_batch(b, cols, ncols, i0, &e0, &e1);
    compress_kernel<<<frag_grid(e1 - e0), kWave, 0, s>>>(b, batch->frag_table,
                                                         reinterpret_cast<unsigned long long *>(batch->frag_size),
                                                         batch->slots, batch->slot_cap, e0, e1);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_snappy_gather_many(const nvt_snappy_col *cols, int ncols, const nvt_snappy_batch *batch, void *stream) {
  if (int rc = check_args(__func__, cols, ncols, batch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint64_t bytes = 0;
  for (int i = 0; i < ncols; ++i) bytes += 2 * cols[i].dense_cap;
  NVT_PROF("snappy_gather", bytes, s);
  auto *size = reinterpret_cast<unsigned long long *>(batch->frag_size);
  auto *pos = reinterpret_cast<unsigned long long *>(batch->frag_pos);
  auto *tot = static_cast<unsigned long long *>(batch->ws);
  const uint64_t n = batch->total_frags, nt = list_ntiles(n + 1);
  scan_tile_kernel<<<stream_grid(nt, 1), kBlock, 0, s>>>(size, n, pos, tot);
  NVT_CHECK_LAUNCH();
  scan_totals_kernel<<<1, kBlock, 0, s>>>(tot, nt);
  NVT_CHECK_LAUNCH();
  scan_add_tiles_kernel<<<stream_grid(n + 1, kBlock * 4), kBlock, 0, s>>>(pos, n, tot);
  NVT_CHECK_LAUNCH();
  for (int i0 = 0; i0 < ncols; i0 += kMaxCols) {
    SBatch b;
    uint64_t e0, e1;
    fill_batch(b, cols, ncols, i0, &e0, &e1);
    gather_kernel<<<frag_grid(e1 - e0), kBlock, 0, s>>>(b, batch->frag_table, size, pos, batch->slots,
                                                        batch->slot_cap, e0, e1);
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

}  // extern "C"
