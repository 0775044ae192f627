// Delimited text on the device (nvtabular_amd/csv_text.py, kernels_csv.py).
//
// Index: two passes over the bytes, tile = 256 lanes x one 16-byte load = 4096 bytes.
//   A lane turns its 16 bytes into three 16-bit masks (quote, separator, newline).  Whether a byte
//   lies inside a quoted field is the parity of the quotes before it: in the lane a prefix XOR of
//   the quote mask (shifts 1, 2, 4, 8), across the lanes of a wave the popcount of the lower bits
//   of the ballot of the lane parities, across the four waves through LDS.
//   count_kernel does not know the parity at the start of its tile, so it records the tile's own
//   parity and its separator / newline counts under both hypotheses (a byte that is outside under
//   one is inside under the other); tile_scan_kernel (one workgroup, 256 records per step) resolves
//   the parity chain and turns the counts into the tile's first separator rank and first row.
//   index_kernel classifies again with the start parity known and stores the position of every
//   separator at its rank.  Field k of row r then needs no walk: it lies between separators
//   r * ncols + k - 1 and r * ncols + k.
// Numbers: parse_kernel, one lane per row and tile of 256 rows, loops over the descriptors of the
//   launch like take_kernel (nvt_loader.hip); a wave's 64 rows make one validity word.
// Strings: str_len_kernel / exclusive_scan_u32 / str_copy_kernel produce Arrow buffers.
#include "nvt_common.hpp"
#include "nvt_csv_field.hpp"
#include "nvt_csv_parse.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

constexpr int kCsvTile = NVT_CSV_TILE;
constexpr unsigned long long kNone = ~0ull;
static_assert(kCsvTile == kBlock * 16, "one 16-byte load per lane");
static_assert(NVT_CSV_SCAN_STEP == kBlock, "one tile record per lane and step");

struct Masks {
  uint32_t quote, sep, nl;
};

// the lane's 16 bytes at pos0 (a multiple of 16) as masks; bytes at or past nbytes are no byte
__device__ __forceinline__ Masks classify(const uint8_t *__restrict__ text, uint64_t nbytes, uint64_t pos0, int sep,
                                          int quote) {
  Masks m{0, 0, 0};
  if (pos0 >= nbytes) return m;
  const uint4 v = *reinterpret_cast<const uint4 *>(text + pos0);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int b = (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFF);
    m.quote |= (uint32_t)(b == quote) << j;
    m.sep |= (uint32_t)(b == sep) << j;
    m.nl |= (uint32_t)(b == '\n') << j;
  }
  const uint64_t left = nbytes - pos0;
  const uint32_t live = left >= 16 ? 0xFFFFu : ((1u << left) - 1);
  m.quote &= live;
  m.sep &= live;
  m.nl &= live;
  return m;
}

// bit j = parity of the quotes in bits [0, j] of q
__device__ __forceinline__ uint32_t prefix_xor16(uint32_t q) {
  q ^= q << 1;
  q ^= q << 2;
  q ^= q << 4;
  q ^= q << 8;
  return q & 0xFFFFu;
}

// The lane's inside-quotes mask given parity 0 at the start of the tile, and the tile's parity.
// Every thread of the block calls it; wpar is 4 words of LDS, free again after the call's barrier
// only once the caller has passed another barrier.
__device__ __forceinline__ uint32_t inside_mask(uint32_t quote_mask, unsigned *wpar, unsigned *tile_parity) {
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  uint32_t pm = prefix_xor16(quote_mask);
  const uint64_t bal = __ballot((pm >> 15) & 1);
  unsigned in = (unsigned)__popcll(bal & ((1ull << lane) - 1)) & 1;
  if (lane == 0) wpar[w] = (unsigned)__popcll(bal) & 1;
  __syncthreads();
  unsigned all = 0;
  for (unsigned k = 0; k < kBlock / kWave; ++k) {
    if (k < w) in ^= wpar[k];
    all ^= wpar[k];
  }
  *tile_parity = all;
  return in ? pm ^ 0xFFFFu : pm;
}

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off, 64);
    if (lane_id() >= (unsigned)off) v += o;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = __shfl_up(v, off, 64);
    if (lane_id() >= (unsigned)off) v += o;
  }
  return v;
}

// tile record before the scan: x = parity, y = separators (parity-0 start | parity-1 start << 16),
// z = newlines likewise; after the scan: x = start parity, y = first separator rank, z = first row
__global__ __launch_bounds__(kBlock) void count_kernel(const uint8_t *__restrict__ text, uint64_t nbytes, int sep,
                                                       int quote, uint4 *__restrict__ recs, uint64_t ntiles) {
  __shared__ unsigned wpar[kBlock / kWave];
  __shared__ unsigned wcnt[2][kBlock / kWave];
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const Masks m = classify(text, nbytes, t * kCsvTile + (uint64_t)threadIdx.x * 16, sep, quote);
    unsigned par;
    const uint32_t in = inside_mask(m.quote, wpar, &par);
    const uint32_t sn = m.sep | m.nl;
    uint32_t cs = (uint32_t)__popc(sn & ~in) | ((uint32_t)__popc(sn & in) << 16);
    uint32_t cn = (uint32_t)__popc(m.nl & ~in) | ((uint32_t)__popc(m.nl & in) << 16);
    cs = wave_incl_scan_u32(cs);
    cn = wave_incl_scan_u32(cn);
    if (lane == 63) {
      wcnt[0][w] = cs;
      wcnt[1][w] = cn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0, n = 0;
      for (unsigned k = 0; k < kBlock / kWave; ++k) {
        s += wcnt[0][k];
        n += wcnt[1][k];
      }
      recs[t] = make_uint4(par, s, n, 0);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void tile_scan_kernel(uint4 *__restrict__ recs, uint64_t ntiles,
                                                           unsigned long long *__restrict__ state) {
  __shared__ unsigned wpar[kBlock / kWave];
  __shared__ uint64_t wsum[kBlock / kWave];
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  unsigned par_c = 0;     // the three carries are identical in every thread
  uint64_t carry = 0;     // separators | rows << 32
  for (uint64_t b0 = 0; b0 < ntiles; b0 += kBlock) {
    const uint64_t i = b0 + threadIdx.x;
    uint4 r = make_uint4(0, 0, 0, 0);
    if (i < ntiles) r = recs[i];
    const uint64_t bal = __ballot(r.x & 1);
    unsigned pin = (unsigned)__popcll(bal & ((1ull << lane) - 1)) & 1;
    if (lane == 0) wpar[w] = (unsigned)__popcll(bal) & 1;
    __syncthreads();
    unsigned all = 0;
    for (unsigned k = 0; k < kBlock / kWave; ++k) {
      if (k < w) pin ^= wpar[k];
      all ^= wpar[k];
    }
    pin ^= par_c;
    const uint64_t v = (uint64_t)(pin ? r.y >> 16 : r.y & 0xFFFFu) | ((uint64_t)(pin ? r.z >> 16 : r.z & 0xFFFFu) << 32);
    const uint64_t inc = wave_incl_scan_u64(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t base = carry, tot = 0;
    for (unsigned k = 0; k < kBlock / kWave; ++k) {
      if (k < w) base += wsum[k];
      tot += wsum[k];
    }
    const uint64_t ex = base + inc - v;
    if (i < ntiles) recs[i] = make_uint4(pin, (uint32_t)ex, (uint32_t)(ex >> 32), 0);
    carry += tot;
    par_c ^= all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    state[NVT_CSV_ST_FIELDS] = carry & 0xFFFFFFFFull;
    state[NVT_CSV_ST_ROWS] = carry >> 32;
    state[NVT_CSV_ST_PARITY] = par_c;
    state[NVT_CSV_ST_BAD_ROW] = kNone;
    state[NVT_CSV_ST_QUOTE_ROW] = kNone;
    state[NVT_CSV_ST_BAD_FIELD] = kNone;
    state[NVT_CSV_ST_SLOW] = 0;
    state[7] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void index_kernel(const uint8_t *__restrict__ text, uint64_t nbytes, int sep,
                                                       int quote, uint32_t ncols, const uint4 *__restrict__ recs,
                                                       uint64_t ntiles, uint32_t *__restrict__ field_end,
                                                       uint64_t nfields, unsigned long long *__restrict__ state) {
  __shared__ unsigned wpar[kBlock / kWave];
  __shared__ unsigned wcnt[kBlock / kWave];
  const unsigned lane = lane_id(), w = threadIdx.x / kWave;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t pos0 = t * kCsvTile + (uint64_t)threadIdx.x * 16;
    const Masks m = classify(text, nbytes, pos0, sep, quote);
    const uint4 rec = recs[t];
    unsigned par;
    uint32_t in = inside_mask(m.quote, wpar, &par);
    if (rec.x & 1) in ^= 0xFFFFu;
    uint32_t out = (m.sep | m.nl) & ~in;   // separators that count
    const uint32_t nlo = m.nl & ~in;       // ... those that end a row
    const uint32_t nli = m.nl & in;        // newlines inside quotes: an error
    const uint32_t c = (uint32_t)__popc(out) | ((uint32_t)__popc(nlo) << 16);
    const uint32_t inc = wave_incl_scan_u32(c);
    if (lane == 63) wcnt[w] = inc;
    __syncthreads();
    uint32_t ex = inc - c;
    for (unsigned k = 0; k < w; ++k) ex += wcnt[k];
    uint64_t rank = (uint64_t)rec.y + (ex & 0xFFFFu);
    const uint64_t row0 = (uint64_t)rec.z + (ex >> 16);
    uint64_t row = row0;
    while (out) {
      const int j = __ffs(out) - 1;
      out &= out - 1;
      if (rank < nfields) field_end[rank] = (uint32_t)(pos0 + j);
      if ((nlo >> j) & 1) {
        if (rank != (row + 1) * (uint64_t)ncols - 1) atomicMin(&state[NVT_CSV_ST_BAD_ROW], (unsigned long long)row);
        ++row;
      }
      ++rank;
    }
    if (nli) {
      const int j = __ffs(nli) - 1;
      atomicMin(&state[NVT_CSV_ST_QUOTE_ROW], (unsigned long long)(row0 + __popc(nlo & ((1u << j) - 1))));
    }
    __syncthreads();
  }
}

// ---- fields ---------------------------------------------------------------------------------------
struct PCol {
  void *out;
  uint64_t *out_valid;
  uint64_t *slow;
  uint32_t k;
  int dtype;
};
struct PBatch {
  PCol c[NVT_CSV_MAX_COLS];
  int n;
};

__global__ __launch_bounds__(kBlock) void parse_kernel(PBatch b, const uint8_t *__restrict__ text, uint64_t nbytes,
                                                       const uint32_t *__restrict__ fe, uint64_t nrows,
                                                       uint32_t ncols, int quote,
                                                       unsigned long long *__restrict__ state) {
  const unsigned lane = lane_id();
  const uint64_t nt = (nrows + kBlock - 1) / kBlock;
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r = t * kBlock + threadIdx.x;
    const bool live = r < nrows;
    for (int ci = 0; ci < b.n; ++ci) {
      const PCol &c = b.c[ci];
      const bool is_float = c.dtype == NVT_F32 || c.dtype == NVT_F64;
      int rc = -1;  // -1: null
      double d = 0;
      int64_t v = 0;
      if (live) {
        Field x = field_at(text, nbytes, fe, r, ncols, c.k);
        if (quoted(text, x, quote)) {
          ++x.s;
          --x.e;
        }
        const int len = (int)(x.e - x.s);
        if (len > 0) {
          if (is_float) {
            rc = csv_parse_f64(text + x.s, len, &d);
          } else {
            rc = csv_parse_i64(text + x.s, len, &v);
            if (rc == NVT_CSV_OK && c.dtype == NVT_I32 && v != (int64_t)(int32_t)v) rc = NVT_CSV_OVERFLOW;
          }
        }
        const bool ok = rc == NVT_CSV_OK;
        switch (c.dtype) {
          case NVT_F64: ((double *)c.out)[r] = ok ? d : (rc < 0 ? __builtin_nan("") : 0.0); break;
          case NVT_F32: ((float *)c.out)[r] = ok ? (float)d : (rc < 0 ? __builtin_nanf("") : 0.0f); break;
          case NVT_I64: ((int64_t *)c.out)[r] = ok ? v : 0; break;
          default: ((int32_t *)c.out)[r] = ok ? (int32_t)v : 0; break;
        }
        if (rc >= NVT_CSV_INVALID)
          atomicMin(&state[NVT_CSV_ST_BAD_FIELD],
                    (unsigned long long)((r << 24) | ((uint64_t)c.k << 2) | (uint64_t)rc));
      }
      // (block-uniform from here: every lane of the wave reaches the ballots)
      const uint64_t word = __ballot(rc == NVT_CSV_OK || rc == NVT_CSV_DECLINED);
      if (lane == 0 && live) c.out_valid[r >> 6] = word;
      if (is_float) {
        const uint64_t sword = __ballot(rc == NVT_CSV_DECLINED);
        if (lane == 0 && live) {
          c.slow[r >> 6] = sword;
          if (sword) atomicAdd(&state[NVT_CSV_ST_SLOW], (unsigned long long)__popcll(sword));
        }
      }
    }
  }
}

// Bytes of the field after unquoting; x becomes the bytes to copy from (quotes stripped).  Inside
// a quoted field a quote must be doubled: *malformed tells when one is not.
__device__ __forceinline__ uint32_t str_len(const uint8_t *__restrict__ text, Field &x, int quote, bool *malformed) {
  *malformed = false;
  if (!quoted(text, x, quote)) return (uint32_t)(x.e - x.s);
  ++x.s;
  --x.e;
  uint32_t pairs = 0;
  for (uint64_t i = x.s; i < x.e; ++i) {
    if (text[i] != quote) continue;
    if (i + 1 < x.e && text[i + 1] == quote) {
      ++pairs;
      ++i;
    } else {
      *malformed = true;
    }
  }
  return (uint32_t)(x.e - x.s) - pairs;  // a doubled quote stands for one
}

__global__ __launch_bounds__(kBlock) void str_len_kernel(const uint8_t *__restrict__ text, uint64_t nbytes,
                                                         const uint32_t *__restrict__ fe, uint64_t nrows,
                                                         uint32_t ncols, uint32_t k, int quote,
                                                         uint32_t *__restrict__ lengths,
                                                         uint64_t *__restrict__ out_valid,
                                                         unsigned long long *__restrict__ state) {
  const unsigned lane = lane_id();
  const uint64_t nt = (nrows + kBlock - 1) / kBlock;
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r = t * kBlock + threadIdx.x;
    const bool live = r < nrows;
    uint32_t len = 0;
    if (live) {
      Field x = field_at(text, nbytes, fe, r, ncols, k);
      bool malformed;
      len = str_len(text, x, quote, &malformed);
      lengths[r] = len;
      if (malformed)
        atomicMin(&state[NVT_CSV_ST_BAD_FIELD],
                  (unsigned long long)((r << 24) | ((uint64_t)k << 2) | (uint64_t)NVT_CSV_INVALID));
    }
    const uint64_t word = __ballot(len > 0);
    if (lane == 0 && live) out_valid[r >> 6] = word;
  }
}

__global__ __launch_bounds__(kBlock) void str_copy_kernel(const uint8_t *__restrict__ text, uint64_t nbytes,
                                                          const uint32_t *__restrict__ fe, uint64_t nrows,
                                                          uint32_t ncols, uint32_t k, int quote,
                                                          const int32_t *__restrict__ offsets,
                                                          uint8_t *__restrict__ chars, uint64_t chars_bytes) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < nrows; r += (uint64_t)gridDim.x * kBlock) {
    Field x = field_at(text, nbytes, fe, r, ncols, k);
    const bool q = quoted(text, x, quote);
    if (q) {
      ++x.s;
      --x.e;
    }
    uint64_t o = (uint64_t)(uint32_t)offsets[r];
    const uint64_t end = (uint64_t)(uint32_t)offsets[r + 1] < chars_bytes ? (uint64_t)(uint32_t)offsets[r + 1] : chars_bytes;
    for (uint64_t i = x.s; i < x.e && o < end; ++i) {
      const uint8_t ch = text[i];
      chars[o++] = ch;
      if (q && ch == quote && i + 1 < x.e && text[i + 1] == quote) ++i;  // the second quote of a doubled one
    }
  }
}

uint64_t csv_ntiles(uint64_t nbytes) { return (nbytes + kCsvTile - 1) / kCsvTile; }

}  // namespace
}  // namespace nvt

using namespace nvt;

#define CSV_CHECK_TEXT()                                                                              \
  NVT_CHECK_ARG(nbytes < (1ull << 31), "nbytes must be below 2^31");                                  \
  NVT_CHECK_ARG(text || nbytes == 0, "null text");                                                    \
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(text) & 15) == 0, "text must be 16-byte aligned");       \
  NVT_CHECK_ARG(quote >= -1 && quote <= 255 && quote != '\n', "quote must be a byte other than newline, or -1")

#define CSV_CHECK_FIELDS()                                                                            \
  NVT_CHECK_ARG(ncols >= 1 && ncols <= (1u << 22), "ncols must be 1 to 2^22");                              \
  NVT_CHECK_ARG(field_end || nrows == 0, "null field_end");                                           \
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(field_end) & 3) == 0, "field_end must be 4-byte aligned"); \
  NVT_CHECK_ARG(nrows <= nbytes && nrows * (uint64_t)ncols <= nbytes, "nrows * ncols must not exceed nbytes")

extern "C" {

int nvt_csv_ws_bytes(uint64_t nbytes, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  NVT_CHECK_ARG(nbytes < (1ull << 31), "nbytes must be below 2^31");
  *bytes = (csv_ntiles(nbytes) + 1) * sizeof(uint4);
  return NVT_OK;
}

int nvt_csv_count(const uint8_t *text, uint64_t nbytes, int sep, int quote, void *ws, uint64_t ws_bytes,
                  uint64_t *state, void *stream) {
  CSV_CHECK_TEXT();
  NVT_CHECK_ARG(sep >= 0 && sep <= 255 && sep != '\n' && sep != quote, "sep must be a byte other than newline and quote");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "workspace must be 16-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (csv_ntiles(nbytes) + 1) * sizeof(uint4), "workspace smaller than nvt_csv_ws_bytes(nbytes)");
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be 8-byte aligned");
  if (nbytes == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t nt = csv_ntiles(nbytes);
  NVT_PROF("csv_count", nbytes, s);
  count_kernel<<<stream_grid(nt, 1), kBlock, 0, s>>>(text, nbytes, sep, quote, reinterpret_cast<uint4 *>(ws), nt);
  NVT_CHECK_LAUNCH();
  tile_scan_kernel<<<1, kBlock, 0, s>>>(reinterpret_cast<uint4 *>(ws), nt, reinterpret_cast<unsigned long long *>(state));
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_csv_index(const uint8_t *text, uint64_t nbytes, int sep, int quote, uint32_t ncols, const void *ws,
                  uint64_t ws_bytes, uint32_t *field_end, uint64_t nfields, uint64_t *state, void *stream) {
  CSV_CHECK_TEXT();
  NVT_CHECK_ARG(sep >= 0 && sep <= 255 && sep != '\n' && sep != quote, "sep must be a byte other than newline and quote");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= (1u << 22), "ncols must be 1 to 2^22");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "workspace must be 16-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (csv_ntiles(nbytes) + 1) * sizeof(uint4), "workspace smaller than nvt_csv_ws_bytes(nbytes)");
  NVT_CHECK_ARG(field_end || nfields == 0, "null field_end");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(field_end) & 3) == 0, "field_end must be 4-byte aligned");
  NVT_CHECK_ARG(nfields <= nbytes, "nfields must not exceed nbytes");
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be 8-byte aligned");
  if (nbytes == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t nt = csv_ntiles(nbytes);
  NVT_PROF("csv_index", nbytes + nfields * 4, s);
  index_kernel<<<stream_grid(nt, 1), kBlock, 0, s>>>(text, nbytes, sep, quote, ncols, reinterpret_cast<const uint4 *>(ws),
                                                     nt, field_end, nfields, reinterpret_cast<unsigned long long *>(state));
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_csv_parse_many(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                       uint32_t ncols, int quote, const nvt_csv_col *cols, int ndesc, uint64_t *state,
                       void *stream) {
  CSV_CHECK_TEXT();
  CSV_CHECK_FIELDS();
  NVT_CHECK_ARG(ndesc >= 0, "ndesc must not be negative");
  NVT_CHECK_ARG(cols || ndesc == 0, "null descriptors");
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be 8-byte aligned");
  for (int i = 0; i < ndesc; ++i) {
    const nvt_csv_col &c = cols[i];
    NVT_CHECK_ARG(c.dtype == NVT_F32 || c.dtype == NVT_F64 || c.dtype == NVT_I32 || c.dtype == NVT_I64,
                  "dtype must be NVT_F32, NVT_F64, NVT_I32 or NVT_I64");
    const bool is_float = c.dtype == NVT_F32 || c.dtype == NVT_F64;
    const unsigned es = (c.dtype == NVT_F32 || c.dtype == NVT_I32) ? 4 : 8;
    NVT_CHECK_ARG(c.k < ncols, "k must be below ncols");
    NVT_CHECK_ARG(nrows == 0 || (c.out && c.out_valid), "null out / out_valid");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.out) & (es - 1)) == 0, "out must be aligned to its element size");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.out_valid) & 7) == 0, "out_valid must be 8-byte aligned");
    NVT_CHECK_ARG(nrows == 0 || !is_float || c.slow, "null slow bitmap of a float column");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.slow) & 7) == 0, "slow must be 8-byte aligned");
  }
  if (nrows == 0 || ndesc == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = stream_grid((nrows + kBlock - 1) / kBlock, 1);
  for (int i0 = 0; i0 < ndesc; i0 += NVT_CSV_MAX_COLS) {
    PBatch b;
    memset(&b, 0, sizeof(b));
    b.n = ndesc - i0 < NVT_CSV_MAX_COLS ? ndesc - i0 : NVT_CSV_MAX_COLS;
    for (int j = 0; j < b.n; ++j) {
      const nvt_csv_col &c = cols[i0 + j];
      b.c[j] = PCol{c.out, reinterpret_cast<uint64_t *>(c.out_valid), reinterpret_cast<uint64_t *>(c.slow), c.k, c.dtype};
    }
    NVT_PROF("csv_parse_many", nrows * (uint64_t)b.n * 16, s);
    parse_kernel<<<grid, kBlock, 0, s>>>(b, text, nbytes, field_end, nrows, ncols, quote,
                                         reinterpret_cast<unsigned long long *>(state));
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_csv_str_ws_bytes(uint64_t nrows, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null output");
  *bytes = (scan_chunks(nrows + 1) + 1) * 8;
  return NVT_OK;
}

int nvt_csv_str_offsets(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                        uint32_t ncols, uint32_t k, int quote, int32_t *offsets, uint8_t *out_valid, void *ws,
                        uint64_t ws_bytes, uint64_t *state, void *stream) {
  CSV_CHECK_TEXT();
  CSV_CHECK_FIELDS();
  NVT_CHECK_ARG(k < ncols, "k must be below ncols");
  NVT_CHECK_ARG(offsets, "null offsets");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(offsets) & 3) == 0, "offsets must be 4-byte aligned");
  NVT_CHECK_ARG(out_valid || nrows == 0, "null out_valid");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(out_valid) & 7) == 0, "out_valid must be 8-byte aligned");
  NVT_CHECK_ARG(ws, "null workspace");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "workspace must be 8-byte aligned");
  NVT_CHECK_ARG(ws_bytes >= (scan_chunks(nrows + 1) + 1) * 8, "workspace smaller than nvt_csv_str_ws_bytes(nrows)");
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be 8-byte aligned");
  if (nrows == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("csv_str_offsets", nrows * 16, s);
  NVT_CHECK_HIP(hipMemsetAsync(offsets + nrows, 0, 4, s));
  str_len_kernel<<<stream_grid((nrows + kBlock - 1) / kBlock, 1), kBlock, 0, s>>>(
      text, nbytes, field_end, nrows, ncols, k, quote, reinterpret_cast<uint32_t *>(offsets),
      reinterpret_cast<uint64_t *>(out_valid), reinterpret_cast<unsigned long long *>(state));
  NVT_CHECK_LAUNCH();
  return exclusive_scan_u32(reinterpret_cast<unsigned *>(offsets), nrows + 1,
                            reinterpret_cast<unsigned long long *>(ws), s);
}

int nvt_csv_str_copy(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                     uint32_t ncols, uint32_t k, int quote, const int32_t *offsets, uint8_t *chars,
                     uint64_t chars_bytes, void *stream) {
  CSV_CHECK_TEXT();
  CSV_CHECK_FIELDS();
  NVT_CHECK_ARG(k < ncols, "k must be below ncols");
  NVT_CHECK_ARG(offsets || nrows == 0, "null offsets");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(offsets) & 3) == 0, "offsets must be 4-byte aligned");
  NVT_CHECK_ARG(chars || chars_bytes == 0, "null chars");
  if (nrows == 0 || chars_bytes == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("csv_str_copy", chars_bytes * 2 + nrows * 12, s);
  str_copy_kernel<<<stream_grid(nrows, kBlock), kBlock, 0, s>>>(text, nbytes, field_end, nrows, ncols, k, quote, offsets,
                                                                chars, chars_bytes);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_csv_parse_f64_host(const char *text, int len, double *out) {
  NVT_CHECK_ARG(out, "null output");
  NVT_CHECK_ARG(text || len == 0, "null text");
  NVT_CHECK_ARG(len >= 0, "len must not be negative");
  return csv_parse_f64(reinterpret_cast<const uint8_t *>(text), len, out);
}

int nvt_csv_parse_i64_host(const char *text, int len, int64_t *out) {
  NVT_CHECK_ARG(out, "null output");
  NVT_CHECK_ARG(text || len == 0, "null text");
  NVT_CHECK_ARG(len >= 0, "len must not be negative");
  return csv_parse_i64(reinterpret_cast<const uint8_t *>(text), len, out);
}

}  // extern "C"
