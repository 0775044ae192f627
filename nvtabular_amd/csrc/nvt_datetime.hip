// Datetime columns on the device (nvtabular_amd/kernels_datetime.py).
//
// field_kernel: a plain stream.  A lane loads 16 bytes (two timestamps), runs dt_field
//   (nvt_datetime.hpp) on each and stores the two int32 as one 8-byte word where `out` allows it.
//   A `ts` that is 8 but not 16 bytes aligned has its first element handled alone, as is the last
//   one of an odd rest.  A null row stores 0 and its slot's bytes are not looked at.
// parse_kernel: the ISO-8601 columns of a CSV partition, one lane per row, after the numeric
//   columns (nvt_csv.hip): the same field index, quote stripping, validity words and error code.
#include "nvt_common.hpp"
#include "nvt_csv_field.hpp"
#include "nvt_datetime.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

template <int UNIT>
__device__ __forceinline__ int32_t field_of(const int64_t v, const uint8_t *__restrict__ valid, uint64_t i, int field) {
  return bit_valid(valid, i) ? dt_field(v, UNIT, field) : 0;
}

// pairs = (n - head) / 2 aligned pairs start at element head (0 or 1); wide: out + head is 8-byte aligned
template <int UNIT>
__global__ __launch_bounds__(kBlock) void field_kernel(const int64_t *__restrict__ ts,
                                                       const uint8_t *__restrict__ valid, uint64_t n, uint64_t head,
                                                       int field, int wide, int32_t *__restrict__ out) {
  const uint64_t pairs = (n - head) / 2;
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < pairs; p += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = head + 2 * p;
    const longlong2 v = *reinterpret_cast<const longlong2 *>(ts + i);
    const int2 r = make_int2(field_of<UNIT>(v.x, valid, i, field), field_of<UNIT>(v.y, valid, i + 1, field));
    if (wide) {
      *reinterpret_cast<int2 *>(out + i) = r;
    } else {
      out[i] = r.x;
      out[i + 1] = r.y;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) out[0] = field_of<UNIT>(ts[0], valid, 0, field);
    const uint64_t last = head + 2 * pairs;
    if (last < n) out[last] = field_of<UNIT>(ts[last], valid, last, field);
  }
}

struct DCol {
  int64_t *out;
  uint64_t *out_valid;
  uint32_t k;
};
struct DBatch {
  DCol c[NVT_CSV_MAX_COLS];
  int n;
};

__global__ __launch_bounds__(kBlock) void parse_kernel(DBatch b, const uint8_t *__restrict__ text, uint64_t nbytes,
                                                       const uint32_t *__restrict__ fe, uint64_t nrows,
                                                       uint32_t ncols, int quote,
                                                       unsigned long long *__restrict__ state) {
  const unsigned lane = lane_id();
  const uint64_t nt = (nrows + kBlock - 1) / kBlock;
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint64_t r = t * kBlock + threadIdx.x;
    const bool live = r < nrows;
    for (int ci = 0; ci < b.n; ++ci) {
      const DCol &c = b.c[ci];
      int rc = -1;  // -1: null
      int64_t v = 0;
      if (live) {
        Field x = field_at(text, nbytes, fe, r, ncols, c.k);
        if (quoted(text, x, quote)) {
          ++x.s;
          --x.e;
        }
        const uint64_t len = x.e - x.s;
        if (len > 0) rc = len <= 29 ? csv_parse_datetime(text + x.s, (int)len, &v) : NVT_CSV_INVALID;
        c.out[r] = rc == NVT_CSV_OK ? v : 0;
        if (rc >= NVT_CSV_INVALID)
          atomicMin(&state[NVT_CSV_ST_BAD_FIELD],
                    (unsigned long long)((r << 24) | ((uint64_t)c.k << 2) | (uint64_t)rc));
      }
      // (block-uniform from here: every lane of the wave reaches the ballot)
      const uint64_t word = __ballot(rc == NVT_CSV_OK);
      if (lane == 0 && live) c.out_valid[r >> 6] = word;
    }
  }
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_dt_field(const int64_t *ts, const uint8_t *valid, uint64_t n, int unit, int field, int32_t *out,
                 void *stream) {
  NVT_CHECK_ARG(unit >= NVT_DT_S && unit <= NVT_DT_NS, "unit must be NVT_DT_S, _MS, _US or _NS");
  NVT_CHECK_ARG(field >= NVT_DT_YEAR && field <= NVT_DT_QUARTER, "field must be one of NVT_DT_YEAR .. NVT_DT_QUARTER");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(ts && out, "null ts / out");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ts) & 7) == 0, "ts must be 8-byte aligned");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "out must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t head = (reinterpret_cast<uintptr_t>(ts) & 15) ? 1 : 0;
  const int wide = (reinterpret_cast<uintptr_t>(out + head) & 7) == 0;
  const unsigned grid = stream_grid((n + 1) / 2, kBlock);
  NVT_PROF("dt_field", n * 12, s);
  switch (unit) {
    case NVT_DT_S: field_kernel<NVT_DT_S><<<grid, kBlock, 0, s>>>(ts, valid, n, head, field, wide, out); break;
    case NVT_DT_MS: field_kernel<NVT_DT_MS><<<grid, kBlock, 0, s>>>(ts, valid, n, head, field, wide, out); break;
    case NVT_DT_US: field_kernel<NVT_DT_US><<<grid, kBlock, 0, s>>>(ts, valid, n, head, field, wide, out); break;
    default: field_kernel<NVT_DT_NS><<<grid, kBlock, 0, s>>>(ts, valid, n, head, field, wide, out); break;
  }
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_dt_fields_host(const int64_t *ts, uint64_t n, int unit, int field, int32_t *out) {
  NVT_CHECK_ARG(unit >= NVT_DT_S && unit <= NVT_DT_NS, "unit must be NVT_DT_S, _MS, _US or _NS");
  NVT_CHECK_ARG(field >= NVT_DT_YEAR && field <= NVT_DT_QUARTER, "field must be one of NVT_DT_YEAR .. NVT_DT_QUARTER");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(ts && out, "null ts / out");
  for (uint64_t i = 0; i < n; ++i) out[i] = dt_field(ts[i], unit, field);
  return NVT_OK;
}

int nvt_csv_parse_datetime(const uint8_t *text, uint64_t nbytes, const uint32_t *field_end, uint64_t nrows,
                           uint32_t ncols, int quote, const nvt_csv_col *cols, int ndesc, uint64_t *state,
                           void *stream) {
  NVT_CHECK_ARG(nbytes < (1ull << 31), "nbytes must be below 2^31");
  NVT_CHECK_ARG(text || nbytes == 0, "null text");
  NVT_CHECK_ARG(quote >= -1 && quote <= 255 && quote != '\n', "quote must be a byte other than newline, or -1");
  NVT_CHECK_ARG(ncols >= 1 && ncols <= (1u << 22), "ncols must be 1 to 2^22");
  NVT_CHECK_ARG(field_end || nrows == 0, "null field_end");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(field_end) & 3) == 0, "field_end must be 4-byte aligned");
  NVT_CHECK_ARG(nrows <= nbytes && nrows * (uint64_t)ncols <= nbytes, "nrows * ncols must not exceed nbytes");
  NVT_CHECK_ARG(ndesc >= 0, "ndesc must not be negative");
  NVT_CHECK_ARG(cols || ndesc == 0, "null descriptors");
  NVT_CHECK_ARG(state, "null state");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0, "state must be 8-byte aligned");
  for (int i = 0; i < ndesc; ++i) {
    const nvt_csv_col &c = cols[i];
    NVT_CHECK_ARG(c.dtype == NVT_I64, "dtype must be NVT_I64 (nanoseconds)");
    NVT_CHECK_ARG(c.k < ncols, "k must be below ncols");
    NVT_CHECK_ARG(nrows == 0 || (c.out && c.out_valid), "null out / out_valid");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.out) & 7) == 0, "out must be 8-byte aligned");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(c.out_valid) & 7) == 0, "out_valid must be 8-byte aligned");
  }
  if (nrows == 0 || ndesc == 0) return NVT_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = stream_grid((nrows + kBlock - 1) / kBlock, 1);
  for (int i0 = 0; i0 < ndesc; i0 += NVT_CSV_MAX_COLS) {
    DBatch b;
    memset(&b, 0, sizeof(b));
    b.n = ndesc - i0 < NVT_CSV_MAX_COLS ? ndesc - i0 : NVT_CSV_MAX_COLS;
    for (int j = 0; j < b.n; ++j) {
      const nvt_csv_col &c = cols[i0 + j];
      b.c[j] = DCol{reinterpret_cast<int64_t *>(c.out), reinterpret_cast<uint64_t *>(c.out_valid), c.k};
    }
    NVT_PROF("csv_parse_datetime", nrows * (uint64_t)b.n * 32, s);
    parse_kernel<<<grid, kBlock, 0, s>>>(b, text, nbytes, field_end, nrows, ncols, quote,
                                         reinterpret_cast<unsigned long long *>(state));
    NVT_CHECK_LAUNCH();
  }
  return NVT_OK;
}

int nvt_csv_parse_datetime_host(const char *text, int len, int64_t *out_ns) {
  NVT_CHECK_ARG(out_ns, "null output");
  NVT_CHECK_ARG(text || len == 0, "null text");
  NVT_CHECK_ARG(len >= 0, "len must not be negative");
  return csv_parse_datetime(reinterpret_cast<const uint8_t *>(text), len, out_ns);
}

}  // extern "C"
