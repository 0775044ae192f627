// Field k of row r of an indexed CSV partition (nvt_csv_index): shared by the parse kernels of
// nvt_csv.hip and nvt_datetime.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvt {

struct Field {
  uint64_t s, e;
};
// field k of row r without the '\r' of a CRLF line end; positions clamped to the text
__device__ __forceinline__ Field field_at(const uint8_t *__restrict__ text, uint64_t nbytes,
                                          const uint32_t *__restrict__ fe, uint64_t r, uint32_t ncols, uint32_t k) {
  const uint64_t f = r * ncols + k;
  Field x;
  x.s = f ? (uint64_t)fe[f - 1] + 1 : 0;
  x.e = fe[f];
  if (x.e > nbytes) x.e = nbytes;
  if (x.s > x.e) x.s = x.e;
  if (k == ncols - 1 && x.e > x.s && text[x.e - 1] == '\r') --x.e;
  return x;
}
__device__ __forceinline__ bool quoted(const uint8_t *__restrict__ text, const Field &x, int quote) {
  return x.e - x.s >= 2 && text[x.s] == quote && text[x.e - 1] == quote;
}

}  // namespace nvt
