// Scalar text -> number routines of the CSV reader (nvt_csv.hip), usable on the host and on the
// device.  Each returns NVT_CSV_OK with *out set, NVT_CSV_DECLINED (the caller must use a slower
// exact parser), NVT_CSV_INVALID (not a number of this type) or NVT_CSV_OVERFLOW (integers only).
//
// csv_parse_f64 is exact or declines -- a result is the double nearest to the decimal text, ties
// to even, i.e. what strtod / Python's float() return:
//   1. at most 19 significant digits w and a decimal exponent q are collected; when w <= 2^53 and
//      |q| <= 22 both w and 10^|q| are doubles and ONE multiply or divide rounds once (Clinger,
//      "How to read floating point numbers accurately", 1990);
//   2. otherwise w * 10^q is taken from the leading 128 bits of w * 5^q (Lemire, "Number parsing
//      at a gigabyte per second", 2021; table: gen_csv_pow5.py).  The one case in which 128 bits
//      may not decide the rounding -- the low product word is all ones outside q in [-27, 55] --
//      is declined;
//   3. more than 19 significant digits are declined.
// The accepted grammar is [+-](digits[.digits] | .digits)[(e|E)[+-]digits] and, in any letter
// case, [+-]inf, [+-]infinity, [+-]nan.  No whitespace, no underscores, no hex floats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nvt_hip.h"

namespace nvt {

constexpr int kPow5MinQ = -342, kPow5MaxQ = 308;
static constexpr uint64_t kCsvPow5[kPow5MaxQ - kPow5MinQ + 1][2] = {
#include "nvt_csv_pow5.inc"
};
static constexpr double kCsvPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                         1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

__host__ __device__ inline uint64_t csv_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
__host__ __device__ inline int csv_clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)x);
#else
  return __builtin_clzll(x);
#endif
}
__host__ __device__ inline double csv_bits_f64(uint64_t b) {
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}
__host__ __device__ inline bool csv_word_is(const uint8_t *p, const char *lower, int n) {
  for (int i = 0; i < n; ++i)
    if ((p[i] | 0x20) != (uint8_t)lower[i]) return false;
  return true;
}

// w != 0, q any: the double nearest to w * 10^q as its bit pattern (sign clear), or declined
__host__ __device__ inline int csv_eisel_lemire(uint64_t w, int64_t q, uint64_t *bits) {
  if (q < kPow5MinQ) {  // w < 2^64 < 2 * 10^19: below half the smallest subnormal
    *bits = 0;
    return NVT_CSV_OK;
  }
  if (q > kPow5MaxQ) {
    *bits = 0x7FF0000000000000ull;
    return NVT_CSV_OK;
  }
  const int lz = csv_clz64(w);
  w <<= lz;
  const uint64_t t_hi = kCsvPow5[q - kPow5MinQ][0], t_lo = kCsvPow5[q - kPow5MinQ][1];
  uint64_t upper = csv_mulhi64(w, t_hi), lower = w * t_hi;
  if ((upper & 0x1FF) == 0x1FF) {  // the 55 bits that decide the rounding may still change
    const uint64_t second_hi = csv_mulhi64(w, t_lo);
    lower += second_hi;
    if (second_hi > lower) ++upper;
  }
  if (lower == 0xFFFFFFFFFFFFFFFFull && !(q >= -27 && q <= 55)) return NVT_CSV_DECLINED;
  const int upperbit = (int)(upper >> 63);
  const int shift = upperbit + 9;  // 64 - 52 - 3
  uint64_t m = upper >> shift;
  // floor(log2(10^q)) + 63, exact for |q| <= 350
  int64_t power2 = (((int64_t)217706 * q) >> 16) + 63 + upperbit - lz + 1023;
  if (power2 <= 0) {  // subnormal (or zero)
    if (-power2 + 1 >= 64) {
      *bits = 0;
      return NVT_CSV_OK;
    }
    m >>= -power2 + 1;
    m += m & 1;
    m >>= 1;
    power2 = m < (1ull << 52) ? 0 : 1;
    *bits = (m & ~(1ull << 52)) | ((uint64_t)power2 << 52);
    return NVT_CSV_OK;
  }
  // exactly half way between two doubles: round to even (only possible when 5^q fits 64 bits)
  if (lower <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == upper) m &= ~1ull;
  m += m & 1;
  m >>= 1;
  if (m >= (2ull << 52)) {
    m = 1ull << 52;
    ++power2;
  }
  m &= ~(1ull << 52);
  if (power2 >= 0x7FF) {
    *bits = 0x7FF0000000000000ull;
    return NVT_CSV_OK;
  }
  *bits = m | ((uint64_t)power2 << 52);
  return NVT_CSV_OK;
}

__host__ __device__ inline int csv_parse_f64(const uint8_t *p, int len, double *out) {
  int i = 0;
  bool neg = false;
  if (len > 0 && (p[0] == '-' || p[0] == '+')) {
    neg = p[0] == '-';
    i = 1;
  }
  if (i >= len) return NVT_CSV_INVALID;
  const uint64_t sign = neg ? 0x8000000000000000ull : 0;
  const uint8_t c0 = p[i] | 0x20;
  if (c0 == 'i' || c0 == 'n') {
    const int rem = len - i;
    if ((rem == 3 && csv_word_is(p + i, "inf", 3)) || (rem == 8 && csv_word_is(p + i, "infinity", 8))) {
      *out = csv_bits_f64(sign | 0x7FF0000000000000ull);
      return NVT_CSV_OK;
    }
    if (rem == 3 && csv_word_is(p + i, "nan", 3)) {
      *out = csv_bits_f64(sign | 0x7FF8000000000000ull);
      return NVT_CSV_OK;
    }
    return NVT_CSV_INVALID;
  }
  uint64_t w = 0;
  int nd = 0;         // significant digits held in w
  int64_t q = 0;      // decimal exponent of w
  bool any = false, many = false;
  for (; i < len; ++i) {
    const unsigned d = (unsigned)p[i] - '0';
    if (d > 9) break;
    any = true;
    if (w == 0 && d == 0) continue;  // leading zero
    if (nd < 19) {
      w = w * 10 + d;
      ++nd;
    } else {
      many = true;
    }
  }
  if (i < len && p[i] == '.') {
    for (++i; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - '0';
      if (d > 9) break;
      any = true;
      if (w == 0 && d == 0) {
        --q;
      } else if (nd < 19) {
        w = w * 10 + d;
        ++nd;
        --q;
      } else {
        many = true;
      }
    }
  }
  if (!any) return NVT_CSV_INVALID;
  if (i < len && (p[i] | 0x20) == 'e') {
    ++i;
    bool eneg = false;
    if (i < len && (p[i] == '+' || p[i] == '-')) {
      eneg = p[i] == '-';
      ++i;
    }
    if (i >= len || (unsigned)p[i] - '0' > 9) return NVT_CSV_INVALID;
    int64_t e = 0;
    for (; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - '0';
      if (d > 9) break;
      if (e < 100000) e = e * 10 + d;
    }
    q += eneg ? -e : e;
  }
  if (i != len) return NVT_CSV_INVALID;
  if (many) return NVT_CSV_DECLINED;
  if (w == 0) {
    *out = csv_bits_f64(sign);
    return NVT_CSV_OK;
  }
  if (w <= (1ull << 53) && q >= -22 && q <= 22) {
    double d = (double)w;
    d = q < 0 ? d / kCsvPow10[-q] : d * kCsvPow10[q];
    *out = neg ? -d : d;
    return NVT_CSV_OK;
  }
  uint64_t bits;
  const int rc = csv_eisel_lemire(w, q, &bits);
  if (rc != NVT_CSV_OK) return rc;
  *out = csv_bits_f64(sign | bits);
  return NVT_CSV_OK;
}

// [+-]digits; exact range check (INT64_MIN parses)
__host__ __device__ inline int csv_parse_i64(const uint8_t *p, int len, int64_t *out) {
  int i = 0;
  bool neg = false;
  if (len > 0 && (p[0] == '-' || p[0] == '+')) {
    neg = p[0] == '-';
    i = 1;
  }
  if (i >= len) return NVT_CSV_INVALID;
  const uint64_t lim = neg ? (1ull << 63) : (1ull << 63) - 1;
  uint64_t acc = 0;
  bool over = false;
  for (; i < len; ++i) {
    const unsigned d = (unsigned)p[i] - '0';
    if (d > 9) return NVT_CSV_INVALID;
    if (over || acc > (lim - d) / 10)
      over = true;
    else
      acc = acc * 10 + d;
  }
  if (over) return NVT_CSV_OVERFLOW;
  *out = neg ? (int64_t)(0 - acc) : (int64_t)acc;
  return NVT_CSV_OK;
}

}  // namespace nvt
