// Scalar calendar routines of the datetime kernels (nvt_datetime.hip), usable on the host and on
// the device, as nvt_csv_parse.hpp is for the number parsers.
//
// dt_field: a count since 1970-01-01T00:00:00 in unit s / ms / us / ns -> one calendar field on
//   the proleptic Gregorian calendar.  The count is floor-divided to (day, second of the day), so
//   1969-12-31 23:59:59 is day -1; the day goes through civil-from-days on 400-year eras (Howard
//   Hinnant, "chrono-Compatible Low-Level Date Algorithms").  Every intermediate fits int64 for
//   every int64 input; the results are specified for years 1 to 9999.
// csv_parse_datetime: ISO-8601 text -> int64 nanoseconds.  Grammar, nothing else:
//   YYYY-MM-DD[(T| )HH:MM[:SS[.f{1,9}]]].  NVT_CSV_INVALID for another shape or an instant the
//   calendar does not have, NVT_CSV_OVERFLOW when it does not fit int64 nanoseconds or equals
//   INT64_MIN (the NaT pattern of numpy and pandas).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nvt_hip.h"

namespace nvt {

__host__ __device__ inline int64_t dt_floor_div(int64_t a, int64_t b, int64_t *rem) {  // b > 0
  int64_t q = a / b, r = a % b;
  if (r < 0) {
    --q;
    r += b;
  }
  *rem = r;
  return q;
}

// whole seconds since the epoch, rounded down (the divisors are constants: no 64-bit divide loop)
__host__ __device__ inline int64_t dt_floor_seconds(int64_t ts, int unit) {
  int64_t r;
  switch (unit) {
    case NVT_DT_MS: return dt_floor_div(ts, 1000, &r);
    case NVT_DT_US: return dt_floor_div(ts, 1000000, &r);
    case NVT_DT_NS: return dt_floor_div(ts, 1000000000, &r);
    default: return ts;
  }
}

__host__ __device__ inline bool dt_is_leap(int64_t y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }

__host__ __device__ inline int32_t dt_field(int64_t ts, int unit, int field) {
  int64_t sod;
  const int64_t days = dt_floor_div(dt_floor_seconds(ts, unit), 86400, &sod);  // |days| < 2^47
  switch (field) {
    case NVT_DT_HOUR: return (int32_t)(sod / 3600);
    case NVT_DT_MINUTE: return (int32_t)(sod / 60 % 60);
    case NVT_DT_SECOND: return (int32_t)(sod % 60);
    case NVT_DT_WEEKDAY: {
      int64_t wd;
      dt_floor_div(days + 3, 7, &wd);  // 1970-01-01 was a Thursday
      return (int32_t)wd;
    }
    default: break;
  }
  int64_t doe;  // day of the 400-year era that starts on 0000-03-01, [0, 146096]
  const int64_t era = dt_floor_div(days + 719468, 146097, &doe);
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;  // [0, 399]
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                // from 1 March, [0, 365]
  const int64_t mp = (5 * doy + 2) / 153;                                     // March = 0
  const int month = (int)(mp < 10 ? mp + 3 : mp - 9);
  const int64_t year = yoe + era * 400 + (month <= 2);
  switch (field) {
    case NVT_DT_YEAR: return (int32_t)year;
    case NVT_DT_MONTH: return month;
    case NVT_DT_DAY: return (int32_t)(doy - (153 * mp + 2) / 5 + 1);
    case NVT_DT_QUARTER: return (month - 1) / 3 + 1;
    default:  // NVT_DT_DAYOFYEAR: 1 January is day 306 of the year that starts in March
      return (int32_t)(mp >= 10 ? doy - 305 : doy + 60 + (dt_is_leap(year) ? 1 : 0));
  }
}

// n decimal digits at p -> *v; false when one of them is no digit
__host__ __device__ inline bool dt_digits(const uint8_t *p, int n, int *v) {
  int acc = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned d = (unsigned)p[i] - '0';
    if (d > 9) return false;
    acc = acc * 10 + (int)d;
  }
  *v = acc;
  return true;
}

__host__ __device__ inline int csv_parse_datetime(const uint8_t *p, int len, int64_t *out) {
  if (!(len == 10 || len == 16 || len == 19 || (len >= 21 && len <= 29))) return NVT_CSV_INVALID;
  int y, mo, d, h = 0, mi = 0, s = 0, ns = 0;
  if (!dt_digits(p, 4, &y) || p[4] != '-' || !dt_digits(p + 5, 2, &mo) || p[7] != '-' || !dt_digits(p + 8, 2, &d))
    return NVT_CSV_INVALID;
  if (len > 10) {
    if ((p[10] != 'T' && p[10] != ' ') || !dt_digits(p + 11, 2, &h) || p[13] != ':' || !dt_digits(p + 14, 2, &mi))
      return NVT_CSV_INVALID;
  }
  if (len > 16) {
    if (p[16] != ':' || !dt_digits(p + 17, 2, &s)) return NVT_CSV_INVALID;
  }
  if (len > 19) {
    if (p[19] != '.' || !dt_digits(p + 20, len - 20, &ns)) return NVT_CSV_INVALID;
    for (int i = len - 20; i < 9; ++i) ns *= 10;
  }
  if (y < 1 || mo < 1 || mo > 12 || d < 1 || h > 23 || mi > 59 || s > 59) return NVT_CSV_INVALID;
  const int mdays = mo == 2 ? (dt_is_leap(y) ? 29 : 28) : ((mo == 4 || mo == 6 || mo == 9 || mo == 11) ? 30 : 31);
  if (d > mdays) return NVT_CSV_INVALID;
  // days-from-civil: the year starts in March, so the leap day is its last
  const int64_t ym = y - (mo <= 2);
  const int64_t era = ym / 400;  // ym >= 0
  const int64_t yoe = ym - era * 400;
  const int64_t doy = (153 * (mo > 2 ? mo - 3 : mo + 9) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  const int64_t days = era * 146097 + doe - 719468;
  const int64_t secs = days * 86400 + h * 3600 + mi * 60 + s;
  // INT64_MAX = 9223372036 s + 854775807 ns; INT64_MIN = -9223372037 s + 145224192 ns
  if (secs > 9223372036ll || (secs == 9223372036ll && ns > 854775807)) return NVT_CSV_OVERFLOW;
  if (secs < -9223372037ll || (secs == -9223372037ll && ns <= 145224192)) return NVT_CSV_OVERFLOW;
  *out = secs >= 0 ? secs * 1000000000ll + ns : (secs + 1) * 1000000000ll + (ns - 1000000000ll);
  return NVT_CSV_OK;
}

}  // namespace nvt
