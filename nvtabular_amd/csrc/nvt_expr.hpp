// Scalar routines of the column-expression interpreter (nvt_expr.hip, include/nvt_hip.h
// nvt_expr_eval): what ONE instruction does to ONE element.  __host__ __device__, so the kernel
// and nvt_expr_eval_host run the same code; on the device `op` is a template constant at every
// call and the switches below fold away.
//
// A register holds one 64-bit slot per element.  Its class says how the slot is read:
//   I64   int64_t (an int8 / int16 / int32-typed value lives here sign-extended: the instruction's
//         `wrap` truncates the result of every op to that width, so wrap-around is the narrow type's)
//   F64   double
//   F32   float in the low 32 bits: float32 ops are float32 ops, one rounding
//   BOOL  int64_t 0 / 1
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nvt_hip.h"

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace nvt {

template <typename T>
struct ExprType {};
template <>
struct ExprType<int64_t> {
  static constexpr bool is_int = true;
};
template <>
struct ExprType<double> {
  static constexpr bool is_int = false;
};
template <>
struct ExprType<float> {
  static constexpr bool is_int = false;
};

template <typename T>
__host__ __device__ inline T expr_from_slot(uint64_t s) {
  if constexpr (sizeof(T) == 4) {
    const uint32_t lo = (uint32_t)s;
    T v;
    memcpy(&v, &lo, 4);
    return v;
  } else {
    T v;
    memcpy(&v, &s, 8);
    return v;
  }
}
template <typename T>
__host__ __device__ inline uint64_t expr_to_slot(T v) {
  if constexpr (sizeof(T) == 4) {
    uint32_t lo;
    memcpy(&lo, &v, 4);
    return lo;
  } else {
    uint64_t s;
    memcpy(&s, &v, 8);
    return s;
  }
}

// sign-extend the low (64 - shift) bits: shift = 0 leaves an int64 alone
__host__ __device__ inline int64_t expr_wrap(int64_t v, int shift) {
  return (int64_t)((uint64_t)v << shift) >> shift;
}

template <typename T>
__host__ __device__ inline T expr_nan() {
  return (T)NAN;
}

__host__ __device__ inline double expr_floor(double x) { return floor(x); }
__host__ __device__ inline float expr_floor(float x) { return floorf(x); }
__host__ __device__ inline double expr_fmod(double a, double b) { return fmod(a, b); }
__host__ __device__ inline float expr_fmod(float a, float b) { return fmodf(a, b); }
__host__ __device__ inline double expr_copysign(double a, double b) { return copysign(a, b); }
__host__ __device__ inline float expr_copysign(float a, float b) { return copysignf(a, b); }

// floats: torch.div(rounding_mode="floor") and torch.remainder (c10::div_floor_floating)
template <typename T>
__host__ __device__ inline T expr_floordiv_f(T a, T b) {
  if (b == 0) return a / b;
  const T mod = expr_fmod(a, b);
  T div = (a - mod) / b;
  if (mod != 0 && (b < 0) != (mod < 0)) div -= (T)1;
  if (div == 0) return expr_copysign((T)0, a / b);
  T fl = expr_floor(div);
  if (div - fl > (T)0.5) fl += (T)1;
  return fl;
}
template <typename T>
__host__ __device__ inline T expr_mod_f(T a, T b) {
  T mod = expr_fmod(a, b);
  if (mod != 0 && (b < 0) != (mod < 0)) mod += b;
  return mod;
}
// integers, by a non-zero divisor, rounding towards minus infinity (unsigned negation: no overflow)
__host__ __device__ inline int64_t expr_floordiv_i(int64_t a, int64_t b) {
  if (b == -1) return (int64_t)(0 - (uint64_t)a);
  const int64_t q = a / b, r = a % b;
  return (r != 0 && (r < 0) != (b < 0)) ? q - 1 : q;
}
__host__ __device__ inline int64_t expr_mod_i(int64_t a, int64_t b) {
  if (b == -1) return 0;
  const int64_t r = a % b;
  return (r != 0 && (r < 0) != (b < 0)) ? r + b : r;
}

__host__ __device__ inline double expr_math(int op, double x) {
  switch (op) {
    case NVT_EXPR_ROUND: return rint(x);  // half to even
    case NVT_EXPR_FLOOR: return floor(x);
    case NVT_EXPR_CEIL: return ceil(x);
    case NVT_EXPR_SQRT: return sqrt(x);
    case NVT_EXPR_LOG: return log(x);
    case NVT_EXPR_LOG1P: return log1p(x);
    case NVT_EXPR_LOG2: return log2(x);
    case NVT_EXPR_LOG10: return log10(x);
    case NVT_EXPR_EXP: return exp(x);
    case NVT_EXPR_EXPM1: return expm1(x);
    case NVT_EXPR_SIN: return sin(x);
    case NVT_EXPR_COS: return cos(x);
    default: return tanh(x);
  }
}
__host__ __device__ inline float expr_math(int op, float x) {
  switch (op) {
    case NVT_EXPR_ROUND: return rintf(x);
    case NVT_EXPR_FLOOR: return floorf(x);
    case NVT_EXPR_CEIL: return ceilf(x);
    case NVT_EXPR_SQRT: return sqrtf(x);
    case NVT_EXPR_LOG: return logf(x);
    case NVT_EXPR_LOG1P: return log1pf(x);
    case NVT_EXPR_LOG2: return log2f(x);
    case NVT_EXPR_LOG10: return log10f(x);
    case NVT_EXPR_EXP: return expf(x);
    case NVT_EXPR_EXPM1: return expm1f(x);
    case NVT_EXPR_SIN: return sinf(x);
    case NVT_EXPR_COS: return cosf(x);
    default: return tanhf(x);
  }
}

// ops whose result has the class of their operands (NVT_EXPR_ADD .. NVT_EXPR_TANH)
template <typename T>
__host__ __device__ inline T expr_arith(int op, T a, T b) {
  if constexpr (ExprType<T>::is_int) {
    const uint64_t ua = (uint64_t)a, ub = (uint64_t)b;
    switch (op) {
      case NVT_EXPR_ADD: return (int64_t)(ua + ub);
      case NVT_EXPR_SUB: return (int64_t)(ua - ub);
      case NVT_EXPR_MUL: return (int64_t)(ua * ub);
      case NVT_EXPR_FLOORDIV: return expr_floordiv_i(a, b);
      case NVT_EXPR_MOD: return expr_mod_i(a, b);
      case NVT_EXPR_NEG: return (int64_t)(0 - ua);
      case NVT_EXPR_ABS: return a < 0 ? (int64_t)(0 - ua) : a;
      case NVT_EXPR_MAX: return a > b ? a : b;
      case NVT_EXPR_MIN: return a < b ? a : b;
      case NVT_EXPR_CLIPLO: return a < b ? b : a;
      case NVT_EXPR_CLIPHI: return a > b ? b : a;
      case NVT_EXPR_SIGN: return (a > 0) - (a < 0);
      case NVT_EXPR_NOT: return ~a;
      case NVT_EXPR_AND: return a & b;
      case NVT_EXPR_OR: return a | b;
      default: return a ^ b;  // NVT_EXPR_XOR
    }
  } else {
    switch (op) {
      case NVT_EXPR_ADD: return a + b;
      case NVT_EXPR_SUB: return a - b;
      case NVT_EXPR_MUL: return a * b;
      case NVT_EXPR_DIV: return a / b;
      case NVT_EXPR_FLOORDIV: return expr_floordiv_f(a, b);
      case NVT_EXPR_MOD: return expr_mod_f(a, b);
      case NVT_EXPR_NEG: return -a;
      case NVT_EXPR_ABS: return expr_copysign(a, (T)1);
      case NVT_EXPR_MAX: return (a != a || b != b) ? expr_nan<T>() : (a > b ? a : b);  // NaN-propagating
      case NVT_EXPR_MIN: return (a != a || b != b) ? expr_nan<T>() : (a < b ? a : b);
      case NVT_EXPR_CLIPLO: return a < b ? b : a;  // a NaN stays; -0.0 is not below a bound of 0.0
      case NVT_EXPR_CLIPHI: return a > b ? b : a;
      case NVT_EXPR_SIGN: return a != a ? a : (T)((a > 0) - (a < 0));
      default: return expr_math(op, a);
    }
  }
}

// the six comparisons and isnan: a NaN compares False, `!=` True
template <typename T>
__host__ __device__ inline bool expr_pred(int op, T a, T b) {
  switch (op) {
    case NVT_EXPR_EQ: return a == b;
    case NVT_EXPR_NE: return a != b;
    case NVT_EXPR_LT: return a < b;
    case NVT_EXPR_LE: return a <= b;
    case NVT_EXPR_GT: return a > b;
    case NVT_EXPR_GE: return a >= b;
    default: return a != a;  // NVT_EXPR_ISNAN
  }
}

// float -> int64 as the x86 conversion does it: truncation, INT64_MIN for NaN and out of range
template <typename T>
__host__ __device__ inline int64_t expr_to_i64(T x) {
  return (x >= (T)-9223372036854775808.0 && x < (T)9223372036854775808.0) ? (int64_t)x : INT64_MIN;
}

// slot of class `from` -> slot of class `to` (NVT_EXPR_CAST); `shift` wraps an integer result
__host__ __device__ inline uint64_t expr_cast(uint64_t s, int from, int to, int shift) {
  if (from == NVT_EXPR_F64 || from == NVT_EXPR_F32) {
    const double x = from == NVT_EXPR_F64 ? expr_from_slot<double>(s) : (double)expr_from_slot<float>(s);
    switch (to) {
      case NVT_EXPR_I64: return (uint64_t)expr_wrap(expr_to_i64(x), shift);
      case NVT_EXPR_BOOL: return x != 0;  // (a NaN is True)
      case NVT_EXPR_F32: return from == NVT_EXPR_F32 ? s : expr_to_slot((float)x);
      default: return expr_to_slot(x);
    }
  }
  const int64_t v = (int64_t)s;  // I64 or BOOL
  switch (to) {
    case NVT_EXPR_I64: return (uint64_t)expr_wrap(v, shift);
    case NVT_EXPR_BOOL: return v != 0;
    case NVT_EXPR_F32: return expr_to_slot((float)v);  // one rounding
    default: return expr_to_slot((double)v);
  }
}

// ---- the program as data: what both entries check before they run it ---------------------------
inline bool expr_op_is_pred(int op) { return op >= NVT_EXPR_EQ && op <= NVT_EXPR_ISNAN; }
inline bool expr_op_is_unary(int op) {
  return op == NVT_EXPR_NEG || op == NVT_EXPR_ABS || op == NVT_EXPR_SIGN || op == NVT_EXPR_NOT ||
         op == NVT_EXPR_ISNAN || (op >= NVT_EXPR_ROUND && op <= NVT_EXPR_TANH);
}
inline bool expr_op_int_only(int op) { return op >= NVT_EXPR_NOT && op <= NVT_EXPR_XOR; }
inline bool expr_op_float_only(int op) {
  return op == NVT_EXPR_DIV || op == NVT_EXPR_ISNAN || (op >= NVT_EXPR_ROUND && op <= NVT_EXPR_TANH);
}
__host__ __device__ inline int expr_wrap_shift(int wrap) { return wrap ? 64 - wrap : 0; }

// class an input column is loaded as: float64 (NaN under a cleared bit) when it has a bitmap
inline int expr_load_class(int dtype, bool has_valid) {
  if (has_valid) return NVT_EXPR_F64;
  switch (dtype) {
    case NVT_F32: return NVT_EXPR_F32;
    case NVT_F64: return NVT_EXPR_F64;
    case NVT_EXPR_DT_BOOL: return NVT_EXPR_BOOL;
    default: return NVT_EXPR_I64;
  }
}
inline bool expr_dtype_known(int dtype) { return dtype >= NVT_F32 && dtype <= NVT_EXPR_DT_BOOL; }
inline int expr_dtype_bytes(int dtype) {
  switch (dtype) {
    case NVT_F64: case NVT_I64: return 8;
    case NVT_F32: case NVT_I32: return 4;
    case NVT_I16: return 2;
    default: return 1;
  }
}

// One instruction on one element's registers: the host twin's inner step, and the statement of
// what the kernel's run8 does to each of its 8 elements.
inline void expr_step(const nvt_expr_instr &in, const uint64_t *consts, uint64_t *reg) {
  const int op = in.op, shift = expr_wrap_shift(in.wrap);
  uint64_t a = reg[in.a];
  uint64_t b = (in.flags & NVT_EXPR_B_CONST) ? consts[in.b] : reg[in.b & 15];
  if (in.flags & NVT_EXPR_SWAP) {
    const uint64_t t = a;
    a = b;
    b = t;
  }
  const uint64_t c = (in.flags & NVT_EXPR_C_CONST) ? consts[in.c] : reg[in.c & 15];
  uint64_t r;
  if (op == NVT_EXPR_SELECT) {
    r = a ? b : c;
  } else if (op == NVT_EXPR_CAST) {
    r = expr_cast(a, in.b, in.cls, shift);
  } else if (expr_op_is_pred(op)) {
    switch (in.cls) {
      case NVT_EXPR_F64: r = expr_pred(op, expr_from_slot<double>(a), expr_from_slot<double>(b)); break;
      case NVT_EXPR_F32: r = expr_pred(op, expr_from_slot<float>(a), expr_from_slot<float>(b)); break;
      default: r = expr_pred(op, (int64_t)a, (int64_t)b); break;
    }
  } else {
    switch (in.cls) {
      case NVT_EXPR_F64: r = expr_to_slot(expr_arith(op, expr_from_slot<double>(a), expr_from_slot<double>(b))); break;
      case NVT_EXPR_F32: r = expr_to_slot(expr_arith(op, expr_from_slot<float>(a), expr_from_slot<float>(b))); break;
      default: r = (uint64_t)expr_wrap(expr_arith(op, (int64_t)a, (int64_t)b), shift); break;
    }
    if (in.cls == NVT_EXPR_BOOL) r &= 1;  // NOT of a bool is the other bool
  }
  reg[in.dst] = r;
}

}  // namespace nvt
