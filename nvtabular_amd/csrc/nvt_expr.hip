// Column expressions: a UDF's expression DAG as ONE launch (include/nvt_hip.h nvt_expr_eval,
// nvtabular_amd/kernels_expr.py).
//
// expr_kernel: a workgroup is one wave and takes tiles of NVT_EXPR_TILE = 512 elements; a lane owns
//   8 consecutive elements, which is one byte of every bitmap and 16 bytes or more of every column
//   but the one-byte ones.  The program and the constants arrive by value in the kernel arguments:
//   decoding is scalar loads and one uniform switch per instruction, no lane diverges on it, and its
//   cost is spread over the lane's 8 elements (run8).
//   The register file is LDS, rf[register][element][lane] of 8-byte slots: a register index is data,
//   and VGPRs indexed by data mean either scratch or a switch over 16 registers around every
//   operand.  In LDS the index is address arithmetic, consecutive lanes hit consecutive banks, and
//   the wave needs no barrier since nobody else sees its slots.  The launch asks for as many
//   registers as the program names (4 KiB each), so a short program leaves room for many waves.
//   Loads and stores: a full lane whose column is 16-byte aligned moves its 8 elements as 16-byte
//   words (8 bytes for one-byte types); the tail and unaligned columns go element by element.
// nvt_expr_eval_host: the same program, element by element, through expr_step (nvt_expr.hpp).
#include "nvt_common.hpp"
#include "nvt_expr.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr int kLaneElems = 8;
constexpr int kExprBlock = kWave;  // one wave
static_assert(kLaneElems * kExprBlock == NVT_EXPR_TILE, "tile = 8 elements of 64 lanes");

struct ExprArgs {
  nvt_expr_instr prog[NVT_EXPR_MAX_INSTR];
  uint64_t consts[NVT_EXPR_MAX_CONSTS];
  const void *in[NVT_EXPR_MAX_INPUTS];
  const uint8_t *valid[NVT_EXPR_MAX_INPUTS];
  uint8_t in_dtype[NVT_EXPR_MAX_INPUTS];
  uint8_t in_wide[NVT_EXPR_MAX_INPUTS];  // the column is 16-byte aligned
  void *out;
  int ninstr, out_dtype, out_wide;
};

__device__ __forceinline__ uint64_t &slot(uint64_t *rf, int reg, int e) {
  return rf[(reg * kLaneElems + e) * kExprBlock + threadIdx.x];
}

// 8 elements of T at p: 16-byte words (one 8-byte word for a one-byte T)
template <typename T>
__device__ __forceinline__ void load_wide(const T *__restrict__ p, T (&v)[kLaneElems]) {
  if constexpr (sizeof(T) == 1) {
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    memcpy(v, &w, 8);
  } else {
    constexpr int kWords = sizeof(T) * kLaneElems / 16;
    uint4 w[kWords];
#pragma unroll
    for (int k = 0; k < kWords; ++k) w[k] = reinterpret_cast<const uint4 *>(p)[k];
    memcpy(v, w, sizeof(w));
  }
}
template <typename T>
__device__ __forceinline__ void store_wide(T *__restrict__ p, const T (&v)[kLaneElems]) {
  if constexpr (sizeof(T) == 1) {
    uint2 w;
    memcpy(&w, v, 8);
    *reinterpret_cast<uint2 *>(p) = w;
  } else {
    constexpr int kWords = sizeof(T) * kLaneElems / 16;
    uint4 w[kWords];
    memcpy(w, v, sizeof(w));
#pragma unroll
    for (int k = 0; k < kWords; ++k) reinterpret_cast<uint4 *>(p)[k] = w[k];
  }
}

// the slot an element of a column of T becomes in a register of class `cls`
template <typename T>
__device__ __forceinline__ uint64_t to_class(T x, int cls) {
  if (cls == NVT_EXPR_F64) return expr_to_slot((double)x);
  if (cls == NVT_EXPR_F32) return expr_to_slot((float)x);
  if (cls == NVT_EXPR_BOOL) return x != 0;
  return (uint64_t)(int64_t)x;
}

// NVT_EXPR_LOAD: elements i0 .. i0 + 7 (those below n) of a column into register dst
template <typename T>
__device__ __forceinline__ void load8(uint64_t *rf, int dst, int cls, const void *__restrict__ col,
                                      const uint8_t *__restrict__ valid, bool wide, uint64_t i0, uint64_t n) {
  if (i0 >= n) return;
  const T *p = reinterpret_cast<const T *>(col) + i0;
  const unsigned bits = valid ? valid[i0 >> 3] : 0xffu;  // (i0 is a multiple of 8)
  const uint64_t null_slot = expr_to_slot((double)NAN);
  if (wide && i0 + kLaneElems <= n) {
    T v[kLaneElems];
    load_wide(p, v);
#pragma unroll
    for (int e = 0; e < kLaneElems; ++e) slot(rf, dst, e) = (bits >> e) & 1 ? to_class(v[e], cls) : null_slot;
  } else {
    const int live = (int)(n - i0 < kLaneElems ? n - i0 : kLaneElems);
    for (int e = 0; e < live; ++e) slot(rf, dst, e) = (bits >> e) & 1 ? to_class(p[e], cls) : null_slot;
  }
}

// the element a slot is stored as: an integer is truncated to the width of T
template <typename T>
__device__ __forceinline__ T from_class(uint64_t s) {
  return (T)(int64_t)s;
}
template <>
__device__ __forceinline__ float from_class<float>(uint64_t s) { return expr_from_slot<float>(s); }
template <>
__device__ __forceinline__ double from_class<double>(uint64_t s) { return expr_from_slot<double>(s); }

template <typename T>
__device__ __forceinline__ void store8(uint64_t *rf, int src, void *__restrict__ out, bool wide, uint64_t i0,
                                       uint64_t n) {
  if (i0 >= n) return;
  T *p = reinterpret_cast<T *>(out) + i0;
  if (wide && i0 + kLaneElems <= n) {
    T v[kLaneElems];
#pragma unroll
    for (int e = 0; e < kLaneElems; ++e) v[e] = from_class<T>(slot(rf, src, e));
    store_wide(p, v);
  } else {
    const int live = (int)(n - i0 < kLaneElems ? n - i0 : kLaneElems);
    for (int e = 0; e < live; ++e) p[e] = from_class<T>(slot(rf, src, e));
  }
}

template <int OP, typename T>
__device__ __forceinline__ uint64_t apply(uint64_t a, uint64_t b, int shift, int cls) {
  if constexpr (OP >= NVT_EXPR_EQ && OP <= NVT_EXPR_ISNAN) {
    return expr_pred<T>(OP, expr_from_slot<T>(a), expr_from_slot<T>(b));
  } else if constexpr (ExprType<T>::is_int) {
    const int64_t r = expr_wrap(expr_arith<int64_t>(OP, (int64_t)a, (int64_t)b), shift);
    return cls == NVT_EXPR_BOOL ? (uint64_t)(r & 1) : (uint64_t)r;
  } else {
    return expr_to_slot(expr_arith<T>(OP, expr_from_slot<T>(a), expr_from_slot<T>(b)));
  }
}

// one instruction on the lane's 8 elements; `in` and the constant are wave-uniform
template <int OP, typename T>
__device__ __forceinline__ void run8(uint64_t *rf, const nvt_expr_instr in, const uint64_t *consts) {
  constexpr bool unary = OP == NVT_EXPR_NEG || OP == NVT_EXPR_ABS || OP == NVT_EXPR_SIGN || OP == NVT_EXPR_NOT ||
                         OP == NVT_EXPR_ISNAN || (OP >= NVT_EXPR_ROUND && OP <= NVT_EXPR_TANH);
  const int shift = expr_wrap_shift(in.wrap);
  const bool swap = in.flags & NVT_EXPR_SWAP;  // op(b, a)
  if (unary) {
#pragma unroll 2
    for (int e = 0; e < kLaneElems; ++e) slot(rf, in.dst, e) = apply<OP, T>(slot(rf, in.a, e), 0, shift, in.cls);
  } else if (in.flags & NVT_EXPR_B_CONST) {
    const uint64_t b = consts[in.b];
#pragma unroll 2
    for (int e = 0; e < kLaneElems; ++e) {
      const uint64_t a = slot(rf, in.a, e);
      slot(rf, in.dst, e) = apply<OP, T>(swap ? b : a, swap ? a : b, shift, in.cls);
    }
  } else {
#pragma unroll 2
    for (int e = 0; e < kLaneElems; ++e) {
      const uint64_t a = slot(rf, in.a, e), b = slot(rf, in.b & 15, e);
      slot(rf, in.dst, e) = apply<OP, T>(swap ? b : a, swap ? a : b, shift, in.cls);
    }
  }
}

#define NVT_EXPR_CASE_INT(OP) \
  case OP: run8<OP, int64_t>(rf, in, args.consts); break;
#define NVT_EXPR_CASE_FLT(OP)                               \
  case OP:                                                  \
    if (in.cls == NVT_EXPR_F64) run8<OP, double>(rf, in, args.consts); \
    else run8<OP, float>(rf, in, args.consts);              \
    break;
#define NVT_EXPR_CASE_ALL(OP)                                                \
  case OP:                                                                   \
    if (in.cls == NVT_EXPR_F64) run8<OP, double>(rf, in, args.consts);       \
    else if (in.cls == NVT_EXPR_F32) run8<OP, float>(rf, in, args.consts);   \
    else run8<OP, int64_t>(rf, in, args.consts);                             \
    break;

__global__ __launch_bounds__(kExprBlock) void expr_kernel(const ExprArgs args, uint64_t n) {
  extern __shared__ __align__(16) uint64_t rf[];
  const uint64_t ntiles = (n + NVT_EXPR_TILE - 1) / NVT_EXPR_TILE;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t i0 = t * NVT_EXPR_TILE + (uint64_t)threadIdx.x * kLaneElems;
    for (int pc = 0; pc < args.ninstr; ++pc) {
      const nvt_expr_instr in = args.prog[pc];
      switch (in.op) {
        case NVT_EXPR_LOAD: {
          const void *col = args.in[in.a];
          const uint8_t *valid = args.valid[in.a];
          const bool wide = args.in_wide[in.a];
          switch (args.in_dtype[in.a]) {
            case NVT_F32: load8<float>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;
            case NVT_F64: load8<double>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;
            case NVT_I32: load8<int32_t>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;
            case NVT_I64: load8<int64_t>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;
            case NVT_I8: load8<int8_t>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;
            case NVT_I16: load8<int16_t>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;
            default: load8<uint8_t>(rf, in.dst, in.cls, col, valid, wide, i0, n); break;  // NVT_U8, bool
          }
          break;
        }
        case NVT_EXPR_CAST: {
          const int shift = expr_wrap_shift(in.wrap);
#pragma unroll 2
          for (int e = 0; e < kLaneElems; ++e) slot(rf, in.dst, e) = expr_cast(slot(rf, in.a, e), in.b, in.cls, shift);
          break;
        }
        case NVT_EXPR_SELECT: {
          const bool kb = in.flags & NVT_EXPR_B_CONST, kc = in.flags & NVT_EXPR_C_CONST;
          const uint64_t cb = args.consts[in.b & 15], cc = args.consts[in.c & 15];
#pragma unroll 2
          for (int e = 0; e < kLaneElems; ++e) {
            const uint64_t b = kb ? cb : slot(rf, in.b & 15, e), c = kc ? cc : slot(rf, in.c & 15, e);
            slot(rf, in.dst, e) = slot(rf, in.a, e) ? b : c;
          }
          break;
        }
        NVT_EXPR_CASE_ALL(NVT_EXPR_ADD)
        NVT_EXPR_CASE_ALL(NVT_EXPR_SUB)
        NVT_EXPR_CASE_ALL(NVT_EXPR_MUL)
        NVT_EXPR_CASE_FLT(NVT_EXPR_DIV)
        NVT_EXPR_CASE_ALL(NVT_EXPR_FLOORDIV)
        NVT_EXPR_CASE_ALL(NVT_EXPR_MOD)
        NVT_EXPR_CASE_ALL(NVT_EXPR_NEG)
        NVT_EXPR_CASE_ALL(NVT_EXPR_ABS)
        NVT_EXPR_CASE_ALL(NVT_EXPR_MAX)
        NVT_EXPR_CASE_ALL(NVT_EXPR_MIN)
        NVT_EXPR_CASE_ALL(NVT_EXPR_CLIPLO)
        NVT_EXPR_CASE_ALL(NVT_EXPR_CLIPHI)
        NVT_EXPR_CASE_ALL(NVT_EXPR_SIGN)
        NVT_EXPR_CASE_INT(NVT_EXPR_NOT)
        NVT_EXPR_CASE_INT(NVT_EXPR_AND)
        NVT_EXPR_CASE_INT(NVT_EXPR_OR)
        NVT_EXPR_CASE_INT(NVT_EXPR_XOR)
        NVT_EXPR_CASE_ALL(NVT_EXPR_EQ)
        NVT_EXPR_CASE_ALL(NVT_EXPR_NE)
        NVT_EXPR_CASE_ALL(NVT_EXPR_LT)
        NVT_EXPR_CASE_ALL(NVT_EXPR_LE)
        NVT_EXPR_CASE_ALL(NVT_EXPR_GT)
        NVT_EXPR_CASE_ALL(NVT_EXPR_GE)
        NVT_EXPR_CASE_FLT(NVT_EXPR_ISNAN)
        NVT_EXPR_CASE_FLT(NVT_EXPR_ROUND)
        NVT_EXPR_CASE_FLT(NVT_EXPR_FLOOR)
        NVT_EXPR_CASE_FLT(NVT_EXPR_CEIL)
        NVT_EXPR_CASE_FLT(NVT_EXPR_SQRT)
        NVT_EXPR_CASE_FLT(NVT_EXPR_LOG)
        NVT_EXPR_CASE_FLT(NVT_EXPR_LOG1P)
        NVT_EXPR_CASE_FLT(NVT_EXPR_LOG2)
        NVT_EXPR_CASE_FLT(NVT_EXPR_LOG10)
        NVT_EXPR_CASE_FLT(NVT_EXPR_EXP)
        NVT_EXPR_CASE_FLT(NVT_EXPR_EXPM1)
        NVT_EXPR_CASE_FLT(NVT_EXPR_SIN)
        NVT_EXPR_CASE_FLT(NVT_EXPR_COS)
        NVT_EXPR_CASE_FLT(NVT_EXPR_TANH)
        default: break;
      }
    }
    const int res = args.prog[args.ninstr - 1].dst;
    const bool wide = args.out_wide;
    switch (args.out_dtype) {
      case NVT_F32: store8<float>(rf, res, args.out, wide, i0, n); break;
      case NVT_F64: store8<double>(rf, res, args.out, wide, i0, n); break;
      case NVT_I32: store8<int32_t>(rf, res, args.out, wide, i0, n); break;
      case NVT_I64: store8<int64_t>(rf, res, args.out, wide, i0, n); break;
      case NVT_I16: store8<int16_t>(rf, res, args.out, wide, i0, n); break;
      default: store8<int8_t>(rf, res, args.out, wide, i0, n); break;  // NVT_I8, bool (0 / 1)
    }
  }
}

// Everything both entries refuse: caps, indices, classes, opcodes, dtypes.  *nregs: registers named.
int check_program(const nvt_expr_instr *program, int ninstr, const uint64_t *consts, const void *const *inputs,
                  const int32_t *input_dtypes, const uint8_t *const *input_valid, int ninputs, uint64_t n,
                  const void *out, int out_dtype, int *nregs) {
#define func_check(cond, msg)                            \
  do {                                                   \
    if (!(cond)) {                                       \
      set_error("nvt_expr_eval: instruction %d: %s", pc, msg); \
      return NVT_EINVAL;                                 \
    }                                                    \
  } while (0)
  int pc = 0;
  func_check(program, "null program");
  func_check(ninstr >= 1 && ninstr <= NVT_EXPR_MAX_INSTR, "ninstr must be 1 .. 64 instructions");
  func_check(ninputs >= 0 && ninputs <= NVT_EXPR_MAX_INPUTS, "ninputs must be 0 .. 8 input columns");
  func_check(ninputs == 0 || (inputs && input_dtypes && input_valid), "null inputs / input_dtypes / input_valid");
  for (int i = 0; i < ninputs; ++i) {
    func_check(expr_dtype_known(input_dtypes[i]), "unknown input dtype");
    func_check(n == 0 || inputs[i], "null input column");
    func_check((reinterpret_cast<uintptr_t>(inputs[i]) & (expr_dtype_bytes(input_dtypes[i]) - 1)) == 0,
               "input column not aligned to its element");
  }
  func_check(expr_dtype_known(out_dtype) && out_dtype != NVT_U8, "unknown out_dtype");
  func_check(n == 0 || out, "null out");
  func_check((reinterpret_cast<uintptr_t>(out) & (expr_dtype_bytes(out_dtype) - 1)) == 0,
             "out not aligned to its element");
  int cls[NVT_EXPR_MAX_REGS];
  for (int r = 0; r < NVT_EXPR_MAX_REGS; ++r) cls[r] = -1;
  int top = 0, any_const = 0;
  for (pc = 0; pc < ninstr; ++pc) {
    const nvt_expr_instr &in = program[pc];
    func_check(in.op < NVT_EXPR_NOPS, "unknown opcode");
    func_check(in.cls <= NVT_EXPR_BOOL, "unknown class");
    func_check(in.dst < NVT_EXPR_MAX_REGS, "register index beyond the 16 registers");
    func_check(in.wrap == 0 || in.wrap == 8 || in.wrap == 16 || in.wrap == 32, "wrap must be 0, 8, 16 or 32");
    func_check((in.flags & ~(NVT_EXPR_B_CONST | NVT_EXPR_C_CONST | NVT_EXPR_SWAP)) == 0, "unknown flags");
    int result = in.cls;
    if (in.op == NVT_EXPR_LOAD) {
      func_check(in.a < ninputs, "input index beyond ninputs");
      func_check(in.cls == expr_load_class(input_dtypes[in.a], input_valid[in.a] != nullptr),
                 "class mismatch: a load has the class of its column (float64 with a bitmap)");
    } else {
      func_check(in.a < NVT_EXPR_MAX_REGS, "register index beyond the 16 registers");
      func_check(cls[in.a] >= 0, "register read before it is written");
      const bool unary = in.op == NVT_EXPR_CAST || expr_op_is_unary(in.op);
      const int want = in.op == NVT_EXPR_SELECT ? NVT_EXPR_BOOL : in.op == NVT_EXPR_CAST ? (int)in.b : (int)in.cls;
      func_check(in.op != NVT_EXPR_CAST || in.b <= NVT_EXPR_BOOL, "unknown class");
      func_check(cls[in.a] == want, "class mismatch: operand a");
      func_check(in.op == NVT_EXPR_SELECT || !(in.flags & NVT_EXPR_C_CONST), "only NVT_EXPR_SELECT has an operand c");
      func_check(!unary || in.flags == 0, "a unary op takes no constant and no swap");
      func_check(in.op != NVT_EXPR_SELECT || !(in.flags & NVT_EXPR_SWAP), "NVT_EXPR_SELECT takes no swap");
      if (!unary) {
        if (in.flags & NVT_EXPR_B_CONST) {
          func_check(in.b < NVT_EXPR_MAX_CONSTS, "constant index beyond the 16 constants");
          any_const = 1;
        } else {
          func_check(in.b < NVT_EXPR_MAX_REGS, "register index beyond the 16 registers");
          func_check(cls[in.b] == in.cls, "class mismatch: operand b");
        }
      }
      if (in.op == NVT_EXPR_SELECT) {
        if (in.flags & NVT_EXPR_C_CONST) {
          func_check(in.c < NVT_EXPR_MAX_CONSTS, "constant index beyond the 16 constants");
          any_const = 1;
        } else {
          func_check(in.c < NVT_EXPR_MAX_REGS, "register index beyond the 16 registers");
          func_check(cls[in.c] == in.cls, "class mismatch: operand c");
        }
      } else if (in.op != NVT_EXPR_CAST) {
        func_check(!expr_op_float_only(in.op) || in.cls == NVT_EXPR_F64 || in.cls == NVT_EXPR_F32,
                   "class mismatch: the op takes floats only");
        func_check(!expr_op_int_only(in.op) || in.cls == NVT_EXPR_I64 || in.cls == NVT_EXPR_BOOL,
                   "class mismatch: the op takes integers and bools only");
        func_check(in.cls != NVT_EXPR_BOOL || expr_op_int_only(in.op) || in.op == NVT_EXPR_EQ || in.op == NVT_EXPR_NE,
                   "class mismatch: a bool takes NOT, AND, OR, XOR, EQ and NE only");
        if (in.cls == NVT_EXPR_I64 && (in.op == NVT_EXPR_FLOORDIV || in.op == NVT_EXPR_MOD))
          func_check(in.flags == NVT_EXPR_B_CONST && consts && consts[in.b] != 0,
                     "integer FLOORDIV / MOD take a non-zero constant divisor");
        if (expr_op_is_pred(in.op)) result = NVT_EXPR_BOOL;
      }
      func_check(in.wrap == 0 || result == NVT_EXPR_I64, "wrap on a result that is not NVT_EXPR_I64");
    }
    cls[in.dst] = result;
    if (in.dst + 1 > top) top = in.dst + 1;
  }
  pc = ninstr - 1;
  func_check(!any_const || consts, "null consts");
  const int rc = cls[program[pc].dst];
  const bool ok = rc == NVT_EXPR_F64   ? out_dtype == NVT_F64
                  : rc == NVT_EXPR_F32 ? out_dtype == NVT_F32
                  : rc == NVT_EXPR_BOOL
                      ? out_dtype == NVT_EXPR_DT_BOOL
                      : (out_dtype == NVT_I8 || out_dtype == NVT_I16 || out_dtype == NVT_I32 || out_dtype == NVT_I64);
  func_check(ok, "class mismatch: out_dtype cannot hold the result register");
#undef func_check
  *nregs = top;
  return NVT_OK;
}

template <typename T>
uint64_t host_load(const void *col, uint64_t i, int cls) {
  const T x = reinterpret_cast<const T *>(col)[i];
  if (cls == NVT_EXPR_F64) return expr_to_slot((double)x);
  if (cls == NVT_EXPR_F32) return expr_to_slot((float)x);
  if (cls == NVT_EXPR_BOOL) return x != 0;
  return (uint64_t)(int64_t)x;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_expr_eval(const nvt_expr_instr *program, int ninstr, const uint64_t *consts, const void *const *inputs,
                  const int32_t *input_dtypes, const uint8_t *const *input_valid, int ninputs, uint64_t n,
                  void *out, int out_dtype, void *stream) {
  if (n == 0) return NVT_OK;
  int nregs = 0;
  const int rc =
      check_program(program, ninstr, consts, inputs, input_dtypes, input_valid, ninputs, n, out, out_dtype, &nregs);
  if (rc != NVT_OK) return rc;
  ExprArgs args;
  memset(&args, 0, sizeof(args));
  memcpy(args.prog, program, sizeof(nvt_expr_instr) * ninstr);
  if (consts) memcpy(args.consts, consts, sizeof(args.consts));
  uint64_t bytes = expr_dtype_bytes(out_dtype);
  for (int i = 0; i < ninputs; ++i) {
    args.in[i] = inputs[i];
    args.valid[i] = input_valid[i];
    args.in_dtype[i] = (uint8_t)input_dtypes[i];
    args.in_wide[i] = (reinterpret_cast<uintptr_t>(inputs[i]) & 15) == 0;
    bytes += expr_dtype_bytes(input_dtypes[i]);
  }
  args.out = out;
  args.ninstr = ninstr;
  args.out_dtype = out_dtype;
  args.out_wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)nregs * kLaneElems * kExprBlock * sizeof(uint64_t);  // <= 64 KiB
  const unsigned grid = stream_grid((n + NVT_EXPR_TILE - 1) / NVT_EXPR_TILE, 1, 32);
  NVT_PROF("expr_eval", n * bytes, s);
  expr_kernel<<<grid, kExprBlock, lds, s>>>(args, n);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_expr_eval_host(const nvt_expr_instr *program, int ninstr, const uint64_t *consts,
                       const void *const *inputs, const int32_t *input_dtypes,
                       const uint8_t *const *input_valid, int ninputs, uint64_t n, void *out, int out_dtype) {
  if (n == 0) return NVT_OK;
  int nregs = 0;
  const int rc =
      check_program(program, ninstr, consts, inputs, input_dtypes, input_valid, ninputs, n, out, out_dtype, &nregs);
  if (rc != NVT_OK) return rc;
  uint64_t none[NVT_EXPR_MAX_CONSTS] = {0};
  if (!consts) consts = none;
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t reg[NVT_EXPR_MAX_REGS] = {0};
    for (int pc = 0; pc < ninstr; ++pc) {
      const nvt_expr_instr &in = program[pc];
      if (in.op != NVT_EXPR_LOAD) {
        expr_step(in, consts, reg);
        continue;
      }
      const uint8_t *valid = input_valid[in.a];
      if (valid && !((valid[i >> 3] >> (i & 7)) & 1)) {
        reg[in.dst] = expr_to_slot((double)NAN);
        continue;
      }
      const void *col = inputs[in.a];
      switch (input_dtypes[in.a]) {
        case NVT_F32: reg[in.dst] = host_load<float>(col, i, in.cls); break;
        case NVT_F64: reg[in.dst] = host_load<double>(col, i, in.cls); break;
        case NVT_I32: reg[in.dst] = host_load<int32_t>(col, i, in.cls); break;
        case NVT_I64: reg[in.dst] = host_load<int64_t>(col, i, in.cls); break;
        case NVT_I8: reg[in.dst] = host_load<int8_t>(col, i, in.cls); break;
        case NVT_I16: reg[in.dst] = host_load<int16_t>(col, i, in.cls); break;
        default: reg[in.dst] = host_load<uint8_t>(col, i, in.cls); break;
      }
    }
    const uint64_t r = reg[program[ninstr - 1].dst];
    switch (out_dtype) {
      case NVT_F32: reinterpret_cast<float *>(out)[i] = expr_from_slot<float>(r); break;
      case NVT_F64: reinterpret_cast<double *>(out)[i] = expr_from_slot<double>(r); break;
      case NVT_I32: reinterpret_cast<int32_t *>(out)[i] = (int32_t)(int64_t)r; break;
      case NVT_I64: reinterpret_cast<int64_t *>(out)[i] = (int64_t)r; break;
      case NVT_I16: reinterpret_cast<int16_t *>(out)[i] = (int16_t)(int64_t)r; break;
      default: reinterpret_cast<int8_t *>(out)[i] = (int8_t)(int64_t)r; break;
    }
  }
  return NVT_OK;
}

}  // extern "C"
