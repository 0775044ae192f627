"""Column expressions: the host driver of nvt_expr_eval (include/nvt_hip.h, csrc/nvt_expr.hip).

What a UDF does to its ``DeviceSeries`` (series.py) is recorded here as a DAG of ``Expr`` nodes and
evaluated by ONE launch when somebody needs the values.  The builders below (``arith``, ``truediv``,
``unary``, ``math``, ``where`` ...) carry the type rules the eager operators had: numpy's
``result_type`` between two columns, an integer column (op) a Python float gives float64, a scalar
otherwise takes the column's dtype.  What the program cannot express raises ``NotFusable`` and the
caller evaluates its operands and runs the torch operator as before.

``compile_program`` orders the DAG topologically (equal subexpressions are one node: nodes are
interned), gives every node a register that is freed after its last use, and collects the constants
table.  A DAG beyond the caps of the kernel (64 instructions, 8 inputs, 16 registers, 16 constants)
is cut: its operands are evaluated first and become inputs.
"""
from __future__ import annotations

import ctypes as C
import struct
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check
from .device import torch_dtype

T = _lib.EXPR_TILE   # elements a workgroup takes at a time (NVT_EXPR_TILE)

_F64, _F32, _BOOL = np.dtype("float64"), np.dtype("float32"), np.dtype("bool")
_DT_CODE = {np.dtype("float32"): _lib.NVT_F32, np.dtype("float64"): _lib.NVT_F64, np.dtype("int32"): _lib.NVT_I32,
            np.dtype("int64"): _lib.NVT_I64, np.dtype("uint8"): _lib.NVT_U8, np.dtype("int8"): _lib.NVT_I8,
            np.dtype("int16"): _lib.NVT_I16, _BOOL: _lib.EXPR_DT_BOOL}
_WRAP = {np.dtype("int8"): 8, np.dtype("int16"): 16, np.dtype("int32"): 32}
_CMP = ("eq", "ne", "lt", "le", "gt", "ge")


class NotFusable(Exception):
    """The expression program cannot express this: evaluate the operands and run it eagerly."""


class _Caps(Exception):
    """The DAG does not fit one program."""


def _cls(dtype) -> int:
    if dtype == _F64:
        return _lib.EXPR_F64
    if dtype == _F32:
        return _lib.EXPR_F32
    return _lib.EXPR_BOOL if dtype == _BOOL else _lib.EXPR_I64


class Const:
    """A scalar operand: the bit pattern of the class it is read in."""
    __slots__ = ("bits",)

    def __init__(self, value, dtype):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise NotFusable("scalar operand")
        if dtype == _F64:
            self.bits = struct.unpack("<Q", struct.pack("<d", float(value)))[0]
        elif dtype == _F32:
            self.bits = int(np.float32(value).view(np.uint32))
        elif dtype.kind == "i" and isinstance(value, (int, np.integer)):
            info = np.iinfo(dtype)
            if not info.min <= int(value) <= info.max:
                raise NotFusable("integer scalar outside the column's dtype")
            self.bits = int(value) & 0xFFFFFFFFFFFFFFFF
        else:
            raise NotFusable("scalar operand")

    @property
    def key(self):
        return ("k", self.bits)


class Expr:
    """A node of the DAG: ``op`` over ``args`` (Expr / Const) giving ``n`` elements of ``dtype``.
    A ``load`` node holds its column (``tensor``, ``valid``); so does a node once evaluated."""
    __slots__ = ("op", "args", "dtype", "n", "device", "swap", "size", "tensor", "valid", "key", "__weakref__")


_INTERN = weakref.WeakValueDictionary()


def _node(op, dtype, args=(), swap=False, tensor=None, valid=None, like=None) -> Expr:
    if tensor is not None:
        key = ("load", tensor.data_ptr(), valid.data_ptr() if valid is not None else 0, str(tensor.dtype),
               int(tensor.numel()), str(tensor.device))
    else:
        size = 1 + sum(a.size for a in args if isinstance(a, Expr))
        if size > _lib.EXPR_MAX_INSTR:   # (an upper bound: shared operands are counted twice)
            args = tuple(leaf(evaluate(a), host=True) if isinstance(a, Expr) and a.op != "load" else a for a in args)
        key = (op, str(dtype), swap) + tuple(a.key if isinstance(a, Const) else id(a) for a in args)
    e = _INTERN.get(key)
    if e is None:
        e = Expr()
        e.op, e.args, e.dtype, e.swap, e.tensor, e.valid, e.key = op, tuple(args), np.dtype(dtype), swap, tensor, valid, key
        e.size = 1 + sum(a.size for a in args if isinstance(a, Expr))
        e.n, e.device = (int(tensor.numel()), tensor.device) if tensor is not None else (like.n, like.device)
        _INTERN[key] = e
    return e


def leaf(t: torch.Tensor, valid=None, host=False) -> Expr:
    """A column as an input of the program; with a bitmap it reads as float64 with NaN under a
    cleared bit.  ``host``: a CPU tensor, evaluated by nvt_expr_eval_host (the CPU suite)."""
    from .device import numpy_dtype

    if not isinstance(t, torch.Tensor) or t.dim() != 1 or (t.device.type != "cuda" and not host):
        raise NotFusable("not a column on the device")
    try:
        dt = np.dtype(numpy_dtype(t.dtype))
    except Exception:
        raise NotFusable(f"{t.dtype} column") from None
    if dt not in _DT_CODE:
        raise NotFusable(f"{t.dtype} column")
    if not t.is_contiguous():
        t = t.contiguous()
    if valid is not None:
        dt = _F64
    elif dt == np.dtype("uint8"):
        dt = np.dtype("int64")
    return _node("load", dt, tensor=t, valid=valid)


def _same_shape(a: Expr, b: Expr):
    if a.n != b.n or a.device != b.device:
        raise NotFusable("operands of different length or device")


# ---- builders: the type rules of the eager operators ------------------------------------------------
def cast(a: Expr, dtype) -> Expr:
    dtype = np.dtype(dtype)
    if a.dtype == dtype:
        return a
    if dtype not in _DT_CODE or dtype == np.dtype("uint8"):
        raise NotFusable(f"cast to {dtype}")
    if a.dtype.kind == "f" and dtype.kind == "i":
        raise NotFusable("float to integer: the NaN check needs the values")
    return _node("cast", dtype, (a,), like=a)


def _promote(a: Expr, b):
    """(a, b) as the eager ``_bin`` hands them to the operator: b an Expr of a's dtype or a Const."""
    if isinstance(b, Expr):
        _same_shape(a, b)
        if a.dtype != b.dtype:
            if a.dtype == _BOOL or b.dtype == _BOOL:
                raise NotFusable("bool with a number")
            dt = np.result_type(a.dtype, b.dtype)
            a, b = cast(a, dt), cast(b, dt)
        return a, b
    if a.dtype == _BOOL:
        raise NotFusable("bool with a scalar")
    if isinstance(b, (float, np.floating)) and a.dtype.kind == "i":
        a = cast(a, _F64)
    return a, Const(b, a.dtype)


def arith(op: str, a: Expr, b, swap=False) -> Expr:
    """add / sub / mul / floordiv / mod / and / or / xor / max / min and the six comparisons;
    ``swap``: b (op) a."""
    a, b = _promote(a, b)
    kind = a.dtype.kind
    if op in ("and", "or", "xor"):
        if kind == "f":
            raise NotFusable("bitwise op on floats")
    elif op in _CMP:
        if kind == "b" and op not in ("eq", "ne"):
            raise NotFusable("ordering of bools")
        return _node(op, _BOOL, (a, b), swap, like=a)
    elif kind == "b":
        raise NotFusable("arithmetic on bools")
    if op in ("floordiv", "mod") and kind == "i" and (not isinstance(b, Const) or b.bits == 0 or swap):
        raise NotFusable("integer // or % by anything but a non-zero scalar")
    if op in ("add", "mul", "and", "or", "xor", "max", "min"):
        swap = False   # commutative: one node for both orders
    return _node(op, a.dtype, (a, b), swap, like=a)


def truediv(a: Expr, b, swap=False) -> Expr:
    """pandas' ``/``: float64 true division whatever the operands are."""
    if isinstance(b, Expr):
        a, b = _promote(a, b)
        b = cast(b, _F64)
    elif a.dtype == _BOOL:
        raise NotFusable("bool with a scalar")
    else:
        b = Const(b, _F64)
    a = cast(a, _F64)
    return _node("div", _F64, (a, b), swap, like=a)


def unary(op: str, a: Expr) -> Expr:
    """neg / abs / sign / not (bitwise on integers, logical on bools) / square."""
    kind = a.dtype.kind
    if op == "not":
        if kind == "f":
            raise NotFusable("~ on floats")
    elif kind == "b":
        raise NotFusable(f"{op} of bools")
    if op == "square":
        return _node("mul", a.dtype, (a, a), like=a)
    return _node(op, a.dtype, (a,), like=a)


def math(op: str, a: Expr) -> Expr:
    """sqrt, log ... tanh, floor, ceil, round: integers and bools are promoted to float64 first."""
    if a.dtype.kind != "f":
        a = cast(a, _F64)
    return _node(op, a.dtype, (a,), like=a)


def isna(a: Expr) -> Expr:
    if a.dtype.kind == "f":
        return _node("isnan", _BOOL, (a,), like=a)
    return _node("ne", _BOOL, (a, a), like=a)   # nothing else is ever null: all False


def select(cond: Expr, a, b, like: Expr) -> Expr:
    if cond.dtype != _BOOL:
        raise NotFusable("condition that is not bool")
    for x in (a, b):
        if isinstance(x, Expr):
            _same_shape(cond, x)
    return _node("select", like.dtype, (cond, a, b), like=like)


def fillna(a: Expr, value) -> Expr:
    return select(isna(a), Const(value, a.dtype), a, a)


def clip(a: Expr, lower, upper) -> Expr:
    if a.dtype == _BOOL or (lower is None and upper is None):
        raise NotFusable("clip")
    for op, bound in (("cliplo", lower), ("cliphi", upper)):
        if bound is None:
            continue
        if a.dtype.kind == "i" and not isinstance(bound, (int, np.integer)) or bound != bound:
            raise NotFusable("clip bound")
        a = _node(op, a.dtype, (a, Const(bound, a.dtype)), like=a)
    return a


def where(a: Expr, cond, other) -> Expr:
    """``a`` where ``cond`` holds, else ``other`` (a scalar or an Expr of a's dtype)."""
    if not isinstance(cond, Expr):
        raise NotFusable("condition")
    _same_shape(a, cond)
    if isinstance(other, Expr):
        if other.dtype != a.dtype:
            raise NotFusable("where between dtypes")
    else:
        if a.dtype == _BOOL:
            raise NotFusable("where on bools")
        if isinstance(other, (float, np.floating)) and a.dtype.kind == "i":
            a = cast(a, _F64)
        other = Const(other, a.dtype)
    return select(cond, a, other, a)


# ---- program ---------------------------------------------------------------------------------------------
def compile_program(root: Expr):
    """(instructions, constants, input nodes) of the DAG under ``root``; _Caps when it does not fit."""
    order, seen, uses = [], set(), {}
    stack = [(root, False)]
    while stack:
        e, done = stack.pop()
        if done:
            order.append(e)
            continue
        if id(e) in seen:
            continue
        seen.add(id(e))
        stack.append((e, True))
        if e.tensor is None:
            for x in e.args:
                if isinstance(x, Expr):
                    stack.append((x, False))
    for e in order:
        if e.tensor is None:
            for x in set(id(x) for x in e.args if isinstance(x, Expr)):
                uses[x] = uses.get(x, 0) + 1
    if len(order) > _lib.EXPR_MAX_INSTR:
        raise _Caps("instructions")
    free, reg, consts, inputs, prog = list(range(_lib.EXPR_MAX_REGS - 1, -1, -1)), {}, [], [], []

    def const(c):
        if c.bits not in consts:
            if len(consts) == _lib.EXPR_MAX_CONSTS:
                raise _Caps("constants")
            consts.append(c.bits)
        return consts.index(c.bits)

    for e in order:
        ins = _lib.ExprInstr()
        if e.tensor is not None:
            if len(inputs) == _lib.EXPR_MAX_INPUTS:
                raise _Caps("inputs")
            ins.op, ins.cls, ins.a = _lib.EXPR_OP["load"], _cls(e.dtype), len(inputs)
            inputs.append(e)
        else:
            ins.op, ins.cls = _lib.EXPR_OP[e.op], _cls(e.dtype if e.op in ("cast", "select") else e.args[0].dtype)
            ins.wrap = _WRAP.get(e.dtype, 0)
            ins.a = reg[id(e.args[0])]
            if e.op == "cast":
                ins.b = _cls(e.args[0].dtype)
            for x, field, flag in zip(e.args[1:], ("b", "c"), (_lib.EXPR_B_CONST, _lib.EXPR_C_CONST)):
                if isinstance(x, Const):
                    setattr(ins, field, const(x))
                    ins.flags |= flag
                else:
                    setattr(ins, field, reg[id(x)])
            if e.swap:
                ins.flags |= _lib.EXPR_SWAP
            for x in set(id(x) for x in e.args if isinstance(x, Expr)):   # a register ends with its last reader
                uses[x] -= 1
                if uses[x] == 0:
                    free.append(reg[x])
        if not free:
            raise _Caps("registers")
        ins.dst = reg[id(e)] = free.pop()
        prog.append(ins)
    return prog, consts, inputs


def run_program(prog, consts, columns, valids, n, out, host=False, stream=None):
    """nvt_expr_eval / nvt_expr_eval_host over the tensors ``columns`` (bitmaps ``valids``) into ``out``."""
    from .device import numpy_dtype

    arr = (_lib.ExprInstr * max(len(prog), 1))(*prog)
    cs = (C.c_uint64 * _lib.EXPR_MAX_CONSTS)(*consts)
    dts = (C.c_int32 * max(len(columns), 1))(*[_DT_CODE[np.dtype(numpy_dtype(t.dtype))] for t in columns])
    ins = _lib.ptr_array([t.data_ptr() for t in columns])
    vs = _lib.ptr_array([v.data_ptr() if v is not None else None for v in valids])
    args = (arr, len(prog), cs, ins, dts, vs, len(columns), n, out.data_ptr(),
            _DT_CODE[np.dtype(numpy_dtype(out.dtype))])
    if host:
        return _lib.load().nvt_expr_eval_host(*args)
    return _lib.load().nvt_expr_eval(*args, stream)


def evaluate(e: Expr) -> torch.Tensor:
    """The values of ``e``: one launch (none for a column handed through as it is)."""
    from . import kernels as K

    if e.tensor is not None and e.valid is None and np.dtype(e.dtype) == _np_dtype(e.tensor):
        return e.tensor
    try:
        prog, consts, inputs = compile_program(e)
    except _Caps:
        if all(not isinstance(a, Expr) or a.tensor is not None for a in e.args):
            raise
        for a in e.args:   # the operands first: each becomes an input
            if isinstance(a, Expr) and a.tensor is None:
                a.tensor = evaluate(a)
        prog, consts, inputs = compile_program(e)
    out = torch.empty(e.n, dtype=torch_dtype(e.dtype), device=e.device)
    columns, valids = [x.tensor for x in inputs], [x.valid for x in inputs]
    if e.device.type == "cuda":
        _lib.require_gpu()
        K.stat_add("expr_eval")
        check(run_program(prog, consts, columns, valids, e.n, out, stream=K.stream_ptr()), "nvt_expr_eval")
    else:
        check(run_program(prog, consts, columns, valids, e.n, out, host=True), "nvt_expr_eval_host")
    if e.tensor is None:
        e.tensor = out
    return out


def _np_dtype(t: torch.Tensor):
    from .device import numpy_dtype

    return np.dtype(numpy_dtype(t.dtype))
