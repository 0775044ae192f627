"""The column-expression program on the CPU (nvt_expr_eval_host, the twin of the gfx950 kernel):
UDFs recorded by DeviceSeries over host columns against the same UDF on pandas."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

torch = pytest.importorskip("torch")

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
N = 43   # not a multiple of 8: the last bitmap byte is partial
_F = [np.nan, 0.0, -0.0, np.inf, -np.inf, 0.5, -0.5, 1.5, 2.5, -2.5, 3.5, 1 / 3, 0.1, -0.1, 3.0, -3.0, 7.25, -7.25,
      1e-300, 1e300, -1e300, 100.0, 4.0, -4.0, 1.0, -1.0, 2.0 ** 53, 6.0, -6.0, 9.0, 0.7, -0.7, 1e-5]
_I = [0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8, 9, -9, 10, -10, 100, -100, 12345, -12345]
# float32 pairs whose product or sum rounds differently through a float64 intermediate
_F32 = [1.0000001, 16777216.0, 0.1, 0.2, 0.3, 1e-20, 3.4e38, 1.1754944e-38, 1 / 3, 2 / 3, 33554430.0, 1e7]


def _fit(values, dtype):
    with np.errstate(over="ignore"):     # (1e300 as float32 is inf)
        return np.resize(np.array(values, dtype=dtype), N)


def _columns():
    rng = np.random.default_rng(11)
    ok = rng.random(N) < 0.7
    return {
        "f": (_fit(_F, "float64"), None),
        "g": (_fit(_F[::-1], "float64"), None),
        "s": (_fit(_F32 + _F, "float32"), None),
        "t": (_fit(_F32[::-1] + [3.0, -3.0], "float32"), None),
        "i": (_fit([I32.min, I32.max, I32.max - 1, I32.min + 1] + _I, "int32"), None),
        "l": (_fit([I64.min, I64.max, I64.max - 1, I64.min + 1] + _I, "int64"), None),
        "h": (_fit([-128, 127] + _I[:20], "int8"), None),
        "b": (_fit([True, False, False, True, True], "bool"), None),
        "n": (_fit(_I, "int64"), ok),          # nullable: float64 with NaN under a cleared bit
        "m": (_fit(_F32, "float32"), ~ok),
    }


def _both(udf):
    from nvtabular_amd import kernels_expr as KE
    from nvtabular_amd.series import DeviceSeries

    host, dev = {}, {}
    for name, (x, ok) in _columns().items():
        host[name] = pd.Series(x if ok is None else np.where(ok, x.astype("float64"), np.nan))
        valid = None if ok is None else torch.from_numpy(np.packbits(ok, bitorder="little"))
        dev[name] = DeviceSeries(KE.leaf(torch.from_numpy(x), valid, host=True), name)
    with np.errstate(all="ignore"):
        return udf(dev).values.numpy(), np.asarray(udf(host))


def _bits(x):
    """Bit patterns with every NaN made the same one."""
    if x.dtype.kind != "f":
        return x
    return np.where(np.isnan(x), np.nan, x).view("uint64" if x.dtype == np.float64 else "uint32")


EXACT = {
    "nullable_add": lambda d: d["n"] + 1,
    "nullable_f32_is_f64": lambda d: d["m"] * 3,
    "fillna_clip": lambda d: d["n"].fillna(0).clip(0) * 2.5,
    "clip_upper_only": lambda d: d["f"].clip(upper=2.5),
    "clip_both_int": lambda d: d["i"].clip(-5, 5),
    "int32_wrap_add": lambda d: d["i"] + 1,
    "int32_wrap_mul": lambda d: d["i"] * 3,
    "int32_abs_neg": lambda d: abs(d["i"]) - (-d["i"]),
    "int8_wrap": lambda d: d["h"] + 100,
    "int64_extremes": lambda d: (d["l"] + 1) * 3 - abs(d["l"]),
    "int_floordiv_3": lambda d: d["l"] // 3,
    "int_floordiv_neg3": lambda d: d["i"] // -3,
    "int_mod_3": lambda d: d["i"] % 3,
    "int_mod_neg3": lambda d: d["l"] % -3,
    "float_floordiv": lambda d: d["f"] // 3,
    "float_floordiv_neg3": lambda d: d["g"] // -3.0,
    "int_float_scalar": lambda d: d["i"] * 0.5,
    "int32_plus_int64": lambda d: d["i"] + d["l"],
    "f32_stays_f32": lambda d: d["s"] * d["t"] + d["s"],
    "f32_scalar": lambda d: (d["s"] + 0.1) * 3,
    "f32_with_int64_is_f64": lambda d: d["s"] * d["l"],
    "truediv": lambda d: d["l"] / d["f"],
    "truediv_scalar": lambda d: 3 / d["i"] + d["f"] / 3,
    "rsub": lambda d: 5 - d["f"],
    "where_scalar": lambda d: d["f"].where(d["g"] > 0, -1.0),
    "where_default_on_int": lambda d: d["i"].where(d["i"] > 0),
    "where_series": lambda d: d["f"].where(d["b"], d["g"]),
    "mask_scalar": lambda d: d["l"].mask(d["l"] < 0, 0),
    "mask_series": lambda d: d["f"].mask(d["f"].isna(), d["g"]),
    "cmp_nan": lambda d: ((d["f"] < d["g"]) | (d["f"] >= d["g"])) ^ (d["f"] == d["f"]),
    "ne_nan": lambda d: (d["n"] != 1) & ~(d["n"] == 1),
    "notna_threshold": lambda d: ((d["n"] > 3) & d["n"].notna()).astype("int8"),
    "threshold_int8": lambda d: (d["l"] > 3).astype("int8"),
    "bitwise": lambda d: (d["i"] & 255) | (d["i"] ^ 7) | ~d["i"],
    "maximum_nan": lambda d: np.maximum(d["f"], d["g"]) - np.minimum(d["f"], d["g"]),
    "round_floor_ceil": lambda d: d["f"].round() + np.floor(d["g"]) - np.ceil(d["f"]),
    "sign_square_sqrt": lambda d: np.sign(d["f"]) * np.square(d["g"]) + np.sqrt(d["f"]),
    "casts": lambda d: d["l"].astype("int32").astype("float32").astype("float64") + d["b"].astype("int64"),
    "shared_subexpression": lambda d: (d["f"] + d["g"]) * (d["f"] + d["g"]),
}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_ops_are_bit_equal_to_pandas(name):
    got, exp = _both(EXACT[name])
    assert got.dtype == exp.dtype
    np.testing.assert_array_equal(_bits(got), _bits(exp))


def test_float_remainder_follows_torch():
    """torch.remainder keeps the dividend's sign on a zero result, numpy takes the divisor's: the
    values are compared, the sign of zero is not."""
    for udf in (lambda d: d["f"] % 3, lambda d: d["g"] % -3.0):
        got, exp = _both(udf)
        np.testing.assert_array_equal(_bits(got + 0.0), _bits(exp + 0.0))


@pytest.mark.parametrize("fn", [np.log, np.log1p, np.log2, np.log10, np.exp, np.expm1, np.sin, np.cos, np.tanh])
def test_transcendental_ops_on_the_host(fn):
    """libm against numpy: a few ulp (the device bound is measured in test_gpu_expr.py)."""
    got, exp = _both(lambda d: fn(d["n"].fillna(0.5) / 7) + fn(d["i"] % 5 + 1))
    assert got.dtype == exp.dtype == np.float64
    np.testing.assert_allclose(got, exp, rtol=8 * 2.0 ** -52, equal_nan=True)


def test_a_dag_beyond_the_caps_is_cut_and_still_right():
    def udf(d):
        x = d["f"]
        for k in range(1, 90):     # 90 instructions, and 20 constants
            x = x * 0.5 + (k % 20)
        return x

    got, exp = _both(udf)
    np.testing.assert_array_equal(_bits(got), _bits(exp))


def _refusal(prog, ninstr=None, out_dtype=None):
    from nvtabular_amd import _lib

    lib = _lib.load()
    x = np.arange(8, dtype=np.int64)
    out = np.zeros(8, dtype=np.float64)
    arr = (_lib.ExprInstr * max(len(prog), 1))(*[_lib.ExprInstr(*p) for p in prog])
    rc = lib.nvt_expr_eval_host(arr, len(prog) if ninstr is None else ninstr, (C.c_uint64 * 16)(),
                                _lib.ptr_array([x.ctypes.data]), (C.c_int32 * 1)(_lib.NVT_I64), _lib.ptr_array([None]),
                                1, 8, out.ctypes.data, _lib.NVT_I64 if out_dtype is None else out_dtype)
    return rc, lib.nvt_last_error()


def test_the_c_entry_refuses_bad_programs():
    from nvtabular_amd import _lib

    op, I, F = _lib.EXPR_OP, _lib.EXPR_I64, _lib.EXPR_F64
    load = (op["load"], I, 0, 0)                       # (op, cls, dst, a, b, c, flags, wrap)
    for prog, word in [
        ([load] + [(op["add"], I, 0, 0, 0)] * 64, b"1 .. 64 instructions"),
        ([load, (op["neg"], I, 16, 0)], b"16 registers"),
        ([load, (op["add"], F, 1, 0, 0)], b"class mismatch"),
        ([load, (op["log"], I, 1, 0)], b"class mismatch"),
        ([load, (200, I, 1, 0)], b"unknown opcode"),
        ([load, (op["add"], I, 1, 0, 16, 0, _lib.EXPR_B_CONST)], b"16 constants"),
        ([load, (op["mod"], I, 1, 0, 0, 0, _lib.EXPR_B_CONST)], b"non-zero constant"),
        ([(op["load"], I, 0, 1)], b"input index"),
        ([(op["neg"], I, 0, 1)], b"before it is written"),
    ]:
        rc, msg = _refusal(prog)
        assert rc == _lib.NVT_EINVAL and word in msg, (prog, msg)
    rc, msg = _refusal([load], out_dtype=_lib.NVT_F64)
    assert rc == _lib.NVT_EINVAL and b"out_dtype" in msg
    assert _refusal([load])[0] == 0
