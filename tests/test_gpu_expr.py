"""The column-expression kernel (csrc/nvt_expr.hip) against numpy / pandas in float64: tails, bitmap
edges and the grid stride, every load and store dtype, the caps, and LambdaOp / Filter on it."""
import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

UFUNCS = (np.log, np.log1p, np.log2, np.log10, np.exp, np.expm1, np.sin, np.cos, np.tanh)
# Largest ulp distance from numpy float64 of the torch elementwise path these ufuncs took before the
# expression kernel, on math_inputs() (profiles/lambda_fused_notes.md: how it was measured).  The
# kernel may exceed it by one ulp: the same library routine under another contraction of the
# multiply-adds around it.
EAGER_ULP = {
    "float64": dict(log=1, log1p=1, log2=1, log10=1, exp=1, expm1=2, sin=1, cos=1, tanh=1),
    "float32": dict(log=2, log1p=1, log2=1, log10=2, exp=1, expm1=1, sin=1, cos=1, tanh=1),
}


def _sizes():
    from nvtabular_amd.kernels_expr import T

    return [0, 1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17]


def math_inputs(dtype):
    from nvtabular_amd.kernels_expr import T

    rng = np.random.default_rng(5)
    return rng.uniform(0.01, 20.0, 2 * T + 17).astype(dtype)


def ulps(got, exp):
    """Largest distance in units of the last place between two float arrays of one dtype."""
    it = np.int64 if got.dtype == np.float64 else np.int32
    a, b = (np.where(v.view(it) < 0, np.iinfo(it).min - v.view(it), v.view(it)).astype(np.int64) for v in (got, exp))
    return int(np.abs(a - b).max())


def _series(x, ok=None):
    from nvtabular_amd import kernels_expr as KE
    from nvtabular_amd.series import DeviceSeries

    valid = None if ok is None else torch.from_numpy(np.packbits(ok, bitorder="little")).cuda()
    return DeviceSeries(KE.leaf(torch.from_numpy(x).cuda(), valid))


def _launches():
    from nvtabular_amd import kernels as K

    return K.STATS.get("expr_eval", 0)


def _same(got, exp):
    got, exp = got.cpu().numpy(), np.asarray(exp)
    assert got.dtype == exp.dtype
    np.testing.assert_array_equal(got, exp)     # (NaN equals NaN here)
    if got.dtype.kind == "f":
        np.testing.assert_array_equal(np.signbit(got), np.signbit(exp))


@pytest.mark.parametrize("n", range(12))
def test_tails_bitmap_edges_and_grid_stride(n):
    n = _sizes()[n]
    rng = np.random.default_rng(n)
    x = rng.integers(-9, 9, n)
    ok = rng.random(n) < 0.6
    w = rng.normal(0, 4, n).astype("float32")
    host = pd.Series(np.where(ok, x.astype("float64"), np.nan))
    before = _launches()
    _same((_series(x, ok).fillna(0).clip(0) * 2.5 + 1).values, host.fillna(0).clip(0) * 2.5 + 1)
    _same((_series(x) > 3).astype("int8").values, (pd.Series(x) > 3).astype("int8"))
    _same((_series(w, ~ok) * _series(x)).values, pd.Series(np.where(~ok, w.astype("float64"), np.nan)) * x)
    assert _launches() - before == 3


@pytest.mark.parametrize("load, udf", [
    ("bool", lambda c: ~c),                             # -> bool
    ("uint8", lambda c: c + 1),                         # -> int64
    ("int8", lambda c: c * 2),                          # -> int8
    ("int16", lambda c: c + 1),                         # -> int16
    ("int32", lambda c: c - 1),                         # -> int32
    ("int64", lambda c: c.astype("float32") * 0.5),     # -> float32
    ("float32", lambda c: c * c),
    ("float64", lambda c: -c),
])
def test_every_load_and_store_dtype(load, udf):
    from nvtabular_amd.kernels_expr import T

    x = np.random.default_rng(3).integers(-100, 100, T + 9).astype(load)
    _same(udf(_series(x)).values, udf(pd.Series(x.astype("int64") if load == "uint8" else x)))


def test_sixteen_instructions_over_eight_inputs_and_an_unaligned_view():
    from nvtabular_amd import kernels_expr as KE
    from nvtabular_amd.series import DeviceSeries
    from nvtabular_amd.kernels_expr import T

    rng = np.random.default_rng(8)
    cols = [rng.normal(0, 1, 2 * T + 18) for k in range(8)]
    dev = [DeviceSeries(torch.from_numpy(c).cuda()[1:]) for c in cols]      # offset views: not 16-byte aligned
    assert all(d._x.data_ptr() % 16 for d in dev)
    total, exp = dev[0], pd.Series(cols[0][1:])
    for d, c in zip(dev[1:], cols[1:]):
        total, exp = total + d, exp + pd.Series(c[1:])
    prog, _, inputs = KE.compile_program((total * 2)._x)
    assert len(prog) == 16 and len(inputs) == 8       # 8 loads, 7 adds, 1 multiply
    _same((total * 2).values, exp * 2)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("fn", UFUNCS)
def test_transcendental_ops_stay_within_one_ulp_of_the_eager_path(fn, dtype):
    x = math_inputs(dtype)
    got = fn(_series(x)).values.cpu().numpy()
    exp = fn(x.astype("float64")).astype(dtype)
    assert got.dtype == exp.dtype
    d = ulps(got, exp)
    print(f"{fn.__name__} {dtype}: {d} ulp")
    assert d <= EAGER_ULP[dtype][fn.__name__] + 1


def _frame(n=3000):
    rng = np.random.default_rng(2)
    df = pd.DataFrame({"a": rng.integers(0, 9, n).astype("int64"), "other": rng.integers(1, 50, n).astype("int32"),
                       "x": pd.array(rng.lognormal(0, 2, n).astype("float32"), dtype="Float32"),   # nullable
                       "b": rng.normal(0, 1, n), "s": rng.choice(["ab", "cde"], n)})
    df.loc[rng.random(n) < 0.2, "x"] = pd.NA
    df.loc[rng.random(n) < 0.3, "b"] = np.nan
    return df


@pytest.mark.parametrize("udf, cols, launches, path", [
    (lambda col: np.log(col.fillna(0).clip(0) + 1), ["x"], 1, "device"),
    (lambda col: (col > 3).astype("int8"), ["a", "other"], 2, "device"),
    (lambda col, df: col / df["other"], ["a", "x"], 2, "device"),
    (lambda col: (col ** 2 + 1) * 0.5, ["a", "b"], None, "device"),        # ** runs eagerly, in the middle
    (lambda col: col.str.slice(0, 1), ["s"], 0, "host"),
])
def test_lambdaop_runs_a_udf_as_one_launch_per_column(udf, cols, launches, path):
    from inspect import signature

    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    df = _frame()
    op = ops.LambdaOp(udf)
    before = _launches()
    out = op.transform(_selector(cols), DeviceFrame.from_pandas(df))
    df["x"] = df["x"].astype("float64")        # pandas' view of the nullable column: NaN
    assert op.last_path == path
    if launches is not None:
        assert _launches() - before == launches
    for c in cols:
        exp = udf(df[c], df) if len(signature(udf).parameters) == 2 else udf(df[c])
        got = out[c].to_pandas(c)
        if exp.dtype == object:
            assert got.tolist() == exp.tolist()
        else:
            assert got.dtype == exp.dtype
            np.testing.assert_allclose(got.to_numpy(), exp.to_numpy(), rtol=4 * 2.0 ** -52)   # (log: a few ulp)


def _selector(cols):
    from nvtabular_amd.selector import ColumnSelector

    return ColumnSelector(cols)


def test_filter_predicate_is_one_launch_and_keeps_pandas_rows():
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    df = _frame()[["a", "b", "other"]]
    op = ops.Filter(lambda d: (d["a"] > 1) & d["b"].notna())
    before = _launches()
    out = op.transform(_selector(["a", "b", "other"]), DeviceFrame.from_pandas(df))
    assert op.last_path == "device" and _launches() - before == 1
    exp = df[(df["a"] > 1) & df["b"].notna()].reset_index(drop=True)
    pd.testing.assert_frame_equal(out.to_pandas(), exp, check_dtype=False)
