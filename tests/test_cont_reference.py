"""The numpy references of cont_reference.py against the pinned pandas oracle, on the CPU.

The GPU matrix (test_gpu_cont_kernels.py) compares every kernel with these references; this file
is what keeps that comparison from being made against a reference that is itself wrong.  Small
frames, with the edge values the GPU matrix uses."""
import math

import numpy as np
import pandas as pd
import pytest

import cont_reference as R
import oracle as O

F32 = np.finfo(np.float32)
F64 = np.finfo(np.float64)
I32 = np.iinfo(np.int32)
I64 = np.iinfo(np.int64)
TS_NS = 1_700_000_000_123_456_789          # a nanosecond timestamp, not a float64

FLOAT_EDGES = {
    "float32": np.array([0.0, -0.0, np.inf, -np.inf, F32.smallest_subnormal, -F32.smallest_subnormal,
                         F32.tiny, F32.max, -F32.max, 1.5, -2.25, 3.0, np.nan, 1e-3, 7.0], dtype=np.float32),
    "float64": np.array([0.0, -0.0, np.inf, -np.inf, F64.smallest_subnormal, -F64.smallest_subnormal,
                         F64.tiny, F64.max, -F64.max, 1.5, -2.25, 3.0, np.nan, 1e-3, 7.0], dtype=np.float64),
}
INT_EDGES = {
    "int32": np.array([0, 1, -1, I32.min, I32.max, 7, -300, 299, 12345, -99999], dtype=np.int32),
    "int64": np.array([0, 1, -1, I64.min, I64.max, I32.min, I32.max, 2**53 + 1, -(2**53 + 1), TS_NS],
                      dtype=np.int64),
}


def _frame(dtype):
    """(pandas column for the oracle, values, null) with a few nulls; an integer column is a
    nullable pandas Int column whose null slots hold a large value in ``values``."""
    if dtype in FLOAT_EDGES:
        x = FLOAT_EDGES[dtype]
        return pd.Series(x), x, None
    x = INT_EDGES[dtype].copy()
    null = np.zeros(x.size, dtype=bool)
    null[[5, 8]] = True
    s = pd.Series(pd.array(x, dtype=dtype.capitalize()))
    s[null] = pd.NA
    x[null] = np.iinfo(x.dtype).max       # arbitrary bytes under a null
    return s, x, null


def _oracle_values(s, out_dtype):
    """Oracle column -> (numpy values in out_dtype with 0 / NaN on missing rows, missing rows)."""
    na = s.isna().to_numpy()
    if np.dtype(out_dtype).kind == "f":
        return s.astype(out_dtype).to_numpy(dtype=out_dtype, na_value=np.nan), na
    return s.fillna(0).to_numpy(dtype=out_dtype), na


def test_int64_clip_is_exact():
    """Clip(min_value=0) on int64 values a float64 cannot hold: the oracle leaves them alone."""
    x = np.array([2**53 + 1, TS_NS, 2**63 - 1, -5, I64.min], dtype=np.int64)
    exp = O.clip_transform(pd.DataFrame({"x": x}), ["x"], min_value=0)["x"].to_numpy()
    np.testing.assert_array_equal(exp, np.array([2**53 + 1, TS_NS, 2**63 - 1, 0, 0], dtype=np.int64))
    R.assert_bits_equal(R.clip(x, None, None, 0, None, np.int64), exp)
    # the float64 round trip the kernel used to make is NOT the oracle
    assert int(np.float64(x[0])) == 2**53 and int(np.float64(x[1])) == 1_700_000_000_123_456_768


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("bounds", [(0, None), (None, 3), (-2, 3), (-(2**53), 2**53), (1.5, None)])
def test_clip_vs_oracle(dtype, bounds):
    s, x, null = _frame(dtype)
    lo, hi = bounds
    if dtype.startswith("int") and (lo, hi) == (-(2**53), 2**53) and dtype == "int32":
        lo, hi = I32.min, I32.max      # bounds that no int32 value reaches
    integral = all(b is None or float(b) == int(b) for b in bounds)
    out_dtype = dtype if (dtype.startswith("float") or integral) else "float64"
    if not integral and dtype.startswith("int"):
        # pandas refuses to put 1.5 into a nullable Int column; the float bound goes with a float64
        # frame, which is what ops.Clip promotes such a column to
        s = s.astype("Float64").astype("float64")
    ref = O.clip_transform(pd.DataFrame({"x": s}), ["x"], lo, hi)["x"]
    exp, na = _oracle_values(ref, out_dtype)
    got = R.clip(x, null, None, lo, hi, out_dtype)
    np.testing.assert_array_equal(R.null_rows(x, null), na)
    R.assert_bits_equal(got, exp, f"clip {dtype} {bounds}")


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
def test_fill_clip_log_vs_oracle(dtype):
    s, x, null = _frame(dtype)
    df = pd.DataFrame({"x": s})
    ref = O.fill_missing(df.copy(), ["x"], 0)
    ref = O.clip_transform(ref, ["x"], min_value=0)
    ref = O.logop_transform(ref, ["x"])["x"].to_numpy(dtype=np.float32)
    got = R.log1p_f32(x, null, 0, 0, None)
    assert not np.isnan(got).any() and not np.isnan(ref).any()
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_array_equal(got[~fin], ref[~fin].astype(np.float64))     # +inf stays +inf
    # the project's float32 log bound (test_gpu_parity.test_fill_clip_log_vs_oracle)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-6, atol=1e-7)


def test_log_special_points():
    x = np.array([0.0, -1.0, -2.0, np.inf, np.nan, 5.0], dtype=np.float64)
    null = np.array([0, 0, 0, 0, 0, 1], dtype=bool)
    got = R.log1p_f32(x, null)
    ref = O.logop_transform(pd.DataFrame({"x": np.where(null, np.nan, x)}), ["x"])["x"].to_numpy()
    assert got[0] == 0.0 and got[1] == -np.inf and np.isnan(got[2]) and got[3] == np.inf
    assert np.isnan(got[4]) and np.isnan(got[5])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(got[:2], ref[:2].astype(np.float64))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("fill", [None, 0, 7])
def test_moments_vs_oracle(dtype, fill):
    rng = np.random.default_rng(3)
    s, x, null = _frame(dtype)
    if dtype.startswith("float"):
        # finite values only: the oracle's sums of +-inf / max are NaN or inf by summation order
        x = np.concatenate([x[np.isfinite(x) & (np.abs(x) < 1e30)], [np.nan],
                            rng.normal(size=50).astype(dtype)]).astype(dtype)
        s = pd.Series(x)
    else:
        keep = np.abs(x.astype(np.float64)) < 2.0**40
        s, x, null = s[keep].reset_index(drop=True), x[keep], null[keep]
    df = pd.DataFrame({"x": s})
    if fill is not None:
        df = O.fill_missing(df, ["x"], fill)
    ref = O.custom_moments([df], ["x"]).loc["x"]
    cnt, tot, sq = R.moments(x, null, fill)
    v = R.moment_terms(x, null, fill)
    assert isinstance(cnt, int) and cnt == int(ref["count"])
    # any summation order is within n * 2**-53 * sum(|terms|) of the exact sum (fsum)
    u = cnt * 2.0**-53
    # (the oracle sums a float32 column in float32, moments.py:70: its own error is n * 2**-24)
    us = cnt * 2.0**-24 if dtype == "float32" else u
    assert abs(tot - float(ref["sum"])) <= us * math.fsum(np.abs(v).tolist())
    assert abs(sq - float(ref["sum2"])) <= u * math.fsum((v * v).tolist())
    mean, std = R.finalize_moments(cnt, float(ref["sum"]), float(ref["sum2"]))
    R.assert_bits_equal(np.array([mean, std]), np.array([float(ref["mean"]), float(ref["std"])]))


def test_moments_integer_valued_data_is_exact():
    rng = np.random.default_rng(5)
    x = rng.integers(-(2**20) + 1, 2**20, 4099).astype(np.float64)
    x[::17] = np.nan
    ref = O.custom_moments([pd.DataFrame({"x": x})], ["x"]).loc["x"]
    cnt, tot, sq = R.moments(x, None, None)
    assert (cnt, tot, sq) == (int(ref["count"]), float(ref["sum"]), float(ref["sum2"]))
    assert R.finalize_moments(0, 0.0, 0.0) == pytest.approx((np.nan, np.nan), nan_ok=True)
    m1 = R.finalize_moments(1, 3.0, 9.0)
    assert m1[0] == 3.0 and np.isnan(m1[1])
    assert R.finalize_moments(4, 8.0, 16.0) == (2.0, 0.0)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
def test_minmax_vs_oracle(dtype):
    s, x, null = _frame(dtype)
    if dtype.startswith("float"):
        s = pd.Series(x)
    mins, maxs = O.minmax_fit([pd.DataFrame({"x": s})], ["x"])
    lo, hi = R.minmax(x, null)
    assert lo == float(mins["x"]) and hi == float(maxs["x"])
    # two partitions folded = one fit over both
    a, b = R.minmax(x[:4], None if null is None else null[:4]), None
    b = R.minmax(x[4:], None if null is None else null[4:], prev=a)
    assert b == (lo, hi)
    e = R.minmax(np.array([np.nan, 3.0]), np.array([False, True]))
    assert np.isnan(e[0]) and np.isnan(e[1])
    assert R.minmax(np.array([], dtype=dtype), None, prev=(1.0, 2.0)) == (1.0, 2.0)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("fill", [0, 7, -3])
def test_pure_fill_vs_oracle(dtype, fill):
    s, x, null = _frame(dtype)
    ref = O.fill_missing(pd.DataFrame({"x": s}), ["x"], fill, add_binary_cols=True)
    got, filled = R.fill_normalize(x, null, fill, False, 0.0, 1.0, dtype)
    np.testing.assert_array_equal(filled.astype(bool), ref["x_filled"].to_numpy(dtype=bool))
    R.assert_bits_equal(got, ref["x"].to_numpy(dtype=dtype), f"fill {dtype}")
    # no fill: NaN (float output) / 0 (integer output)
    got, filled2 = R.fill_normalize(x, null, None, False, 0.0, 1.0, dtype)
    np.testing.assert_array_equal(filled, filled2)
    m = filled.astype(bool)
    assert (np.isnan(got[m]).all() if dtype.startswith("float") else (got[m] == 0).all())
    R.assert_bits_equal(got[~m], np.asarray(x)[~m], "untouched rows")


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
@pytest.mark.parametrize("out_dtype", ["float64", "float32"])
@pytest.mark.parametrize("std", [2.5, 0.0, 1e-3])
def test_fill_normalize_vs_oracle(dtype, out_dtype, std):
    s, x, null = _frame(dtype)
    mean = 1.25
    df = pd.DataFrame({"x": s})
    if dtype.startswith("int"):
        # the reference normalises a plain numpy column; nulls become NaN in float64, where every
        # int32 and these int64 values convert the way the kernel converts them
        df = pd.DataFrame({"x": s.astype("Float64").astype("float64")})
    with np.errstate(all="ignore"):
        for fill in (None, 0, 7):
            d = df.copy() if fill is None else O.fill_missing(df.copy(), ["x"], fill)
            ref = O.normalize_transform(d, ["x"], {"x": mean}, {"x": std}, out_dtype)["x"].to_numpy()
            got, filled = R.fill_normalize(x, null, fill, True, mean, std, out_dtype)
            R.assert_bits_equal(got, ref, f"normalize {dtype}->{out_dtype} std={std} fill={fill}")
            np.testing.assert_array_equal(filled.astype(bool), R.null_rows(x, null))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
def test_bucketize_vs_oracle(dtype):
    s, x, null = _frame(dtype)
    for b in ([], [0.0], [-1.0, 0.0, 3.0], [-np.inf, 0.0, 0.0, 1.5, np.inf],
              [np.nextafter(1.5, 0), 1.5, np.nextafter(1.5, 2)]):
        got = R.bucketize(x, null, b)
        m = R.null_rows(x, null)
        assert got.dtype == np.int32 and (got[m] == len(b)).all()
        if len(b):
            # the oracle digitizes plain numpy values; NaN sorts last there as well
            vals = np.where(m, np.nan, x.astype(np.float64))
            ref = O.bucketize(pd.DataFrame({"x": vals}), {"x": b})["x"].to_numpy()
            np.testing.assert_array_equal(got, ref)
        else:
            assert (got == 0).all()
    x = np.array([np.nextafter(1.5, 0), 1.5, np.nextafter(1.5, 2)])
    np.testing.assert_array_equal(R.bucketize(x, None, [1.5]), [0, 1, 1])


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_hash_bucket_vs_oracle(dtype):
    s, x, null = _frame(dtype)
    for nb in (1, 7, 2**31 - 1):
        ref = O.hash_bucket_op(pd.DataFrame({"x": s}), nb, ["x"])["x"].to_numpy()
        got = R.hash_bucket(x, null, nb)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(R.hash64(x, null), O.nvt_hash64(np.where(null, 0, x)))


def test_widen_popcount():
    b = np.array([True, False, True, True, False, True, True, True, True], dtype=bool)
    np.testing.assert_array_equal(R.widen(b), b.astype(np.int64))
    np.testing.assert_array_equal(R.widen(INT_EDGES["int32"]), INT_EDGES["int32"].astype(np.int64))
    assert R.popcount(b) == 7
    bits = R.pack_bits(b)
    assert bits.tolist() == [0b11101101, 0b1]


@pytest.mark.parametrize("kfold", [1, 3])
@pytest.mark.parametrize("p_smooth", [20, 0])
def test_te_apply_vs_oracle(tmp_path, kfold, p_smooth):
    """Both te_apply forms against target_encoding_transform (float64 output, so that only the
    arithmetic is compared): group ids and statistics are taken from the oracle's own fit."""
    rng = np.random.default_rng(11)
    n = 600
    cat = rng.integers(0, 12, n).astype(np.int64)
    y = rng.normal(size=n).round(2)
    fit = pd.DataFrame({"c": cat[:400], "y": y[:400]})
    stats, means = O.target_encoding_fit([fit], ["c"], ["y"], str(tmp_path), kfold=kfold, fold_seed=None)
    df = pd.DataFrame({"c": np.concatenate([cat[400:], [99, 100]])})      # two unseen keys
    ref = O.target_encoding_transform(df.copy(), ["c"], ["y"], stats, means, kfold=kfold, fold_seed=None,
                                      p_smooth=p_smooth, out_dtype=np.float64)["TE_c_y"].to_numpy()
    agg = pd.read_parquet(stats["c"])
    agg.columns = ["c", "count", "sum"]
    agg = agg.sort_values("c", ignore_index=True)
    g = pd.Series(np.arange(len(agg)), index=agg["c"]).reindex(df["c"]).fillna(-1).to_numpy(dtype=np.int64)
    y_mean = means["y"]
    if kfold == 1:
        got, s, c, use = R.te_apply(g, None, agg["sum"], agg["count"], None, None, p_smooth, y_mean)
    else:
        fold = O.add_fold(len(df), kfold, None).astype(np.int64)
        af = pd.read_parquet(stats["__fold___c"])
        af.columns = ["f", "c", "count", "sum"]
        # sparse form: one row per (fold, key) pair that was seen
        key = pd.MultiIndex.from_frame(af[["f", "c"]])
        gf = pd.Series(np.arange(len(af)), index=key).reindex(
            pd.MultiIndex.from_arrays([fold, df["c"]])).fillna(-1).to_numpy(dtype=np.int64)
        got, s, c, use = R.te_apply(g, gf, agg["sum"], agg["count"], af["sum"], af["count"], p_smooth, y_mean)
        # dense form: [group, fold] tables, count 0 where the pair was not seen
        sf = np.zeros(len(agg) * kfold)
        cf = np.zeros(len(agg) * kfold, dtype=np.int64)
        pos = pd.Series(np.arange(len(agg)), index=agg["c"]).reindex(af["c"]).to_numpy() * kfold + af["f"].to_numpy()
        sf[pos], cf[pos] = af["sum"].to_numpy(), af["count"].to_numpy()
        got2, _, _, use2 = R.te_apply_folds(g, fold, kfold, agg["sum"], agg["count"], sf, cf, p_smooth, y_mean)
        np.testing.assert_array_equal(use, use2)
        R.assert_bits_equal(got2, got, "dense vs sparse fold statistics")
    assert use.any() and (~use).any()
    R.assert_bits_equal(got, ref, f"te_apply kfold={kfold} p={p_smooth}")
    assert np.all(R.te_bound(s[use], c[use], 20, y_mean) >= 0)


def test_gather():
    src = np.array([1.5, -2.75, 1e10, np.nan])
    g = np.array([0, -1, 2, 1, 3, -1], dtype=np.int64)
    out = R.gather(src, g, np.nan, np.float64)
    R.assert_bits_equal(out, np.array([1.5, np.nan, 1e10, -2.75, np.nan, np.nan]))
    np.testing.assert_array_equal(R.gather(src[:3], g[:4], 0, np.int64), [1, 0, 10**10, -2])
