"""list_reference.py against independent formulations, on the CPU: the slice against the vectorised
numpy restatement of test_gpu_session_ops.py (clamp arithmetic instead of Python slicing), the
length fold against numpy, the lag against pandas' groupby(...).shift and a per-row loop."""
import numpy as np
import pandas as pd
import pytest

import list_reference as R
from test_gpu_session_ops import _vector_expected

INT64_MAX, INT64_MIN = R.INT64_MAX, R.INT64_MIN


def _frame(seed, n, maxlen, first=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, n)
    lens[rng.random(n) < 0.2] = 0
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off + first, rng


def test_pack_bits():
    ok = np.array([1, 0, 1, 1, 0, 0, 0, 0, 1], dtype=bool)
    got = R.pack_bits(ok)
    assert got.tolist() == [0b00001101, 0b00000001, 0, 0, 0, 0, 0, 0]
    assert R.pack_bits(np.zeros(0, bool)).size == 0
    assert R.pack_bits(np.ones(64, bool)).tolist() == [255] * 8
    assert R.pack_bits(np.ones(65, bool)).tolist() == [255] * 8 + [1] + [0] * 7


@pytest.mark.parametrize("start,end", [(0, 10), (1, 11), (-10, INT64_MAX), (-10, -2), (-5, 0), (0, INT64_MAX),
                                       (1, -1), (3, 2), (INT64_MIN, INT64_MAX), (INT64_MIN, 4), (7, INT64_MIN),
                                       (INT64_MAX, INT64_MAX), (-1, INT64_MAX), (0, 1), (0, 0)])
@pytest.mark.parametrize("first", [0, 17])
def test_slice_matches_the_vectorised_statement(start, end, first):
    off, rng = _frame(5, 300, 12, first)
    nl = int(off[-1] - off[0])
    vals = rng.integers(-1000, 1000, nl).astype(np.int32)
    valid = rng.random(nl) < 0.7
    exp_off, src = _vector_expected(off - first, (start, end), None)
    got_v, got_ok, got_off = R.slice_rows(vals, valid, off, start, end)
    np.testing.assert_array_equal(got_off, exp_off)
    np.testing.assert_array_equal(R.slice_offsets(off, start, end), exp_off)
    np.testing.assert_array_equal(got_v, vals[src])
    np.testing.assert_array_equal(got_ok, valid[src])
    # padded: the widest sliced row, and one leaf more
    for width in (int(np.diff(exp_off).max()), int(np.diff(exp_off).max()) + 1):
        p_off, p_src = _vector_expected(off - first, (start, end), width)
        got_v, got_ok, got_off = R.slice_rows(vals, valid, off, start, end, width, -7)
        np.testing.assert_array_equal(got_off, p_off)
        np.testing.assert_array_equal(got_v, np.where(p_src < 0, np.int32(-7), vals[np.maximum(p_src, 0)]))
        np.testing.assert_array_equal(got_ok, np.where(p_src < 0, True, valid[np.maximum(p_src, 0)]))
        got_v, got_ok, _ = R.slice_rows(vals, None, off, start, end, width, -7)
        assert got_ok.all() and len(got_ok) == len(got_v)


def test_slice_offsets_of_rows_no_memory_could_hold():
    off = [5, 5 + (1 << 33), 5 + (1 << 33), 5 + (1 << 33) + (1 << 40), 8 + (1 << 33) + (1 << 40)]
    assert R.slice_offsets(off, -10, INT64_MAX).tolist() == [0, 10, 10, 20, 23]
    assert R.slice_offsets(off, 3, 5).tolist() == [0, 2, 2, 4, 4]
    assert R.slice_offsets(off, 1, -1).tolist() == [0, (1 << 33) - 2, (1 << 33) - 2, (1 << 33) + (1 << 40) - 4,
                                                    (1 << 33) + (1 << 40) - 3]
    assert R.len_minmax(off) == (0, 1 << 40)


def test_len_minmax():
    off, _ = _frame(9, 500, 40, 3)
    d = np.diff(off)
    assert R.len_minmax(off) == (int(d.min()), int(d.max()))
    assert R.len_minmax([4]) == (INT64_MAX, INT64_MIN)
    assert R.len_minmax([4, 4]) == (0, 0)


def _lag_loop(keys, x, valid, shift):
    """One row at a time, scalars only."""
    n = len(x)
    out = np.full(n, np.nan, dtype=np.float32)
    for i in range(n):
        j = i - shift
        if not 0 <= j < n:
            continue
        if any((kv is not None and not (kv[i] and kv[j])) or not (k[i] == k[j]) for k, kv in keys):
            continue
        if valid is not None and not (valid[i] and valid[j]):
            continue
        if x.dtype == np.float32:
            out[i] = x[i] - x[j]
        elif x.dtype == np.float64:
            out[i] = np.float32(x[i] - x[j])
        else:
            out[i] = np.float32(float(int(x[i])) - float(int(x[j])))
    return out


def _same(a, b):
    assert a.dtype == b.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))                  # NaN positions
    np.testing.assert_array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


X_DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint8]


def _x(dt, n, rng):
    if dt == np.uint8:
        return rng.integers(0, 256, n).astype(dt)
    if dt == np.int32:
        return rng.integers(-(2 ** 31), 2 ** 31, n).astype(dt)
    if dt == np.int64:
        return (rng.integers(-(2 ** 62), 2 ** 62, n) | 1).astype(dt)          # beyond 2^53, odd
    return (rng.standard_normal(n) * 1e6 + 1e9).astype(dt)                   # differences that round in float32


@pytest.mark.parametrize("dt", X_DTYPES)
@pytest.mark.parametrize("shift", [0, 1, -1, 2, -3, 64, -64, 65, INT64_MAX, INT64_MIN])
def test_lag_matches_the_loop(dt, shift):
    rng = np.random.default_rng(3)
    n = 65
    x = _x(dt, n, rng)
    valid = rng.random(n) < 0.8
    kf = rng.integers(0, 3, n).astype(np.float64)
    kf[rng.random(n) < 0.1] = np.nan
    keys = [(rng.integers(0, 2, n).astype(np.int32), rng.random(n) < 0.9), (kf, None)]
    with np.errstate(all="ignore"):
        for ks in ([], keys[:1], keys):
            for v in (None, valid):
                _same(R.lag(ks, x, v, shift), _lag_loop(ks, x, v, shift))


@pytest.mark.parametrize("dt", X_DTYPES)
@pytest.mark.parametrize("shift", [1, -1, 2, 5])
def test_lag_matches_pandas(dt, shift):
    """pandas: x - groupby(keys)[x].shift(shift), rows whose key is null form no group.  The
    operator compares row i with row i - shift, so the two agree where every group is one run of
    adjacent rows: the frame is ordered by its keys, as a session frame is."""
    rng = np.random.default_rng(11)
    n = 400
    x = _x(dt, n, rng)
    k1 = np.sort(rng.integers(0, 4, n)).astype(np.int64)
    k2 = rng.integers(0, 3, n).astype(np.float64)
    k2[rng.random(n) < 0.1] = np.nan
    order = np.lexsort((k2, k1))                                             # NaN last inside every k1
    k2 = k2[order]
    df = pd.DataFrame({"k1": k1, "k2": k2, "x": x})
    exp = (df["x"] - df.groupby(["k1", "k2"])["x"].shift(shift)).to_numpy().astype(np.float32)
    _same(R.lag([(k1, None), (k2, None)], x, None, shift), exp)
    exp = (df["x"] - df.groupby("k1")["x"].shift(shift)).to_numpy().astype(np.float32)
    _same(R.lag([(k1, None)], x, None, shift), exp)
    exp = (df["x"] - df["x"].shift(shift)).to_numpy().astype(np.float32)
    _same(R.lag([], x, None, shift), exp)
