"""nunique_reference.seg_nunique against pandas' groupby(k)[c].nunique() (dropna=True) on a small
frame, for every dtype the kernel takes, with and without nulls."""
import numpy as np
import pandas as pd
import pytest

import nunique_reference as R

DTYPES = ["float32", "float64", "int32", "int64", "uint8", "bool"]


def _frame(dtype, nulls, seed):
    rng = np.random.default_rng(seed)
    n, ngroups = 400, 23
    key = rng.integers(-1, ngroups, n)                # -1: a null key
    key[key == 7] = 8                                 # group 7 has no rows at all
    if dtype == "bool":
        v = rng.random(n) < 0.5
    elif dtype.startswith("float"):
        v = rng.integers(-4, 5, n).astype(dtype) / 2
        v[rng.random(n) < 0.15] = np.nan
        v[rng.random(n) < 0.05] = np.inf
        v[rng.random(n) < 0.05] = -0.0
    else:
        v = rng.integers(0, 9, n).astype(dtype)
    ok = rng.random(n) >= 0.25 if nulls else None
    if nulls:
        ok[key == 3] = False                          # a group of nulls only
    return key, v, ok, ngroups


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_pandas_nunique(dtype, nulls):
    key, v, ok, ngroups = _frame(dtype, nulls, DTYPES.index(dtype) * 2 + nulls)
    order = np.argsort(np.where(key < 0, ngroups, key), kind="stable")
    rng = np.random.default_rng(5)
    for a in np.unique(key):                          # rows of a group in any order
        sl = np.flatnonzero(key[order] == a)
        order[sl] = rng.permutation(order[sl])
    words = R.words_of(np.where(key < 0, ngroups, key)[order], order)
    got = R.seg_nunique(words, ngroups, [v], [ok])[0]

    s = pd.Series(v).astype("float64" if dtype != "bool" else "object")
    if ok is not None:
        s[~ok] = np.nan
    df = pd.DataFrame({"k": pd.array(np.where(key < 0, 0, key), dtype="Int64"), "v": s})
    df.loc[key < 0, "k"] = pd.NA
    exp = df.groupby("k")["v"].nunique().reindex(range(ngroups), fill_value=0).to_numpy()
    np.testing.assert_array_equal(got, exp)
    assert got[7] == 0 and (not nulls or got[3] == 0)


def test_reference_edge_values():
    i64 = np.iinfo(np.int64)
    ends = np.array([i64.max, i64.max - 1, i64.max, i64.min + 1, i64.min, i64.max - 1, i64.min, i64.min + 1])
    zeros = np.array([-0.0, 0.0, np.inf, -np.inf, np.inf, np.nan, 0.0, np.nan])
    words = R.words_of(np.zeros(8, np.int64))
    got = R.seg_nunique(words, 1, [ends, zeros], [None, None])
    assert got.tolist() == [[4], [3]]
    assert R.seg_nunique(words[:0], 3, [ends], [None]).tolist() == [[0, 0, 0]]
