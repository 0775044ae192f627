"""groupby_reference.py pinned to pandas (no GPU): ``table_groups`` / ``merge_groups`` equal
``df.groupby(keys, dropna=False, sort=True).agg(...)`` on nullable frames of one, two and three key
columns, ``lookup`` a left merge on the key columns, ``sort_key_order`` a chain of
``sort_values(kind="stable", na_position="last")`` from the least to the most significant column,
``order_rows`` + ``seg_aggregate`` the oracle's Groupby operator (list / first / last / sum / count
per group, in both directions) and a pandas groupby over the group ids.  The one place where the
reference departs from pandas on purpose -- the two int64 values next to the reserved null image
tie -- has a test of its own.  The kernel-level tests of test_gpu_groupby_kernels.py compare the
device with these references."""
import numpy as np
import pandas as pd
import pytest

import groupby_reference as R
import oracle as O

VAL_DTYPES = ["float32", "float64", "int32", "int64", "uint8", "bool"]
I64 = np.iinfo(np.int64)


def _keys(rng, n, nkeys):
    """nkeys int64 columns over few values (extremes among them) with ~15 % nulls each; the bytes
    under a null are a key of the column, 0 or anything."""
    pool = np.array([0, 1, -1, 7, I64.min, I64.max, 2**40, -(2**40)], np.int64)
    keys, valid = [], []
    for k in range(nkeys):
        col = pool[rng.integers(0, pool.size if k == 0 else 4, n)]
        ok = rng.random(n) >= 0.15
        col[~ok] = pool[rng.integers(0, pool.size, int((~ok).sum()))]
        keys.append(col)
        valid.append(ok)
    return keys, valid


def _values(rng, n, dtype, nulls=True):
    """(column, validity): multiples of 2^-4 for floats (with NaN), small integers otherwise."""
    if dtype.startswith("float"):
        v = (rng.integers(-2**14, 2**14, n) / 16.0).astype(dtype)
        v[rng.random(n) < 0.1] = np.nan
    elif dtype == "bool":
        v = rng.random(n) < 0.4
    elif dtype == "uint8":
        v = rng.integers(0, 256, n).astype(np.uint8)
    else:
        v = rng.integers(-1000, 1000, n).astype(dtype)
    return v, (rng.random(n) >= 0.2 if nulls else None)


def _f64_with_nan(v, valid):
    x = np.asarray(v).astype(np.float64)
    return x if valid is None else np.where(valid, x, np.nan)


def _key_frame(keys, valid):
    df = pd.DataFrame()
    for k, (col, ok) in enumerate(zip(keys, valid)):
        arr = pd.array(col, dtype="Int64")
        if ok is not None:
            arr[~ok] = pd.NA
        df[f"k{k}"] = arr
    return df


def _pandas_groups(keys, key_valid, vals, val_valid):
    """The pandas groupby(dropna=False) of the rows, as a dict in the layout and order of
    R.table_groups."""
    nk = len(keys)
    df = _key_frame(keys, key_valid)
    kcols = list(df.columns)
    df["first_ok"] = df["k0"].notna().astype(np.int64)
    agg = {"first_ok": ["size", "sum"]}
    for j, (v, w) in enumerate(zip(vals, val_valid)):
        df[f"v{j}"] = _f64_with_nan(v, w)
        df[f"q{j}"] = df[f"v{j}"] ** 2
        agg[f"v{j}"] = ["sum", "min", "max"]
        agg[f"q{j}"] = ["sum"]
    gb = df.groupby(kcols, dropna=False, sort=True).agg(agg).reset_index()
    nm = np.zeros(len(gb), np.int64)
    gk = []
    for k in range(nk):
        na = gb[f"k{k}"].isna().to_numpy()
        nm |= na.astype(np.int64) << k
        gk.append(gb[f"k{k}"].fillna(0).to_numpy(dtype=np.int64))
    f = lambda c, a: gb[(c, a)].to_numpy(dtype=np.float64)  # noqa: E731
    nv = len(vals)
    return R.sort_groups(dict(
        keys=gk, null_mask=nm.astype(np.uint8), size=gb[("first_ok", "size")].to_numpy(dtype=np.int64),
        count=gb[("first_ok", "sum")].to_numpy(dtype=np.int64),
        sum=[f(f"v{j}", "sum") for j in range(nv)], sumsq=[f(f"q{j}", "sum") for j in range(nv)],
        min=[f(f"v{j}", "min") for j in range(nv)], max=[f(f"v{j}", "max") for j in range(nv)]))


_same_groups = R.assert_same_groups


@pytest.mark.parametrize("nkeys", [1, 2, 3])
def test_table_groups_equals_pandas_groupby_dropna_false(nkeys):
    rng = np.random.default_rng(10 + nkeys)
    n = 1500
    keys, kvalid = _keys(rng, n, nkeys)
    cols = [_values(rng, n, dt) for dt in VAL_DTYPES]
    cols.append((np.full(n, np.nan), None))                       # a column without any entry
    vals, vvalid = [c[0] for c in cols], [c[1] for c in cols]
    got = R.table_groups(keys, kvalid, vals, vvalid, sumsq=True, minmax=True)
    exp = _pandas_groups(keys, kvalid, vals, vvalid)
    _same_groups(got, exp, f"{nkeys} keys")
    assert (got["null_mask"] != 0).any() and got["n"] > 2**nkeys
    assert np.isnan(got["min"][-1]).all() and (got["sum"][-1] == 0).all()
    # (null_mask, key tuple) ascending, every tuple once, row_group points at the row's own tuple
    tup = list(zip(got["null_mask"].tolist(), *[k.tolist() for k in got["keys"]]))
    assert tup == sorted(set(tup))
    for k in range(nkeys):
        stored = np.where(kvalid[k], keys[k], 0)
        R.first_mismatch(got["keys"][k][got["row_group"]], stored, f"row_group key {k}")
    # flags off: the lists are absent; no bitmaps = all valid
    plain = R.table_groups(keys, None, vals[:1], None)
    assert plain["sumsq"] is None and plain["min"] is None and not plain["null_mask"].any()
    assert int(plain["size"].sum()) == n == int(plain["count"].sum())


def test_a_null_component_and_a_valid_zero_are_different_groups():
    keys = [np.array([0, 5, 0, 0], np.int64), np.array([9, 0, 0, 0], np.int64)]
    valid = [np.array([1, 0, 1, 0], bool), np.array([0, 1, 1, 1], bool)]
    g = R.table_groups(keys, valid, [], None)
    assert g["null_mask"].tolist() == [0, 1, 2] and g["size"].tolist() == [1, 2, 1]
    assert g["keys"][0].tolist() == [0, 0, 0] and g["keys"][1].tolist() == [0, 0, 0]
    assert g["count"].tolist() == [1, 0, 1]
    _same_groups(dict(g, sum=[], sumsq=[], min=[], max=[]), _pandas_groups(keys, valid, [], []), "zeros")


@pytest.mark.parametrize("nkeys", [1, 3])
def test_merge_groups_equals_the_groupby_of_all_rows(nkeys):
    rng = np.random.default_rng(20 + nkeys)
    n, cut = 1200, 500
    keys, kvalid = _keys(rng, n, nkeys)
    v, w = _values(rng, n, "float64")
    w[:cut] &= keys[0][:cut] != 7              # key 7: no entry in the first part -> NaN min there
    part = lambda s: R.table_groups([k[s] for k in keys], [o[s] for o in kvalid], [v[s]], [w[s]],  # noqa: E731
                                    sumsq=True, minmax=True)
    a, b = part(slice(0, cut)), part(slice(cut, n))
    assert np.isnan(a["min"][0]).any() and not np.isnan(a["min"][0]).all()
    exp = _pandas_groups(keys, kvalid, [v], [w])
    _same_groups(R.merge_groups(a, b), exp, "a + b")
    _same_groups(R.merge_groups(b, a), exp, "b + a")
    empty = part(slice(0, 0))
    _same_groups(R.merge_groups(empty, a), dict(a), "empty + a")
    # without the optional lists on one side the result has none
    assert R.merge_groups(dict(a, sumsq=None, min=None, max=None), b)["min"] is None


@pytest.mark.parametrize("nkeys", [1, 2, 3])
def test_lookup_equals_a_left_merge_on_the_keys(nkeys):
    rng = np.random.default_rng(30 + nkeys)
    keys, kvalid = _keys(rng, 800, nkeys)
    g = R.table_groups(keys, kvalid, [], None)
    R.first_mismatch(R.lookup(g["keys"], g["null_mask"], keys, kvalid), g["row_group"], "own rows")
    # other rows against every second group: pandas' merge matches NA with NA
    sub = dict(keys=[k[::2] for k in g["keys"]], null_mask=g["null_mask"][::2])
    rows, rvalid = _keys(rng, 600, nkeys)
    left = _key_frame(rows, rvalid)
    right = _key_frame(sub["keys"], [(sub["null_mask"] >> k) & 1 == 0 for k in range(nkeys)])
    right["g"] = np.arange(len(right))
    exp = left.merge(right, how="left", on=list(left.columns))["g"].fillna(-1).to_numpy(dtype=np.int64)
    got = R.lookup(sub["keys"], sub["null_mask"], rows, rvalid)
    R.first_mismatch(got, exp, "left merge")
    assert (got == -1).any() and (got >= 0).any()
    # a table without null groups answers -1 for every row with a null component
    no_null = g["null_mask"] == 0
    got = R.lookup([k[no_null] for k in g["keys"]], g["null_mask"][no_null], keys, kvalid)
    some_null = ~np.logical_and.reduce(kvalid)
    assert (got[some_null] == -1).all() and (got[~some_null] >= 0).all()


def _sort_column(rng, n, dtype, ascending):
    """Column with duplicates, the edges of its type, NaN and nulls; never BOTH int64 values that
    the reserved null image makes a tie (test_the_reserved_null_image_...)."""
    valid = rng.random(n) >= 0.2
    if dtype.startswith("float"):
        tiny = np.finfo(dtype).smallest_subnormal
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 1.5, -1.5,
                         np.finfo(dtype).max, np.finfo(dtype).min, 3.0], dtype)
    elif dtype == "bool":
        return rng.random(n) < 0.5, valid
    elif dtype == "uint8":
        pool = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    else:
        i = np.iinfo(dtype)
        pool = np.array([i.min, i.min + 1, i.max - 1, i.max, 0, -1, 1, 77], dtype)
        if dtype == "int64":
            pool = np.delete(pool, 2 if ascending else 1)
    return pool[rng.integers(0, pool.size, n)], valid


def _pandas_series(v, valid):
    if v.dtype.kind == "f":
        return pd.Series(np.where(valid, v, np.nan).astype(v.dtype))
    if v.dtype == np.bool_:
        v = v.view(np.uint8)
    arr = pd.array(v, dtype={"int32": "Int32", "int64": "Int64", "uint8": "UInt8"}[v.dtype.name])
    arr[~valid] = pd.NA
    return pd.Series(arr)


def _pandas_order(cols, ascending):
    df = pd.DataFrame({f"c{j}": _pandas_series(v, ok) for j, (v, ok) in enumerate(cols)})
    for j in reversed(range(len(cols))):       # one column at a time, least significant first
        df = df.sort_values(f"c{j}", ascending=ascending, kind="stable", na_position="last")
    return df.index.to_numpy(dtype=np.int64)


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", VAL_DTYPES)
def test_sort_key_order_equals_stable_sort_values_nulls_last(dtype, ascending):
    rng = np.random.default_rng(40 + VAL_DTYPES.index(dtype))
    v, valid = _sort_column(rng, 700, dtype, ascending)
    got = R.sort_key_order([(v, valid)], ascending)
    R.first_mismatch(got, _pandas_order([(v, valid)], ascending), f"{dtype} asc={ascending}")
    assert sorted(got.tolist()) == list(range(700))
    # no bitmap: NaN alone sorts last
    R.first_mismatch(R.sort_key_order([(v, None)], ascending),
                     _pandas_order([(v, np.ones(700, bool))], ascending), "no bitmap")


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
def test_sort_key_order_of_several_columns(ascending):
    rng = np.random.default_rng(50)
    n = 900
    cols = [(rng.integers(0, 4, n).astype(np.uint8), rng.random(n) >= 0.1),
            _sort_column(rng, n, "float32", ascending), _sort_column(rng, n, "int64", ascending)]
    for m in (2, 3):
        R.first_mismatch(R.sort_key_order(cols[:m], ascending), _pandas_order(cols[:m], ascending),
                         f"{m} columns asc={ascending}")
    mixed = R.sort_key_order(cols[:2], [ascending, not ascending])
    df = pd.DataFrame({"a": _pandas_series(*cols[0]), "b": _pandas_series(*cols[1])})
    df = df.sort_values("b", ascending=not ascending, kind="stable", na_position="last")
    df = df.sort_values("a", ascending=ascending, kind="stable", na_position="last")
    R.first_mismatch(mixed, df.index.to_numpy(dtype=np.int64), "one direction per column")


def test_signed_zeros_tie_and_keep_row_order():
    for dtype in (np.float32, np.float64):
        for zeros in ([0.0, -0.0], [-0.0, 0.0]):
            v = np.array(zeros + [1.0, -1.0], dtype)
            assert R.sort_key_order([(v, None)], True).tolist() == [3, 0, 1, 2]
            assert R.sort_key_order([(v, None)], False).tolist() == [2, 0, 1, 3]
            R.first_mismatch(R.sort_key_order([(v, None)], True),
                             _pandas_order([(v, np.ones(4, bool))], True), "pandas agrees")


def test_the_reserved_null_image_ties_the_two_int64_values_at_the_far_end():
    """include/nvt_hip.h, nvt_sort_key_u64: where pandas orders by value, the 64-bit key ties
    INT64_MAX with INT64_MAX - 1 ascending and INT64_MIN with INT64_MIN + 1 descending."""
    hi = np.array([I64.max, I64.max - 1, 0, I64.max - 2], np.int64)
    assert _pandas_order([(hi, np.ones(4, bool))], True).tolist() == [2, 3, 1, 0]
    assert R.sort_key_order([(hi, None)], True).tolist() == [2, 3, 0, 1]         # the tie: row order
    assert R.sort_key_order([(hi, None)], False).tolist() == [0, 1, 3, 2]        # exact descending
    lo = np.array([I64.min + 1, I64.min, 0, I64.min + 2], np.int64)
    assert _pandas_order([(lo, np.ones(4, bool))], False).tolist() == [2, 3, 0, 1]
    assert R.sort_key_order([(lo, None)], False).tolist() == [2, 3, 0, 1]        # the tie: row order
    assert R.sort_key_order([(lo[[1, 0, 2, 3]], None)], False).tolist() == [2, 3, 0, 1]
    assert R.sort_key_order([(lo, None)], True).tolist() == [1, 0, 3, 2]         # exact ascending
    # a null still sorts behind the tied pair; int32 and floats have no such tie
    assert R.sort_key_order([(hi, np.array([1, 1, 0, 1], bool))], True).tolist() == [3, 0, 1, 2]
    i32 = np.iinfo(np.int32)
    for asc in (True, False):
        v = np.array([i32.max, i32.max - 1, i32.min + 1, i32.min], np.int32)
        assert R.sort_key_order([(v, None)], asc).tolist() == ([3, 2, 1, 0] if asc else [0, 1, 2, 3])
        f = np.array([-np.inf, np.finfo(np.float64).min, np.inf, np.finfo(np.float64).max])
        assert R.sort_key_order([(f, None)], asc).tolist() == ([0, 1, 3, 2] if asc else [2, 3, 1, 0])


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
@pytest.mark.parametrize("nkeys", [1, 2])
def test_order_rows_and_seg_aggregate_equal_the_oracles_groupby_operator(nkeys, ascending):
    """list / first / last / sum / count of the reference project's Groupby (oracle.groupby_op)
    from R.table_groups -> R.lookup -> R.order_rows -> R.seg_aggregate, the chain ops/groupby.py
    runs on the device."""
    rng = np.random.default_rng(60 + nkeys)
    n = 600
    keys, kvalid = _keys(rng, n, nkeys)
    ts = rng.integers(0, 40, n).astype(np.int32)                   # many ties: stability shows
    x = (rng.integers(-2**10, 2**10, n) / 16.0).astype(np.float32)
    df = _key_frame(keys, kvalid)
    kcols = list(df.columns)
    df["ts"], df["x"] = ts, x
    exp = O.groupby_op(df, kcols + ["x"], kcols, sort_cols=["ts"], ascending=ascending,
                       aggs={"x": ["list", "first", "last", "sum", "count"]})
    g = R.table_groups(keys, kvalid, [], None)
    real = g["null_mask"] == 0                                      # (they come first, by key tuple)
    gkeys = [k[real] for k in g["keys"]]
    G = int(real.sum())
    gid = R.lookup(gkeys, g["null_mask"][real], keys, kvalid)
    assert (gid == -1).sum() == (~np.logical_and.reduce(kvalid)).sum() > 0
    words = R.order_rows(n, [(ts, None)], ascending, gid, G)
    size, count, sm, _, _, _ = R.seg_aggregate(words, G, [x], [None])
    assert sorted((words & 0xFFFFFFFF).tolist()) == list(range(n))
    R.first_mismatch((words >> 32)[int(size.sum()):], np.full(n - int(size.sum()), G), "null rows last")
    off = np.concatenate([[0], np.cumsum(size)])
    rows = words[:off[-1]] & 0xFFFFFFFF
    assert len(exp) == G
    for k, c in enumerate(kcols):
        R.first_mismatch(exp[c].to_numpy(dtype=np.int64), gkeys[k], c)
    for i in range(G):
        lst = x[rows[off[i]:off[i + 1]]]
        np.testing.assert_array_equal(np.asarray(exp["x_list"][i], np.float32), lst)
        first, last = (lst[0], lst[-1]) if ascending else (lst[-1], lst[0])   # groupby.py:287-296
        assert exp["x_first"][i] == first and exp["x_last"][i] == last
    np.testing.assert_array_equal(exp["x_sum"].to_numpy(), sm[0].astype(np.float32))
    np.testing.assert_array_equal(exp["x_count"].to_numpy(), count[0].astype(np.int32))
    # neither sort columns nor group ids: the rows as they are
    R.first_mismatch(R.order_rows(n), np.arange(n, dtype=np.int64), "identity")


def test_seg_aggregate_equals_a_pandas_groupby_over_the_group_ids():
    rng = np.random.default_rng(70)
    n, G = 2000, 37
    gid = rng.integers(0, G, n)
    gid[np.isin(gid, [5, 20, G - 1])] = 4                            # empty groups, one at the end
    gid[rng.random(n) < 0.05] = -1
    cols = [_values(rng, n, dt) for dt in VAL_DTYPES]
    cols[1][1][gid == 7] = False                                     # group 7: no entry in column 1
    vals, vvalid = [c[0] for c in cols], [c[1] for c in cols]
    words = R.order_rows(n, (), True, gid, G)
    df = pd.DataFrame({"g": gid})
    for j, (v, w) in enumerate(cols):
        df[f"v{j}"] = _f64_with_nan(v, w)
        df[f"q{j}"] = df[f"v{j}"] ** 2
    gb = df[df["g"] >= 0].groupby("g")
    full = lambda s, fill: s.reindex(range(G)).fillna(fill).to_numpy()  # noqa: E731
    for w in (words, rng.permutation(words)):                          # the reference needs no order
        size, count, sm, sq, mn, mx = R.seg_aggregate(w, G, vals, vvalid, sumsq=True, minmax=True)
        R.first_mismatch(size, full(gb.size(), 0).astype(np.int64), "size")
        for j in range(len(cols)):
            R.first_mismatch(count[j], full(gb[f"v{j}"].count(), 0).astype(np.int64), f"count {j}")
            np.testing.assert_array_equal(sm[j], full(gb[f"v{j}"].sum(), 0.0))
            np.testing.assert_array_equal(sq[j], full(gb[f"q{j}"].sum(), 0.0))
            np.testing.assert_array_equal(mn[j], full(gb[f"v{j}"].min(), np.inf))
            np.testing.assert_array_equal(mx[j], full(gb[f"v{j}"].max(), -np.inf))
    assert size[5] == 0 and size[G - 1] == 0 and count[1][7] == 0 and size[7] > 0
    assert mn[1][7] == np.inf and mx[1][7] == -np.inf and sm[1][7] == 0
    assert (count[0] != count[2]).any()                                # a count per column
    # flags off, no columns
    size2, count2, sm2, sq2, mn2, mx2 = R.seg_aggregate(words, G, [], None)
    R.first_mismatch(size2, size, "size alone")
    assert count2.shape == (0, G) and sm2.shape == (0, G) and sq2 is None and mn2 is None and mx2 is None
    # a group of infinities keeps them (the count tells them from "no entry")
    inf = np.array([np.inf, np.inf, -np.inf, 1.0])
    _, c, _, _, lo, hi = R.seg_aggregate(np.array([0, 1, (1 << 32) | 2, (2 << 32) | 3]), 4, [inf], None,
                                         minmax=True)
    assert lo[0].tolist() == [np.inf, -np.inf, 1.0, np.inf] and hi[0].tolist() == [np.inf, -np.inf, 1.0, -np.inf]
    assert c[0].tolist() == [2, 1, 1, 0]
