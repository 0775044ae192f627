"""Dataset.shuffle_by_keys on the device: the Groupby workflow that needs it, the properties of
the shuffle (rows preserved, one partition per key, stable, empty partitions present, schema
unchanged), key and payload kinds, and the argument errors."""
import numpy as np
import pandas as pd
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


def _parts(ds):
    return [p.to_pandas() for p in ds.to_iter()]


def _key_tuples(df, keys):
    return {tuple(None if pd.isna(v) else v for v in row) for row in df[keys].itertuples(index=False, name=None)}


def _sorted(df, by):
    return df.sort_values(by, kind="stable", na_position="last", ignore_index=True)


def test_groupby_needs_and_gets_the_shuffle():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(11)
    n = 3000
    df = pd.DataFrame({
        "user_id": rng.integers(0, 50, n).astype("int64"),
        "session_id": rng.integers(0, 4, n).astype("int64"),
        "ts": rng.permutation(n).astype("int64"),            # unique: the sort is unambiguous
        "item": rng.integers(0, 1000, n).astype("int64"),
        "x": rng.normal(size=n).astype("float32"),
    })
    df.loc[rng.random(n) < 0.1, "x"] = np.nan
    keys = ["user_id", "session_id"]
    sel = ["user_id", "session_id", "ts", "item", "x"]
    aggs = {"item": "list", "ts": ["first", "last"], "x": ["sum", "count"]}
    ds = nvt.Dataset([df.iloc[i * 1000:(i + 1) * 1000].reset_index(drop=True) for i in range(3)])
    assert ds.npartitions == 3
    feats = sel >> ops.Groupby(groupby_cols=keys, sort_cols=["ts"], aggs=aggs)
    wf = nvt.Workflow(feats)
    exp = O.groupby_op(df, sel, keys, ["ts"], aggs)
    exp = _sorted(exp, keys)
    n_keys = len(_key_tuples(df, keys))
    assert len(exp) == n_keys

    unshuffled = wf.fit_transform(ds).to_ddf().compute()
    assert len(unshuffled) > n_keys          # the input really needed the shuffle

    got = wf.transform(ds.shuffle_by_keys(keys)).to_ddf().compute()
    got = _sorted(got, keys)
    assert sorted(got.columns) == sorted(exp.columns) and len(got) == len(exp) == n_keys
    for c in keys + ["ts_first", "ts_last", "x_count"]:
        np.testing.assert_array_equal(got[c].to_numpy().astype("int64"), exp[c].to_numpy().astype("int64"), err_msg=c)
    for g, e in zip(got["item_list"], exp["item_list"]):
        assert list(g) == list(e)
    np.testing.assert_allclose(got["x_sum"].to_numpy().astype("float64"), exp["x_sum"].to_numpy().astype("float64"),
                               rtol=1e-5, atol=1e-6, equal_nan=True)


def test_reference_session_example_through_the_nvtabular_name():
    import nvtabular as nvt
    from nvtabular import ops

    rng = np.random.default_rng(12)
    n = 600
    df = pd.DataFrame({"user_id": rng.integers(0, 20, n).astype("int64"), "ts": rng.permutation(n).astype("int64"),
                       "item": rng.integers(0, 99, n).astype("int64")})
    groupby_cols = ["user_id"]
    dataset = nvt.Dataset(df, npartitions=4)
    feats = ["user_id", "ts", "item"] >> ops.Groupby(groupby_cols=groupby_cols, sort_cols=["ts"],
                                                     aggs={"item": ["list", "count"]})
    workflow = nvt.Workflow(feats)
    dataset = dataset.shuffle_by_keys(keys=groupby_cols)
    got = _sorted(workflow.fit_transform(dataset).to_ddf().compute(), groupby_cols)
    exp = _sorted(O.groupby_op(df, ["user_id", "ts", "item"], groupby_cols, ["ts"], {"item": ["list", "count"]}),
                  groupby_cols)
    assert got["user_id"].tolist() == exp["user_id"].tolist()
    assert [list(x) for x in got["item_list"]] == [list(x) for x in exp["item_list"]]
    assert got["item_count"].tolist() == exp["item_count"].tolist()


def _frame(n, seed, row0):
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({
        "k1": rng.integers(0, 7, n).astype("int64"),
        "k2": pd.array(rng.integers(0, 3, n), dtype="Int64"),
        "row": np.arange(row0, row0 + n, dtype="int64"),
        "f": rng.normal(size=n).astype("float32"),
        "v": pd.array(rng.integers(0, 100, n), dtype="Int64"),
    })
    if n:
        df.loc[rng.random(n) < 0.2, "k2"] = pd.NA
        df.loc[rng.random(n) < 0.3, "v"] = pd.NA
    return df


@pytest.mark.parametrize("npartitions", [1, 3, 8])
def test_shuffle_properties(npartitions):
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceFrame

    sizes = [0, 1, 65, 1000]
    frames, row0 = [], 0
    for i, n in enumerate(sizes):
        frames.append(_frame(n, 20 + i, row0))
        row0 += n
    # device frames keep the dtypes of the zero-row partition (pandas would infer none)
    ds = nvt.Dataset([DeviceFrame.from_pandas(f) for f in frames])
    keys = ["k1", "k2"]
    out = ds.shuffle_by_keys(keys, npartitions=npartitions)
    assert out.npartitions == npartitions
    assert out.schema.column_names == ds.schema.column_names == list(frames[0].columns)
    dev_parts = list(out.to_iter())
    assert len(dev_parts) == npartitions
    src_dtypes = {c: col.dtype for c, col in next(iter(ds.to_iter())).items()}
    for part in dev_parts:
        assert part.columns == list(frames[0].columns)
        assert {c: col.dtype for c, col in part.items()} == src_dtypes      # also in an empty partition
    parts = [p.to_pandas() for p in dev_parts]
    whole = pd.concat([f.astype({"k2": "float64", "v": "float64"}) for f in frames], ignore_index=True)
    got = pd.concat([p.astype({"k2": "float64", "v": "float64"}) for p in parts], ignore_index=True)
    # the multiset of rows, nulls included ("row" is unique)
    pd.testing.assert_frame_equal(_sorted(got, ["row"]), _sorted(whole, ["row"]), check_dtype=False)
    # every key tuple in exactly one output partition (a null is a key value)
    seen = {}
    for i, p in enumerate(parts):
        for t in _key_tuples(p, keys):
            assert seen.setdefault(t, i) == i, t
    assert set(seen) == _key_tuples(whole, keys)
    if npartitions == 8:
        assert sum(len(p) > 0 for p in parts) >= 4
    # stability: input order inside every output partition
    for p in parts:
        assert (np.diff(p["row"].to_numpy()) > 0).all()


def test_string_key_round_trips():
    import nvtabular_amd as nvt

    rng = np.random.default_rng(30)
    names = np.array(["ann", "bo", "cy", "dee", "eve", "fay", "gus"], dtype=object)
    a = pd.DataFrame({"name": rng.choice(names[:5], 200), "row": np.arange(200)})
    b = pd.DataFrame({"name": rng.choice(names[3:], 300), "row": np.arange(200, 500)})   # new strings here
    b.loc[rng.random(300) < 0.1, "name"] = None
    out = nvt.Dataset([a, b]).shuffle_by_keys("name", npartitions=3)
    parts = _parts(out)
    got = _sorted(pd.concat(parts, ignore_index=True), ["row"])
    exp = pd.concat([a, b], ignore_index=True)
    assert [None if pd.isna(x) else x for x in got["name"]] == [None if pd.isna(x) else x for x in exp["name"]]
    seen = {}
    for i, p in enumerate(parts):
        for t in _key_tuples(p, ["name"]):
            assert seen.setdefault(t, i) == i
        assert (np.diff(p["row"].to_numpy()) > 0).all()


def test_float_key_and_pending_fill_key():
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceFrame

    rng = np.random.default_rng(31)
    n = 500
    df = pd.DataFrame({"fk": rng.integers(-4, 4, n) / 4.0, "ik": pd.array(rng.integers(0, 5, n), dtype="Int64"),
                       "row": np.arange(n)})
    df.loc[:3, "fk"] = [0.0, -0.0, np.nan, np.nan]
    df.loc[rng.random(n) < 0.3, "ik"] = pd.NA
    halves = [df.iloc[:250].reset_index(drop=True), df.iloc[250:].reset_index(drop=True)]
    parts = _parts(nvt.Dataset(halves).shuffle_by_keys("fk", npartitions=4))
    where = {}
    for i, p in enumerate(parts):
        for v in p["fk"]:
            k = "nan" if v != v else float(v) + 0.0
            assert where.setdefault(k, i) == i
    assert sorted(pd.concat(parts)["row"].tolist()) == list(range(n))
    # a pending FillMissing constant is the key value: nulls and real 2s meet in one partition
    frames = []
    for h in halves:
        f = DeviceFrame.from_pandas(h)
        f["ik"].fill = 2
        frames.append(f)
    parts = _parts(nvt.Dataset(frames).shuffle_by_keys(["ik"], npartitions=4))
    where = {}
    for i, p in enumerate(parts):
        assert not p["ik"].isna().any()
        for v in p["ik"]:
            assert where.setdefault(int(v), i) == i
    got = _sorted(pd.concat(parts, ignore_index=True), ["row"])
    np.testing.assert_array_equal(got["ik"].to_numpy().astype("int64"), df["ik"].fillna(2).to_numpy().astype("int64"))


def test_payload_kinds_and_list_column():
    import nvtabular_amd as nvt

    rng = np.random.default_rng(32)
    n = 700
    lists = [rng.integers(0, 50, int(k)).astype("int64") for k in rng.integers(0, 4, n)]   # empty lists too
    df = pd.DataFrame({
        "k": rng.integers(0, 9, n).astype("int32"),
        "row": np.arange(n, dtype="int64"),
        "flag": rng.random(n) < 0.5,
        "u8": rng.integers(0, 255, n).astype("uint8"),
        "i32": rng.integers(-1000, 1000, n).astype("int32"),
        "i16": rng.integers(-30000, 30000, n).astype("int16"),      # what ReduceDtypeSize writes
        "f64": rng.normal(size=n),
        "nul": pd.array(rng.integers(0, 100, n), dtype="Int64"),
        "lst": lists,
    })
    df.loc[rng.random(n) < 0.25, "nul"] = pd.NA
    # null list rows, in the last two input partitions only (the first two have none); the ingest
    # makes a row of length 0 of a null row (list columns carry no row validity)
    null_rows = np.flatnonzero(rng.random(n) < 0.15)
    null_rows = null_rows[null_rows >= 200]
    assert (null_rows < 400).any() and (null_rows >= 400).any()
    for r in null_rows:
        df.at[r, "lst"] = None
    want_lists = [[] if x is None else list(x) for x in df["lst"]]
    assert sum(len(x) == 0 for x in want_lists) > len(null_rows)        # empty lists too
    cut = [0, 130, 131, 400, n]
    frames = [df.iloc[cut[i]:cut[i + 1]].reset_index(drop=True) for i in range(4)]
    out = nvt.Dataset(frames).shuffle_by_keys("k", npartitions=5)
    dev_parts = list(out.to_iter())
    parts = [p.to_pandas() for p in dev_parts]
    got = _sorted(pd.concat(parts, ignore_index=True), ["row"])
    assert len(got) == n
    for c in ("k", "flag", "u8", "i32", "i16", "f64"):
        np.testing.assert_array_equal(got[c].to_numpy(), df[c].to_numpy(), err_msg=c)
        assert got[c].dtype == df[c].dtype, c
    np.testing.assert_array_equal(got["nul"].to_numpy().astype("float64"), df["nul"].to_numpy(dtype="float64", na_value=np.nan))
    assert [list(x) for x in got["lst"]] == want_lists
    for p, d in zip(parts, dev_parts):
        assert (np.diff(p["row"].to_numpy()) > 0).all()
        off = d["lst"].offsets.cpu().numpy()
        assert off[0] == 0 and off[-1] == d["lst"].data.numel() and len(off) == len(p) + 1
        np.testing.assert_array_equal(np.diff(off), [len(want_lists[r]) for r in p["row"]])
        leaves = d["lst"].data.cpu().numpy().tolist()
        assert leaves == [v for r in p["row"] for v in want_lists[r]]
    where = {}
    for i, p in enumerate(parts):
        for v in set(p["k"]):
            assert where.setdefault(int(v), i) == i


def test_list_column_with_null_leaves():
    import pyarrow as pa

    import nvtabular_amd as nvt

    a = pa.table({"k": pa.array([1, 2, 1, 3], pa.int64()),
                  "lst": pa.array([[1, None], None, [3], [None, 5, 6]], pa.list_(pa.int64()))})   # a null row
    b = pa.table({"k": pa.array([3, 1], pa.int64()), "lst": pa.array([[7], [None]], pa.list_(pa.int64()))})
    out = nvt.Dataset([a, b]).shuffle_by_keys("k", npartitions=2)
    rows = {}
    for part in out.to_iter():
        t = part.to_arrow()
        for k, l in zip(t.column("k").to_pylist(), t.column("lst").to_pylist()):
            rows.setdefault(k, []).append(l)
    # the null row comes out as the ingest defines it: a row of length 0
    assert rows == {1: [[1, None], [3], [None]], 2: [[]], 3: [[None, 5, 6], [7]]}


def test_errors():
    import nvtabular_amd as nvt

    df = pd.DataFrame({"a": [1, 2, 3, 4], "b": [1.0, 2.0, 3.0, 4.0], "c": [5, 6, 7, 8], "d": [0, 1, 0, 1],
                       "e": [9, 9, 9, 9], "l": [[1], [2, 3], [], [4]]})
    ds = nvt.Dataset(df)
    with pytest.raises(ValueError, match="nope"):
        ds.shuffle_by_keys(["a", "nope"])
    with pytest.raises(TypeError, match="list"):
        ds.shuffle_by_keys("l")
    with pytest.raises(NotImplementedError):
        ds.shuffle_by_keys(["a", "b", "c", "d", "e"])
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="npartitions"):
            ds.shuffle_by_keys("a", npartitions=bad)
    with pytest.raises(NotImplementedError, match="hive-partitioned directories are not tracked by this Dataset"):
        ds.shuffle_by_keys("a", hive_data=True)
    lens = [len(p) for p in ds.shuffle_by_keys("a", hive_data=False, npartitions=2).to_iter()]
    assert len(lens) == 2 and sum(lens) == 4
