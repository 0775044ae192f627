"""ReduceDtypeSize, DataStats and DropLowCardinality through Workflow on the device, against
numpy / pandas computed here."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import ops
from nvtabular_amd.device import DeviceFrame

pytestmark = pytest.mark.gpu


def _fit_transform(graph, df, npartitions=1):
    wf = nvt.Workflow(graph)
    out = wf.fit_transform(nvt.Dataset(df, npartitions=npartitions)).to_ddf().compute()
    return wf, out


def test_reduce_dtype_size_reference_frame():
    df = pd.DataFrame({"int16": np.array([2**15 - 1, 0], dtype="int64"),
                       "int32": np.array([2**30, -(2**30)], dtype="int64"),
                       "int64": np.array([2**60, -(2**60)], dtype="int64"),
                       "float32": np.array([1.0, 2.0], dtype="float64")})
    wf, out = _fit_transform(list(df.columns) >> ops.ReduceDtypeSize(), df)
    for c in df.columns:
        assert out[c].dtype == np.dtype(c), c
        np.testing.assert_array_equal(out[c].to_numpy(), df[c].astype(c).to_numpy())
        assert wf.output_schema[c].dtype == np.dtype(c)


BOUNDS = {"max127": (127, "int8"), "max128": (128, "int16"), "min-128": (-128, "int8"), "min-129": (-129, "int16"),
          "max32767": (32767, "int16"), "max32768": (32768, "int32"), "max2^31-1": (2**31 - 1, "int32"),
          "max2^31": (2**31, "int64")}


def test_reduce_dtype_size_boundaries_nulls_three_partitions():
    n = 48                                              # three partitions of 16 rows
    rng = np.random.default_rng(5)
    data = {}
    for name, (v, _) in BOUNDS.items():
        x = rng.integers(-5, 6, n).astype(np.int64)
        x[n // 2] = v                                   # the extreme value sits in the middle partition
        data[name] = x
    df = pd.DataFrame(data)
    nul = rng.integers(-100, 101, n).astype(np.int64)
    nul[n // 2 + 1] = 300
    df["nullable"] = pd.array(nul, dtype="Int64")
    df.loc[[0, 3, 17, 40, 47], "nullable"] = pd.NA
    df["allnull"] = pd.array([pd.NA] * n, dtype="Int64")
    op = ops.ReduceDtypeSize()
    wf, out = _fit_transform(list(df.columns) >> op, df, npartitions=3)
    for name, (v, want) in BOUNDS.items():
        assert op.dtypes[name] == np.dtype(want) and out[name].dtype == np.dtype(want), name
        assert op.ranges[name] == (int(df[name].min()), int(df[name].max())) and isinstance(op.ranges[name][0], int)
        np.testing.assert_array_equal(out[name].to_numpy(), df[name].to_numpy().astype(want))
        assert wf.output_schema[name].dtype == np.dtype(want)
    assert op.dtypes["nullable"] == np.dtype("int16") and str(out["nullable"].dtype) == "Int16"
    assert out["nullable"].isna().tolist() == df["nullable"].isna().tolist()
    assert out["nullable"].dropna().astype("int64").tolist() == df["nullable"].dropna().astype("int64").tolist()
    assert op.ranges["allnull"] == (None, None) and op.dtypes["allnull"] == np.dtype("int64")
    assert out["allnull"].isna().all()
    # a later partition with a value outside the fitted range wraps as numpy does
    late = df.copy()
    late.loc[1, "max127"], late.loc[2, "max127"], late.loc[3, "max32767"] = 128, -1000, 2**31 + 5
    got = wf.transform(late)
    np.testing.assert_array_equal(got["max127"].to_numpy(), late["max127"].to_numpy().astype("int8"))
    np.testing.assert_array_equal(got["max32767"].to_numpy(), late["max32767"].to_numpy().astype("int16"))
    assert got["max127"][1] == -128


def test_reduce_dtype_size_list_column_and_float_dtype():
    rows = [[1, 2, 300], [], [-7], [4, 5]]
    df = pd.DataFrame({"l": rows, "f": np.array([0.1, 1e39, np.nan, -2.5])})
    frame = DeviceFrame.from_pandas(df)
    op = ops.ReduceDtypeSize()
    wf = nvt.Workflow(["l", "f"] >> op)
    wf.fit(nvt.Dataset(df))
    out = wf.transform(frame)
    assert out["l"].data.dtype == torch.int16 and out["f"].data.dtype == torch.float32
    assert torch.equal(out["l"].offsets, frame["l"].offsets)
    assert out["l"].data.cpu().tolist() == [1, 2, 300, -7, 4, 5] and op.ranges["l"] == (-7, 300)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(out["f"].data.cpu().numpy(), df["f"].to_numpy().astype(np.float32))
    assert wf.output_schema["l"].dtype == np.dtype("int16") and wf.output_schema["l"].is_list
    keep = ops.ReduceDtypeSize(float_dtype=np.float64)
    _, same = _fit_transform(["f"] >> keep, df[["f"]])
    assert same["f"].dtype == np.float64 and keep.dtypes["f"] == np.dtype("float64")
    # a float is never widened, and bool / uint8 columns are neither read nor changed
    mixed = pd.DataFrame({"f32": np.array([0.5, 2.5], dtype=np.float32), "b": [True, False],
                          "u8": np.array([1, 200], dtype=np.uint8), "i": np.array([1, 2], dtype=np.int64)})
    _, got = _fit_transform(list(mixed.columns) >> keep, mixed)
    assert keep.dtypes == {"f32": np.dtype("float32"), "i": np.dtype("int8")} and set(keep.ranges) == {"f32", "i"}
    assert [str(t) for t in got.dtypes] == ["float32", "bool", "uint8", "int8"]
    for c in mixed.columns:
        assert got[c].tolist() == mixed[c].tolist()


def test_reduced_columns_round_trip_through_parquet(tmp_path):
    import pyarrow.parquet as pq

    df = pd.DataFrame({"a": np.arange(-50, 50, dtype=np.int64), "b": np.arange(100, dtype=np.int64) * 300 - 9000,
                       "c": np.arange(100, dtype=np.int64) << 20})
    df["n"] = pd.array(np.arange(100) % 90, dtype="Int64")
    df.loc[[5, 50], "n"] = pd.NA
    wf = nvt.Workflow(list(df.columns) >> ops.ReduceDtypeSize())
    wf.fit_transform(nvt.Dataset(df)).to_parquet(str(tmp_path))
    files = sorted(p for p in tmp_path.iterdir() if p.suffix == ".parquet")
    tab = pq.read_table(str(files[0]))
    assert [str(tab.schema.field(c).type) for c in ("a", "b", "c", "n")] == ["int8", "int16", "int32", "int8"]
    assert tab["a"].to_pylist() == df["a"].tolist() and tab["b"].to_pylist() == df["b"].tolist()
    assert tab["n"].to_pylist() == [None if v is pd.NA else int(v) for v in df["n"]]
    # and back in through this engine's reader
    back = nvt.Dataset(str(files[0])).to_ddf().compute()
    assert back["a"].dtype == np.int8 and back["b"].dtype == np.int16 and back["a"].tolist() == df["a"].tolist()


def _stats_frame(n=3000):
    rng = np.random.default_rng(11)

    def holes(s):
        s = s.copy()
        s[rng.random(n) < 0.1] = None
        return s

    df = pd.DataFrame({
        "i32": holes(pd.Series(rng.integers(-1000, 1000, n), dtype="Int32")),
        "i64": holes(pd.Series(rng.integers(-(2**40), 2**40, n), dtype="Int64")),
        "f32": holes(pd.Series((rng.normal(size=n) * 30).astype(np.float32))),
        "f64": holes(pd.Series(rng.normal(size=n) * 1e3 + 5)),
        "empty": pd.Series([pd.NA] * n, dtype="Int64"),
    })
    words = np.array(["a", "bb", "naïve", "日本語", "", "long-ish word", "x" * 40, "ccc"], dtype=object)
    s = pd.Series(words[rng.integers(0, len(words), n)], dtype=object)
    s[rng.random(n) < 0.1] = None
    df["s"] = s
    df.loc[7, "i64"] = 2**53 + 1
    return df


def test_data_stats_against_pandas():
    df = _stats_frame()
    op = ops.DataStats()
    wf = nvt.Workflow(list(df.columns) >> op)
    ds = nvt.Dataset(df, npartitions=3)
    wf.fit(ds)
    out = op.output
    assert list(out) == list(df.columns)
    for c in df.columns:
        s, st = df[c], out[c]
        is_float = c in ("f32", "f64")
        assert set(st) == {"dtype", "min", "max", "mean", "std", "per_nan"} | (set() if is_float else {"cardinality"}), c
        assert all(type(v) in (int, float, str) for v in st.values()), (c, st)       # YAML-able scalars
        assert st["per_nan"] == 100 * (1 - s.count() / len(s)), c
        if c == "empty":
            assert all(math.isnan(st[k]) for k in ("min", "max", "mean", "std"))
            assert st["per_nan"] == 100.0 and st["cardinality"] == 0 and st["dtype"] == "int64"
            continue
        if c == "s":
            lens = s.dropna().str.len()
            assert st["dtype"] == "object" and (st["min"], st["max"]) == (int(lens.min()), int(lens.max()))
            assert st["cardinality"] == s.nunique()
            np.testing.assert_allclose([st["mean"], st["std"]], [lens.mean(), lens.std()], rtol=2e-6)
            continue
        v = s.dropna()
        assert st["dtype"] == str(np.dtype(getattr(s.dtype, "numpy_dtype", s.dtype))), c
        if is_float:
            assert st["min"] == float(v.min()) and st["max"] == float(v.max()), c
        else:
            assert st["min"] == int(v.min()) and st["max"] == int(v.max()) and type(st["min"]) is int, c
            assert st["cardinality"] == v.nunique(), c
        vals = v.astype(np.float64)
        np.testing.assert_allclose([st["mean"], st["std"]], [vals.mean(), vals.std()], rtol=2e-6, err_msg=c)
    assert out["i64"]["max"] == 2**53 + 1
    # transform is the identity
    got = wf.transform(df)
    for c in ("i32", "i64", "f32", "f64"):
        np.testing.assert_array_equal(got[c].to_numpy(dtype=np.float64, na_value=np.nan),
                                      df[c].to_numpy(dtype=np.float64, na_value=np.nan))
    assert got["s"].where(got["s"].notna(), None).tolist() == df["s"].where(df["s"].notna(), None).tolist()
    with pytest.raises(NotImplementedError):
        nvt.Workflow(["l"] >> ops.DataStats()).fit(nvt.Dataset(pd.DataFrame({"l": [[1, 2], [3]]})))


def test_drop_low_cardinality_after_fit_transform():
    df = pd.DataFrame({"col1": ["a", "a", "a", "a", "a"], "col2": ["a", "a", "a", "a", "b"],
                       "col3": ["a", "a", "b", "b", "c"]})
    wf = nvt.Workflow(list(df.columns) >> ops.Categorify() >> ops.DropLowCardinality())
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()       # (output_schema not touched before)
    assert list(out.columns) == ["col2", "col3"]
    assert out["col2"].tolist() == [3, 3, 3, 3, 4] and out["col3"].tolist() == [3, 3, 4, 4, 5]
    assert wf.output_schema.column_names == ["col2", "col3"]
    # a non-categorical column passes through
    df["x"] = np.arange(5, dtype=np.float64)
    cats = ["col1", "col2", "col3"] >> ops.Categorify()
    wf = nvt.Workflow((cats + ["x"]) >> ops.DropLowCardinality())
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    assert sorted(out.columns) == ["col2", "col3", "x"] and out["x"].tolist() == df["x"].tolist()
    assert sorted(wf.output_schema.column_names) == ["col2", "col3", "x"]


def test_save_load_transforms_without_refit(tmp_path):
    df = _stats_frame(600)[["i32", "i64", "f64"]]
    red, st = ops.ReduceDtypeSize(), ops.DataStats()
    wf = nvt.Workflow(list(df.columns) >> st >> red)
    first = wf.fit_transform(nvt.Dataset(df, npartitions=3)).to_ddf().compute()
    wf.save(str(tmp_path))
    back = nvt.Workflow.load(str(tmp_path))
    second = back.transform(df)
    assert [str(t) for t in second.dtypes] == [str(t) for t in first.dtypes] == ["Int16", "float64", "float32"]   # (int64 with nulls: pandas' float convention)
    for c in df.columns:
        np.testing.assert_array_equal(second[c].to_numpy(dtype=np.float64, na_value=np.nan),
                                      first[c].to_numpy(dtype=np.float64, na_value=np.nan))
    loaded = [n.op for n in nvt.node.iter_nodes(back.output_node) if isinstance(n.op, ops.DataStats)][0]
    assert loaded.output.keys() == st.output.keys()
    for c in st.output:
        for k, v in st.output[c].items():
            assert loaded.output[c][k] == v or (v != v and loaded.output[c][k] != loaded.output[c][k]), (c, k)
    assert st.output["i32"]["dtype"] == "int32" and red.dtypes["i32"] == np.dtype("int16")
    # narrow columns are no input of DataStats
    with pytest.raises(TypeError, match="int16"):
        nvt.Workflow(["i32"] >> ops.ReduceDtypeSize() >> ops.DataStats()).fit(nvt.Dataset(df))
