"""The host side of hive-partitioned parquet (nvtabular_amd/hive.py and its plumbing in io.py) without
a GPU: discovery, key dtypes, the schema and partition count of a directory pyarrow wrote, and the
argument errors of ``to_parquet(partition_on=...)`` that are raised before anything exists."""
import json
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import nvtabular_amd as nvt
from nvtabular_amd import hive
from nvtabular_amd.io import Shuffle


def _table(n=12):
    return pa.table({"x": pa.array(np.arange(n), type=pa.int64()),
                     "day": pa.array([1, 2, None] * (n // 3), type=pa.int64()),
                     "tag": pa.array(["a/b", "7", ""] * (n // 3), type=pa.string())})


def _write(root, cols=("day", "tag")):
    pq.write_to_dataset(_table(), str(root), partition_cols=list(cols))


def test_discovery_walks_sorted_leaf_directories(tmp_path):
    _write(tmp_path)
    lay = hive.discover(str(tmp_path))
    assert lay.keys == ["day", "tag"]
    rel = [os.path.relpath(os.path.dirname(f), tmp_path) for f in lay.files]
    assert rel == sorted(rel) and len(rel) == 3
    assert set(rel) == {"day=1/tag=a%2Fb", "day=2/tag=7", "day=__HIVE_DEFAULT_PARTITION__/tag="}
    assert sorted(lay.values.values(), key=str) == sorted([("1", "a/b"), ("2", "7"), (None, "")], key=str)
    # a directory with parquet files at its top level is not a hive dataset
    pq.write_table(_table(), str(tmp_path / "flat.parquet"))
    assert hive.discover(str(tmp_path)) is None
    assert hive.discover(str(tmp_path / "missing")) is None


def test_key_names_must_agree(tmp_path):
    _write(tmp_path)
    os.makedirs(tmp_path / "tag=q" / "day=5")
    pq.write_table(pa.table({"x": [1]}), str(tmp_path / "tag=q" / "day=5" / "f.parquet"))
    with pytest.raises(ValueError, match="partitioned on"):
        hive.discover(str(tmp_path))


def test_key_that_is_a_file_column_is_refused(tmp_path):
    os.makedirs(tmp_path / "x=1")
    pq.write_table(pa.table({"x": [1, 2], "y": [3, 4]}), str(tmp_path / "x=1" / "f.parquet"))
    with pytest.raises(ValueError, match="also columns inside the files"):
        nvt.Dataset(str(tmp_path))


def test_dtype_inference(tmp_path):
    _write(tmp_path)
    assert hive.layout_of(str(tmp_path)).dtypes == ["int64", "string"]   # "7" next to "a/b": string
    assert hive.infer_dtypes(["k"], [("7",), ("-12",), (None,)]) == ["int64"]
    assert hive.infer_dtypes(["k"], [("7",), ("x",)]) == ["string"]
    assert hive.infer_dtypes(["k"], [("+7",)]) == ["string"] and hive.infer_dtypes(["k"], [("",)]) == ["string"]
    # _metadata.json comes first
    with open(tmp_path / "_metadata.json", "w") as f:
        json.dump({"partition_on": [{"col_name": "day", "dtype": "int32"}]}, f)
    assert hive.layout_of(str(tmp_path)).dtypes == ["int32", "string"]


def test_schema_and_partitions_of_a_pyarrow_dataset(tmp_path):
    _write(tmp_path)
    ds = nvt.Dataset(str(tmp_path))
    assert ds.schema.column_names == ["x", "day", "tag"]          # keys last, in path order
    assert ds.schema["day"].dtype == np.dtype("int64") and not ds.schema["day"].is_list
    assert ds.npartitions == 3
    with pytest.raises(FileNotFoundError):
        os.makedirs(tmp_path / "empty")
        nvt.Dataset(str(tmp_path / "empty"))
    with pytest.raises(NotImplementedError):
        ds.shuffle_by_keys(["day"], hive_data=True)


def test_argument_errors_come_before_anything_is_created(tmp_path):
    df = pd.DataFrame({"k": np.arange(6) % 2, "s": list("ababab"), "f": np.arange(6) / 2, "x": np.arange(6),
                       "t": pd.to_datetime(np.arange(6), unit="s"), "b": np.arange(6) % 2 == 0})
    ds = nvt.Dataset(df)
    out = tmp_path / "out"
    os.makedirs(out)
    bad = [(dict(partition_on=["k"], out_files_per_proc=2), ValueError, "out_files_per_proc"),
           (dict(partition_on=["k"], shuffle=Shuffle.PER_WORKER), ValueError, "PER_WORKER"),
           (dict(partition_on=["k", "k"]), ValueError, "repeats"),
           (dict(partition_on=["nope"]), ValueError, "no columns"),
           (dict(partition_on=[]), ValueError, "1 to 4"),
           (dict(partition_on=["k", "s", "x", "f", "t"]), ValueError, "1 to 4"),
           (dict(partition_on="k", max_partitions=0), ValueError, "max_partitions"),
           (dict(partition_on="k", max_partitions=1 << 40), ValueError, "open files"),
           (dict(partition_on=["f"]), TypeError, "cast it first"),
           (dict(partition_on=["t"]), TypeError, "cast it first"),
           (dict(partition_on=["b"]), TypeError, "cast it first")]
    for kw, exc, match in bad:
        with pytest.raises(exc, match=match):
            ds.to_parquet(str(out), **kw)
        assert os.listdir(out) == [], kw
    small = nvt.Dataset(df[["k", "s"]])
    with pytest.raises(ValueError, match="no data column"):
        small.to_parquet(str(out), partition_on=["k", "s"])
    assert os.listdir(out) == []
