"""Hive-partitioned parquet end to end on the device: ``Dataset.to_parquet(partition_on=...)`` read back
by pyarrow and by ``Dataset(path)``, a dataset pyarrow wrote read by ``Dataset(path)``, and a Workflow
over a hive dataset.  20 000 rows in three input partitions, the middle one empty; ``x`` numbers the
rows, so sorting by it aligns any read-back with the input and the order inside a directory is the
order of ``x``."""
import glob
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.dataset as pads
import pyarrow.parquet as pq
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import hive, ops

pytestmark = pytest.mark.gpu

STRINGS = ["a/b", "x=y", "p%q r", "é", "", None]
N = 20_000
KEYS = ["day", "tag"]
DATA = ["x", "f", "s", "l", "t"]


@pytest.fixture(scope="module")
def df():
    rng = np.random.default_rng(2024)
    day = np.where(rng.random(N) < 0.1, None, rng.integers(-3, 4, N) * 1000)
    f = rng.normal(size=N).astype(np.float32).astype(object)
    f[rng.random(N) < 0.2] = None
    lens = rng.integers(0, 4, N)
    leaves = rng.integers(0, 10 ** 12, int(lens.sum()))
    ends = np.cumsum(lens)
    return pd.DataFrame({
        "day": pd.array(day, dtype="Int64"),
        "tag": np.array(STRINGS, dtype=object)[rng.integers(0, 6, N)],
        "x": np.arange(N, dtype=np.int64),
        "f": pd.array(f, dtype="Float32"),
        "s": np.array(["u", "vv", "", "wörd"], dtype=object)[rng.integers(0, 4, N)],
        "l": [leaves[e - n: e].tolist() for e, n in zip(ends, lens)],
        "t": pd.to_datetime(rng.integers(0, 2 * 10 ** 18, N), unit="ns"),
    })


def parts(df):
    cut = 11_003
    return [df.iloc[:cut].reset_index(drop=True), df.iloc[:0].reset_index(drop=True),
            df.iloc[cut:].reset_index(drop=True)]


def dataset(df):
    return nvt.Dataset(parts(df))


def normal(got: pd.DataFrame, df: pd.DataFrame):
    """``got`` in input order with the input's dtypes, column by column comparable to ``df``."""
    got = got.sort_values("x").reset_index(drop=True)
    assert len(got) == len(df) and (got["x"].to_numpy() == df["x"].to_numpy()).all()
    out = {}
    for c in df.columns:
        if c in ("day", "f"):
            out[c] = pd.array(got[c].to_numpy(dtype=np.float64, na_value=np.nan), dtype="Float64")
        elif c == "l":
            out[c] = [list(map(int, v)) for v in got[c]]
        elif c in ("tag", "s"):
            out[c] = [None if v is None or v is pd.NA or (isinstance(v, float) and np.isnan(v)) else str(v) for v in got[c]]
        else:
            out[c] = got[c].to_numpy()
    return out


def assert_same_rows(got: pd.DataFrame, df: pd.DataFrame):
    got, want = normal(got, df), normal(df, df)
    for c in df.columns:
        if c in ("day", "f"):
            np.testing.assert_array_equal(got[c].to_numpy(dtype=np.float64, na_value=np.nan),
                                          want[c].to_numpy(dtype=np.float64, na_value=np.nan), err_msg=c)
        elif c in ("l", "tag", "s"):
            assert got[c] == want[c], c
        else:
            np.testing.assert_array_equal(got[c], want[c], err_msg=c)


def leaf_dirs(root):
    return sorted({os.path.relpath(os.path.dirname(f), root) for f in glob.glob(os.path.join(root, "**", "*.parquet"),
                                                                               recursive=True)})


def expected_dirs(df, keys=KEYS):
    tuples = {tuple(None if pd.isna(v) else v for v in t) for t in df[keys].itertuples(index=False, name=None)}
    return sorted(hive.dir_name(keys, t) for t in tuples)


def read_with_pyarrow(root):
    return pads.dataset(root, partitioning="hive", format="parquet",
                        ignore_prefixes=["_", "."]).to_table().to_pandas()


def read_with_dataset(root, **kw):
    ds = nvt.Dataset(root, **kw)
    frames = list(ds.to_iter())
    return ds, frames, pd.concat([f.to_pandas() for f in frames], ignore_index=True)


@pytest.fixture(scope="module")
def written(df, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hive") / "out")
    dataset(df).to_parquet(out, partition_on=KEYS, cats=["tag", "s"], conts=["f"], labels=["x"])
    return out


def test_round_trip_through_pyarrow(df, written):
    assert leaf_dirs(written) == expected_dirs(df)
    assert len(leaf_dirs(written)) == 8 * 6
    assert_same_rows(read_with_pyarrow(written), df)
    for d in leaf_dirs(written):
        files = glob.glob(os.path.join(written, d, "*.parquet"))
        assert [os.path.basename(f) for f in files] == ["part_0.parquet"]
        assert pq.read_schema(files[0]).names == DATA            # no key column in the files
        day, tag = (hive.decode_segment(hive.parse_dir(seg)[1]) for seg in d.split("/"))
        rows = df[(df["day"].isna() if day is None else (df["day"] == int(day)).fillna(False)) &
                  (df["tag"].isna() if tag is None else (df["tag"] == tag))]
        md = pq.ParquetFile(files[0])
        np.testing.assert_array_equal(md.read(columns=["x"]).column("x").to_numpy(), rows["x"].to_numpy())
        assert md.num_row_groups <= 2                             # one per input partition that has rows for it
    # the summary files: relative paths, the keys and their dtypes, index lists without the keys
    import json

    meta = json.load(open(os.path.join(written, "_metadata.json")))
    assert meta["partition_on"] == [{"col_name": "day", "dtype": "int64"}, {"col_name": "tag", "dtype": "string"}]
    assert sorted(e["file_name"] for e in meta["file_stats"]) == sorted(d + "/part_0.parquet" for d in leaf_dirs(written))
    assert sum(e["num_rows"] for e in meta["file_stats"]) == N
    assert [e["col_name"] for e in meta["cats"]] == ["s"] and [e["col_name"] for e in meta["labels"]] == ["x"]
    listed = open(os.path.join(written, "_file_list.txt")).read().split()
    assert int(listed[0]) == 48 and sorted(listed[1:]) == sorted(e["file_name"] for e in meta["file_stats"])
    assert pq.read_metadata(os.path.join(written, "_metadata")).num_rows == N


def test_round_trip_through_dataset(df, written, tmp_path):
    ds, frames, got = read_with_dataset(written)
    assert ds.schema.column_names == DATA + KEYS and list(got.columns) == DATA + KEYS      # key columns last
    assert ds.npartitions == len(frames) > 48
    assert all(f["day"].data.dtype == torch.int64 and f["tag"].strings is not None for f in frames)
    assert_same_rows(got, df)


def test_key_dtypes_recorded_and_inferred(df, tmp_path):
    small = df[["x", "s"]].copy()
    small["k"] = (df["x"] % 3).astype(np.int32)
    out = str(tmp_path / "out")
    nvt.Dataset(small).to_parquet(out, partition_on="k")
    assert leaf_dirs(out) == ["k=0", "k=1", "k=2"]
    ds, frames, got = read_with_dataset(out)
    assert ds.schema["k"].dtype == np.dtype("int32") and all(f["k"].data.dtype == torch.int32 for f in frames)
    np.testing.assert_array_equal(got.sort_values("x")["k"].to_numpy(), small["k"].to_numpy())
    os.remove(os.path.join(out, "_metadata.json"))
    ds, frames, got = read_with_dataset(out)                      # inferred: every segment is -?[0-9]+
    assert ds.schema["k"].dtype == np.dtype("int64") and all(f["k"].data.dtype == torch.int64 for f in frames)
    np.testing.assert_array_equal(got.sort_values("x")["k"].to_numpy(), small["k"].to_numpy())


@pytest.mark.parametrize("route", ["dictionary+snappy", "pyarrow-snappy", "per-partition-shuffle"])
def test_writer_routes(df, tmp_path, route):
    kw = {"dictionary+snappy": dict(use_dictionary=True, device_compression="snappy"),
          "pyarrow-snappy": dict(compression="snappy"),
          "per-partition-shuffle": dict(shuffle=nvt.io.Shuffle.PER_PARTITION, statistics=True)}[route]
    out = str(tmp_path / "out")
    dataset(df).to_parquet(out, partition_on=KEYS, **kw)
    assert leaf_dirs(out) == expected_dirs(df)
    assert_same_rows(read_with_pyarrow(out), df)
    some = glob.glob(os.path.join(out, leaf_dirs(out)[0], "*.parquet"))[0]
    md = pq.read_metadata(some)
    assert ("parquet-cpp" in (md.created_by or "")) == (route == "pyarrow-snappy")
    assert md.schema.names[:1] == ["x"] and "day" not in md.schema.names
    if route == "pyarrow-snappy":
        assert {md.row_group(0).column(i).compression for i in range(md.row_group(0).num_columns)} == {"SNAPPY"}


def test_read_through_pyarrow_route(df, written, monkeypatch):
    monkeypatch.setattr(nvt.io, "PLAIN_PARQUET_READ", False)
    ds, frames, got = read_with_dataset(written)
    assert list(got.columns) == DATA + KEYS
    assert_same_rows(got, df)


def test_dataset_pyarrow_wrote(df, tmp_path):
    root = str(tmp_path / "theirs")
    pq.write_to_dataset(pa.Table.from_pandas(df, preserve_index=False), root, partition_cols=KEYS)
    assert leaf_dirs(root) == expected_dirs(df)
    ds, frames, got = read_with_dataset(root)
    assert ds.schema.column_names == DATA + KEYS
    theirs = read_with_pyarrow(root)
    assert list(theirs.columns) == list(got.columns)
    assert_same_rows(got, theirs[df.columns].sort_values("x").reset_index(drop=True).astype({"day": "Int64"}))
    assert_same_rows(got, df)
    for f in ds.to_iter(columns=["tag", "x"]):
        assert f.columns == ["tag", "x"] and len(f["tag"]) == len(f["x"]) > 0
    only_keys = list(ds.to_iter(columns=["day"]))
    assert sum(len(f) for f in only_keys) == N and all(f.columns == ["day"] for f in only_keys)


def test_workflow_over_a_hive_dataset(df, written, tmp_path):
    def run(ds, where):
        wf = nvt.Workflow((["tag"] >> ops.Categorify(out_path=str(tmp_path / where))) +
                          (["f"] >> ops.FillMissing() >> ops.Normalize()))
        return wf.fit_transform(ds).to_ddf().compute().sort_values(["tag", "f"]).reset_index(drop=True)

    # (the hive dataset holds the rows in another order: compared as sorted multisets)
    flat, hived = run(dataset(df), "flat"), run(nvt.Dataset(written), "hive")
    assert len(flat) == len(hived) == N
    np.testing.assert_array_equal(hived["tag"].to_numpy(), flat["tag"].to_numpy())
    # float32 outputs of float64 moments summed in another partition order: a few ulps of float32
    np.testing.assert_allclose(hived["f"].to_numpy(), flat["f"].to_numpy(), rtol=1e-5, atol=1e-6)


def test_rejected_arguments(df, tmp_path):
    out = str(tmp_path / "few")
    with pytest.raises(ValueError, match="max_partitions"):
        dataset(df).to_parquet(out, partition_on=KEYS, max_partitions=3)
    for f in glob.glob(os.path.join(out, "**", "*.parquet"), recursive=True):
        pq.read_metadata(f)                                        # whatever is left has its footer
    assert glob.glob(os.path.join(out, "**", "*.parquet"), recursive=True) == []
    out = str(tmp_path / "float")
    os.makedirs(out)
    with pytest.raises(TypeError, match="cast it first"):
        dataset(df).to_parquet(out, partition_on=["f"])
    assert os.listdir(out) == []
    with pytest.raises(ValueError, match="max_partitions"):          # pyarrow's writer aborts the same way
        dataset(df).to_parquet(str(tmp_path / "few2"), partition_on=KEYS, max_partitions=3, compression="snappy")
    assert glob.glob(os.path.join(str(tmp_path / "few2"), "**", "*.parquet"), recursive=True) == []
