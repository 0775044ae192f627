"""``Dataset(path, filters=...)`` end to end on the device: the rows every consumer sees are the rows
``pyarrow.parquet.read_table(path, filters=...)`` returns -- for a file the hand-written reader takes,
one it leaves to pyarrow (a uint32 column) and files written by ``to_parquet(statistics=True)``; with
and without the prefetch thread; for ``to_iter(columns=...)`` without the filter's columns; for a hive
tree, the csv engine and frames in memory; through ``Workflow.fit`` / ``transform``, the dataloader and
both parquet writers.  5000 rows in row groups of 700, so that row groups and the 2048-row tiles of
the compaction do not coincide."""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.dataset as pads
import pyarrow.parquet as pq
import pytest

import filter_terms_reference as R

pytestmark = pytest.mark.gpu

N = 5000
T0 = pd.Timestamp("2024-03-01")


def make_frame(seed=17, n=N):
    rng = np.random.default_rng(seed)
    words = np.array(["a", "b", "zebra", "é", "longer string"], dtype=object)
    df = pd.DataFrame({
        "row": np.arange(n, dtype=np.int64),
        "k": np.arange(n, dtype=np.int64),                                   # sorted: row groups get pruned
        "i": pd.array(rng.integers(-3, 8, n), dtype="Int32"),
        "f": (rng.integers(-8, 9, n) * 0.25).astype(np.float32),
        "d": rng.normal(size=n),
        "b": rng.random(n) < 0.5,
        "s": words[rng.integers(0, len(words), n)],
        "t": (np.datetime64(T0, "ms") + rng.integers(0, 96, n) * np.timedelta64(1, "h")).astype("datetime64[ms]"),
        "y": rng.integers(0, 2, n).astype(np.int64),
    })
    df.loc[rng.random(n) < 0.1, "i"] = pd.NA
    df.loc[rng.random(n) < 0.05, "f"] = np.nan
    df.loc[rng.random(n) < 0.1, "s"] = None
    df.loc[rng.random(n) < 0.1, "t"] = pd.NaT
    return df


def arrow_of(df, extra=None):
    fields = {"row": pa.int64(), "k": pa.int64(), "i": pa.int32(), "f": pa.float32(), "d": pa.float64(),
              "b": pa.bool_(), "s": pa.string(), "t": pa.timestamp("ms"), "y": pa.int64()}
    cols = {c: pa.array(df[c], type=t, from_pandas=True) for c, t in fields.items() if c in df}
    for name, arr in (extra or {}).items():
        cols[name] = arr
    return pa.table(cols)


FILTERS = [
    [("k", "<", 1000)],
    [("k", ">=", 4000), ("i", "==", 3)],
    [("i", "in", [1, 2, 3])],
    [("i", "not in", [0, 1])],
    [("i", ">", 1.0), ("i", "<=", 5)],
    [("f", ">", 0.5)],
    [("f", "!=", 0.25)],
    [("f", "in", [0.25, -1.5])],
    [("d", "<=", 0.0), ("d", ">", -1)],
    [("b", "==", True)],
    [("b", "!=", True), ("k", ">", 2500)],
    [("s", "==", "b")],
    [("s", "in", ["a", "zebra", "nope"])],
    [("s", "not in", ["a"])],
    [("s", "!=", "é"), ("f", "<", 1.0)],
    [("t", ">=", T0 + pd.Timedelta(hours=24)), ("t", "<", np.datetime64("2024-03-03", "ms"))],
    [("t", "in", [T0, T0 + pd.Timedelta(hours=5)])],
    [[("k", "<", 300)], [("k", ">", 4700), ("s", "==", "a")]],
    [[("i", "==", 7), ("b", "==", False)], [("f", "<", -1.5)], [("t", "==", T0), ("k", ">=", 700), ("k", "<", 2100)]],
    [("k", "in", [])],
    [("k", "==", -5)],
]
IDS = [str(i) for i in range(len(FILTERS))]


def same_rows(got: pd.DataFrame, want: pd.DataFrame, columns=None):
    """The same columns in the same order and the same values; dtypes as each side's conventions give
    them (an int column with nulls is float64 on one side and Int32 on the other, ...)."""
    columns = list(want.columns) if columns is None else columns
    assert list(got.columns) == columns, (list(got.columns), columns)
    assert len(got) == len(want), (len(got), len(want))
    if len(want) == 0:
        return
    for c in columns:
        g, w = got[c].reset_index(drop=True), want[c].reset_index(drop=True)
        gn, wn = g.isna().to_numpy(), w.isna().to_numpy()
        np.testing.assert_array_equal(gn, wn, err_msg=f"{c}: nulls")
        np.testing.assert_array_equal(_values(g[~gn]), _values(w[~wn]), err_msg=c)


def _values(s: pd.Series):
    if s.dtype.kind == "M":
        return s.to_numpy().astype("datetime64[ms]")
    if pd.api.types.is_numeric_dtype(s.dtype) or pd.api.types.is_bool_dtype(s.dtype):
        return s.to_numpy(dtype=np.float64)          # (exact for every value these tests hold)
    vals = s.to_numpy()
    if len(vals) and isinstance(vals[0], (bool, np.bool_, int, float, np.number)):
        return vals.astype(np.float64)               # (an object column of bools / numbers next to nulls)
    return vals


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The frame and three copies of it on disk: {kind: (path for Dataset, path for pyarrow)}."""
    import nvtabular_amd as nvt
    from nvtabular_amd.parquet_plain import PlainParquetFile

    tmp = tmp_path_factory.mktemp("dsfilters")
    df = make_frame()
    plain = str(tmp / "plain.parquet")
    pq.write_table(arrow_of(df), plain, row_group_size=700)
    assert PlainParquetFile(plain).decodable
    fallback = str(tmp / "fallback.parquet")
    u = pa.array((np.arange(N) % 977).astype(np.uint32))
    pq.write_table(arrow_of(df, {"u": u}), fallback, row_group_size=700)
    assert not PlainParquetFile(fallback).decodable
    own = str(tmp / "own")
    nvt.Dataset(df, npartitions=7).to_parquet(own, statistics=True)
    assert len([f for f in os.listdir(own) if f.endswith(".parquet")]) == 7
    return df, {"plain": plain, "fallback": fallback, "own": own}


def pyarrow_read(path, filters, columns=None):
    return pq.read_table(path, filters=filters, columns=columns).to_pandas()


@pytest.mark.parametrize("filters", FILTERS, ids=IDS)
@pytest.mark.parametrize("kind", ["plain", "fallback", "own"])
def test_compute_equals_pyarrow(files, kind, filters):
    import nvtabular_amd as nvt

    df, paths = files
    ds = nvt.Dataset(paths[kind], filters=filters)
    want = pyarrow_read(paths[kind], filters)
    got = ds.compute()
    same_rows(got, want)
    st = ds.filter_stats
    assert st["rows_out"] == len(want) and st["rows_in"] >= st["rows_out"]
    if kind != "own":
        groups = -(-N // 700)
        assert st["row_groups_kept"] + st["row_groups_pruned"] == groups and st["row_groups_kept"] == ds.npartitions
        md = pq.ParquetFile(paths[kind]).metadata
        assert st["rows_in"] == sum(md.row_group(g).num_rows for _, gs in ds._pieces for g in gs)
        first = filters[0][0] if isinstance(filters[0], list) else filters[0]
        if first[0] == "k":
            assert st["row_groups_pruned"] > 0       # k is sorted: its statistics prune


def test_prefetch_and_plain_iteration_agree(files):
    import nvtabular_amd as nvt

    df, paths = files
    filters = [[("k", "<", 1500), ("s", "!=", "a")], [("f", "in", [0.5, 1.0]), ("k", ">", 3000)]]
    want = pyarrow_read(paths["plain"], filters)
    for prefetch in (True, False):
        ds = nvt.Dataset(paths["plain"], filters=filters)
        parts = [p.to_pandas() for p in ds.to_iter(prefetch=prefetch)]
        assert len(parts) == ds.npartitions
        same_rows(pd.concat(parts, ignore_index=True), want)
        assert ds.filter_stats["rows_out"] == len(want)
    # head() sees the filtered rows too (the first partition keeps more than 3 rows)
    same_rows(nvt.Dataset(paths["plain"], filters=filters).head(3), want.head(3))


def test_to_iter_columns_without_the_filter_columns(files):
    import nvtabular_amd as nvt

    df, paths = files
    filters = [("k", ">=", 600), ("k", "<", 3000), ("s", "in", ["a", "b"])]
    want = pyarrow_read(paths["plain"], filters)[["d", "i"]]
    for kind in ("plain", "fallback"):
        for prefetch in (True, False):
            ds = nvt.Dataset(paths[kind], filters=filters)
            parts = list(ds.to_iter(columns=["d", "i"], prefetch=prefetch))
            assert all(p.columns == ["d", "i"] for p in parts)
            same_rows(pd.concat([p.to_pandas() for p in parts], ignore_index=True), want)
    # ... and a column of the filter that is asked for stays
    ds = nvt.Dataset(paths["plain"], filters=filters)
    parts = list(ds.to_iter(columns=["s", "d"]))
    assert all(p.columns == ["s", "d"] for p in parts)


def test_hive_tree_equals_pyarrow_dataset(files, tmp_path):
    import nvtabular_amd as nvt

    df, _ = files
    h = df[["row", "i", "f", "s"]].copy()
    h["day"] = (df["k"] // 1000).astype(np.int64)
    h["site"] = np.where(df["k"] % 3 == 0, None, np.where(df["k"] % 3 == 1, "x", "y y"))
    table = pa.table({"row": pa.array(h["row"]), "i": pa.array(h["i"], type=pa.int32(), from_pandas=True),
                      "f": pa.array(h["f"]), "s": pa.array(h["s"], type=pa.string(), from_pandas=True),
                      "day": pa.array(h["day"]), "site": pa.array(h["site"], type=pa.string(), from_pandas=True)})
    root = str(tmp_path / "hive")
    pq.write_to_dataset(table, root, partition_cols=["day", "site"], max_rows_per_group=300)
    part = pads.partitioning(pa.schema([("day", pa.int64()), ("site", pa.string())]), flavor="hive")
    cases = [
        [("day", "==", 2)],
        [("day", "in", [0, 4]), ("site", "==", "y y")],
        [("site", "not in", ["x"]), ("i", ">", 2)],
        [("site", "!=", "x"), ("f", "<=", 0.0)],
        [[("day", "<", 1), ("s", "==", "a")], [("site", "==", "x"), ("day", ">=", 4), ("i", "in", [0, 1])]],
    ]
    for filters in cases:
        ds = nvt.Dataset(root, filters=filters)
        got = ds.compute()
        want = pads.dataset(root, partitioning=part).to_table(filter=pq.filters_to_expression(filters)).to_pandas()
        assert list(got.columns) == ["row", "i", "f", "s", "day", "site"]      # the key columns last, in path order
        same_rows(got.sort_values("row"), want.sort_values("row")[list(got.columns)])
        assert ds.filter_stats["files_pruned"] > 0 and ds.filter_stats["rows_out"] == len(want)
        assert len(want) > 0


def reference_rows(df, filters):
    from nvtabular_amd.filters import normalize

    cols = {}
    for c in df.columns:
        valid = df[c].notna().to_numpy()
        vals = df[c].to_numpy(dtype=np.float64, na_value=0) if str(df[c].dtype) == "Int32" else df[c].to_numpy()
        if str(df[c].dtype) == "Int32":
            vals = vals.astype(np.int64)
        cols[c] = (vals, valid)
    return df[R.keep_mask(normalize(filters), cols, len(df))].reset_index(drop=True)


MEMORY_FILTERS = [
    [("i", ">=", 2), ("f", "<", 1.0)],
    [("s", "in", ["a", "é"])],
    [[("f", "in", [0.5])], [("i", "not in", [1, 2, 3]), ("s", "!=", "b")]],
    [("d", ">", 0.25), ("y", "==", 1)],
]


@pytest.mark.parametrize("filters", MEMORY_FILTERS, ids=[str(i) for i in range(len(MEMORY_FILTERS))])
def test_frames_in_memory(files, filters):
    import nvtabular_amd as nvt

    df, _ = files
    src = df[["row", "i", "f", "d", "s", "y"]]
    ds = nvt.Dataset(src, npartitions=3, filters=filters)
    want = reference_rows(src, filters)
    assert 0 < len(want) < N
    same_rows(ds.compute(), want)
    assert ds.filter_stats["rows_in"] == N and ds.filter_stats["rows_out"] == len(want)
    # shuffle_by_keys sees the filtered rows
    out = ds.shuffle_by_keys("y", npartitions=2).compute()
    same_rows(out.sort_values("row"), want.sort_values("row"))


def test_csv_engine(files, tmp_path):
    import nvtabular_amd as nvt

    df, _ = files
    src = pd.DataFrame({"row": df["row"], "k": df["k"], "f": df["f"].astype(np.float64), "y": df["y"],
                        "w": np.where(df["k"] % 2 == 0, "even", "odd")})
    path = str(tmp_path / "t.csv")
    src.to_csv(path, index=False)
    for filters in ([("k", ">=", 100), ("f", ">", 0.0), ("w", "==", "odd")],
                    [[("f", "in", [0.25, 2.0])], [("w", "not in", ["odd"]), ("k", "<", 50)]]):
        ds = nvt.Dataset(path, engine="csv", part_size=16384, filters=filters)
        assert ds.npartitions > 1
        want = reference_rows(src, filters)
        assert 0 < len(want) < N
        same_rows(ds.compute(), want)
        assert ds.filter_stats["rows_in"] == N and ds.filter_stats["rows_out"] == len(want)


def test_empty_partitions_stay_and_a_workflow_fits_over_them(files, tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df, paths = files
    filters = [("f", ">", 1.75)]                      # no statistics-pruning on f: partitions stay
    src = df[["row", "k", "f", "d", "s"]].copy()
    src.loc[src["k"] >= 1200, "f"] = 0.0             # ... and every partition but the first loses all rows
    ds = nvt.Dataset(src, npartitions=4, filters=filters)
    lens = [len(p) for p in ds.to_iter()]
    assert len(lens) == 4 and lens[0] > 0 and lens[1:] == [0, 0, 0]
    empty = list(ds.to_iter())[2]
    assert empty.columns == list(src.columns) and len(empty) == 0
    wf = nvt.Workflow((["s"] >> ops.Categorify(out_path=str(tmp_path / "c"))) + (["d"] >> ops.Normalize()))
    wf.fit(ds)
    out = wf.transform(ds).to_ddf().compute()
    assert len(out) == lens[0]
    # a parquet partition filtered to 0 rows by the kernel, not by the statistics
    pds = nvt.Dataset(paths["plain"], filters=[("f", "==", 0.125)])
    assert pds.npartitions == 8 and [len(p) for p in pds.to_iter()] == [0] * 8


def test_workflow_equals_the_same_on_prefiltered_rows(files, tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df, paths = files
    filters = [[("k", "<", 2000), ("f", ">=", 0.0)], [("s", "in", ["zebra", "b"]), ("k", ">", 3500)]]
    want = pyarrow_read(paths["plain"], filters)
    assert 500 < len(want) < N

    def run(ds, out):
        norm = ["d"] >> ops.Normalize()
        wf = nvt.Workflow((["s", "y"] >> ops.Categorify(out_path=str(tmp_path / out))) + norm)
        wf.fit(ds)
        return wf.transform(ds).to_ddf().compute(), norm.op

    got, gop = run(nvt.Dataset(paths["plain"], filters=filters), "a")
    exp, eop = run(nvt.Dataset(want[["s", "y", "d"]]), "b")
    assert len(got) == len(exp) == len(want)
    for c in ("s", "y"):
        np.testing.assert_array_equal(got[c].to_numpy(), exp[c].to_numpy(), err_msg=c)    # bit-equal indices
    # means / stds: 1e-6 relative, the tolerance of test_gpu_parity.py
    assert abs(gop.means["d"] - eop.means["d"]) <= 1e-6 * abs(eop.means["d"])
    assert abs(gop.stds["d"] - eop.stds["d"]) <= 1e-6 * abs(eop.stds["d"])
    np.testing.assert_allclose(got["d"].to_numpy(), exp["d"].to_numpy(), rtol=1e-6, atol=1e-6)


def test_dataloader_counts_the_filtered_rows(files):
    import nvtabular_amd as nvt
    from nvtabular_amd.loader.torch import TorchAsyncItr

    df, paths = files
    filters = [("k", ">=", 650), ("k", "<", 4100), ("b", "==", True)]
    want = pyarrow_read(paths["plain"], filters)
    for ds in (nvt.Dataset(paths["plain"], filters=filters),
               nvt.Dataset(df[["k", "d", "b", "y"]], npartitions=3, filters=filters)):
        loader = TorchAsyncItr(ds, cats=["k"], conts=["d"], labels=["y"], batch_size=256)
        assert len(loader) == -(-len(want) // 256)
        seen, ks = 0, []
        for x, y in loader:
            seen += int(y.shape[0])
            ks.append(x["k"].reshape(-1).cpu().numpy())
        assert seen == len(want)
        np.testing.assert_array_equal(np.sort(np.concatenate(ks)), np.sort(want["k"].to_numpy()))


@pytest.mark.parametrize("writer", ["plain", "pyarrow"])
def test_to_parquet_writes_the_filtered_rows(files, tmp_path, writer):
    import nvtabular_amd as nvt

    df, paths = files
    filters = [[("k", "<", 900), ("s", "!=", "a")], [("t", ">=", T0 + pd.Timedelta(hours=48)), ("k", ">", 4200)]]
    want = pyarrow_read(paths["plain"], filters)
    out = str(tmp_path / writer)
    kw = {} if writer == "plain" else {"compression": "snappy"}
    nvt.Dataset(paths["plain"], filters=filters).to_parquet(out, **kw)
    back = pq.read_table(out).to_pandas()
    same_rows(back.sort_values("row"), want.sort_values("row"))
