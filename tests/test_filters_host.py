"""The host half of ``Dataset(filters=...)`` (nvtabular_amd/filters.py and Dataset construction): no
GPU.  Errors are raised when the Dataset is built; statistics pruning keeps exactly the row groups
that can hold a passing row, and never drops one that does (300 random DNFs against pyarrow); hive
pruning drops files on their path alone, before their footers are opened."""
import datetime
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import nvtabular_amd as nvt
from nvtabular_amd import filters as F


# ---- parsing and validation ---------------------------------------------------------------------------
def frame():
    return pd.DataFrame({
        "i": np.arange(6, dtype=np.int32), "f": np.arange(6, dtype=np.float32), "b": [True, False] * 3,
        "s": list("abcabc"), "t": pd.to_datetime(["2024-01-01"] * 6).astype("datetime64[ms]"),
        "l": [[1], [2, 3], [], [4], [5], [6]],
    })


def test_normalisation():
    assert F.normalize([("a", "=", 1)]) == [[("a", "==", 1)]]
    assert F.normalize((("a", "<", 1), ("b", "in", [1]))) == [[("a", "<", 1), ("b", "in", [1])]]
    assert F.normalize([[("a", "=", 1)], [("b", "not in", [2])]]) == [[("a", "==", 1)], [("b", "not in", [2])]]
    ds = nvt.Dataset(frame(), filters=[("i", "=", 2.0), ("s", "in", ["b", "a", "b"])])
    assert ds._filter.as_tuples() == [[("i", "==", 2), ("s", "in", ("a", "b"))]]
    assert ds.filter_stats == {"files_pruned": 0, "row_groups_pruned": 0, "row_groups_kept": 0, "rows_in": 0,
                               "rows_out": 0}
    assert nvt.Dataset(frame())._filter is None and nvt.Dataset(frame()).filter_stats is None
    # the schema does not change
    assert ds.schema == nvt.Dataset(frame()).schema


@pytest.mark.parametrize("bad", [[], [[]], [[("i", "==", 1)], []], [("i", "~", 1)], [("i", "is", None)],
                                 [("i", "==")], "i == 1", [("nope", "==", 1)], [[("i", "==", 1)], [("nope", "<", 2)]]])
def test_value_errors_at_construction(bad):
    with pytest.raises(ValueError):
        nvt.Dataset(frame(), filters=bad)


@pytest.mark.parametrize("bad", [
    [("s", "<", "b")], [("s", ">=", "b")], [("s", "==", 1)], [("s", "in", ["a", 2])], [("s", "in", "ab")],
    [("l", "==", 1)], [("i", "==", 1.5)], [("i", "==", "1")], [("i", "==", True)], [("i", "in", 3)],
    [("f", "==", "1")], [("f", "<", None)], [("b", "==", 1)], [("b", "==", "True")],
    [("t", ">", "2024-01-01")], [("t", ">", 5)], [("t", "==", datetime.date(2024, 1, 1))],
])
def test_type_errors_at_construction(bad):
    with pytest.raises(TypeError):
        nvt.Dataset(frame(), filters=bad)


def test_limits_and_datetime_units():
    wide = pd.DataFrame({f"c{k}": np.arange(3) for k in range(17)})
    nvt.Dataset(wide, filters=[(f"c{k}", ">=", 0) for k in range(16)])
    with pytest.raises(ValueError, match="16"):
        nvt.Dataset(wide, filters=[(f"c{k}", ">=", 0) for k in range(17)])
    nvt.Dataset(wide, filters=[[("c0", "!=", k)] for k in range(64)])
    with pytest.raises(ValueError, match="64"):
        nvt.Dataset(wide, filters=[[("c0", "!=", k)] for k in range(65)])
    with pytest.raises(ValueError, match="int64"):
        nvt.Dataset(wide, filters=[("c0", "==", 1 << 63)])
    for ok in (pd.Timestamp("2024-01-01 00:00:00.250"), datetime.datetime(2024, 1, 1, 0, 0, 1),
               np.datetime64("2024-01-01T00:00:00.001")):
        nvt.Dataset(frame(), filters=[("t", "<=", ok)])
    for bad in (pd.Timestamp("2024-01-01 00:00:00.000250"), np.datetime64("2024-01-01T00:00:00.000001"),
                datetime.datetime(2024, 1, 1, 0, 0, 0, 1)):
        with pytest.raises(ValueError, match="whole"):
            nvt.Dataset(frame(), filters=[("t", "<=", bad)])
    with pytest.raises(ValueError, match="callable"):
        nvt.Dataset(lambda: iter([]), filters=[("a", "==", 1)])
    flt = nvt.Dataset(frame(), filters=[("t", "==", pd.Timestamp("2024-01-01 00:00:01"))])._filter
    assert flt.as_tuples() == [[("t", "==", 1704067201000)]]


def test_errors_come_before_any_file_is_read(tmp_path):
    """A parquet source: the filter is checked against the footer's schema; a csv source: against the
    header."""
    p = str(tmp_path / "a.parquet")
    pq.write_table(pa.table({"x": [1, 2, 3], "s": ["a", "b", "c"]}), p)
    with pytest.raises(ValueError, match="nope"):
        nvt.Dataset(p, filters=[("nope", "==", 1)])
    with pytest.raises(TypeError):
        nvt.Dataset(p, filters=[("s", "<", "b")])
    c = str(tmp_path / "a.csv")
    pd.DataFrame({"x": [1, 2, 3], "y": [0.5, 1.5, 2.5]}).to_csv(c, index=False)
    with pytest.raises(ValueError, match="nope"):
        nvt.Dataset(c, filters=[("nope", "==", 1)])
    with pytest.raises(TypeError):
        nvt.Dataset(c, filters=[("x", "==", 0.5)])
    assert nvt.Dataset(c, filters=[("y", ">", 1)])._filter.as_tuples() == [[("y", ">", 1.0)]]


# ---- statistics pruning --------------------------------------------------------------------------------
def crafted(path):
    """8 row groups of 10 rows: x = 0..9, 10..19, ... (group 3 all null); f the same as floats, with
    a NaN in group 5; s = "k00".."k79"; t = that many seconds after 2024-01-01."""
    x = pa.array(np.arange(80, dtype=np.int64), mask=(np.arange(80) // 10 == 3))
    f = np.arange(80, dtype=np.float64)
    f[55] = np.nan
    s = pa.array([f"k{k:02d}" for k in range(80)])
    t = pa.array((np.datetime64("2024-01-01", "ms") + np.arange(80) * np.timedelta64(1, "s")), type=pa.timestamp("ms"))
    b = pa.array(np.arange(80) // 10 % 2 == 0)
    pq.write_table(pa.table({"x": x, "f": pa.array(f), "s": s, "t": t, "b": b}), path, row_group_size=10)
    return path


def kept_groups(path, filters, **kw):
    ds = nvt.Dataset(path, filters=filters, **kw)
    groups = [g for _, gs in ds._pieces for g in gs]
    st = ds.filter_stats
    assert st["row_groups_kept"] == len(groups) and st["row_groups_pruned"] == 8 - len(groups) and st["files_pruned"] == 0
    return groups


def test_statistics_pruning_per_operator(tmp_path):
    p = crafted(str(tmp_path / "c.parquet"))
    every, not3 = list(range(8)), [0, 1, 2, 4, 5, 6, 7]
    assert kept_groups(p, [("x", "==", 25)]) == [2]
    assert kept_groups(p, [("x", "==", 35)]) == []                 # the group of nulls: nothing passes ==
    assert kept_groups(p, [("x", "==", 100)]) == []
    assert kept_groups(p, [("x", "!=", 25)]) == every              # != never prunes
    assert kept_groups(p, [("x", "<", 20)]) == [0, 1]
    assert kept_groups(p, [("x", "<=", 20)]) == [0, 1, 2]
    assert kept_groups(p, [("x", ">", 59)]) == [6, 7]
    assert kept_groups(p, [("x", ">=", 59)]) == [5, 6, 7]
    assert kept_groups(p, [("x", "in", [5, 71, 35, 1000])]) == [0, 7]
    assert kept_groups(p, [("x", "in", [])]) == []
    assert kept_groups(p, [("x", "not in", [5])]) == every         # not in never prunes (a null passes it)
    assert kept_groups(p, [("x", ">=", 10), ("x", "<", 30)]) == [1, 2]
    assert kept_groups(p, [[("x", "<", 10)], [("x", ">", 69)]]) == [0, 7]
    assert kept_groups(p, [[("x", "<", 10)], [("s", "!=", "k05")]]) == every
    # a float group with a NaN: pyarrow writes min / max over the other values; a NaN statistic keeps
    assert kept_groups(p, [("f", "==", 52.0)]) == [5]
    assert kept_groups(p, [("f", ">", 60)]) == [6, 7]
    assert kept_groups(p, [("f", "<", 0.5)]) == [0]
    assert kept_groups(p, [("f", "in", [3, 77.0, 200])]) == [0, 7]
    # strings by range (== and in only), datetimes, bools
    assert kept_groups(p, [("s", "==", "k42")]) == [4]
    assert kept_groups(p, [("s", "in", ["k00", "k79", "zz"])]) == [0, 7]
    assert kept_groups(p, [("s", "!=", "k42")]) == every
    assert kept_groups(p, [("t", "<", pd.Timestamp("2024-01-01 00:00:10"))]) == [0]
    assert kept_groups(p, [("t", ">=", np.datetime64("2024-01-01T00:01:10"))]) == [7]
    assert kept_groups(p, [("b", "==", True)]) == [0, 2, 4, 6]
    assert kept_groups(p, [("b", "==", False), ("x", "<", 40)]) == [1]
    # several row groups per piece: pruned one by one, a piece that loses all of them disappears
    ds = nvt.Dataset(p, filters=[("x", "in", [25, 49, 71])], row_groups_per_part=3)
    assert [gs for _, gs in ds._pieces] == [[2], [4], [7]] and ds.npartitions == 3
    ds = nvt.Dataset(p, filters=[("x", ">=", 20)], row_groups_per_part=3)
    assert [gs for _, gs in ds._pieces] == [[2], [4, 5], [6, 7]]
    assert not3 == [g for g in every if g != 3]


def test_missing_or_unfit_statistics_keep_the_group(tmp_path):
    p = str(tmp_path / "nostats.parquet")
    pq.write_table(pa.table({"x": np.arange(40, dtype=np.int64), "f": np.full(40, np.nan)}), p, row_group_size=10,
                   write_statistics=False)
    ds = nvt.Dataset(p, filters=[("x", "==", 1000)])
    assert len(ds._pieces) == 4 and ds.filter_stats["row_groups_pruned"] == 0
    q = str(tmp_path / "nan.parquet")
    pq.write_table(pa.table({"f": np.full(40, np.nan)}), q, row_group_size=10)
    assert len(nvt.Dataset(q, filters=[("f", "<", 0)])._pieces) == 4         # no min / max over NaNs
    # a user schema that calls an int column float: the statistic's type does not fit the term
    from nvtabular_amd.schema import ColumnSchema, Schema

    r = crafted(str(tmp_path / "c.parquet"))
    schema = Schema([ColumnSchema("x", np.float64), ColumnSchema("f", np.float64)])
    assert len(nvt.Dataset(r, schema=schema, filters=[("x", "==", 1000.5)])._pieces) == 8


def soundness_files(tmp_path):
    rng = np.random.default_rng(3)
    paths = []
    for k in range(3):
        n = 240
        base = np.sort(rng.integers(0, 60, n)) if k < 2 else rng.integers(0, 60, n)
        i = pa.array(base.astype(np.int32), mask=rng.random(n) < 0.2)
        f = (base * 0.5 - 7).astype(np.float32)
        f[rng.random(n) < 0.05] = np.nan
        s = pa.array([f"w{v % 17:02d}" for v in base], mask=rng.random(n) < 0.1)
        t = pa.array(np.datetime64("2024-01-01", "ms") + base * np.timedelta64(1, "h"), type=pa.timestamp("ms"),
                     mask=rng.random(n) < 0.1)
        b = pa.array(base % 3 == 0, mask=rng.random(n) < 0.3)
        allnull = pa.array(np.zeros(n, dtype=np.int64), mask=np.ones(n, dtype=bool))
        p = str(tmp_path / f"s{k}.parquet")
        pq.write_table(pa.table({"i": i, "f": pa.array(f), "s": s, "t": t, "b": b, "z": allnull}), p,
                       row_group_size=20, write_statistics=(k != 1) or ["i", "s"])
        paths.append(p)
    return paths


def test_pruning_is_sound_against_pyarrow(tmp_path):
    """300 random DNFs over three files (sorted with statistics, sorted with statistics on two columns
    only, unsorted): every row group in which pyarrow finds a passing row is kept."""
    paths = soundness_files(tmp_path)
    rng = np.random.default_rng(99)
    consts = {"i": [0, 5, 17, 30, 59, 100, -1], "f": [-7.0, -6.75, 0.0, 3.5, 22.5, 100, -0.0],
              "s": ["w00", "w05", "w16", "w99", ""], "b": [True, False], "z": [0, 1],
              "t": [pd.Timestamp("2024-01-01") + pd.Timedelta(hours=h) for h in (0, 7, 30, 59, 500)]}
    pruned = 0
    for _ in range(300):
        dnf = []
        for _ in range(rng.integers(1, 4)):
            conj = []
            for _ in range(rng.integers(1, 4)):
                c = list(consts)[rng.integers(0, len(consts))]
                ops = [op for op in F.OPS if not (c == "s" and op in F.ORDERED)]
                op = ops[rng.integers(0, len(ops))]
                pool = consts[c]
                if op in ("in", "not in"):
                    v = [pool[j] for j in rng.permutation(len(pool))[: rng.integers(1, 4)]]
                else:
                    v = pool[rng.integers(0, len(pool))]
                conj.append((c, op, v))
            dnf.append(conj)
        ds = nvt.Dataset(paths, filters=dnf)
        kept = {(f, g) for f, gs in ds._pieces for g in gs}
        pruned += ds.filter_stats["row_groups_pruned"]
        assert ds.filter_stats["row_groups_pruned"] + ds.filter_stats["row_groups_kept"] == 36
        for f in paths:
            pf = pq.ParquetFile(f)
            expr = pq.filters_to_expression(dnf)
            for g in range(pf.num_row_groups):
                if (f, g) not in kept:
                    assert pf.read_row_group(g).filter(expr).num_rows == 0, (dnf, f, g)
    assert pruned > 1000         # (the check above is not vacuous)


# ---- hive pruning -------------------------------------------------------------------------------------
def hive_tree(root):
    days, sites = [1, 2, 3, None], ["a", "b b", None]
    rows = []
    for d in days:
        for s in sites:
            for k in range(4):
                rows.append({"x": len(rows), "day": d, "site": s})
    df = pd.DataFrame(rows)
    table = pa.Table.from_pandas(df, preserve_index=False).cast(
        pa.schema([("x", pa.int64()), ("day", pa.int64()), ("site", pa.string())]))
    pq.write_to_dataset(table, root, partition_cols=["day", "site"])
    return df


def dirs_of(ds, root):
    return sorted({os.path.relpath(os.path.dirname(f), root) for f, _ in ds._pieces})


NULL = "__HIVE_DEFAULT_PARTITION__"


def test_hive_pruning(tmp_path):
    root = str(tmp_path / "h")
    hive_tree(root)
    full = nvt.Dataset(root)
    assert len(full._pieces) == 12 and full.schema.column_names == ["x", "day", "site"]
    # garbage in a directory that every filter below prunes: its footer must never be opened
    junk = os.path.join(root, "day=3", "site=a", "junk.parquet")
    with open(junk, "wb") as fh:
        fh.write(b"this is not a parquet file")
    with pytest.raises(Exception):
        nvt.Dataset(root)

    def check(filters, want_dirs, pruned):
        ds = nvt.Dataset(root, filters=filters)
        assert dirs_of(ds, root) == sorted(want_dirs), filters
        assert ds.filter_stats["files_pruned"] == pruned, (filters, ds.filter_stats)
        assert ds.schema.column_names == ["x", "day", "site"]
        return ds

    sites = ["site=a", "site=b%20b", f"site={NULL}"]
    # an int64 key (13 files: the junk file counts)
    check([("day", "==", 1)], [f"day=1/{s}" for s in sites], 10)
    check([("day", "<", 3), ("day", ">", 1)], [f"day=2/{s}" for s in sites], 10)
    check([("day", "in", [1, 2, 7])], [f"day={d}/{s}" for d in (1, 2) for s in sites], 7)
    # a string key
    check([("site", "==", "b b"), ("day", "!=", 3)], ["day=1/site=b%20b", "day=2/site=b%20b"], 11)   # (a null fails !=)
    check([("site", "in", ["b b", "zz"]), ("day", "<=", 2)], ["day=1/site=b%20b", "day=2/site=b%20b"], 11)
    # the null directory: a null passes `not in` and fails ==
    check([("site", "not in", ["a", "b b"])], [f"day={d}/site={NULL}" for d in (1, 2, 3, NULL)], 9)
    check([("day", "not in", [1, 2, 3])], [f"day={NULL}/{s}" for s in sites], 10)
    check([("day", "==", 2), ("site", "==", "a")], ["day=2/site=a"], 12)
    check([("day", "not in", [3]), ("site", "!=", "a")], [f"day={d}/site=b%20b" for d in (1, 2)] +
          [f"day={NULL}/site=b%20b"], 10)
    # an OR of two conjunctions on different keys
    check([[("day", "==", 1)], [("site", "==", "b b"), ("day", "!=", 3)]],
          [f"day=1/{s}" for s in sites] + ["day=2/site=b%20b"], 9)
    # a data column next to a key: the key prunes files, the statistics prune row groups
    ds = check([("day", "==", 1), ("x", ">=", 8)], ["day=1/site=" + NULL], 10)
    assert ds.filter_stats["row_groups_pruned"] == 2 and ds.filter_stats["row_groups_kept"] == 1
    # nothing survives: an empty dataset, not an error (the schema comes from the first file)
    os.remove(junk)
    ds = check([("day", "==", 9)], [], 12)
    assert ds.npartitions == 0
    # ordered comparisons on a string key and unknown keys are refused like any column's
    with pytest.raises(TypeError):
        nvt.Dataset(root, filters=[("site", "<", "b")])
    with pytest.raises(TypeError):
        nvt.Dataset(root, filters=[("day", "==", "1")])
