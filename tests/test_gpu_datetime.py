"""Datetime columns on the device: nvt_dt_field against the same function on the host, LambdaOp's
``.dt`` route, ISO-8601 columns of the CSV engine, timestamps through the hand-written parquet
reader and writer, the type through every row-moving path, and the operator guard.  Every
comparison is integer-exact; the frames have 1000 rows."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import _lib, ops, parquet_plain
from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap
from nvtabular_amd.selector import ColumnSelector

pytestmark = pytest.mark.gpu

UNITS = ("s", "ms", "us", "ns")
UNIT_CODE = {"s": _lib.DT_S, "ms": _lib.DT_MS, "us": _lib.DT_US, "ns": _lib.DT_NS}
PER_SECOND = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}
N = 1000
NS = np.dtype("datetime64[ns]")
GUARD = r"column 'ts' is datetime64\[ns\]; convert it first"


def dev():
    return torch.device("cuda", torch.cuda.current_device())


# ---- nvt_dt_field against nvt_dt_fields_host -----------------------------------------------------------
def _counts(unit, n, rng):
    """n counts in `unit` inside years 1 to 9999 (ns: the whole int64 range but the NaT pattern)."""
    if unit == "ns":
        return rng.integers(np.iinfo(np.int64).min + 1, np.iinfo(np.int64).max, n, dtype=np.int64, endpoint=True)
    k = PER_SECOND[unit]
    return rng.integers(-62135596800 * k, 253402300800 * k, n, dtype=np.int64)


@pytest.mark.parametrize("unit", UNITS)
def test_dt_field_matches_host(unit):
    lib = _lib.load()
    rng = np.random.default_rng(11)
    stream = torch.cuda.current_stream().cuda_stream
    for n in (1, 63, 64, 65, 127, 129, 1000):
        ts = _counts(unit, n, rng)
        ok = np.ones(n, dtype=bool)
        ok[[i for i in (0, 62, 63, 64, 65, 126, 127, 128, n - 1) if i < n and n > 1]] = False
        poisoned = ts.copy()
        poisoned[~ok] = np.iinfo(np.int64).min      # a null row's slot is never a result
        bitmap = torch.from_numpy(pack_bitmap(ok)).to(dev())
        for base in (0, 1):         # (1: `ts` is 8 but not 16 bytes aligned)
            srcs = []
            for host_counts in (ts, poisoned):
                buf = torch.zeros(n + 2, dtype=torch.int64, device=dev())
                buf[base:base + n] = torch.from_numpy(host_counts).to(dev())
                srcs.append(buf[base:])
                assert srcs[-1].data_ptr() % 16 == 8 * base
            for field in range(9):
                exp = np.empty(n, dtype=np.int32)
                assert lib.nvt_dt_fields_host(ts.ctypes.data, n, UNIT_CODE[unit], field, exp.ctypes.data) == 0
                # without a bitmap every slot is a result; with one a null row is 0 whatever its slot holds
                cases = ((srcs[0], None, exp, 1), (srcs[1], bitmap, np.where(ok, exp, 0), 1),
                         (srcs[1], bitmap, np.where(ok, exp, 0), 2))
                for src, valid, want, at in cases:     # (at: `out` starts 4 or 8 bytes into its buffer)
                    out = torch.full((n + 4,), -7, dtype=torch.int32, device=dev())
                    rc = lib.nvt_dt_field(src.data_ptr(), valid.data_ptr() if valid is not None else None, n,
                                          UNIT_CODE[unit], field, out[at:].data_ptr(), stream)
                    assert rc == 0, lib.nvt_last_error()
                    got = out.cpu().numpy()
                    np.testing.assert_array_equal(got[at:at + n], want,
                                                  err_msg=f"{unit} field {field} n {n} base {base} at {at}")
                    assert (got[:at] == -7).all() and (got[at + n:] == -7).all()


# ---- the 1000-row frame --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    rng = np.random.default_rng(3)
    ns = rng.integers(pd.Timestamp("1960-01-01").value, pd.Timestamp("2035-01-01").value, N, dtype=np.int64)
    ns[:40] = ns[40:80]                                   # ties for the sort, repeats for Categorify
    full = pd.Series(ns.view(NS))
    ts = full.copy()
    ts[rng.random(N) < 0.1] = pd.NaT
    ts[[0, 63, 64, N - 1]] = pd.NaT
    return pd.DataFrame({"k": rng.integers(0, 37, N).astype(np.int64), "ts": ts, "full": full,
                         "x": rng.random(N)})


@pytest.fixture(scope="module")
def frame(host):
    return DeviceFrame.from_pandas(host, dev())


def _ts_equal(got: pd.Series, exp: pd.Series, unit="ns"):
    assert got.dtype == np.dtype(f"datetime64[{unit}]"), got.dtype
    np.testing.assert_array_equal(got.isna().to_numpy(), exp.isna().to_numpy())
    np.testing.assert_array_equal(got.to_numpy().view(np.int64), exp.to_numpy().view(np.int64))


# ---- LambdaOp --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ts", "full"])
@pytest.mark.parametrize("what", ["hour", "weekday", "seconds"])
def test_lambdaop_on_device_equals_pandas(host, frame, name, what):
    f = {"hour": lambda c: c.dt.hour, "weekday": lambda c: c.dt.weekday,
         "seconds": lambda c: c.astype("datetime64[s]")}[what]
    op = ops.LambdaOp(f)
    out = op.transform(ColumnSelector([name]), frame)
    assert op.last_path == "device"
    got, exp = out[name].to_pandas(name), f(host[name])
    assert got.dtype == exp.dtype, (got.dtype, exp.dtype)
    if what == "seconds":
        assert out[name].logical == np.dtype("datetime64[s]")
        _ts_equal(got, exp, "s")
    else:
        assert exp.dtype == (np.float64 if name == "ts" else np.int32)
        np.testing.assert_array_equal(got.to_numpy(), exp.to_numpy())


def test_lambdaop_other_surface_equals_pandas(host, frame):
    cases = {
        "fields": lambda c: c.dt.year * 10000 + c.dt.month * 100 + c.dt.day + c.dt.dayofyear + c.dt.quarter
        + c.dt.minute + c.dt.second + c.dt.day_of_week,
        "int64": lambda c: c.astype("int64"),
        "isna": lambda c: c.isna(),
        "notna": lambda c: c.notna(),
        "from_int": lambda c: (c.astype("int64") // 1000000000).astype("datetime64[s]"),
        "compare": lambda c, df: c <= df["full"],
        "differs": lambda c, df: c != df["full"],
    }
    for label, f in cases.items():
        for name in ("ts", "full"):
            if label == "from_int" and name == "ts":
                continue        # (NaT as INT64_MIN // 10^9 is a count, not a NaT, in pandas as here)
            op = ops.LambdaOp(f)
            out = op.transform(ColumnSelector([name]), frame)
            assert op.last_path == "device", label
            got = out[name].to_pandas(name)
            exp = f(host[name], host) if label in ("compare", "differs") else f(host[name])
            assert got.dtype == exp.dtype, (label, name, got.dtype, exp.dtype)
            if exp.dtype.kind == "M":
                _ts_equal(got, exp, "s")
            else:
                np.testing.assert_array_equal(got.to_numpy(), exp.to_numpy(), err_msg=f"{label} {name}")


def test_lambdaop_floor_goes_to_the_host_and_stays_a_datetime(host, frame):
    op = ops.LambdaOp(lambda c: c.dt.floor("D"))
    out = op.transform(ColumnSelector(["ts"]), frame)
    assert op.last_path == "host"
    assert out["ts"].logical == NS and out["ts"].data.is_cuda
    _ts_equal(out["ts"].to_pandas("ts"), host["ts"].dt.floor("D"))
    for f in (lambda c: c + pd.Timedelta(days=1), lambda c: c.dt.strftime("%Y"), lambda c: c.dt.tz_localize("UTC")):
        op = ops.LambdaOp(f)
        op.transform(ColumnSelector(["full"]), frame)
        assert op.last_path == "host"


# ---- CSV -------------------------------------------------------------------------------------------------
def _csv_rows(n, rng):
    """(text of every field, expected instant or None) for two timestamp columns in every shape."""
    def one(i):
        if i % 11 == 3:
            return "", None
        ns = int(rng.integers(pd.Timestamp("1700-01-01").value, pd.Timestamp("2250-01-01").value))
        t = pd.Timestamp(ns).strftime("%Y-%m-%d %H:%M:%S.%f") + f"{ns % 1000:03d}"
        t = t[:10] + ("T" if i % 2 else " ") + t[11:]
        k = i % 12
        t = t[:10] if k == 0 else t[:16] if k == 1 else t[:19] if k == 2 else t[:20 + k - 2]
        return t, t
    return [(one(i), one(i + 5)) for i in range(n)]


def test_csv_parse_dates_against_pandas(tmp_path):
    rng = np.random.default_rng(5)
    n = 400
    rows = _csv_rows(n, rng)
    lines = ["a_ts,id,s,z_ts"]
    for i, ((ta, _), (tz, _)) in enumerate(rows):
        a = f'"{ta}"' if i % 3 == 0 else ta             # quoted (an empty quoted field is empty too)
        lines.append(f"{a},{i},w{i % 7},{tz}")
    text = "\r\n".join(lines) + "\r\n"
    assert len(text) > 3 * _lib.CSV_TILE
    path = tmp_path / "t.csv"
    path.write_bytes(text.encode())
    body = len(text) - len(lines[0]) - 2
    ds = nvt.Dataset(str(path), engine="csv", parse_dates=["a_ts", "z_ts"], part_size=body // 3 + 1)
    assert ds.npartitions == 3
    parts = list(ds.to_iter())
    assert sum(len(p) for p in parts) == n
    for name, j in (("a_ts", 0), ("z_ts", 1)):
        exp = pd.to_datetime(pd.Series([r[j][1] for r in rows]), format="ISO8601")
        assert exp.dtype == NS and exp.isna().sum() > 10
        got = pd.concat([p[name].to_pandas(name) for p in parts], ignore_index=True)
        for p in parts:
            assert p[name].logical == NS and p[name].data.dtype == torch.int64
            m = p[name].valid_mask_host()
            assert (p[name].data.cpu().numpy()[~m] == 0).all()
        _ts_equal(got, exp)
    ids = np.concatenate([p["id"].data.cpu().numpy() for p in parts])
    np.testing.assert_array_equal(ids, np.arange(n))
    # through a Workflow: the canonical UDF on a column read from text
    wf = nvt.Workflow(["a_ts"] >> ops.LambdaOp(lambda c: c.dt.hour))
    got = wf.fit_transform(ds).to_ddf().compute()["a_ts"]
    exp = pd.to_datetime(pd.Series([r[0][1] for r in rows]), format="ISO8601").dt.hour
    np.testing.assert_array_equal(got.to_numpy(), exp.to_numpy())


@pytest.mark.parametrize("bad, what", [("2024-02-30", "calendar"), ("2024-01-05 10:00:00Z", "calendar"),
                                       ("2262-04-11 23:47:16.854775808", "range")])
def test_csv_malformed_field_names_row_and_column(tmp_path, bad, what):
    lines = ["id,ts"] + [f"{i},2024-01-05 10:00:{i % 60:02d}" for i in range(300)]
    lines[1 + 217] = f"217,{bad}"
    path = tmp_path / "bad.csv"
    path.write_text("\n".join(lines) + "\n")
    ds = nvt.Dataset(str(path), engine="csv", parse_dates=["ts"])
    with pytest.raises(ValueError) as e:
        list(ds.to_iter())
    msg = str(e.value)
    assert "row 217" in msg and "column 'ts'" in msg and repr(bad) in msg and what in msg


# ---- parquet ---------------------------------------------------------------------------------------------
def test_parquet_in_transform_out_stays_on_the_hand_written_path(tmp_path, host):
    mask = host["ts"].isna().to_numpy()
    ns = host["full"].to_numpy().view(np.int64)
    table = pa.table({
        "t_us": pa.array(ns // 1000, type=pa.timestamp("us"), mask=mask),
        "t_ns": pa.array(ns, type=pa.timestamp("ns"), mask=mask),
        "t_ms": pa.array(ns // 1000000, type=pa.timestamp("ms", "UTC")),
        "x": pa.array(host["x"].to_numpy()),
    })
    src = str(tmp_path / "in.parquet")
    pq.write_table(table, src, row_group_size=400)
    before = dict(parquet_plain.READER_CHUNKS)
    ds = nvt.Dataset(src, engine="parquet", row_groups_per_part=2)
    for c, u in (("t_us", "us"), ("t_ns", "ns"), ("t_ms", "ms")):
        assert ds.schema[c].dtype == np.dtype(f"datetime64[{u}]")
    wf = nvt.Workflow(["t_us", "t_ns", "t_ms", "x"] >> ops.AddTags(["user"]))
    out_dir = str(tmp_path / "out")
    wf.transform(ds).to_parquet(out_dir)
    assert parquet_plain.READER_CHUNKS["pyarrow"] == before["pyarrow"]
    assert parquet_plain.READER_CHUNKS["plain"] == before["plain"] + 3 * 4
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".parquet"))
    assert len(files) == 2
    for f in files:
        assert pq.read_metadata(os.path.join(out_dir, f)).created_by == "nvtabular_amd plain writer"
    got = pa.concat_tables([pq.read_table(os.path.join(out_dir, f)) for f in files])
    for c in ("t_us", "t_ns", "t_ms", "x"):
        want = table.column(c)
        if c == "t_ms":
            want = want.cast(pa.timestamp("ms"))          # the zone is dropped, the instants stay
        assert got.column(c).type == want.type, c
        assert got.column(c).combine_chunks().equals(want.combine_chunks()), c


def test_seconds_column_is_written_by_pyarrow(tmp_path, host):
    s = host["ts"].astype("datetime64[s]")
    out_dir = str(tmp_path / "sec")
    nvt.Dataset(DeviceFrame.from_pandas(pd.DataFrame({"ts": s}), dev())).to_parquet(out_dir)
    path = os.path.join(out_dir, "part_0.parquet")
    assert pq.read_metadata(path).created_by != "nvtabular_amd plain writer"
    back = pq.read_table(path).column("ts").to_pandas()
    np.testing.assert_array_equal(back.isna().to_numpy(), s.isna().to_numpy())
    np.testing.assert_array_equal(back.to_numpy().astype("datetime64[s]").view(np.int64)[~s.isna()],
                                  s.to_numpy().view(np.int64)[~s.isna()])


# ---- propagation ------------------------------------------------------------------------------------------
def test_filter_and_dropna_keep_the_type(host, frame):
    out = ops.Filter(f=lambda df: df[df["x"] > 0.5]).transform(ColumnSelector(list(frame.columns)), frame)
    exp = host[host["x"] > 0.5].reset_index(drop=True)
    assert out["ts"].logical == NS and out["full"].logical == NS
    _ts_equal(out["ts"].to_pandas("ts"), exp["ts"])
    _ts_equal(out["full"].to_pandas("full"), exp["full"])
    out = ops.Dropna().transform(ColumnSelector(["ts"]), frame)
    exp = host.dropna(subset=["ts"]).reset_index(drop=True)
    assert len(out) == len(exp) < N
    _ts_equal(out["ts"].to_pandas("ts"), exp["ts"])
    _ts_equal(out["full"].to_pandas("full"), exp["full"])
    np.testing.assert_array_equal(out["k"].data.cpu().numpy(), exp["k"].to_numpy())


def test_filter_then_dropna_through_a_workflow(host, frame):
    op = ops.Filter(f=lambda df: df[df["x"] < 0.25])
    wf = nvt.Workflow(["k", "ts", "x"] >> op >> ops.Dropna())
    got = wf.transform(nvt.Dataset(frame)).to_ddf().compute()
    exp = host[host["x"] < 0.25][["k", "ts", "x"]].dropna().reset_index(drop=True)
    _ts_equal(got["ts"], exp["ts"])
    np.testing.assert_array_equal(got["k"].to_numpy(), exp["k"].to_numpy())


@pytest.mark.parametrize("label", ["notna", "hour", "compare"])
def test_filter_predicate_on_a_datetime_column(host, frame, label):
    f = {"notna": lambda df: df[df["ts"].notna()],
         "hour": lambda df: df[(df["ts"].dt.hour < 12) & (df["full"].dt.year >= 1990)],
         "compare": lambda df: df[(df["ts"] <= df["full"]) & (df["x"] < 0.5)]}[label]
    op = ops.Filter(f=f)
    out = op.transform(ColumnSelector(list(frame.columns)), frame)
    assert op.last_path == "device"
    exp = f(host).reset_index(drop=True)
    assert 0 < len(exp) < N and len(out) == len(exp)
    _ts_equal(out["ts"].to_pandas("ts"), exp["ts"])
    _ts_equal(out["full"].to_pandas("full"), exp["full"])
    np.testing.assert_array_equal(out["k"].data.cpu().numpy(), exp["k"].to_numpy())


def _sorted_rows(df):
    """Rows in an order that does not depend on how they were partitioned."""
    key = pd.DataFrame({"k": df["k"].to_numpy(), "x": df["x"].to_numpy()})
    return df.iloc[np.lexsort((key["x"], key["k"]))].reset_index(drop=True)


@pytest.mark.parametrize("key", ["ts", "k"])
def test_shuffle_by_keys_as_key_and_as_carried_column(host, frame, key):
    halves = [frame.take_rows(torch.arange(0, 504, device=dev())), frame.take_rows(torch.arange(504, N, device=dev()))]
    out = nvt.Dataset(halves).shuffle_by_keys(key, npartitions=4)
    parts = list(out.to_iter())
    assert len(parts) == 4 and sum(len(p) for p in parts) == N
    seen = {}
    for i, p in enumerate(parts):
        assert p["ts"].logical == NS and p["full"].logical == NS
        df = p.to_pandas()
        assert df["ts"].dtype == NS
        for v in df[key].to_numpy().view(np.int64) if key == "ts" else df[key].to_numpy():
            assert seen.setdefault(int(v), i) == i         # one key value, one partition (NaT too)
    got = _sorted_rows(pd.concat([p.to_pandas() for p in parts], ignore_index=True))
    exp = _sorted_rows(host)
    _ts_equal(got["ts"], exp["ts"])
    _ts_equal(got["full"], exp["full"])


@pytest.mark.parametrize("how", ["left", "inner"])
def test_join_external_carries_datetimes_on_both_sides(host, frame, how):
    rng = np.random.default_rng(9)
    keys = np.arange(0, 37, 2, dtype=np.int64)        # half of the keys match
    born = pd.Series(rng.integers(0, 2 * 10 ** 18, len(keys)).view(NS))
    born[[1, 5]] = pd.NaT
    ext = pd.DataFrame({"k": keys, "born": born, "born_us": born.astype("datetime64[us]")})
    op = ops.JoinExternal(ext, on="k", how=how)
    out = op.transform(ColumnSelector(list(frame.columns)), frame)
    exp = host.merge(ext, on="k", how=how).reset_index(drop=True)
    assert len(out) == len(exp)
    got = out.to_pandas()
    np.testing.assert_array_equal(got["k"].to_numpy(), exp["k"].to_numpy())
    _ts_equal(got["ts"], exp["ts"])
    _ts_equal(got["full"], exp["full"])
    _ts_equal(got["born"], exp["born"])
    _ts_equal(got["born_us"], exp["born_us"], "us")
    with pytest.raises(TypeError, match="datetime"):
        keyed = ext[["born", "born_us"]].rename(columns={"born": "ts"})
        nvt.Workflow(["ts", "x"] >> ops.JoinExternal(keyed, on="ts")).transform(nvt.Dataset(frame)).to_ddf().compute()


def test_take_rows_keeps_the_type(host, frame):
    idx = np.random.default_rng(2).permutation(N)[:333]
    out = frame.take_rows(torch.from_numpy(idx).to(dev()))
    assert out["ts"].logical == NS
    _ts_equal(out["ts"].to_pandas("ts"), host["ts"].iloc[idx].reset_index(drop=True))


def test_groupby_sort_first_last_list_count(host, frame):
    op = ops.Groupby(groupby_cols=["k"], sort_cols=["ts"], aggs={"ts": ["first", "last", "list", "count"]})
    wf = nvt.Workflow(["k", "ts"] >> op)
    out = wf.transform(frame)
    for c in ("ts_first", "ts_last", "ts_list"):
        assert out[c].logical == NS, c
    assert out["ts_list"].is_list and out["ts_count"].logical is None
    got = out.to_pandas()
    ordered = host.sort_values("ts", kind="stable", na_position="last")
    groups = ordered.groupby("k", sort=True)["ts"]
    np.testing.assert_array_equal(got["k"].to_numpy(), np.array(sorted(host["k"].unique())))
    # first / last are the first / last ROW of the ordered group (a NaT sorts last), as in cuDF
    _ts_equal(got["ts_first"], groups.apply(lambda s: s.iloc[0]).reset_index(drop=True))
    _ts_equal(got["ts_last"], groups.apply(lambda s: s.iloc[-1]).reset_index(drop=True))
    np.testing.assert_array_equal(got["ts_count"].to_numpy(), groups.count().to_numpy())
    assert got["ts_count"].dtype == np.int32
    for row, (_, s) in zip(got["ts_list"], groups):
        assert row.dtype == NS
        np.testing.assert_array_equal(np.isnat(row), s.isna().to_numpy())
        np.testing.assert_array_equal(row.view(np.int64)[~np.isnat(row)], s.to_numpy().view(np.int64)[~s.isna()])
    # a datetime key column comes back as one
    out = nvt.Workflow(["full", "x"] >> ops.Groupby(groupby_cols=["full"], aggs={"x": "count"})).transform(frame)
    assert out["full"].logical == NS
    _ts_equal(out["full"].to_pandas("full"), pd.Series(np.sort(host["full"].unique())))


# ---- the guard and the operators that take the counts -------------------------------------------------------
def test_guard_rejects_operators_that_compute_on_numbers(host, frame, tmp_path):
    ds = nvt.Dataset(frame)
    graphs = {
        "Normalize": ["ts"] >> ops.Normalize(),
        "DifferenceLag": ["ts"] >> ops.DifferenceLag("k"),
        "Groupby": ["k", "ts"] >> ops.Groupby(groupby_cols=["k"], aggs={"ts": ["count", "mean"]}),
        "Clip": ["ts"] >> ops.Clip(min_value=0),
        # dependency columns, which no selector names: cont_cols and the target
        "JoinGroupby": ["k"] >> ops.JoinGroupby(cont_cols=["ts"], stats=["mean"], out_path=str(tmp_path / "jg")),
        "TargetEncoding": ["k"] >> ops.TargetEncoding("ts", kfold=1, p_smooth=5, out_path=str(tmp_path / "te")),
        "FillMissing": ["ts"] >> ops.FillMissing(),
    }
    for label, graph in graphs.items():
        with pytest.raises(TypeError, match=GUARD) as e:
            nvt.Workflow(graph).fit_transform(ds).to_ddf().compute()
        assert str(e.value).startswith(f"{label}: ")
        assert "LambdaOp(lambda c: c.dt.hour)" in str(e.value)
    # the documented way out
    graph = ["ts"] >> ops.LambdaOp(lambda c: c.dt.hour) >> ops.FillMissing(-1) >> ops.Normalize()
    out = nvt.Workflow(graph).fit_transform(ds).to_ddf().compute()
    assert len(out) == N and out["ts"].notna().all()


def test_categorify_and_hashbucket_see_the_int64_counts(host, frame, tmp_path):
    as_int = DeviceFrame({"ts": DeviceColumn(frame["ts"].data, frame["ts"].valid)})
    outs = []
    for i, f in enumerate((frame[["ts"]], as_int)):
        wf = nvt.Workflow(["ts"] >> ops.Categorify(out_path=str(tmp_path / f"c{i}")))
        out = wf.fit_transform(nvt.Dataset(f)).to_ddf().compute()
        outs.append(out["ts"].to_numpy())
    assert outs[0].dtype.kind == "i" and outs[0].max() > 800
    np.testing.assert_array_equal(outs[0], outs[1])
    outs = [nvt.Workflow(["ts"] >> ops.HashBucket(100)).transform(f)["ts"] for f in (frame[["ts"]], as_int)]
    assert outs[0].logical is None
    np.testing.assert_array_equal(outs[0].data.cpu().numpy(), outs[1].data.cpu().numpy())


def test_pass_through_operators_leave_the_column_alone(host, frame):
    graph = ["ts", "k"] >> ops.ReduceDtypeSize() >> ops.Rename(postfix="_r") >> ops.AddTags(["item"])
    wf = nvt.Workflow(graph)
    out = wf.fit_transform(nvt.Dataset(frame))
    assert wf.output_schema["ts_r"].dtype == NS
    part = next(iter(out.to_iter()))
    assert part["ts_r"].logical == NS and part["k_r"].data.dtype == torch.int8
    _ts_equal(part["ts_r"].to_pandas("ts_r"), host["ts"])


def test_dataloader_null_row_of_an_arrow_column_is_zero():
    from nvtabular_amd.loader.torch import TorchAsyncItr

    n = 300
    counts = np.arange(1, n + 1, dtype=np.int64) * 10 ** 9
    ok = np.ones(n, dtype=bool)
    ok[[0, 63, 64, 65, n - 1]] = False
    slots = counts.copy()
    slots[~ok] = np.iinfo(np.int64).min            # what Arrow leaves under a NaT
    arr = pa.Array.from_buffers(pa.timestamp("ns"), n, [pa.py_buffer(np.packbits(ok, bitorder="little")),
                                                        pa.py_buffer(slots)])
    assert arr.null_count == 5
    col = DeviceColumn.from_arrow(arr, dev())
    assert col.logical == NS
    frame = DeviceFrame({"ts": col, "x": DeviceColumn(torch.arange(n, dtype=torch.float32, device=dev()))})
    loader = TorchAsyncItr(nvt.Dataset(frame), batch_size=128, cats=["ts"], conts=["x"], shuffle=False)
    got = np.concatenate([x["ts"].reshape(-1).cpu().numpy() for x, _ in loader])
    np.testing.assert_array_equal(got, np.where(ok, counts, 0))


def test_lists_of_timestamps_are_not_the_type():
    arr = pa.array([[1, 2], [], [3]], type=pa.list_(pa.timestamp("ns")))
    col = DeviceColumn.from_arrow(arr, dev())
    assert col.is_list and col.logical is None and col.data.dtype == torch.int64
    np.testing.assert_array_equal(col.data.cpu().numpy(), [1, 2, 3])
    with pytest.raises(TypeError, match="lists of datetime64"):
        DeviceColumn.from_pandas(pd.Series([[pd.Timestamp(1)], [pd.Timestamp(2)]]), dev())


def test_dataloader_hands_out_the_counts(host, frame):
    from nvtabular_amd.loader.torch import TorchAsyncItr

    ds = nvt.Dataset(frame[["full", "x"]])
    loader = TorchAsyncItr(ds, batch_size=256, cats=["full"], conts=["x"], shuffle=False)
    got = []
    for x, _ in loader:
        t = x["full"]
        assert t.dtype == torch.int64
        got.append(t.reshape(-1).cpu().numpy())
    np.testing.assert_array_equal(np.concatenate(got), host["full"].to_numpy().view(np.int64))
