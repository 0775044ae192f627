"""Datetime columns without a GPU: the calendar function and the ISO-8601 parser of
nvt_datetime.hpp through their host entry points, the host conversions of DeviceColumn on
torch.device("cpu"), the parquet footer handling and the CSV options.  Every comparison is
integer-exact."""
import ctypes as C

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from nvtabular_amd import _lib, csv_text
from nvtabular_amd.device import DeviceColumn, DeviceFrame
from nvtabular_amd.parquet_plain import PlainParquetFile, PlainParquetWriter
from nvtabular_amd.schema import Schema

OK, INVALID, OVERFLOW = 0, 2, 3
UNITS = ("s", "ms", "us", "ns")
UNIT_CODE = {"s": _lib.DT_S, "ms": _lib.DT_MS, "us": _lib.DT_US, "ns": _lib.DT_NS}
PER_SECOND = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}
# pandas' attribute of every field code, in the order of NVT_DT_YEAR .. NVT_DT_QUARTER
FIELDS = ("year", "month", "day", "hour", "minute", "second", "dayofweek", "dayofyear", "quarter")
FIRST_NS, LAST_NS = "1677-09-21 00:12:43.145224193", "2262-04-11 23:47:16.854775807"
CPU = torch.device("cpu")


def fields_host(ts, unit, field):
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    out = np.full(len(ts), -7, dtype=np.int32)
    rc = _lib.load().nvt_dt_fields_host(ts.ctypes.data, len(ts), UNIT_CODE[unit], field, out.ctypes.data)
    assert rc == 0, _lib.load().nvt_last_error()
    return out


def parse_host(text):
    raw = text.encode()
    out = C.c_int64(-7)
    rc = _lib.load().nvt_csv_parse_datetime_host(raw, len(raw), C.byref(out))
    return rc, out.value


# ---- nvt_dt_fields_host ---------------------------------------------------------------------------
def test_fields_every_day_of_years_1_to_9999():
    days = np.arange(np.datetime64("0001-01-01", "D"), np.datetime64("10000-01-01", "D")).astype("datetime64[D]")
    assert len(days) == 3652059
    idx = pd.DatetimeIndex(days.astype("datetime64[s]"))
    ts = days.astype(np.int64) * 86400
    for code, name in enumerate(FIELDS):
        np.testing.assert_array_equal(fields_host(ts, "s", code), getattr(idx, name).to_numpy(), err_msg=name)


def _edge_instants(unit):
    """Counts in `unit` around the places the calendar arithmetic can go wrong."""
    k = PER_SECOND[unit]
    days = ["1969-12-31", "1970-01-01", "1970-01-02", "1900-02-28", "1900-03-01", "2000-02-29", "2000-03-01",
            "2100-02-28", "2100-03-01", "2024-12-31", "2023-12-31"]
    out = []
    for d in days:
        midnight = int(np.datetime64(d, "s").astype(np.int64)) * k
        out += [midnight - 1, midnight, midnight + 1, midnight + 86399 * k, midnight + 86400 * k - 1]
    if unit == "ns":
        out += [pd.Timestamp(FIRST_NS).value, pd.Timestamp(LAST_NS).value]
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("unit", UNITS)
def test_fields_edges_all_units(unit):
    ts = _edge_instants(unit)
    idx = pd.DatetimeIndex(ts.view(f"datetime64[{unit}]"))
    assert idx.dtype == np.dtype(f"datetime64[{unit}]")
    for code, name in enumerate(FIELDS):
        np.testing.assert_array_equal(fields_host(ts, unit, code), getattr(idx, name).to_numpy(),
                                      err_msg=f"{unit} {name}")


def test_fields_day_before_the_epoch_is_day_minus_one():
    ts = np.array([-1], dtype=np.int64)     # 1969-12-31 23:59:59
    got = [int(fields_host(ts, "s", f)[0]) for f in range(9)]
    assert got == [1969, 12, 31, 23, 59, 59, 2, 365, 4]


def test_fields_any_int64_is_defined():
    # (no result is specified out there; the call must come back and the time of day must be one)
    ts = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).min + 1, np.iinfo(np.int64).max], dtype=np.int64)
    for unit in UNITS:
        assert ((0 <= fields_host(ts, unit, _lib.DT_HOUR)) & (fields_host(ts, unit, _lib.DT_HOUR) < 24)).all()
        assert ((0 <= fields_host(ts, unit, _lib.DT_WEEKDAY)) & (fields_host(ts, unit, _lib.DT_WEEKDAY) < 7)).all()
        assert ((1 <= fields_host(ts, unit, _lib.DT_MONTH)) & (fields_host(ts, unit, _lib.DT_MONTH) <= 12)).all()


def test_fields_bad_arguments_and_empty():
    lib = _lib.load()
    ts = np.zeros(4, dtype=np.int64)
    out = np.full(4, -7, dtype=np.int32)
    for unit, field in ((-1, 0), (4, 0), (0, -1), (0, 9)):
        assert lib.nvt_dt_fields_host(ts.ctypes.data, 4, unit, field, out.ctypes.data) == _lib.NVT_EINVAL
    assert lib.nvt_dt_fields_host(None, 0, 0, 0, None) == 0          # n = 0: a no-op
    assert (out == -7).all()
    # the device entry validates before it touches the GPU
    assert lib.nvt_dt_field(ts.ctypes.data, None, 4, 7, 0, out.ctypes.data, None) == _lib.NVT_EINVAL
    assert lib.nvt_dt_field(ts.ctypes.data, None, 4, 0, 12, out.ctypes.data, None) == _lib.NVT_EINVAL
    assert lib.nvt_dt_field(None, None, 0, 0, 0, None, None) == 0


# ---- nvt_csv_parse_datetime_host ---------------------------------------------------------------
def _random_texts(n, seed):
    """n instants inside the nanosecond range, written in every optional shape of the grammar."""
    rng = np.random.default_rng(seed)
    lo, hi = pd.Timestamp(FIRST_NS).value, pd.Timestamp(LAST_NS).value
    # (a shorter shape cuts the instant off, which must not carry it below the first valid one)
    ns = rng.integers(pd.Timestamp("1677-09-22").value, hi, n, dtype=np.int64, endpoint=True)
    ns[:2] = lo, hi
    full = pd.DatetimeIndex(ns.view("datetime64[ns]")).strftime("%Y-%m-%d %H:%M:%S.%f").to_numpy()
    nano = ns % 1000
    shape = rng.integers(0, 12, n)       # 0 date, 1 minutes, 2 seconds, 3..11 that many fraction digits
    shape[:2] = 11
    sep = np.where(rng.random(n) < 0.5, "T", " ")
    texts = []
    for i in range(n):
        t = f"{full[i]}{nano[i]:03d}"    # YYYY-MM-DD HH:MM:SS.fffffffff
        t = t[:10] + sep[i] + t[11:]
        k = int(shape[i])
        texts.append(t[:10] if k == 0 else t[:16] if k == 1 else t[:19] if k == 2 else t[:20 + k - 2])
    return texts


def test_parse_random_instants_match_pandas():
    texts = _random_texts(100_000, 7)
    assert {len(t) for t in texts} == {10, 16, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29}
    exp = pd.to_datetime(pd.Series(texts), format="ISO8601")
    assert exp.dtype == np.dtype("datetime64[ns]")
    exp = exp.to_numpy().view(np.int64)
    lib = _lib.load()
    got = np.empty(len(texts), dtype=np.int64)
    out = C.c_int64()
    for i, t in enumerate(texts):
        raw = t.encode()
        assert lib.nvt_csv_parse_datetime_host(raw, len(raw), C.byref(out)) == OK, t
        got[i] = out.value
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("text", [FIRST_NS, LAST_NS, "2024-02-29", "2000-02-29T23:59", "1970-01-01 00:00:00",
                                  "1969-12-31 23:59:59.999999999", "2024-01-05 10:00:00.1", "2024-01-05T10:00:00.123456789"])
def test_parse_valid(text):
    assert parse_host(text) == (OK, pd.Timestamp(text).value)


def test_parse_extremes_are_the_int64_limits():
    assert parse_host(FIRST_NS) == (OK, np.iinfo(np.int64).min + 1)
    assert parse_host(LAST_NS) == (OK, np.iinfo(np.int64).max)


@pytest.mark.parametrize("text", ["2024-13-05", "2023-02-29", "2024-02-30", "2024-01-05 24:00:00",
                                  "2024-01-05 23:59:60", "2024-1-5", "20240105", "2024-01-05 10",
                                  "2024-01-05 10:00:00Z", " 2024-01-05", "2024-01-05 10:00:00.1234567891",
                                  "2024-00-05", "2024-01-00", "2024-04-31", "1900-02-29", "2024-01-05 10:60",
                                  "2024-01-05 ", "2024-01-05 10:00:00.", "2024-01-05  10:00", "2024-01-05t10:00",
                                  "2024-01-05 10:00:00+01:00", "2024/01/05", "-024-01-05", "2024-01-05 1o:00", ""])
def test_parse_invalid(text):
    assert parse_host(text) == (INVALID, -7)


@pytest.mark.parametrize("text", ["2262-04-11 23:47:16.854775808", "1677-09-21 00:12:43.145224192",
                                  "2262-04-12", "1677-09-20", "9999-12-31 23:59:59.999999999", "0001-01-01"])
def test_parse_overflow(text):
    assert parse_host(text) == (OVERFLOW, -7)


# ---- DeviceColumn on the host -------------------------------------------------------------------
def _series(unit, n=21):
    """n instants on both sides of the epoch with NaT in rows 0, 7, 8 and the last."""
    base = np.arange(n, dtype=np.int64) * 86_399 - 5 * 86_400 + 1
    s = pd.Series((base * PER_SECOND[unit] + 7 * (unit != "s")).view(f"datetime64[{unit}]"), name="ts")
    s[[0, 7, 8, n - 1]] = pd.NaT
    return s


@pytest.mark.parametrize("unit", UNITS)
def test_pandas_round_trip(unit):
    s = _series(unit)
    col = DeviceColumn.from_pandas(s, CPU)
    assert col.logical == np.dtype(f"datetime64[{unit}]") and col.data.dtype == torch.int64
    assert col.strings is None and col.offsets is None and col.fill is None
    mask = s.isna().to_numpy()
    np.testing.assert_array_equal(col.valid_mask_host(), ~mask)
    data = col.data.numpy()
    assert (data[mask] == 0).all()                                  # never INT64_MIN under a null
    np.testing.assert_array_equal(data[~mask], s.to_numpy().view(np.int64)[~mask])
    back = col.to_pandas("ts")
    assert back.dtype == s.dtype
    pd.testing.assert_series_equal(back, s)
    assert col.shallow_copy().logical == col.logical
    assert col.like(col.data[:3]).logical == col.logical


@pytest.mark.parametrize("unit", UNITS)
def test_pandas_round_trip_without_nulls(unit):
    s = _series(unit).dropna().reset_index(drop=True)
    col = DeviceColumn.from_pandas(s, CPU)
    assert col.valid is None
    pd.testing.assert_series_equal(col.to_pandas("ts"), s)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("tz", [None, "Europe/Berlin"])
def test_arrow_round_trip(unit, tz):
    s = _series(unit)
    arr = pa.Array.from_pandas(s, type=pa.timestamp(unit, tz))
    assert arr.null_count == 4
    col = DeviceColumn.from_arrow(arr, CPU)
    assert col.data.dtype == torch.int64 and col.logical == np.dtype(f"datetime64[{unit}]")
    mask = s.isna().to_numpy()
    np.testing.assert_array_equal(col.valid_mask_host(), ~mask)
    np.testing.assert_array_equal(col.data.numpy()[~mask], s.to_numpy().view(np.int64)[~mask])
    table = DeviceFrame({"ts": col}).to_arrow()
    assert table.column("ts").type == pa.timestamp(unit)           # the zone is dropped
    assert table.column("ts").combine_chunks().equals(arr.cast(pa.timestamp(unit)))
    pd.testing.assert_series_equal(col.to_pandas("ts"), s)


def test_arrow_counts_above_2_53_are_exact():
    v = np.array([(1 << 62) + 1, -(1 << 62) - 1, (1 << 53) + 1], dtype=np.int64)
    col = DeviceColumn.from_arrow(pa.array(v, type=pa.timestamp("ns")), CPU)
    np.testing.assert_array_equal(col.data.numpy(), v)
    sliced = pa.array(np.concatenate([[0], v]), type=pa.timestamp("ns"), mask=np.array([0, 0, 1, 0], bool))[1:]
    col = DeviceColumn.from_arrow(sliced, CPU)
    np.testing.assert_array_equal(col.valid_mask_host(), [True, False, True])
    np.testing.assert_array_equal(col.data.numpy()[[0, 2]], v[[0, 2]])


@pytest.mark.parametrize("unit", ["ns", "us"])
def test_tz_aware_comes_back_naive_utc(unit):
    s = pd.Series(pd.date_range("2024-03-30 22:00", periods=8, freq="h", tz="Europe/Berlin", unit=unit), name="ts")
    s[3] = pd.NaT
    col = DeviceColumn.from_pandas(s, CPU)
    assert col.logical == np.dtype(f"datetime64[{unit}]")
    exp = s.dt.tz_convert("UTC").dt.tz_localize(None)
    assert exp[0] == pd.Timestamp("2024-03-30 21:00")
    pd.testing.assert_series_equal(col.to_pandas("ts"), exp)


def test_schema_from_frame_reports_the_logical_dtype():
    frame = DeviceFrame({f"t_{u}": DeviceColumn.from_pandas(_series(u), CPU) for u in UNITS})
    frame["n"] = DeviceColumn(torch.arange(21))
    schema = Schema.from_frame(frame)
    for u in UNITS:
        assert schema[f"t_{u}"].dtype == np.dtype(f"datetime64[{u}]")
    assert schema["n"].dtype == np.dtype("int64")


def test_logical_is_keyword_only_and_checked():
    t = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        DeviceColumn(t, None, None, None, None, np.dtype("datetime64[ns]"))
    for bad in ("int64", "timedelta64[ns]", "datetime64[D]", "datetime64[2s]"):
        with pytest.raises(TypeError):
            DeviceColumn(t, logical=bad)
    assert DeviceColumn(t, logical="datetime64[ms]").logical == np.dtype("datetime64[ms]")
    assert DeviceColumn(t).logical is None


def test_take_and_slice_rows_keep_the_type():
    frame = DeviceFrame({"ts": DeviceColumn.from_pandas(_series("us", 24), CPU)})
    exp = _series("us", 24)
    idx = torch.tensor([23, 0, 5, 7, 9])
    got = frame.take_rows(idx)["ts"]
    assert got.logical == np.dtype("datetime64[us]")
    pd.testing.assert_series_equal(got.to_pandas("ts"), exp.iloc[idx.numpy()].reset_index(drop=True))
    got = frame.slice_rows(8, 20)["ts"]
    pd.testing.assert_series_equal(got.to_pandas("ts")[:12], exp.iloc[8:20].reset_index(drop=True))


# ---- parquet ----------------------------------------------------------------------------------------
def test_pyarrow_timestamp_file_is_eligible(tmp_path):
    n = 50
    v = (np.arange(n, dtype=np.int64) * 1_000_003 - 10_000_000) * 1000   # (whole microseconds as ns too)
    mask = np.zeros(n, bool)
    mask[[0, 7, 8, n - 1]] = True
    table = pa.table({
        "ms": pa.array(v, type=pa.timestamp("ms"), mask=mask),
        "us": pa.array(v, type=pa.timestamp("us"), mask=mask),
        "ns": pa.array(v, type=pa.timestamp("ns"), mask=mask),
        "tz": pa.array(v, type=pa.timestamp("us", "Europe/Berlin"), mask=mask),
        "x": pa.array(v),
    })
    for version in ("2.6", "1.0"):      # (1.0: legacy converted types only, ns is coerced to us)
        path = str(tmp_path / f"t{version}.parquet")
        pq.write_table(table, path, compression="none", use_dictionary=False, version=version)
        pf = PlainParquetFile(path)
        assert pf.eligible, pf.why
        assert pf.units == ["ms", "us", "ns" if version == "2.6" else "us", "us", None]
        assert pf.dtypes == [np.dtype("int64")] * 5


def test_date32_stays_ineligible(tmp_path):
    path = str(tmp_path / "d.parquet")
    pq.write_table(pa.table({"d": pa.array([1, 2], type=pa.date32())}), path)
    assert not PlainParquetFile(path).eligible


@pytest.mark.parametrize("unit", ["ms", "us", "ns"])
def test_plain_writer_timestamps_read_back_by_pyarrow(tmp_path, unit):
    n = 1000
    v = np.arange(n, dtype=np.int64) * 999_983 - 400_000_000
    ok = np.ones(n, bool)
    ok[[0, 7, 8, n - 1]] = False
    path = str(tmp_path / "w.parquet")
    w = PlainParquetWriter(path, ["ts", "plain", "full"], [np.int64, np.int64, np.int64],
                           logical=[np.dtype(f"datetime64[{unit}]"), None, f"datetime64[{unit}]"])
    w.write_row_group([(v[ok], np.packbits(ok, bitorder="little")), (v, None), (v, None)], n)
    w.close()
    table = pq.read_table(path)
    assert table.schema.field("ts").type == pa.timestamp(unit)
    assert table.schema.field("full").type == pa.timestamp(unit)
    assert table.schema.field("plain").type == pa.int64()
    assert table.column("ts").combine_chunks().equals(pa.array(v, type=pa.timestamp(unit), mask=~ok))
    assert table.column("full").combine_chunks().equals(pa.array(v, type=pa.timestamp(unit)))
    pf = PlainParquetFile(path)
    assert pf.eligible and pf.units == [unit, None, unit]


def test_plain_writer_refuses_seconds(tmp_path):
    with pytest.raises(TypeError):
        PlainParquetWriter(str(tmp_path / "s.parquet"), ["ts"], [np.int64], logical=["datetime64[s]"])


# ---- CSV options ------------------------------------------------------------------------------------
def _csv(tmp_path):
    p = tmp_path / "a.csv"
    p.write_text("id,ts,when\n1,2024-01-05 10:00:00,2024-01-05\n2,,2024-01-06\n")
    return str(p)


def test_csv_parse_dates_schema(tmp_path):
    src = csv_text.CsvSource(_csv(tmp_path), parse_dates=["ts"])
    assert src.dtypes == {"id": "int64", "ts": "datetime64[ns]", "when": "string"}   # not named: a string
    schema = src.schema()
    assert schema["ts"].dtype == np.dtype("datetime64[ns]")
    assert schema["when"].dtype == np.dtype(object)


def test_csv_parse_dates_reaches_the_source_from_dataset(tmp_path):
    from nvtabular_amd.io import Dataset

    ds = Dataset(_csv(tmp_path), engine="csv", parse_dates=["ts", "when"])
    assert ds.schema["ts"].dtype == ds.schema["when"].dtype == np.dtype("datetime64[ns]")


def test_csv_parse_dates_errors(tmp_path):
    p = _csv(tmp_path)
    with pytest.raises(ValueError, match="unknown column"):
        csv_text.CsvSource(p, parse_dates=["nope"])
    with pytest.raises(ValueError, match="list of column names"):
        csv_text.CsvSource(p, parse_dates=True)
    with pytest.raises(ValueError, match="both"):
        csv_text.CsvSource(p, parse_dates=["ts"], dtypes={"ts": "string"})
    with pytest.raises(TypeError, match="parse_dates"):
        csv_text.CsvSource(p, dtypes={"ts": "datetime64[ns]"})


# ---- the guard's view of dependency columns, lists of timestamps -------------------------------------
def test_guard_names_dependency_columns(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.node import iter_nodes

    frame = DeviceFrame({"k": DeviceColumn(torch.arange(21) % 3), "x": DeviceColumn(torch.rand(21)),
                         "ts": DeviceColumn.from_pandas(_series("ns"), CPU)})
    graphs = {
        "cont_cols": (["k"] >> ops.JoinGroupby(cont_cols=["ts"], stats=["mean"], out_path=str(tmp_path)), ["ts"]),
        "target": (["k"] >> ops.TargetEncoding("ts", kfold=1, p_smooth=5, out_path=str(tmp_path)), ["ts"]),
        "selected": (["ts"] >> ops.JoinGroupby(cont_cols=["x"], stats=["mean"], out_path=str(tmp_path)), ["ts"]),
        "numbers": (["k"] >> ops.JoinGroupby(cont_cols=["x"], stats=["mean"], out_path=str(tmp_path)), []),
    }
    for label, (graph, want) in graphs.items():
        wf = nvt.Workflow(graph).fit_schema(Schema.from_frame(frame))
        node = [n for n in iter_nodes(wf.output_node) if isinstance(n.op, (ops.JoinGroupby, ops.TargetEncoding))][0]
        assert node.op.datetime_rejects(node.input_columns, frame) == want, label


def test_lists_of_timestamps_are_not_the_type():
    arr = pa.array([[1, 2], [], [3]], type=pa.list_(pa.timestamp("ns")))
    col = DeviceColumn.from_arrow(arr, CPU)
    assert col.is_list and col.logical is None and col.data.dtype == torch.int64
    np.testing.assert_array_equal(col.data.numpy(), [1, 2, 3])
    with pytest.raises(TypeError, match="lists of datetime64"):
        DeviceColumn.from_pandas(pd.Series([[pd.Timestamp(1)], [pd.Timestamp(2)]]), CPU)
