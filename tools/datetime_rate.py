#!/usr/bin/env python3
"""Rates of the two datetime kernels next to pandas on the host, for the same column.

  python tools/datetime_rate.py [--rows N] [--text-rows M] [--reps K] [--out FILE]

1. nvt_dt_field: N datetime64[ns] instants with 5 % NaT on the device, every field once per pass;
   the host does ``Series.dt.<field>`` on the same values.
2. nvt_csv_parse_datetime: a CSV of M rows ``id,ts`` (ISO-8601 with microseconds, 5 % empty) whose
   bytes are on the device and indexed already; the launch is timed alone, and the whole
   ``Dataset(engine="csv", parse_dates=["ts"])`` read beside it; the host does
   ``pd.to_datetime(text, format="ISO8601")`` on the column's strings (reading and splitting the file is
   not in its time).
Device times are HIP events around K back-to-back launches after a warm-up; host times are the
median of 3 passes.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("year", "month", "day", "hour", "minute", "second", "dayofweek", "dayofyear", "quarter")


def device_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_s(fn, passes=3):
    out = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def field_rates(rows, reps):
    import torch

    from nvtabular_amd import kernels_datetime as KD
    from nvtabular_amd.device import DeviceColumn

    rng = np.random.default_rng(0)
    ns = rng.integers(pd.Timestamp("1980-01-01").value, pd.Timestamp("2040-01-01").value, rows, dtype=np.int64)
    s = pd.Series(ns.view("datetime64[ns]"))
    s[rng.random(rows) < 0.05] = pd.NaT
    col = DeviceColumn.from_pandas(s, torch.device("cuda", torch.cuda.current_device()))
    out = {}
    for f in FIELDS:
        ms = device_ms(lambda: KD.dt_field(col.data, col.valid, "ns", f), reps)
        hs = host_s(lambda: getattr(s.dt, f))
        # bytes the kernel moves: 8 in, 4 out and an eighth of a byte of bitmap per row
        out[f] = {"device_ms": round(ms, 4), "device_rows_per_s": round(rows / ms * 1e3),
                  "device_GB_per_s": round(rows * 12.125 / ms / 1e6, 1),
                  "pandas_s": round(hs, 4), "pandas_rows_per_s": round(rows / hs)}
    return out


def write_csv(path, rows):
    rng = np.random.default_rng(1)
    us = rng.integers(pd.Timestamp("1980-01-01").value // 1000, pd.Timestamp("2040-01-01").value // 1000, rows)
    text = pd.Series(np.datetime_as_string(us.view("datetime64[us]"), unit="us").astype(object))   # YYYY-MM-DDTHH:MM:SS.ffffff
    text[rng.random(rows) < 0.05] = ""
    pd.DataFrame({"id": np.arange(rows), "ts": text}).to_csv(path, index=False)
    return text


def parse_rates(rows, reps):
    import torch

    import nvtabular_amd as nvt
    from nvtabular_amd import _lib
    from nvtabular_amd import kernels as K
    from nvtabular_amd import kernels_csv as KC
    from nvtabular_amd.csv_text import CsvSource

    lib = _lib.load()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "t.csv")
        text = write_csv(path, rows)
        size = os.path.getsize(path)
        src = CsvSource(path, parse_dates=["ts"], part_size=1 << 30)
        assert len(src.ranges) == 1
        buf, nbytes = src.read_range(0)
        dev = torch.device("cuda", torch.cuda.current_device())
        d_text = buf.to(dev)
        field_end, nfields, nrows, state, parity = KC.index_fields(d_text, nbytes, ord(","), ord('"'), 2)
        assert nrows == rows and nfields == 2 * rows and not parity
        data = torch.empty(rows, dtype=torch.int64, device=dev)
        valid = torch.empty(((rows + 63) // 64) * 8, dtype=torch.uint8, device=dev)
        desc = (_lib.CsvCol * 1)()
        desc[0].out, desc[0].out_valid, desc[0].k, desc[0].dtype = data.data_ptr(), valid.data_ptr(), 1, _lib.NVT_I64

        def launch():
            K.check(lib.nvt_csv_parse_datetime(d_text.data_ptr(), nbytes, field_end.data_ptr(), rows, 2, ord('"'), desc,
                                               1, state.data_ptr(), K.stream_ptr()), "nvt_csv_parse_datetime")

        ms = device_ms(launch, reps)
        exp = pd.to_datetime(text.where(text != "", None), format="ISO8601")
        got = data.cpu().numpy()
        ok = exp.notna().to_numpy()
        assert (got[ok] == exp.to_numpy().view(np.int64)[ok]).all() and (got[~ok] == 0).all()
        field_bytes = int(text.str.len().sum())

        def whole():
            for part in nvt.Dataset(path, engine="csv", parse_dates=["ts"]).to_iter():
                pass
            torch.cuda.synchronize()

        whole()
        ws = host_s(whole)
        strings = text.where(text != "", None)
        hs = host_s(lambda: pd.to_datetime(strings, format="ISO8601"))
        return {"rows": rows, "file_bytes": size, "field_bytes": field_bytes,
                "kernel_ms": round(ms, 4), "kernel_rows_per_s": round(rows / ms * 1e3),
                "kernel_field_GB_per_s": round(field_bytes / ms / 1e6, 2),
                "dataset_read_s": round(ws, 4), "dataset_rows_per_s": round(rows / ws),
                "pandas_to_datetime_s": round(hs, 4), "pandas_rows_per_s": round(rows / hs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--text-rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("datetime_rate.py measures on the GPU: none is visible")
    res = {"rows": a.rows, "fields": field_rates(a.rows, a.reps), "csv": parse_rates(a.text_rows, a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
