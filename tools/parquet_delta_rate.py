"""Dataset(path) of a DELTA_BINARY_PACKED + snappy file: the hand-written parquet reader
(io.PLAIN_PARQUET_READ on: delta pages staged on the host, nvt_pq_delta_decode on the device) against
the pyarrow path (the switch off: what such a file took before the reader knew delta pages),
alternating, in one process.  The file, written by pyarrow: an increasing int64 id, a timestamp[us]
and a random int32 column, `rows` rows in row groups of 1 Mi.

A read is every partition of ``Dataset(path).to_iter()`` on the device, timed to
``torch.cuda.synchronize()`` behind it: 2 warm-up rounds, then `runs` timed ones.  Then one partition
is taken apart: host staging, the bytes that cross PCIe per value, and ``fill_holes`` alone (HIP
events, median of 20; the three launches apart come from a kernel trace of this script).  Prints one
JSON line at the end.

    python tools/parquet_delta_rate.py [rows] [runs] [out_dir]"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

import nvtabular_amd as nvt
from nvtabular_amd import io as nio
from nvtabular_amd import kernels_parquet_delta as KPD
from nvtabular_amd import parquet_plain as PP


def read(path):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = list(nvt.Dataset(path).to_iter())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, sum(len(p) for p in parts)


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_dir = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="pq_delta_")
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(0)
    table = pa.table({
        "id": pa.array(np.cumsum(rng.integers(1, 100, rows)) + 10**12),
        "ts": pa.array(np.int64(1_700_000_000_000_000) + np.cumsum(rng.integers(0, 10**6, rows)), type=pa.timestamp("us")),
        "r": pa.array(rng.integers(-2**31, 2**31, rows).astype(np.int32)),
    })
    path = os.path.join(out_dir, "delta.parquet")
    pq.write_table(table, path, column_encoding={c: "DELTA_BINARY_PACKED" for c in table.column_names},
                   use_dictionary=False, compression="snappy", row_group_size=1 << 20)
    res = {"rows": rows, "file_bytes": os.path.getsize(path)}
    times = {True: [], False: []}
    for k in range(2 + runs):
        for on in (True, False):
            nio.PLAIN_PARQUET_READ = on
            before = dict(PP.READER_CHUNKS)
            dt, n = read(path)
            assert n == rows and (PP.READER_CHUNKS["pyarrow"] == before["pyarrow"]) == on
            if k >= 2:
                times[on].append(dt)
    res["reader_s"] = statistics.median(times[True])
    res["pyarrow_s"] = statistics.median(times[False])
    # one partition (row group 0) taken apart
    pf = PP.PlainParquetFile(path)
    t0 = time.perf_counter()
    staged = PP.read_row_groups_staged(pf, [0])
    res["host_stage_s"] = time.perf_counter() - t0
    n0 = pf.row_groups[0]["num_rows"]
    crossing = sum(sc.delta.nbytes + 16 * sc.delta.nmbs + 40 * sc.delta.npages for sc in staged.values())
    res["pcie_bytes_per_value"] = crossing / (n0 * len(staged))
    res["plain_bytes_per_value"] = sum(sc.values.element_size() for sc in staged.values()) / len(staged)
    dev = torch.device("cuda")
    items = [(sc.delta, torch.empty(sc.nvalid, dtype=sc.values.dtype, device=dev)) for sc in staged.values()]
    ev = []
    for _ in range(22):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        KPD.fill_holes(items)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    res["fill_holes_ms"] = statistics.median(a.elapsed_time(b) for a, b in ev[2:])
    res["fill_holes_values"] = n0 * len(staged)
    for (_, out), name in zip(items, staged):
        want = table.column(name).slice(0, n0).cast(pa.int64() if name == "ts" else table.schema.field(name).type)
        assert np.array_equal(out.cpu().numpy(), want.to_numpy()), name
    print(json.dumps(res))
    if len(sys.argv) <= 3:
        shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
