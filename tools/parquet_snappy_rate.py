"""to_parquet in four modes -- default, use_dictionary=True, device_compression="snappy", both --
alternating in one process, on the two workloads of tools/parquet_dict_rate.py:

* criteo: the Categorify + Normalize output of the benchmark's Criteo-shaped frame (26 int64 label
  columns, 13 float columns);
* session: int64 item-id lists, a second list column with null leaves that shares the offsets, and a
  flat user id.

Per workload and mode: the median wall time of to_parquet (a host clock around a call that ends with
every file closed), rows/s, the io.LAST_TIMING split (snappy_s among it), bytes per row, how many
chunks say SNAPPY, and the snappy_* launches and read-backs per row group.  The default mode is the
yardstick for time (it is what the parent commit writes); the compression="snappy" route through
pyarrow's writer, on a prefix of the frame, is the yardstick for size.  Then the compress kernel
alone: one more snappy write under the library's profiler gives the time of the snappy_compress
launches and the input bytes they took -> GB/s per launch.  One JSON line at the end.

    python tools/parquet_snappy_rate.py [rows] [runs] [out_dir]"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyarrow.parquet as pq
import torch

import nvtabular_amd as nvt
from nvtabular_amd import io as nio
from nvtabular_amd import kernels as K
from parquet_dict_rate import criteo_frame, parquet_bytes, session_frame

COUNTERS = ("snappy_plan", "snappy_compress", "snappy_gather", "snappy_readback", "pqdict_readback")
PYARROW_PREFIX = 1 << 20
MODES = {"default": {}, "use_dictionary": {"use_dictionary": True}, "snappy": {"device_compression": "snappy"},
         "both": {"use_dictionary": True, "device_compression": "snappy"}}


def snappy_chunks(out):
    n = total = 0
    for f in os.listdir(out):
        if f.endswith(".parquet"):
            md = pq.read_metadata(os.path.join(out, f))
            for g in range(md.num_row_groups):
                for j in range(md.num_columns):
                    total += 1
                    n += md.row_group(g).column(j).compression == "SNAPPY"
    return n, total


def measure(name, frame, runs, base):
    rows = len(frame)
    out = tempfile.mkdtemp(dir=base)
    times, phases = {m: [] for m in MODES}, {m: [] for m in MODES}
    sizes, counts, chunks = {}, {}, {}

    def once(mode):
        shutil.rmtree(out, ignore_errors=True)
        torch.cuda.synchronize()
        before = {k: K.STATS.get(k, 0) for k in COUNTERS}
        t0 = time.perf_counter()
        nvt.Dataset(frame).to_parquet(out, **MODES[mode])
        dt = time.perf_counter() - t0
        sizes[mode] = parquet_bytes(out)
        groups = pq.read_metadata(os.path.join(out, "part_0.parquet")).num_row_groups
        counts[mode] = {k: round((K.STATS.get(k, 0) - before[k]) / groups, 2) for k in COUNTERS}
        return dt

    try:
        for mode in MODES:                   # warm-up: code objects, pinned pools, page cache
            once(mode)
            chunks[mode] = snappy_chunks(out)
        for _ in range(runs):
            for mode in MODES:               # alternating: all see the same machine
                dt = once(mode)
                times[mode].append(dt)
                phases[mode].append(dict(nio.LAST_TIMING))
                print(f"{name:8s} {mode:15s} {1e3 * dt:8.0f} ms  {rows / dt / 1e6:7.2f} M rows/s", flush=True)
        # the compress kernel alone, under the library's profiler (a run of its own)
        shutil.rmtree(out, ignore_errors=True)
        K.profile_begin()
        nvt.Dataset(frame).to_parquet(out, device_compression="snappy")
        torch.cuda.synchronize()
        prof = K.profile_end()
        kernel = {}
        for k in ("snappy_plan", "snappy_compress", "snappy_gather"):
            if k in prof:
                ms, launches, nbytes = prof[k]
                kernel[k] = {"ms": round(ms, 3), "scopes": launches, "input_bytes": nbytes,
                             "GB_s": round(nbytes / ms / 1e6, 2) if ms else None}
        # the size yardstick: pyarrow's writer with its snappy codec, on a prefix
        n = min(rows, PYARROW_PREFIX)
        prefix = frame.take_rows(torch.arange(n, device=frame[next(iter(frame.columns))].data.device))
        prefix_bytes = {}
        for mode in MODES:
            shutil.rmtree(out, ignore_errors=True)
            nvt.Dataset(prefix).to_parquet(out, **MODES[mode])
            prefix_bytes[mode] = parquet_bytes(out)
        shutil.rmtree(out, ignore_errors=True)
        t0 = time.perf_counter()
        nvt.Dataset(prefix).to_parquet(out, compression="snappy")
        pa_s = time.perf_counter() - t0
        prefix_bytes["pyarrow_snappy"] = parquet_bytes(out)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    res = {"rows": rows, "prefix_rows": n, "prefix_bytes": prefix_bytes,
           "pyarrow_snappy_prefix_M_rows_s": round(n / pa_s / 1e6, 2), "kernels": kernel}
    for mode in MODES:
        med = statistics.median(times[mode])
        res[mode] = {"s": round(med, 4), "all_s": [round(x, 4) for x in times[mode]],
                     "M_rows_s": round(rows / med / 1e6, 2), "file_bytes": sizes[mode],
                     "bytes_per_row": round(sizes[mode] / rows, 2),
                     "time_over_default": round(med / statistics.median(times["default"]), 3),
                     "snappy_chunks": list(chunks[mode]),
                     "phases_s": {k: round(statistics.median(p[k] for p in phases[mode]), 4) for k in phases[mode][0]},
                     "per_row_group": counts[mode]}
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    base = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8 << 20
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)          # (no GPU: this raises; nothing here is measured on a CPU)
    torch.zeros(1, device=dev)
    tmp = tempfile.mkdtemp(dir=base)
    try:
        result = {"criteo": measure("criteo", criteo_frame(rows, dev, tmp), runs, base),
                  "session": measure("session", session_frame(rows, dev), runs, base)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
