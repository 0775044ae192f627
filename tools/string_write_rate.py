"""to_parquet rate of frames with a flat string column: the PLAIN writer's string route against the
route such frames took before it (pyarrow's writer behind DeviceFrame.to_arrow), in one process --
the old route is taken with io.PLAIN_PARQUET off, as NVT_PLAIN_PARQUET=0 sets it.

    python tools/string_write_rate.py [--rows 20000000] [--reps 5] [--cases a,b,ca,cb] [--out FILE.jsonl]

Cases: a   one column of 100 distinct strings
       b   one column of mostly distinct 16-character hex ids
       ca  a beside 26 int64 and 13 float32 columns      cb  b beside the same 39 columns
Every route runs once unmeasured, then ``reps`` times; the median, all samples and the LAST_TIMING
breakdown of the median run are printed as one JSON line per case and route."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import torch

import nvtabular_amd as nvt
from nvtabular_amd import io as nio
from nvtabular_amd.device import DeviceColumn, DeviceFrame


def few_strings(rng, n, dev):
    words = pa.array([f"category-{i:03d}" for i in range(100)])
    idx = pa.array(rng.integers(0, 100, n).astype(np.int32))
    return DeviceColumn.from_arrow(pa.DictionaryArray.from_arrays(idx, words), dev)


def hex_ids(rng, n, dev):
    """n draws (with replacement) from n random 16-character ids: about 63 % of the rows are distinct."""
    pool = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)[rng.integers(0, 16, (n, 16))]
    chars = np.ascontiguousarray(pool[rng.integers(0, n, n)]).reshape(-1)
    offsets = np.arange(n + 1, dtype=np.int64) * 16
    arr = pa.Array.from_buffers(pa.large_string(), n, [None, pa.py_buffer(offsets), pa.py_buffer(chars)])
    return DeviceColumn.from_arrow(arr, dev)


def numbers(rng, n, dev):
    cols = {}
    for j in range(26):
        cols[f"C{j}"] = DeviceColumn(torch.from_numpy(rng.integers(0, 1 << 20, n)).to(dev))
    for j in range(13):
        cols[f"I{j}"] = DeviceColumn(torch.from_numpy(rng.normal(size=n).astype(np.float32)).to(dev))
    return cols


def timed(frame, out_dir, plain):
    nio.PLAIN_PARQUET = plain
    shutil.rmtree(out_dir, ignore_errors=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nvt.Dataset(frame).to_parquet(out_dir)
    dt = time.perf_counter() - t0
    size = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir) if f.endswith(".parquet"))
    return dt, size, ({k: round(v, 4) for k, v in nio.LAST_TIMING.items()} if plain else {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,b,ca,cb")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.rows
    tmp = tempfile.mkdtemp()
    lines = []
    for case in args.cases.split(","):
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        cols = {"s": (few_strings if case.endswith("a") else hex_ids)(rng, n, dev)}
        if case.startswith("c"):
            cols.update(numbers(rng, n, dev))
        frame = DeviceFrame(cols)
        print(f"# case {case}: {n} rows, {len(cols)} columns, {len(cols['s'].strings)} distinct strings, "
              f"built in {time.perf_counter() - t0:.1f} s", flush=True)
        for route, plain in (("plain", True), ("pyarrow", False)):
            out_dir = os.path.join(tmp, f"{case}_{route}")
            timed(frame, out_dir, plain)                                  # warm: allocator, page cache, imports
            runs = sorted((timed(frame, out_dir, plain) for _ in range(args.reps)), key=lambda r: r[0])
            dt, size, phases = runs[len(runs) // 2]
            line = dict(case=case, route=route, rows=n, columns=len(cols), median_s=round(dt, 4),
                        m_rows_per_s=round(n / dt / 1e6, 2), samples_s=[round(r[0], 4) for r in runs],
                        file_gb=round(size / 1e9, 3), phases=phases)
            lines.append(line)
            print(json.dumps(line), flush=True)
            shutil.rmtree(out_dir, ignore_errors=True)
        del frame, cols
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
