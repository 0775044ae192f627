"""to_parquet of a session-shaped frame: four list columns that share one offsets tensor (what
Groupby(list) >> ListSlice hands over; 8 leaves per row on average; int64, int64 with 10 % null
leaves, int32 and float32 leaves) beside two flat columns, written by the hand-written PLAIN writer
and by pyarrow's writer (io.PLAIN_PARQUET = False: what list columns took before the PLAIN writer
knew them), alternating, in one process.  Prints the median of each, the PLAIN path's phases
(io.LAST_TIMING) and one JSON line.

    python tools/list_parquet_rate.py [rows] [runs] [out_dir]

rows defaults to what a quarter of the free space under out_dir (default: the temp directory)
holds, at most 8 M."""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import nvtabular_amd as nvt
from nvtabular_amd import io as nio
from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap

LEAF_BYTES = 8 + 8 + 4 + 4          # the four list columns
ROW_BYTES = 8 * LEAF_BYTES + 12     # 8 leaves per row + the flat columns


def frame_of(rows, dev, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 17, rows)                 # 0 .. 16 leaves, 8 on average
    off = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    leaves = int(off[-1])
    d_off = torch.from_numpy(off).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    ok = torch.from_numpy(pack_bitmap(rng.random(leaves) >= 0.1)).to(dev)
    return DeviceFrame({
        "user_id": DeviceColumn(t(np.arange(rows, dtype=np.int64))),
        "item_id_list": DeviceColumn(t(rng.integers(0, 1 << 40, leaves).astype(np.int64)), None, d_off),
        "ts_list": DeviceColumn(t(rng.integers(0, 1 << 40, leaves).astype(np.int64)), ok, d_off),
        "category_list": DeviceColumn(t(rng.integers(0, 1000, leaves).astype(np.int32)), None, d_off),
        "price_list": DeviceColumn(t(rng.random(leaves).astype(np.float32)), None, d_off),
        "count": DeviceColumn(t(lens.astype(np.int32))),
    }), leaves


def main():
    base = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    free = shutil.disk_usage(base).free
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else int(min(8 << 20, free // 4 // ROW_BYTES))
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)
    frame, leaves = frame_of(rows, dev)
    out = tempfile.mkdtemp(dir=base)
    times = {"plain": [], "pyarrow": []}
    phases, sizes = [], {}

    def once(mode):
        nio.PLAIN_PARQUET = mode == "plain"
        shutil.rmtree(out, ignore_errors=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nvt.Dataset(frame).to_parquet(out)
        dt = time.perf_counter() - t0
        sizes[mode] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out) if f.endswith(".parquet"))
        return dt

    try:
        for mode in ("plain", "pyarrow"):        # warm-up: code objects, pinned pools, page cache
            once(mode)
        for _ in range(runs):
            for mode in ("plain", "pyarrow"):    # alternating: both see the same machine
                dt = once(mode)
                times[mode].append(dt)
                if mode == "plain":
                    phases.append(dict(nio.LAST_TIMING))
                print(f"{mode:8s} {1e3 * dt:8.0f} ms  {rows / dt / 1e6:7.2f} M rows/s", flush=True)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    med = {m: statistics.median(v) for m, v in times.items()}
    split = {k: round(statistics.median(p[k] for p in phases), 4) for k in phases[0]}
    result = {"rows": rows, "leaves": leaves, "runs": runs,
              "plain_s": round(med["plain"], 4), "pyarrow_s": round(med["pyarrow"], 4),
              "plain_all_s": [round(x, 4) for x in times["plain"]],
              "pyarrow_all_s": [round(x, 4) for x in times["pyarrow"]],
              "plain_M_rows_s": round(rows / med["plain"] / 1e6, 2),
              "pyarrow_M_rows_s": round(rows / med["pyarrow"] / 1e6, 2),
              "plain_GB_s": round(sizes["plain"] / med["plain"] / 1e9, 2),
              "file_bytes": sizes, "plain_phases_s": split}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
