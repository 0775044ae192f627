"""Dataset(path) of session-shaped files with list columns: the hand-written parquet reader
(io.PLAIN_PARQUET_READ on: host decode of the level streams, nvt_pqlist_unpack on the device) against
the pyarrow path (the switch off: what nested files took before the reader knew lists), alternating,
in one process.  Two files hold the frame of tools/list_parquet_rate.py (four list columns that share
their offsets, one of them with 10 % null leaves, two flat columns): one written by this package's
PLAIN writer, one by pyarrow with its defaults (snappy + dictionary).  A read is every partition of
``Dataset(path).to_iter()`` on the device, timed to ``torch.cuda.synchronize()`` behind it.  Prints
the median of each, the split of the hand-written path of one partition (host decode / copies +
unpack + expand / the unpack kernels alone) and one JSON line.

    python tools/list_parquet_read_rate.py [rows] [runs] [out_dir]"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyarrow.parquet as pq
import torch

import nvtabular_amd as nvt
from list_parquet_rate import frame_of
from nvtabular_amd import io as nio
from nvtabular_amd import kernels as K
from nvtabular_amd import kernels_parquet_list as KPL
from nvtabular_amd import parquet_plain as PP


def read(path):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = list(nvt.Dataset(path).to_iter())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, sum(len(p) for p in parts)


def split_of(path, runs):
    """One partition (row group 0) of the hand-written path taken apart: medians in seconds."""
    pf = PP.PlainParquetFile(path)
    assert pf.readable, pf.why_not
    pool = nio._plain_read_pool()
    dev = torch.device("cuda", 0)
    host, device, kernel = [], [], []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        staged = PP.read_row_groups_staged(pf, [0], pool=pool)
        host.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nio.StagedPartition(staged).to_device(dev)
        torch.cuda.synchronize()
        device.append(time.perf_counter() - t0)
        # the unpack launches alone, on streams that are on the device already
        lists = [sc for sc in staged.values() if sc.is_list and sc.same_as is None]
        bufs = [(sc, sc.rep[: ((sc.slots + 63) // 64) * 8].to(dev), sc.dfn[: ((sc.slots * sc.width + 63) // 64) * 8].to(dev))
                for sc in lists]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for sc, rep, dfn in bufs:
            KPL.unpack_levels(rep, dfn, sc.width, sc.slots, sc.leaf_level, sc.max_def, sc.rows, sc.leaves,
                              sc.nvalid < sc.leaves)
        b.record()
        torch.cuda.synchronize()
        kernel.append(a.elapsed_time(b) / 1e3)
    med = lambda v: round(statistics.median(v[1:]), 5)
    return {"rows": pf.row_groups[0]["num_rows"], "distinct_level_streams": len(lists),
            "slots": sum(sc.slots for sc in lists), "host_decode_s": med(host), "to_device_s": med(device),
            "unpack_kernels_s": med(kernel)}


def main():
    base = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 2 << 20
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    frame, leaves = frame_of(rows, torch.device("cuda", 0))
    out = tempfile.mkdtemp(dir=base)
    result = {"rows": rows, "leaves": 4 * leaves, "runs": runs, "files": {}}
    try:
        own = os.path.join(out, "own")
        nvt.Dataset(frame).to_parquet(own)
        theirs = os.path.join(out, "pyarrow.parquet")
        pq.write_table(frame.to_arrow(), theirs)
        del frame
        for kind, path in (("plain_writer", own), ("pyarrow_defaults", theirs)):
            files = [os.path.join(path, f) for f in os.listdir(path) if f.endswith(".parquet")] if os.path.isdir(path) \
                else [path]
            times = {"plain": [], "pyarrow": []}
            for it in range(runs + 1):                      # (the first round warms both up)
                for mode in ("plain", "pyarrow"):           # alternating: both see the same machine
                    nio.PLAIN_PARQUET_READ = mode == "plain"
                    before = dict(PP.READER_CHUNKS)
                    dt, got = read(path)
                    assert got == rows
                    other = "pyarrow" if mode == "plain" else "plain"
                    assert PP.READER_CHUNKS[other] == before[other] and PP.READER_CHUNKS[mode] > before[mode]
                    if it:
                        times[mode].append(dt)
                        print(f"{kind:17s} {mode:8s} {1e3 * dt:8.1f} ms  {rows / dt / 1e6:7.2f} M rows/s", flush=True)
            med = {m: statistics.median(v) for m, v in times.items()}
            md = pq.read_metadata(files[0])
            result["files"][kind] = {
                "file_bytes": sum(os.path.getsize(f) for f in files), "row_groups": md.num_row_groups,
                "plain_s": round(med["plain"], 4), "pyarrow_s": round(med["pyarrow"], 4),
                "plain_all_s": [round(x, 4) for x in times["plain"]],
                "pyarrow_all_s": [round(x, 4) for x in times["pyarrow"]],
                "plain_M_rows_s": round(rows / med["plain"] / 1e6, 2),
                "pyarrow_M_rows_s": round(rows / med["pyarrow"] / 1e6, 2),
                "plain_M_leaves_s": round(4 * leaves / med["plain"] / 1e6, 1),
                "pyarrow_M_leaves_s": round(4 * leaves / med["pyarrow"] / 1e6, 1),
                "split_of_row_group_0": split_of(files[0], runs)}
        result["unpack_launches"] = K.STATS.get("pqlist_unpack", 0)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
