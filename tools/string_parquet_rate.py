"""Dataset(path) of files with string columns: the hand-written parquet reader (io.PLAIN_PARQUET_READ
on: entries, run table and packed index bytes staged on the host; nvt_pq_expand_runs, hashing and the
dict on the device) against the pyarrow path (the switch off: what such files took before the reader
knew strings), alternating, in one process.  One file per case, written by pyarrow with its defaults:

  a  a Zipf column of 16-character hex ids, about `rows / 10` distinct (row groups mix dictionary and
     PLAIN pages once the dictionary passes its size limit)
  b  a column of 100 distinct short strings
  c  both beside 13 float32 and 13 int32 columns

A read is every partition of ``Dataset(path).to_iter()`` on the device with its dict built, timed to
``torch.cuda.synchronize()`` behind it: 2 warm-up rounds, then `runs` timed ones.  For the reader-on
path one more profiled read gives the kernel scopes (NVT_PROF) and the launch counts (K.STATS), and
one partition is taken apart into host decode and device work.  Then nvt_pq_expand_runs alone: HIP
events, median of 20, `kernel_values` values at widths 7 and 21, in bytes moved (packed bytes read +
4 bytes per value written) over time.  Prints one JSON line at the end.

    python tools/string_parquet_rate.py [rows] [runs] [out_dir] [kernel_values]"""
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
from nvtabular_amd import kernels as K
from nvtabular_amd import kernels_parquet_str as KPS
from nvtabular_amd import parquet_plain as PP

HBM_BYTES_S = 8e12   # the figure the other notes measure against


def columns_of(rows, seed=0):
    rng = np.random.default_rng(seed)
    distinct = max(1, rows // 10)
    pool = pa.array([f"{int(v):016x}" for v in rng.integers(0, 1 << 63, distinct)])
    ids = pool.take(pa.array((rng.zipf(1.1, rows) - 1) % distinct))
    small = pa.array([f"cat_{i}" for i in range(100)]).take(pa.array(rng.integers(0, 100, rows)))
    nums = {}
    for j in range(13):
        nums[f"f{j}"] = pa.array(rng.normal(size=rows).astype("float32"))
        nums[f"i{j}"] = pa.array(rng.integers(0, 1 << 20, rows).astype("int32"))
    return ids, small, nums


def read(path):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = list(nvt.Dataset(path).to_iter())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, sum(len(p) for p in parts), sum(len(c.strings) for p in parts for _, c in p.items() if c.strings is not None)


def split_of(path, runs=3):
    """Row group 0 of the reader-on path taken apart: medians in seconds."""
    pf = PP.PlainParquetFile(path)
    pool, dev = nio._plain_read_pool(), torch.device("cuda", 0)
    host, device = [], []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        staged = PP.read_row_groups_staged(pf, [0], pool=pool)
        host.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nio.StagedPartition(staged).to_device(dev)
        torch.cuda.synchronize()
        device.append(time.perf_counter() - t0)
    strs = {n: dict(entries=sc.strs.entries, runs=sc.strs.nruns, packed_bytes=sc.strs.npacked, chars=sc.strs.nchars)
            for n, sc in staged.items() if sc.strs is not None}
    return {"rows": pf.row_groups[0]["num_rows"], "host_decode_s": round(statistics.median(host[1:]), 5),
            "to_device_s": round(statistics.median(device[1:]), 5), "staged": strs}


def kernel_alone(nvalues, width, reps=20):
    """nvt_pq_expand_runs on one table of bit-packed runs of 504 values (what pyarrow writes)."""
    rng = np.random.default_rng(width)
    per = 504
    nruns = -(-nvalues // per)
    run_bytes = (per * width // 8 + 3) & ~3
    packed = rng.integers(0, 256, nruns * run_bytes + 8, dtype=np.uint8)
    runs = np.zeros((nruns + 1, 4), dtype=np.uint32)
    runs[:nruns, 0] = np.arange(nruns, dtype=np.uint64) * per
    runs[:nruns, 1] = 1 | (width << 8)
    runs[:nruns, 3] = np.arange(nruns, dtype=np.uint64) * (run_bytes // 4)
    runs[nruns] = (nvalues, 3, 0, 0)
    d_runs = torch.from_numpy(runs.view(np.int32).reshape(-1)).cuda()
    d_packed = torch.from_numpy(packed).cuda()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    times = []
    for it in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = KPS.expand_runs(d_runs, nruns, runs[nruns], d_packed, 1 << width, nvalues, bad)
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            times.append(a.elapsed_time(b) / 1e3)
        del out
    assert int(bad.cpu()[0]) == 0
    med = statistics.median(times)
    moved = packed.size + 16 * (nruns + 1) + 4 * nvalues
    return {"values": nvalues, "width": width, "median_s": round(med, 6), "min_s": round(min(times), 6),
            "max_s": round(max(times), 6), "bytes_moved": moved, "GB_s": round(moved / med / 1e9, 1),
            "fraction_of_8TB_s": round(moved / med / HBM_BYTES_S, 3)}


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    base = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    kvalues = int(sys.argv[4]) if len(sys.argv) > 4 else 45_000_000
    out = tempfile.mkdtemp(dir=base)
    result = {"rows": rows, "runs": runs, "cases": {}}
    try:
        ids, small, nums = columns_of(rows)
        tables = {"a_zipf_hex_ids": pa.table({"id": ids}), "b_100_short_strings": pa.table({"cat": small}),
                  "c_both_beside_26_numbers": pa.table(dict({"id": ids, "cat": small}, **nums))}
        for case, t in tables.items():
            path = os.path.join(out, case + ".parquet")
            pq.write_table(t, path)
            tables[case] = None
            times = {"on": [], "off": []}
            dict_entries = 0
            for it in range(runs + 2):                      # (two rounds warm both up)
                for mode in ("on", "off"):                  # alternating: both see the same machine
                    nio.PLAIN_PARQUET_READ = mode == "on"
                    before = dict(PP.READER_CHUNKS)
                    dt, got, dict_entries = read(path)
                    assert got == rows
                    moved, still = ("plain", "pyarrow") if mode == "on" else ("pyarrow", "plain")
                    assert PP.READER_CHUNKS[still] == before[still] and PP.READER_CHUNKS[moved] > before[moved]
                    if it >= 2:
                        times[mode].append(dt)
                        print(f"{case:26s} reader {mode:3s} {1e3 * dt:9.1f} ms  {rows / dt / 1e6:7.2f} M rows/s", flush=True)
            # where the reader-on time goes: kernel scopes + launch counts of one more read
            nio.PLAIN_PARQUET_READ = True
            stats0 = dict(K.STATS)
            K.profile_begin()
            read(path)
            prof = K.profile_report()
            md = pq.read_metadata(path)
            result["cases"][case] = {
                "file_bytes": os.path.getsize(path), "row_groups": md.num_row_groups, "dict_entries_built": dict_entries,
                "on_median_s": round(statistics.median(times["on"]), 4),
                "off_median_s": round(statistics.median(times["off"]), 4),
                "on_all_s": [round(x, 4) for x in times["on"]], "off_all_s": [round(x, 4) for x in times["off"]],
                "on_M_rows_s": round(rows / statistics.median(times["on"]) / 1e6, 2),
                "off_M_rows_s": round(rows / statistics.median(times["off"]) / 1e6, 2),
                "profiled_read": {"busy_ms": prof.get("busy_ms"), "span_ms": prof.get("span_ms"),
                                  "kernels_ms_launches": {k: [round(v[0], 3), v[1]] for k, v in prof["kernels"].items()}},
                "stats": {k: v - stats0.get(k, 0) for k, v in K.STATS.items() if v != stats0.get(k, 0)},
                "split_of_row_group_0": split_of(path)}
            print(json.dumps({case: result["cases"][case]}), flush=True)
        result["expand_runs_alone"] = [kernel_alone(kvalues, w) for w in (7, 21)]
    finally:
        shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
