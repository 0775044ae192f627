"""Dataset(path) of pyarrow's default file (snappy, every column dictionary-encoded, row groups of 1 Mi)
in the Criteo shape: 26 int64 id columns whose cardinalities run from 2 to beyond the 1 MiB dictionary
limit (those chunks fall back to PLAIN pages) and 13 float32 columns.

    python tools/parquet_dict_in_rate.py write PATH [rows]      writes the file (8 M rows)
    python tools/parquet_dict_in_rate.py read PATH [runs] [tree] one fresh process = one measurement: 1 warm-up
                                                                 read, then `runs` timed ones (every partition of
                                                                 ``Dataset(path).to_iter()`` on the device, to
                                                                 ``torch.cuda.synchronize()``); `tree`: the checkout
                                                                 whose nvtabular_amd is imported (the parent commit's
                                                                 build for the comparison), default this one
    python tools/parquet_dict_in_rate.py parts PATH             one partition (row group 0) taken apart: host staging
                                                                 with and without device_dict, the bytes that cross
                                                                 PCIe per value, ``fill_holes`` alone (HIP events,
                                                                 median of 20) and its store bandwidth

Each mode prints one JSON line.  NVT_PQ_DEVICE_DICT=0 / 1 selects the route in `read`."""
import json
import os
import statistics
import sys
import time

import numpy as np

CARDS = [2, 4, 10, 30, 100, 300, 1000, 3000, 10**4, 3 * 10**4, 5 * 10**4, 8 * 10**4, 10**5, 1.2 * 10**5, 1.3 * 10**5,
         2 * 10**5, 3 * 10**5, 5 * 10**5, 10**6, 2 * 10**6, 4 * 10**6, 10**7, 10**8, 10**9, 10**10, 10**12]


def write(path, rows):
    import pyarrow as pa
    import pyarrow.parquet as pq

    rng = np.random.default_rng(0)
    cols = {f"C{i + 1}": (rng.zipf(1.2, rows) % int(c)) * 7919 for i, c in enumerate(CARDS)}
    for i in range(13):
        cols[f"I{i + 1}"] = np.floor(rng.lognormal(2, 2, rows)).astype(np.float32)
    pq.write_table(pa.table(cols), path, row_group_size=1 << 20)
    print(json.dumps({"rows": rows, "file_bytes": os.path.getsize(path)}))


def read(path, runs, tree):
    sys.path.insert(0, tree)
    import torch

    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import parquet_plain as PP

    times = []
    for _ in range(1 + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(len(p) for p in nvt.Dataset(path).to_iter())
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert PP.READER_CHUNKS["pyarrow"] == 0
    print(json.dumps({"tree": os.path.abspath(tree), "device_dict": getattr(nio, "PQ_DEVICE_DICT", None), "rows": n,
                      "median_s": statistics.median(times[1:]), "times_s": [round(t, 4) for t in times]}))


def parts(path, tree):
    sys.path.insert(0, tree)
    import torch

    from nvtabular_amd import kernels_parquet_dict_in as KDI
    from nvtabular_amd import parquet_plain as PP

    pf, res = PP.PlainParquetFile(path), {}
    for on in (False, True, False, True):
        t0 = time.perf_counter()
        staged = PP.read_row_groups_staged(pf, [0], device_dict=on)
        res[f"host_stage_s_device_dict_{int(on)}"] = time.perf_counter() - t0
    n0, dev = pf.row_groups[0]["num_rows"], torch.device("cuda")
    crossing = filled = full = 0
    for sc in staged.values():
        full += sc.nvalid * sc.values.element_size()
        st = sc.dict_stage
        if st is None:
            crossing += sc.nvalid * sc.values.element_size()
            continue
        recs = KDI.run_records(st)
        keep = (recs[:-1, 1] & 0xFF) == 4
        kept = int((recs[1:, 0][keep].astype(np.int64) - recs[:-1, 0][keep]).sum())
        crossing += st.ndict_bytes + 16 * (st.nruns + 1) + st.npacked + 8 + kept * sc.values.element_size()
        filled += (sc.nvalid - kept) * sc.values.element_size()
    res["pcie_bytes_per_value"] = crossing / (n0 * len(staged))
    res["host_resolved_bytes_per_value"] = full / (n0 * len(staged))
    items = [(sc.dict_stage, KDI.values_to_device(sc, dev)) for sc in staged.values() if sc.dict_stage is not None]
    ev = []
    for _ in range(22):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        bad = KDI.fill_holes(items)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    assert int(bad.cpu()[0]) == 0
    host = PP.read_row_groups_staged(pf, [0])
    for (name, sc), (_, out) in zip(((k, v) for k, v in staged.items() if v.dict_stage is not None), items):
        assert torch.equal(out.cpu(), host[name].values[: sc.nvalid]), name
    res["fill_holes_ms"] = statistics.median(a.elapsed_time(b) for a, b in ev[2:])   # (with the copies of the stages)
    res["filled_bytes"], res["columns_filled"] = filled, len(items)
    res["fill_store_GBps"] = filled / res["fill_holes_ms"] / 1e6
    print(json.dumps(res))


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mode, path = sys.argv[1], sys.argv[2]
    if mode == "write":
        write(path, int(sys.argv[3]) if len(sys.argv) > 3 else 8_000_000)
    elif mode == "read":
        read(path, int(sys.argv[3]) if len(sys.argv) > 3 else 3, sys.argv[4] if len(sys.argv) > 4 else here)
    else:
        parts(path, here)
