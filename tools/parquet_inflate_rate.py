"""Dataset(path) of the Criteo-shaped frame of tools/parquet_dict_in_rate.py (26 int64 id columns, 13
float32 columns, row groups of 1 Mi) in the three forms whose snappy PLAIN pages the device can inflate.

    python tools/parquet_inflate_rate.py write DIR [rows]        writes DIR/default.parquet (pyarrow's defaults),
                                                                  DIR/plain.parquet (use_dictionary=False) and
                                                                  DIR/device/ (to_parquet(device_compression="snappy"))
    python tools/parquet_inflate_rate.py read PATH [runs] [tree]  one fresh process = one measurement: 1 warm-up
                                                                  read, then `runs` timed ones (every partition of
                                                                  ``Dataset(path).to_iter()`` on the device, to
                                                                  ``torch.cuda.synchronize()``); `tree`: the checkout
                                                                  whose nvtabular_amd is imported (the parent commit's
                                                                  build for the comparison), default this one
    python tools/parquet_inflate_rate.py parts PATH               one partition (row group 0 of the first file) taken
                                                                  apart: host staging with and without
                                                                  device_inflate, the share of pages and bytes that
                                                                  took the route, the bytes that cross PCIe per
                                                                  value, ``fill_holes`` alone (HIP events, median of
                                                                  20) and its store bandwidth

Each mode prints one JSON line.  NVT_PQ_DEVICE_INFLATE=0 / 1 selects the route in `read`."""
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

from parquet_dict_in_rate import CARDS


def write(out, rows):
    import pandas as pd
    import pyarrow as pa
    import pyarrow.parquet as pq

    import nvtabular_amd as nvt

    rng = np.random.default_rng(0)
    cols = {f"C{i + 1}": (rng.zipf(1.2, rows) % int(c)) * 7919 for i, c in enumerate(CARDS)}
    for i in range(13):
        cols[f"I{i + 1}"] = np.floor(rng.lognormal(2, 2, rows)).astype(np.float32)
    os.makedirs(out, exist_ok=True)
    pq.write_table(pa.table(cols), os.path.join(out, "default.parquet"), row_group_size=1 << 20)
    pq.write_table(pa.table(cols), os.path.join(out, "plain.parquet"), row_group_size=1 << 20, use_dictionary=False)
    nvt.Dataset(pd.DataFrame(cols)).to_parquet(os.path.join(out, "device"), device_compression="snappy")
    sizes = {n: sum(os.path.getsize(f) for f in _files(os.path.join(out, n)))
             for n in ("default.parquet", "plain.parquet", "device")}
    print(json.dumps({"rows": rows, "bytes": sizes}))


def _files(path):
    return sorted(glob.glob(os.path.join(path, "*.parquet"))) if os.path.isdir(path) else [path]


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
    print(json.dumps({"tree": os.path.abspath(tree), "device_inflate": getattr(nio, "PQ_DEVICE_INFLATE", None),
                      "inflate_pages": PP.READER_CHUNKS.get("inflate_pages"), "rows": n,
                      "median_s": statistics.median(times[1:]), "times_s": [round(t, 4) for t in times]}))


def parts(path, tree):
    sys.path.insert(0, tree)
    import torch

    from nvtabular_amd import kernels_parquet_inflate as KPI
    from nvtabular_amd import parquet_plain as PP

    pf, res = PP.PlainParquetFile(_files(path)[0]), {}
    for on in (False, True, False, True):
        t0 = time.perf_counter()
        staged = PP.read_row_groups_staged(pf, [0], device_inflate=on)
        res[f"host_stage_s_device_inflate_{int(on)}"] = time.perf_counter() - t0
    n0, dev = pf.row_groups[0]["num_rows"], torch.device("cuda")
    crossing = filled = full = pages = 0
    for sc in staged.values():
        width = sc.values.element_size()
        full += sc.nvalid * width
        st = sc.inflate
        if st is None:
            crossing += sc.nvalid * width
            continue
        holes = int(st.records()[:, 3].sum())
        crossing += st.nbytes + 40 * st.npages + sc.nvalid * width - holes
        filled += holes
        pages += st.npages
    res["pages_routed"], res["share_of_value_bytes_routed"] = pages, filled / max(full, 1)
    res["pcie_bytes_per_value"] = crossing / (n0 * len(staged))
    res["host_inflated_bytes_per_value"] = full / (n0 * len(staged))
    items = [(sc.inflate, KPI.values_to_device(sc, dev)) for sc in staged.values() if sc.inflate is not None]
    ev = []
    for _ in range(22):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        handle = KPI.fill_holes(items)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    KPI.raise_failed(handle)
    host = PP.read_row_groups_staged(pf, [0])
    for (name, sc), (_, out) in zip(((k, v) for k, v in staged.items() if v.inflate is not None), items):
        assert torch.equal(out.cpu(), host[name].values[: sc.nvalid]), name
    res["fill_holes_ms"] = statistics.median(a.elapsed_time(b) for a, b in ev[2:])   # (with the copies of the stages)
    res["filled_bytes"], res["columns_filled"] = filled, len(items)
    res["fill_store_GBps"] = filled / res["fill_holes_ms"] / 1e6
    print(json.dumps(res))


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    mode, path = sys.argv[1], sys.argv[2]
    if mode == "write":
        write(path, int(sys.argv[3]) if len(sys.argv) > 3 else 8_000_000)
    elif mode == "read":
        read(path, int(sys.argv[3]) if len(sys.argv) > 3 else 3, sys.argv[4] if len(sys.argv) > 4 else here)
    else:
        parts(path, here)
