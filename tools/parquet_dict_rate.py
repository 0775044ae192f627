"""to_parquet with and without use_dictionary=True, alternating in one process, on two workloads:

* criteo: the Categorify + Normalize output of the benchmark's Criteo-shaped frame (bench.synth_criteo:
  26 int64 label columns, 13 float columns);
* session: int64 item-id lists (8 leaves per row on average, ids over `items` distinct values with a
  power law), a second list column with 10 % null leaves that shares the offsets, and a flat user id.

Per workload and mode: the median wall time of to_parquet (a host clock around a call that ends with
every file closed), rows/s, the io.LAST_TIMING split, bytes written, and the pqdict_* / pqlist_*
launches and read-backs per row group.  The run without the option is the yardstick for time (it is
what the writer did before the option existed); pyarrow's writer with compression=None and its default
dictionary, on a prefix of the frame, is the yardstick for size.  Then the cost of the dictionary
build alone (nvt_pq_dict_build, device events) per value, for 4 M int64 values over several numbers of
distinct values.  One JSON line at the end.

    python tools/parquet_dict_rate.py [rows] [runs] [out_dir]"""
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

import nvtabular_amd as nvt
from nvtabular_amd import _lib
from nvtabular_amd import io as nio
from nvtabular_amd import kernels as K
from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap

COUNTERS = ("pqdict_build", "pqdict_pack", "pqdict_readback", "pqlist_plan", "pqlist_pack_many", "pqlist_readback")
PYARROW_PREFIX = 1 << 20


def criteo_frame(rows, dev, tmp):
    import bench

    raw = bench.synth_criteo(rows, dev)
    cats = [c for c in raw.columns if c.startswith("C")]
    conts = [c for c in raw.columns if c.startswith("I")]
    wf = bench.build_workflow(cats, conts, os.path.join(tmp, "wf"))
    ds = nvt.Dataset(raw)
    wf.fit(ds)
    parts = list(wf.transform(ds).to_iter())
    assert len(parts) == 1
    return parts[0]


def session_frame(rows, dev, items=200_000, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 17, rows)
    off = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    leaves = int(off[-1])
    ids = np.minimum((rng.pareto(1.1, leaves) * 50).astype(np.int64), items - 1)
    d_off = torch.from_numpy(off).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    ok = torch.from_numpy(pack_bitmap(rng.random(leaves) >= 0.1)).to(dev)
    return DeviceFrame({
        "user_id": DeviceColumn(t(np.arange(rows, dtype=np.int64))),
        "item_id_list": DeviceColumn(t(ids), None, d_off),
        "category_list": DeviceColumn(t(ids % 1000), ok, d_off),
    })


def parquet_bytes(out):
    return sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out) if f.endswith(".parquet"))


def measure(name, frame, runs, base):
    rows = len(frame)
    out = tempfile.mkdtemp(dir=base)
    times, phases, sizes, counts, groups = {False: [], True: []}, {False: [], True: []}, {}, {}, {}

    def once(dic):
        shutil.rmtree(out, ignore_errors=True)
        torch.cuda.synchronize()
        before = {k: K.STATS.get(k, 0) for k in COUNTERS}
        t0 = time.perf_counter()
        nvt.Dataset(frame).to_parquet(out, use_dictionary=True if dic else None)
        dt = time.perf_counter() - t0
        sizes[dic] = parquet_bytes(out)
        md = pq.read_metadata(os.path.join(out, "part_0.parquet"))
        groups[dic] = md.num_row_groups
        counts[dic] = {k: round((K.STATS.get(k, 0) - before[k]) / md.num_row_groups, 2) for k in COUNTERS}
        return dt, md

    try:
        for dic in (False, True):            # warm-up: code objects, pinned pools, page cache
            _, md = once(dic)
        encoded = sum("RLE_DICTIONARY" in md.row_group(g).column(j).encodings
                      for g in range(md.num_row_groups) for j in range(md.num_columns))
        for _ in range(runs):
            for dic in (False, True):        # alternating: both see the same machine
                dt, _ = once(dic)
                times[dic].append(dt)
                phases[dic].append(dict(nio.LAST_TIMING))
                print(f"{name:8s} use_dictionary={str(dic):5s} {1e3 * dt:8.0f} ms  {rows / dt / 1e6:7.2f} M rows/s", flush=True)
        # the size yardstick: pyarrow's writer, no codec, its default dictionary, on a prefix
        n = min(rows, PYARROW_PREFIX)
        prefix = frame.take_rows(torch.arange(n, device=frame[next(iter(frame.columns))].data.device))
        shutil.rmtree(out, ignore_errors=True)
        nvt.Dataset(prefix).to_parquet(out, use_dictionary=True)
        ours = parquet_bytes(out)
        shutil.rmtree(out, ignore_errors=True)
        nvt.Dataset(prefix).to_parquet(out)
        ours_plain = parquet_bytes(out)
        pa_path = os.path.join(out, "pyarrow_yardstick.pq")
        t0 = time.perf_counter()
        pq.write_table(prefix.to_arrow(), pa_path, compression=None)
        pa_s = time.perf_counter() - t0
        pa_bytes = os.path.getsize(pa_path)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    res = {"rows": rows, "row_groups": groups[True], "chunks_dictionary_encoded": encoded,
           "chunks": md.num_row_groups * md.num_columns, "prefix_rows": n,
           "prefix_bytes": {"plain": ours_plain, "use_dictionary": ours, "pyarrow_uncompressed_dictionary": pa_bytes},
           "pyarrow_prefix_M_rows_s": round(n / pa_s / 1e6, 2)}
    for dic, key in ((False, "plain"), (True, "use_dictionary")):
        med = statistics.median(times[dic])
        res[key] = {"s": round(med, 4), "all_s": [round(x, 4) for x in times[dic]],
                    "M_rows_s": round(rows / med / 1e6, 2), "file_bytes": sizes[dic],
                    "bytes_per_row": round(sizes[dic] / rows, 1),
                    "phases_s": {k: round(statistics.median(p[k] for p in phases[dic]), 4) for k in phases[dic][0]},
                    "per_row_group": counts[dic]}
    res["time_ratio_dictionary_over_plain"] = round(res["use_dictionary"]["s"] / res["plain"]["s"], 3)
    res["size_ratio_dictionary_over_plain"] = round(sizes[True] / sizes[False], 3)
    print(json.dumps({name: res}), flush=True)
    return res


def build_cost(dev, n=1 << 22, reps=5):
    """nvt_pq_dict_build alone (table claims, radix sort of the distinct values, ranks): device events
    around `reps` calls after a warm-up -> {distinct values: ns per value}."""
    lib = _lib.load()
    out = {}
    need = C.c_uint64()
    _lib.check(lib.nvt_pq_dict_ws_bytes(n, 1 << 20, 1, C.byref(need)), "nvt_pq_dict_ws_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    dic = torch.empty(1 << 20, dtype=torch.int64, device=dev)
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    for d in (100, 10_000, 1_000_000, 3_000_000):
        vals = (torch.randint(0, d, (n,), device=dev, dtype=torch.int64) * 2654435761) % (1 << 40)
        call = lambda: _lib.check(lib.nvt_pq_dict_build(vals.data_ptr(), _lib.NVT_I64, n, 1 << 20, dic.data_ptr(),
                                                        state.data_ptr(), ws.data_ptr(), ws.numel(), K.stream_ptr()),
                                  "nvt_pq_dict_build")
        call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        st = state.cpu().numpy()
        out[str(d)] = {"ms": round(a.elapsed_time(b) / reps, 4), "ns_per_value": round(a.elapsed_time(b) / reps * 1e6 / n, 4),
                       "distinct": int(st[0]), "overflow": int(st[1])}
    print(json.dumps({"build_cost_4M_int64": out}), flush=True)
    return out


def main():
    base = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8 << 20
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)          # (no GPU: this raises; nothing here is measured on a CPU)
    torch.zeros(1, device=dev)
    tmp = tempfile.mkdtemp(dir=base)
    try:
        result = {"criteo": measure("criteo", criteo_frame(rows, dev, tmp), runs, base),
                  "session": measure("session", session_frame(rows, dev), runs, base),
                  "build_cost_4M_int64": build_cost(dev)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
