"""Filter rate: ``Dataset(filters=...)`` 's device route against what ``ops.Filter`` offers for the same
predicate, and a hive directory read through ``filters=`` against reading all of it
(profiles/filters_notes.md).

  python tools/dataset_filter_rate.py [--rows 4000000] [--days 32] [--reps 7] [--out DIR]

Part 1, on a Criteo-shaped frame on the device (13 float32 ``I*`` with NaN, 26 int32 ``C*``, an int64
label and a string column ``S`` of 4 distinct values), the predicate
``C1 in [lo, hi)  AND  C2 in {16 ids}  AND  S == "b"``:

  terms        kernels_compact.filter_frame: nvt_compact_keep_terms + the compaction (one read-back)
  terms_kernel nvt_compact_keep_terms alone (device events), and its bytes per second over the bytes of
               the three columns it names plus the mask it writes
  lambda       ops.Filter with the equivalent lambda: ``isin`` and a string column are not on
               DeviceSeries, so this is the host route (the whole frame through pandas)
  lambda_num   ops.Filter with the numeric half rewritten for the device route (the range, and the set
               as an OR of ==), against ``terms_num``, the same two-column predicate through filter_frame

Part 2, a hive tree ``day=0 .. day=D-1`` of equal files: ``Dataset(root, filters=[("day", "==", 7)])``
iterated to the end, against ``Dataset(root)`` iterated to the end with ``ops.Filter(day == 7)`` on
every partition.  Times are host clock around work that ends in a device synchronise; each line is the
median and the minimum of ``--reps`` runs after one warm-up."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_frame(rows, seed=0):
    import torch

    from nvtabular_amd.device import DeviceColumn, DeviceFrame
    from nvtabular_amd.strings import string_key64

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    frame = DeviceFrame()
    for k in range(1, 14):
        x = torch.randn(rows, device="cuda", generator=g)
        x[torch.rand(rows, device="cuda", generator=g) < 0.1] = float("nan")
        frame[f"I{k}"] = DeviceColumn(x)
    for k in range(1, 27):
        frame[f"C{k}"] = DeviceColumn(torch.randint(0, 64 if k == 2 else 1000, (rows,), device="cuda", generator=g,
                                                    dtype=torch.int32))
    frame["label"] = DeviceColumn(torch.randint(0, 2, (rows,), device="cuda", generator=g))
    words = ["a", "b", "c", "d"]
    keys = torch.from_numpy(string_key64(words)).cuda()
    frame["S"] = DeviceColumn(keys[torch.randint(0, 4, (rows,), device="cuda", generator=g)], None, None, None,
                              dict(zip(string_key64(words).tolist(), words)))
    return frame


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(out), "min_ms": 1e3 * min(out), "reps": reps}


def kernel_alone(frame, flt, reps):
    """nvt_compact_keep_terms by itself between two device events."""
    import torch

    from nvtabular_amd import _lib, kernels as K
    from nvtabular_amd import kernels_compact as KC

    n = len(frame)
    low = flt.lower({c: frame[c].data.dtype.is_floating_point for c in flt.columns})
    descs = (_lib.FilterCol * len(low.columns))()
    for d, c in zip(descs, low.columns):
        d.x, d.valid, d.dtype = frame[c].data.data_ptr(), K.ptr(frame[c].valid), KC._FILTER_CODE[frame[c].data.dtype]
    terms = (_lib.FilterTerm * len(low.terms))()
    for d, (j, op, conj, set_len, set_off, value) in zip(terms, low.terms):
        d.col, d.op, d.conj, d.set_len, d.set_off = j, op, conj, set_len, set_off
        if low.floats[j]:
            d.value.f = value
        else:
            d.value.i = value
    sets = torch.from_numpy(low.sets.view("int64").copy()).cuda()
    ws = KC._plan_ws(n, sets.device)
    lib = _lib.load()

    def launch():
        _lib.check(lib.nvt_compact_keep_terms(descs, len(low.columns), terms, len(low.terms), sets.data_ptr(),
                                              int(low.sets.size), n, ws.data_ptr(), ws.numel(), K.stream_ptr()),
                   "nvt_compact_keep_terms")

    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 10)
    nbytes = sum(frame[c].data.element_size() for c in low.columns) * n + n // 8
    ms = statistics.median(times)
    return {"median_ms": ms, "min_ms": min(times), "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6}


def part1(rows, reps):
    from nvtabular_amd import filters as F
    from nvtabular_amd import ops
    from nvtabular_amd.kernels_compact import filter_frame
    from nvtabular_amd.schema import Schema
    from nvtabular_amd.selector import ColumnSelector

    frame = make_frame(rows)
    ids = list(range(0, 64, 4))
    dnf = [("C1", ">=", 100), ("C1", "<", 600), ("C2", "in", ids), ("S", "==", "b")]
    num = dnf[:3]
    schema = Schema.from_frame(frame)
    flt, flt_num = F.validate(F.normalize(dnf), schema), F.validate(F.normalize(num), schema)
    sel = ColumnSelector(frame.columns)

    def lam(df):
        return (df["C1"] >= 100) & (df["C1"] < 600) & df["C2"].isin(ids) & (df["S"] == "b")

    def lam_num(df):
        hit = df["C2"] == ids[0]
        for v in ids[1:]:
            hit = hit | (df["C2"] == v)
        return (df["C1"] >= 100) & (df["C1"] < 600) & hit

    host, dev = ops.Filter(lam), ops.Filter(lam_num)
    res = {"rows": rows, "columns": len(frame.columns)}
    a, b = filter_frame(frame, flt), host.transform(sel, frame)
    assert host.last_path == "host" and len(a) == len(b), (host.last_path, len(a), len(b))
    c, d = filter_frame(frame, flt_num), dev.transform(sel, frame)
    assert dev.last_path == "device" and len(c) == len(d)
    res["kept"], res["kept_num"] = len(a), len(c)
    # the variants alternate inside every repetition block
    res["terms"] = timed(lambda: filter_frame(frame, flt), reps)
    res["lambda_num"] = timed(lambda: dev.transform(sel, frame), reps)
    res["terms_num"] = timed(lambda: filter_frame(frame, flt_num), reps)
    res["terms_again"] = timed(lambda: filter_frame(frame, flt), reps)
    res["lambda"] = timed(lambda: host.transform(sel, frame), 2)
    res["terms_kernel"] = kernel_alone(frame, flt, reps)
    return res


def part2(rows, days, reps, tmp):
    import pyarrow as pa
    import pyarrow.parquet as pq

    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.selector import ColumnSelector

    rng = np.random.default_rng(1)
    per = rows // days
    root = os.path.join(tmp, "hive")
    for d in range(days):
        cols = {f"I{k}": rng.normal(size=per).astype(np.float32) for k in range(1, 5)}
        cols.update({f"C{k}": rng.integers(0, 1000, per).astype(np.int32) for k in range(1, 7)})
        os.makedirs(os.path.join(root, f"day={d}"))
        pq.write_table(pa.table(cols), os.path.join(root, f"day={d}", "part.parquet"), row_group_size=per)
    only = ops.Filter(lambda df: df["day"] == 7)

    def filtered():
        ds = nvt.Dataset(root, filters=[("day", "==", 7)])
        return sum(len(p) for p in ds.to_iter())

    def whole():
        ds = nvt.Dataset(root)
        return sum(len(only.transform(ColumnSelector(p.columns), p)) for p in ds.to_iter())

    assert filtered() == whole() == per
    return {"rows": per * days, "days": days, "kept": per, "filters": timed(filtered, reps),
            "whole_then_filter": timed(whole, reps), "filters_again": timed(filtered, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--days", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "dataset_filter_rate.py measures on the GPU"
    res = {"part1": part1(args.rows, args.reps)}
    with tempfile.TemporaryDirectory() as tmp:
        res["part2"] = part2(args.rows, args.days, args.reps, tmp)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "dataset_filter_rate.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
