"""Join rate: ops.JoinExternal (kernels_join.py) against the same join built from existing pieces.

The left frame is bench.synth_criteo (45 M rows, seeded).  It is joined on the categorical C3 against
external tables of 10^5 / 10^6 / 10^7 distinct keys (the column's own ids first, then ids it does not
hold) with four payload columns (int64, float32, float64, string), how = left and inner, two ways:
  join       JoinExternal.transform (index built once, before the timing)
  baseline   nvt_gb_index_build / nvt_gb_lookup (row -> external row), then torch index_select per
             column (inner: nonzero of the matches, index_select of every left column too)
and prints one JSON line per case: median wall time per call (CUDA events), algorithmic bytes (key
read, external values gathered and written, validity bitmaps; inner: the left columns read and
written), GB/s and the fraction of 8 TB/s.  Kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/join_rate.py --reps 3``.

    python tools/join_rate.py [--rows 45000000] [--reps 10] [--keys 100000,1000000,10000000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def timed(fn, reps):
    import torch

    times, out = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], out


def external_table(left_keys, d, seed):
    import numpy as np
    import pyarrow as pa
    import torch

    have = torch.unique(left_keys).cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(seed)
    keys = have[:d]
    if len(keys) < d:   # ids the column does not hold (synth_criteo ids are below 2^31)
        keys = np.concatenate([keys, (1 << 31) + np.arange(d - len(keys), dtype=np.int64)])
    rng.shuffle(keys)
    return pa.table({
        "C3": pa.array(keys),
        "p_i64": pa.array(rng.integers(0, 1 << 40, d), pa.int64()),
        "p_f32": pa.array(rng.standard_normal(d).astype(np.float32)),
        "p_f64": pa.array(rng.standard_normal(d)),
        "p_str": pa.array([f"s{i}" for i in range(100_000)]).take(pa.array(rng.integers(0, 100_000, d))),
    })


def baseline(frame, ext_frame, how):
    import torch

    from nvtabular_amd.kernels_groupby import GroupbyTable

    d = len(ext_frame)
    tab = GroupbyTable(1, 0, 2 * d)
    tab.index_build([ext_frame["C3"].data], None)
    key = frame["C3"]

    def run():
        idx = tab.lookup([key.data], [key.valid])
        out = {}
        if how == "inner":
            rows = (idx >= 0).nonzero().flatten()
            for name, col in frame.items():
                out[name] = col.data.index_select(0, rows)
            idx = idx.index_select(0, rows)
        else:
            idx = idx.clamp(min=0)
        for name, col in ext_frame.items():
            if name != "C3":
                out[name] = col.data.index_select(0, idx)
        return out

    return run


def algorithmic_bytes(frame, payload, n, m, how):
    total = n * frame["C3"].data.element_size()
    for _, col in payload.items():
        total += 2 * m * col.data.element_size() + m // 8
    if how == "inner":
        total += n   # keep mask
        for _, col in frame.items():
            total += (n + m) * col.data.element_size() + ((n + m) // 8 if col.valid is not None else 0)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keys", default="100000,1000000,10000000")
    args = ap.parse_args()

    import torch

    import bench
    from nvtabular_amd import _lib, ops
    from nvtabular_amd.selector import ColumnSelector

    _lib.load()
    dev = torch.device("cuda", 0)
    frame = bench.synth_criteo(args.rows, dev)
    sel = ColumnSelector(list(frame.columns))
    for d in (int(x) for x in args.keys.split(",")):
        ext = external_table(frame["C3"].data, d, d)
        for how in ("left", "inner"):
            op = ops.JoinExternal(ext, on="C3", how=how)
            out = op.transform(sel, frame)   # builds the index
            torch.cuda.synchronize()
            t_join, out = timed(lambda: op.transform(sel, frame), args.reps)
            m = len(out)
            payload = {c: out[c] for c in ("p_i64", "p_f32", "p_f64", "p_str")}
            nbytes = algorithmic_bytes(frame, payload, args.rows, m, how)
            row = {"rows": args.rows, "distinct_keys": d, "how": how, "out_rows": m,
                   "join_ms": round(t_join, 3), "algorithmic_bytes": nbytes,
                   "join_GBps": round(nbytes / t_join / 1e6, 1),
                   "frac_of_8TBps": round(nbytes / (t_join * 1e-3) / PEAK, 3)}
            try:
                run = baseline(frame, op._external_frame(), how)
                t_base, _ = timed(run, max(1, args.reps // 3))
                row.update(baseline_ms=round(t_base, 3), speedup=round(t_base / t_join, 2))
            except Exception as e:   # (reported, not hidden)
                row.update(baseline_error=str(e)[:200])
            print(json.dumps(row), flush=True)
            del out, op
        del ext


if __name__ == "__main__":
    main()
