"""Row compaction rate: kernels_compact.compact_frame against DeviceFrame.take_rows.

Compacts the 45 M-row x 39-column frame of bench.synth_criteo (seeded) at keep fractions 0.99 /
0.5 / 0.01 (a seeded uniform mask) two ways:
  compact     kernels_compact.compact_frame(frame, keep): keep mask + plan + ONE nvt_compact_many
  take_rows   DeviceFrame.take_rows(keep.nonzero()): the torch gather of the parquet shuffle
checks that both give the same buffers bit for bit, and prints one JSON line per keep fraction:
median wall time per call (CUDA events; each includes the call's one read-back), algorithmic
bytes (every column read once, the kept rows written once, bitmaps included, plus the mask) and
the rate as GB/s and as a fraction of 8 TB/s.  Kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/filter_rate.py --reps 3``.

    python tools/filter_rate.py [--rows 45000000] [--reps 10] [--fractions 0.99,0.5,0.01]
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


def algorithmic_bytes(frame, n, m):
    total = n  # the keep mask (one byte per row)
    for _, col in frame.items():
        w = col.data.element_size()
        total += (n + m) * w
        if col.valid is not None:
            total += (n + m) // 8
    return total


def same(a, b):
    import torch

    for name in a.columns:
        x, y = a[name], b[name]
        if not x.data.view(torch.uint8).equal(y.data.view(torch.uint8)):
            return False
        if (x.valid is None) != (y.valid is None) or (x.valid is not None and not x.valid.equal(y.valid)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fractions", default="0.99,0.5,0.01")
    args = ap.parse_args()

    import torch

    import bench
    from nvtabular_amd import _lib
    from nvtabular_amd.kernels_compact import compact_frame

    _lib.load()
    dev = torch.device("cuda", 0)
    frame = bench.synth_criteo(args.rows, dev)
    for frac in (float(f) for f in args.fractions.split(",")):
        g = torch.Generator(device=dev).manual_seed(20261016)
        keep = torch.rand(args.rows, device=dev, generator=g) < frac
        torch.cuda.synchronize()
        t_new, a = timed(lambda: compact_frame(frame, keep), args.reps)
        t_ref, b = timed(lambda: frame.take_rows(keep.nonzero().flatten()), max(1, args.reps // 3))
        m = len(a)
        nbytes = algorithmic_bytes(frame, args.rows, m)
        print(json.dumps({
            "rows": args.rows, "columns": len(frame.columns), "keep_fraction": frac, "kept": m,
            "bit_equal": same(a, b), "compact_ms": round(t_new, 3), "take_rows_ms": round(t_ref, 3),
            "speedup": round(t_ref / t_new, 2), "algorithmic_bytes": nbytes,
            "compact_GBps": round(nbytes / t_new / 1e6, 1), "frac_of_8TBps": round(nbytes / (t_new * 1e-3) / PEAK, 3),
        }), flush=True)
        del a, b, keep


if __name__ == "__main__":
    main()
