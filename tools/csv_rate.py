#!/usr/bin/env python3
"""Delimited text in: Dataset(engine="csv") against what a user had before it,
pyarrow.csv.read_csv with the same types followed by Dataset(table), both to device frames, on the
same machine in the same run.

  python tools/csv_rate.py [--rows N] [--reps K] [--dir DIR]

Writes a Criteo-shaped TSV (1 label, 13 integer and 26 hex-string columns; empties in both kinds),
times both routes (median of K passes after a warm-up), and prints one JSON line: GB/s of text for
both, the per-kernel split of one pass (HIP events recorded inside the library) and the share of
float fields that the device parser handed to the host on repr() of random doubles."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INTS = ["I%d" % i for i in range(1, 14)]
CATS = ["C%d" % i for i in range(1, 27)]
NAMES = ["label"] + INTS + CATS
CARDS = [10, 100, 1000, 10_000, 100_000]


def write_tsv(path, rows, seed=0, block=250_000):
    rng = np.random.default_rng(seed)
    vocabs = [np.array(["%08x" % ((k * 2654435761 + 97 * j) & 0xFFFFFFFF) for k in range(CARDS[j % len(CARDS)])],
                       dtype=object) for j in range(len(CATS))]
    with open(path, "w") as f:
        for r0 in range(0, rows, block):
            n = min(block, rows - r0)
            cols = {"label": rng.integers(0, 2, n).astype(str).astype(object)}
            for c in INTS:
                v = np.floor(rng.lognormal(2, 2, n)).astype(np.int64).astype(str).astype(object)
                v[rng.random(n) < 0.1] = ""
                cols[c] = v
            for j, c in enumerate(CATS):
                v = vocabs[j][rng.zipf(1.2, n) % len(vocabs[j])]
                v[rng.random(n) < 0.05] = ""
                cols[c] = v
            pd.DataFrame(cols).to_csv(f, sep="\t", header=False, index=False)
    return os.path.getsize(path)


def timed(fn, reps):
    import torch

    fn()   # warm-up: allocator pools, pinned staging, kernel load
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--part-size", default="128MiB")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()

    import pyarrow as pa
    import pyarrow.csv as pc
    import torch

    import nvtabular_amd as nvt
    from nvtabular_amd import kernels as K

    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or pa.cpu_count()
    pa.set_cpu_count(threads)
    dtypes = {"label": "int32", **{c: "int64" for c in INTS}, **{c: "string" for c in CATS}}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, "criteo_like.tsv")
        size = write_tsv(path, args.rows)

        def device_route():
            rows = 0
            for frame in nvt.Dataset(path, engine="csv", sep="\t", names=NAMES, dtypes=dtypes,
                                     part_size=args.part_size).to_iter():
                rows += len(frame)
            assert rows == args.rows

        arrow_types = {"label": pa.int32(), **{c: pa.int64() for c in INTS}, **{c: pa.string() for c in CATS}}

        def arrow_route():
            table = pc.read_csv(path, read_options=pc.ReadOptions(column_names=NAMES),
                                parse_options=pc.ParseOptions(delimiter="\t"),
                                convert_options=pc.ConvertOptions(column_types=arrow_types, null_values=[""],
                                                                  strings_can_be_null=True))
            rows = 0
            for frame in nvt.Dataset(table).to_iter():
                rows += len(frame)
            assert rows == args.rows

        dev_s, dev_all = timed(device_route, args.reps)
        arw_s, arw_all = timed(arrow_route, args.reps)
        K.profile_begin()
        device_route()
        torch.cuda.synchronize()
        rep = K.profile_report()
        kernels = {k: round(v[0], 3) for k, v in sorted(rep["kernels"].items(), key=lambda kv: -kv[1][0])}

        # slow-path share: one float64 column of repr() of random doubles
        rng = np.random.default_rng(1)
        vals = np.concatenate([rng.standard_normal(100_000) * 10.0 ** rng.integers(-30, 30, 100_000),
                               rng.integers(0, 0x7FF0 << 48, 100_000, dtype=np.uint64).view(np.float64)])
        fpath = os.path.join(tmp, "doubles.csv")
        with open(fpath, "w") as f:
            f.write("x\n" + "\n".join(repr(float(v)) for v in vals) + "\n")
        before = dict(K.STATS)
        for _ in nvt.Dataset(fpath, dtypes={"x": "float64"}).to_iter():
            pass
        fields = K.STATS.get("csv_float_fields", 0) - before.get("csv_float_fields", 0)
        slow = K.STATS.get("csv_slow_fields", 0) - before.get("csv_slow_fields", 0)

    print(json.dumps({
        "device": torch.cuda.get_device_name(0), "rows": args.rows, "text_bytes": size, "part_size": args.part_size,
        "csv_engine_s": round(dev_s, 4), "csv_engine_GBps": round(size / dev_s / 1e9, 3),
        "csv_engine_all_s": [round(x, 4) for x in dev_all],
        "pyarrow_threads": threads, "pyarrow_route_s": round(arw_s, 4),
        "pyarrow_route_GBps": round(size / arw_s / 1e9, 3), "pyarrow_route_all_s": [round(x, 4) for x in arw_all],
        "kernel_ms_one_pass": kernels, "kernel_busy_ms": round(rep.get("busy_ms", 0.0), 3),
        "float_fields": fields, "float_fields_slow_path": slow,
        "slow_path_share": (slow / fields) if fields else None,
    }))


if __name__ == "__main__":
    main()
