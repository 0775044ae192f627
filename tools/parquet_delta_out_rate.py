"""to_parquet of one row group (2^23 rows) of one int64 column, with and without column_encoding: an
ascending timestamp-like column and a random id column that falls back to PLAIN.  The variants alternate
inside every repeat; host clock around the call and a device synchronise; then sizing + scan + pack of one
chunk alone between device events.  Prints one JSON object (profiles/parquet_delta_out_notes.md).
Run from the repository root: PYTHONPATH=. python tools/parquet_delta_out_rate.py"""
import json
import os
import shutil
import statistics
import tempfile
import time

import numpy as np
import torch

import nvtabular_amd as nvt
from nvtabular_amd import kernels_parquet_delta_out as KDO
from nvtabular_amd.device import DeviceColumn, DeviceFrame

ROWS, REPS, WARM = 1 << 23, 9, 2
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
cols = {"ts": 1_700_000_000_000 + np.cumsum(rng.integers(0, 2000, ROWS)).astype(np.int64),
        "id": rng.integers(-2**63, 2**63 - 1, ROWS, dtype=np.int64)}
frames = {k: DeviceFrame({k: DeviceColumn(torch.from_numpy(v).to(dev))}) for k, v in cols.items()}
root = tempfile.mkdtemp()
times, sizes = {}, {}
variants = [(c, e) for c in cols for e in (None, "DELTA_BINARY_PACKED")]
for rep in range(WARM + REPS):
    for c, e in variants:   # (alternating the variants inside every repeat)
        out = os.path.join(root, f"{c}_{e}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nvt.Dataset(frames[c]).to_parquet(out, column_encoding=e)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep >= WARM:
            times.setdefault(f"{c}/{e or 'PLAIN'}", []).append(dt * 1e3)
        sizes[f"{c}/{e or 'PLAIN'}"] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out) if f.endswith(".parquet"))
        shutil.rmtree(out)
# the kernels alone: sizing + scan + pack of one chunk, device events
kern = {}
ps = torch.clamp(torch.arange(9, device=dev, dtype=torch.int64) << 20, max=ROWS)
for c in cols:
    v = torch.from_numpy(cols[c]).to(dev)
    for rep in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dl = KDO.encode(v, ps)
        b.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            kern.setdefault(c, []).append(a.elapsed_time(b))
    kern[c + "_pays"] = int(dl.table[1])
res = {"rows": ROWS, "reps": REPS, "sizes_bytes": sizes,
       "to_parquet_ms": {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()},
       "encode_kernels_ms": {k: (dict(median=statistics.median(v), min=min(v), max=max(v)) if isinstance(v, list) else v)
                             for k, v in kern.items()}}
print(json.dumps(res, indent=1))
shutil.rmtree(root)
