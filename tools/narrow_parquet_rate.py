"""to_parquet and Dataset(path) on the Criteo-shaped frame of tools/parquet_dict_rate.py plus one int8
label and one bool column: seconds to write, seconds to read this project's file back, seconds to
read pyarrow's default file of the same frame, bytes per row, who wrote the file (created_by) and how
many column chunks went to the hand-written reader / to pyarrow.  It uses the public interface only,
so the same script run in a checkout of the parent commit measures the parent (which takes pyarrow's
route for the whole frame).  One JSON line at the end.

    python tools/narrow_parquet_rate.py [rows] [runs] [out_dir]"""
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
import pyarrow.parquet as pq
import torch

import nvtabular_amd as nvt
from nvtabular_amd import parquet_plain as PP
from nvtabular_amd.device import DeviceColumn, DeviceFrame
from parquet_dict_rate import criteo_frame, parquet_bytes


def read_all(path):
    """Seconds until every partition of Dataset(path) is a DeviceFrame; (plain, pyarrow) chunks."""
    before = dict(PP.READER_CHUNKS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = 0
    for part in nvt.Dataset(path, engine="parquet").to_iter():
        rows += len(part)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, rows, {k: PP.READER_CHUNKS[k] - before[k] for k in before}


def main():
    base = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8 << 20
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda", 0)          # (no GPU: this raises; nothing here is measured on a CPU)
    torch.zeros(1, device=dev)
    tmp = tempfile.mkdtemp(dir=base)
    out, ref = os.path.join(tmp, "out"), os.path.join(tmp, "pyarrow")
    try:
        frame = criteo_frame(rows, dev, tmp)
        rng = np.random.default_rng(0)
        cols = dict(frame.items())
        cols["click"] = DeviceColumn(torch.from_numpy((rng.random(rows) < 0.03).astype(np.int8)).to(dev))
        cols["seen"] = DeviceColumn(torch.from_numpy(rng.random(rows) < 0.5).to(dev))
        frame = DeviceFrame(cols)
        os.makedirs(ref)
        pq.write_table(frame.to_arrow(), os.path.join(ref, "part_0.parquet"))   # pyarrow's defaults
        write_s, read_s, read_ref_s = [], [], []
        for run in range(runs + 1):              # (run 0 warms up: code objects, pinned pools, page cache)
            shutil.rmtree(out, ignore_errors=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nvt.Dataset(frame).to_parquet(out)
            w = time.perf_counter() - t0
            r, n, chunks = read_all(out)
            rr, n_ref, chunks_ref = read_all(ref)
            assert n == rows and n_ref == rows
            print(f"run {run}: write {w:.3f} s, read {r:.3f} s, read pyarrow's file {rr:.3f} s", flush=True)
            if run:
                write_s.append(w)
                read_s.append(r)
                read_ref_s.append(rr)
        md = pq.read_metadata(os.path.join(out, "part_0.parquet"))
        res = {"rows": rows, "columns": len(frame.columns), "created_by": md.created_by,
               "write_s": round(statistics.median(write_s), 3), "read_s": round(statistics.median(read_s), 3),
               "read_pyarrow_file_s": round(statistics.median(read_ref_s), 3),
               "all": {"write_s": [round(x, 3) for x in write_s], "read_s": [round(x, 3) for x in read_s],
                       "read_pyarrow_file_s": [round(x, 3) for x in read_ref_s]},
               "bytes_per_row": round(parquet_bytes(out) / rows, 2),
               "pyarrow_file_bytes_per_row": round(parquet_bytes(ref) / rows, 2),
               "reader_chunks": chunks, "reader_chunks_pyarrow_file": chunks_ref}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
