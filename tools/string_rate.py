"""String column construction: host path against device path.

Times DeviceColumn construction for a string column of hex ids (Zipf over ~2 M distinct values)
two ways:
  host    strings.string_column_to_device(arr.to_pandas())  -- pandas' SipHash per row on one core
  device  kernels_strings: upload of the Arrow buffers, nvt_str_hash, nvt_str_dedup (+ read-back),
          nvt_str_gather + the Python dict build
and checks that both give the same keys and dict.  Prints one JSON line per variant.

    python tools/string_rate.py [--rows 45000000] [--distinct 2000000] [--lens 16,32] [--skip-host]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_column(rows, distinct, length, seed=0):
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    vocab = pa.array([f"{x:0{length}x}"[-length:] for x in rng.integers(1 << 62, 1 << 63, distinct)])
    if length > 16:
        vocab = pa.array([f"{s}{s[::-1]}"[:length] for s in vocab.to_pylist()])
    idx = ((rng.zipf(1.1, rows) - 1) % distinct).astype(np.int32)
    return pa.DictionaryArray.from_arrays(pa.array(idx), vocab).dictionary_decode()


def device_path(arr, dev):
    import torch

    from nvtabular_amd import kernels_strings as KS
    from nvtabular_amd.device import DeviceColumn

    sync = torch.cuda.synchronize
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    sync()
    t0 = time.perf_counter()
    b = KS.upload(arr, dev)
    sync()
    t1 = time.perf_counter()
    ev[0].record()
    keys = KS.hash_buffers(b)
    ev[1].record()
    m, bad, rep_keys, rep_strs = KS.dedup(keys, b.valid, b)
    ev[2].record()
    t2 = time.perf_counter()
    strs = KS.gather(rep_strs, b)
    ev[3].record()
    t3 = time.perf_counter()
    lut = dict(zip(rep_keys.cpu().numpy().tolist(), strs.to_pylist()))
    t4 = time.perf_counter()
    col = DeviceColumn(keys, b.valid, None, None, lut)
    sync()
    assert bad == 0
    return col, {
        "h2d_s": t1 - t0,
        "hash_kernel_ms": ev[0].elapsed_time(ev[1]),
        "dedup_kernels_ms": ev[1].elapsed_time(ev[2]),
        "gather_and_copy_back_ms": ev[2].elapsed_time(ev[3]),
        "gather_s": t3 - t2,
        "dict_build_s": t4 - t3,
        "total_s": t4 - t0,
        "distinct": m,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45_000_000)
    ap.add_argument("--distinct", type=int, default=2_000_000)
    ap.add_argument("--lens", default="16,32")
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from nvtabular_amd import _lib
    from nvtabular_amd.strings import string_column_to_device

    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    device_path(make_column(10_000, 1000, 16, seed=1), dev)   # warm-up: code objects, allocator
    for length in (int(x) for x in args.lens.split(",")):
        arr = make_column(args.rows, args.distinct, length)
        res = {"rows": args.rows, "len": length, "chars_bytes": arr.nbytes}
        col, dres = device_path(arr, dev)
        res["device"] = dres
        if not args.skip_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = arr.to_pandas()
            t1 = time.perf_counter()
            host = string_column_to_device(s, dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res["host"] = {"to_pandas_s": t1 - t0, "hash_dict_upload_s": t2 - t1, "total_s": t2 - t0}
            res["equal"] = bool(np.array_equal(col.data.cpu().numpy(), host.data.cpu().numpy())
                                and col.strings == host.strings and list(col.strings) == list(host.strings))
            res["speedup"] = res["host"]["total_s"] / dres["total_s"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
