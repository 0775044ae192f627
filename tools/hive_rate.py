"""Rates of the hive-partitioned write: the split of one partition by a low-cardinality key
(nvt_join_hash + nvt_key_labels + nvt_partition_plan + one take_rows) and the whole
``Dataset.to_parquet(partition_on=...)`` against the route a user had before it, ``part.to_arrow()``
followed by ``pyarrow.parquet.write_to_dataset(partition_cols=...)``, in one process.

    python tools/hive_rate.py [--rows 8000000] [--out FILE] [--tmp DIR] [--no-write] [--no-split] [--pair-baseline]

Workload: one frame of the Criteo-shaped output (26 int64 categorical ids, 13 float32 continuous
columns, one label) plus a 24-value int64 key ``day`` and a 100-value string key ``site``; split on
``day`` and on (``day``, ``site``).  Device steps: HIP events, median of 20.  Steps that read back
(the split as the writer runs it, the groupby-table route, the writes): wall clock around a device
synchronise, median of 5 (writes: of 3; pyarrow's route on the key pair: one run, only with
``--pair-baseline``).  The label kernel is set against a device copy that moves the
same bytes (22 per row: tag and null byte read twice, the label written), the fraction is of 8 TB/s,
and against labelling through the groupby tables (nvt_gb_update + compact + lookup)."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nvtabular_amd as nvt  # noqa: E402
from nvtabular_amd import _lib  # noqa: E402
from nvtabular_amd import kernels as K  # noqa: E402
from nvtabular_amd import kernels_labels as KL  # noqa: E402
from nvtabular_amd.device import DeviceColumn, DeviceFrame  # noqa: E402
from nvtabular_amd.kernels_groupby import GroupbyTable  # noqa: E402
from nvtabular_amd.kernels_join import key_descs  # noqa: E402
from nvtabular_amd.kernels_partition import key_modes, plan_from_ids  # noqa: E402
from nvtabular_amd.strings import string_key64  # noqa: E402

PEAK = 8e12


def event_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def wall_ms(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2]


def workload(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cols = {f"C{c}": DeviceColumn(torch.randint(0, 1 << 20, (n,), device=dev, generator=g)) for c in range(26)}
    cols.update({f"I{c}": DeviceColumn(torch.randn(n, device=dev, generator=g)) for c in range(13)})
    cols["label"] = DeviceColumn(torch.randint(0, 2, (n,), device=dev, generator=g))
    cols["day"] = DeviceColumn(torch.randint(0, 24, (n,), device=dev, generator=g))
    names = [f"site-{i:03d}" for i in range(100)]
    keys = string_key64(names)
    lut = dict(zip(keys.tolist(), names))
    pick = torch.randint(0, 100, (n,), device=dev, generator=g)
    cols["site"] = DeviceColumn(torch.from_numpy(keys).to(dev)[pick], None, None, None, lut)
    return DeviceFrame(cols)


def split_steps(frame, keys, dev):
    lib = _lib.load()
    n, nk = len(frame), len(keys)
    modes = key_modes([frame], keys)
    descs, alive = key_descs([frame[k] for k in keys], modes)
    tag = torch.empty(n, dtype=torch.int64, device=dev)
    nulls = torch.empty(n, dtype=torch.uint8, device=dev)
    words = torch.empty((nk, n), dtype=torch.int64, device=dev) if nk > 1 else None
    label = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.zeros(2 + _lib.LABEL_MAX // 2, dtype=torch.int64, device=dev)
    need = C.c_uint64()
    _lib.check(lib.nvt_key_labels_ws_bytes(n, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def hash_():
        _lib.check(lib.nvt_join_hash(descs, nk, n, tag.data_ptr(), K.ptr(words), nulls.data_ptr(), K.stream_ptr()))

    def labels():
        _lib.check(lib.nvt_key_labels(tag.data_ptr(), nulls.data_ptr(), K.ptr(words), nk, n, label.data_ptr(),
                                      out.data_ptr() + 16, out.data_ptr(), ws.data_ptr(), need.value, K.stream_ptr()))

    hash_()
    labels()
    D, status = (int(v) for v in out[:2].cpu())
    assert status == 0, status
    perm, _ = plan_from_ids(label, D)
    data = frame.drop(keys)
    src = torch.empty(n * 11, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def gb_route():
        t = GroupbyTable(nk, 1, 4 * D)
        kd = [frame[k].data for k in keys]
        t.update(kd, [None] * nk, [frame["I0"].data], [None])
        t.compact()
        return t.lookup(kd, [None] * nk)

    bytes_moved = n * 22
    res = {"keys": keys, "rows": n, "distinct": D,
           "hash_ms": event_ms(hash_), "labels_ms": event_ms(labels),
           "plan_ms": event_ms(lambda: plan_from_ids(label, D)),
           "permute_ms": event_ms(lambda: data.take_rows(perm), reps=5, warm=1),
           "stream_same_bytes_ms": event_ms(lambda: dst.copy_(src)),
           "split_as_run_ms": wall_ms(lambda: (KL.split_plan(frame, keys), data.take_rows(perm))),
           "labels_via_groupby_tables_ms": wall_ms(gb_route)}
    res["labels_frac_of_8TBs"] = bytes_moved / (res["labels_ms"] * 1e-3) / PEAK
    res["stream_frac_of_8TBs"] = bytes_moved / (res["stream_same_bytes_ms"] * 1e-3) / PEAK
    del alive
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}


def write_routes(frame, keys, tmp, baseline=True):
    import pyarrow.parquet as pq

    def ours():
        out = os.path.join(tmp, "ours")
        shutil.rmtree(out, ignore_errors=True)
        nvt.Dataset(frame).to_parquet(out, partition_on=keys, max_partitions=4096)

    def theirs():
        out = os.path.join(tmp, "theirs")
        shutil.rmtree(out, ignore_errors=True)
        pq.write_to_dataset(frame.to_arrow(), out, partition_cols=keys, max_partitions=4096)

    # pyarrow's route is host work of seconds to minutes: timed without a warm-up call, once when the
    # key has thousands of directories; every figure is printed as soon as it is there
    res = {"keys": keys, "rows": len(frame), "to_parquet_partition_on_ms": round(wall_ms(ours, reps=3), 1)}
    print(json.dumps(res), file=sys.stderr, flush=True)
    if baseline:
        res["to_arrow_write_to_dataset_ms"] = round(wall_ms(theirs, reps=3 if len(keys) == 1 else 1, warm=0), 1)
        res["speedup"] = round(res["to_arrow_write_to_dataset_ms"] / res["to_parquet_partition_on_ms"], 2)
        print(json.dumps(res), file=sys.stderr, flush=True)
    for d in ("ours", "theirs"):
        shutil.rmtree(os.path.join(tmp, d), ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--no-write", action="store_true", help="skip the two whole-write routes")
    ap.add_argument("--no-split", action="store_true", help="skip the split steps")
    ap.add_argument("--pair-baseline", action="store_true",
                    help="also time pyarrow's route on the key pair (2400 directories: many minutes of host work)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    frame = workload(a.rows, dev)
    res = []
    for keys in ([] if a.no_split else (["day"], ["day", "site"])):
        res.append(dict(split_steps(frame, keys, dev), what="split"))
        torch.cuda.empty_cache()
    if not a.no_write:
        with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
            for keys in (["day"], ["day", "site"]):
                try:
                    res.append(dict(write_routes(frame, keys, tmp, len(keys) == 1 or a.pair_baseline), what="write"))
                except (ValueError, OSError) as e:   # (the limit of open files, a full disk: recorded)
                    res.append({"what": "write", "keys": keys, "failed": f"{type(e).__name__}: {e}"})
    res.append({"what": "readbacks", "per_split": {k: v for k, v in K.STATS.items() if "readback" in k}})
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
