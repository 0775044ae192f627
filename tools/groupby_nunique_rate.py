"""Groupby nunique: what the aggregation adds to a Groupby step, on one card.

Two frames of an int64 key column and an int64 item column (and the same items as int32):
  session   many groups of about ten rows (--rows / 10 users)
  large     a few very large groups (--large-groups users)
For each frame, alternating, repeated --reps times after a warm-up of every variant:
  groupby_count_ms           ops.Groupby(aggs={"item": ["count"]}) on the resident frame
  groupby_count_nunique_ms   the same with ["count", "nunique"]: the difference is the added cost
  seg_aggregate_ms           K.seg_aggregate alone on the ordered rows (device events)
  seg_nunique_i64_ms / seg_nunique_i32_ms   K.seg_nunique alone on the same rows
and checks the nunique column against numpy on the host.  Prints one JSON line per frame.

    python tools/groupby_nunique_rate.py [--rows 20000000] [--large-groups 4] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_frame(rows, groups, items, seed):
    import numpy as np
    import torch

    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    user = rng.integers(0, groups, rows).astype(np.int64)
    item = rng.integers(0, items, rows).astype(np.int64)
    frame = DeviceFrame({"user": DeviceColumn(torch.from_numpy(user).cuda()),
                         "item": DeviceColumn(torch.from_numpy(item).cuda())})
    return frame, user, item


def host_nunique(user, item):
    import numpy as np

    span = int(item.max()) + 1                        # (user, item) pairs as one int64
    pairs = np.unique(user * span + item)
    return np.unique(pairs // span, return_counts=True)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def time_frame(name, frame, user, item, reps):
    import numpy as np
    import torch

    from nvtabular_amd import ColumnSelector, ops
    from nvtabular_amd import kernels as K

    sel = ColumnSelector(["user", "item"])
    variants = {"groupby_count_ms": ops.Groupby(groupby_cols=["user"], aggs={"item": ["count"]}),
                "groupby_count_nunique_ms": ops.Groupby(groupby_cols=["user"], aggs={"item": ["count", "nunique"]})}
    times = {k: [] for k in variants}
    out = {}
    for rep in range(reps + 1):                       # rep 0: warm-up of every variant
        for k, op in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[k] = op.transform(sel, frame)
            torch.cuda.synchronize()
            if rep:
                times[k].append((time.perf_counter() - t0) * 1e3)
    got = out["groupby_count_nunique_ms"]
    keys, exp = host_nunique(user, item)
    ok = bool(np.array_equal(got["user"].data.cpu().numpy(), keys)
              and np.array_equal(got["item_nunique"].data.cpu().numpy(), exp)
              and np.array_equal(got["item_count"].data.cpu().numpy(),
                                 out["groupby_count_ms"]["item_count"].data.cpu().numpy()))

    # the kernels alone, on the rows the operator would order: group id = rank of the key
    rank = torch.from_numpy(np.searchsorted(keys, user)).cuda()
    ngroups = int(keys.size)
    n = int(user.size)
    words = K.order_rows(n, rank.device, (), rank, ngroups)
    item64 = frame["item"].data
    item32 = item64.to(torch.int32)
    kernels = {"seg_aggregate_ms": lambda: K.seg_aggregate(words, ngroups, [item64], [None]),
               "seg_nunique_i64_ms": lambda: K.seg_nunique(words, ngroups, [item64], [None]),
               "seg_nunique_i32_ms": lambda: K.seg_nunique(words, ngroups, [item32], [None])}
    ktimes = {k: [] for k in kernels}
    for rep in range(reps + 1):
        for k, fn in kernels.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            torch.cuda.synchronize()
            if rep:
                ktimes[k].append(a.elapsed_time(b))
            if k == "seg_nunique_i32_ms" and rep == 0:
                ok = ok and bool(np.array_equal(res[0].cpu().numpy(), exp))
    res = {"frame": name, "rows": n, "groups": ngroups, "equal_numpy": ok}
    for k, v in {**times, **ktimes}.items():
        res[k] = round(median(v), 3)
        res[k.replace("_ms", "_spread_ms")] = [round(min(v), 3), round(max(v), 3)]
    res["added_ms"] = round(res["groupby_count_nunique_ms"] - res["groupby_count_ms"], 3)
    res["nunique_i64_rows_per_s"] = round(n / (res["seg_nunique_i64_ms"] * 1e-3))
    res["nunique_i32_rows_per_s"] = round(n / (res["seg_nunique_i32_ms"] * 1e-3))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--large-groups", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    from nvtabular_amd import _lib

    _lib.require_gpu()
    time_frame("warmup", *make_frame(50_000, 5_000, 1000, seed=1), reps=1)   # code objects, allocator
    time_frame("session", *make_frame(args.rows, max(args.rows // 10, 1), 50_000, seed=2), reps=args.reps)
    time_frame("large", *make_frame(args.rows, args.large_groups, 50_000, seed=3), reps=args.reps)


if __name__ == "__main__":
    main()
