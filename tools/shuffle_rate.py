"""Shuffle rate: kernels_partition.shuffle_frames against the same shuffle built from torch pieces
and against a plain copy of the same bytes.

The frame is seeded: --rows rows (20 M) x (2 int64 keys, 4 float32, 2 int64 with a validity bitmap),
cut into --inputs input partitions (4), shuffled into P = 8 / 64 / 1024 output partitions.  Timed in
one process, alternating, per P:
  shuffle   shuffle_frames (nvt_join_hash, nvt_partition_ids, nvt_partition_plan, one read-back of
            the counts, nvt_partition_gather_many per output partition)
  torch     the restatement: the same partition ids, torch.argsort(pid, stable=True) per input,
            DeviceFrame.take_rows, torch.bincount read back, then per output partition the slices
            of every input concatenated with torch.cat
  copy      torch's clone of every column and bitmap: the streaming floor for the same bytes
and printed as one JSON line per (P, what): median / min / max wall time over --reps calls (CUDA
events around a call that ends in a synchronise), rows/s, and GB/s over the algorithmic bytes (every
value and bitmap read once and written once).  Kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/shuffle_rate.py --reps 3``.

    python tools/shuffle_rate.py [--rows 20000000] [--inputs 4] [--reps 7] [--parts 8,64,1024]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_frames(rows, inputs, seed=0):
    import torch

    from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap_device

    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    frames = []
    for i in range(inputs):
        n = rows * (i + 1) // inputs - rows * i // inputs
        cols = {
            "k1": DeviceColumn(torch.randint(0, 1 << 20, (n,), generator=g, device=dev, dtype=torch.int64)),
            "k2": DeviceColumn(torch.randint(0, 1 << 10, (n,), generator=g, device=dev, dtype=torch.int64)),
        }
        for j in range(4):
            cols[f"f{j}"] = DeviceColumn(torch.rand(n, generator=g, device=dev, dtype=torch.float32))
        for j in range(2):
            valid = pack_bitmap_device(torch.rand(n, generator=g, device=dev) > 0.1)
            cols[f"v{j}"] = DeviceColumn(torch.randint(0, 1 << 40, (n,), generator=g, device=dev, dtype=torch.int64),
                                         valid)
        frames.append(DeviceFrame(cols))
    return frames


def frame_bytes(frames):
    total = 0
    for f in frames:
        for _, c in f.items():
            total += c.data.numel() * c.data.element_size() + (c.valid.numel() if c.valid is not None else 0)
    return total


def torch_shuffle(frames, keys, P):
    import torch

    from nvtabular_amd import kernels_partition as KP
    from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap_device
    from nvtabular_amd import kernels as K

    modes = KP.key_modes(frames, keys)
    moved, counts = [], []
    for f in frames:
        pid = KP.partition_ids(f, keys, P, modes).to(torch.int64)
        order = torch.argsort(pid, stable=True)
        moved.append(f.take_rows(order))
        counts.append(torch.bincount(pid, minlength=P))
    cnt = torch.stack(counts).cpu().numpy()
    off = cnt.cumsum(axis=1) - cnt
    # bitmaps do not slice at arbitrary rows: unpack each moved bitmap ONCE, cut per output, re-pack
    masks = {name: [K.unpack_bitmap(m[name].valid, len(m)) for m in moved]
             for name in frames[0].columns if frames[0][name].valid is not None}
    out = []
    for p in range(P):
        cols = {}
        for name in frames[0].columns:
            pieces = [m[name].data[off[i, p]: off[i, p] + cnt[i, p]] for i, m in enumerate(moved)]
            valid = None
            if name in masks:
                bits = [b[off[i, p]: off[i, p] + cnt[i, p]] for i, b in enumerate(masks[name])]
                valid = pack_bitmap_device(torch.cat(bits))
            cols[name] = DeviceColumn(torch.cat(pieces), valid)
        out.append(DeviceFrame(cols))
    return out


def copy_frames(frames):
    return [[(c.data.clone(), c.valid.clone() if c.valid is not None else None) for _, c in f.items()]
            for f in frames]


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--inputs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", default="8,64,1024")
    args = ap.parse_args()

    import torch

    from nvtabular_amd import _lib
    from nvtabular_amd.kernels_partition import shuffle_frames

    _lib.require_gpu()
    frames = make_frames(args.rows, args.inputs)
    keys = ["k1", "k2"]
    nbytes = 2 * frame_bytes(frames)
    for P in [int(x) for x in args.parts.split(",")]:
        runs = {"shuffle": lambda: shuffle_frames(frames, keys, P),
                "torch": lambda: torch_shuffle(frames, keys, P),
                "copy": lambda: copy_frames(frames)}
        for fn in runs.values():   # warm-up: code objects, allocator pools
            timed(fn)
        times = {k: [] for k in runs}
        for _ in range(args.reps):   # alternating, so that drift hits all three alike
            for k, fn in runs.items():
                times[k].append(timed(fn))
        # same rows in the same places
        a, b = shuffle_frames(frames, keys, P), torch_shuffle(frames, keys, P)
        for fa, fb in zip(a, b):
            for name in fa.columns:
                assert torch.equal(fa[name].data, fb[name].data), (P, name)
                if fa[name].valid is not None:
                    assert torch.equal(fa[name].valid, fb[name].valid), (P, name)
        del a, b
        for k, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            print(json.dumps({"P": P, "what": k, "rows": args.rows, "inputs": args.inputs, "reps": args.reps,
                              "ms_median": round(med, 3), "ms_min": round(ts[0], 3), "ms_max": round(ts[-1], 3),
                              "rows_per_s": round(args.rows / (med * 1e-3)),
                              "GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
