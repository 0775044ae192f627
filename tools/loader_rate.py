"""Chunk-gather rate of the dataloader: the batch-gather kernels against the torch composition
they replace (DeviceFrame.take_rows + .to() casts + torch.stack), in one process, HIP events,
median of 20.  Both sides are asserted bit-equal before anything is timed.

    python tools/loader_rate.py [--rows 45000000] [--parts 8] [--list-rows 20000000] [--out FILE]
    python tools/loader_rate.py --loader [--runs 5] [--out FILE]

``--loader`` times what the dataloader itself does per chunk, ``TorchAsyncItr._gather`` with
``shuffle=True``: the same rows as ONE partition (``parts_per_chunk=1``) and cut into four
(``parts_per_chunk=4``), in dict mode, stacked mode and for a list column; ``--runs`` repeated runs of
a median of 10 each, reported as the median of the runs and their spread (lowest and highest run).
It goes through the loader only, so the same file measures any commit that has the loader.  Where
the multi-source kernels exist it also times the two candidates for the plain dict-mode columns of a
chunk of four partitions: the kernel, and ``torch.cat`` + ``torch.index_select``.

Workload: a Criteo-shaped transformed frame (26 int64 categorical ids, 13 float32 continuous
columns, one label) in ``--parts`` partitions; one chunk = one partition, shuffled.  Bytes moved =
index + sources read + outputs written; the fraction is of 8 TB/s."""
import argparse
import json
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nvtabular_amd import kernels_loader as KD  # noqa: E402
from nvtabular_amd.device import DeviceColumn, DeviceFrame  # noqa: E402

PEAK = 8e12


def median_ms(fn, reps=20, warm=3):
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


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def scalar_workload(m, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cols = {}
    for c in range(26):
        cols[f"C{c}"] = DeviceColumn(torch.randint(0, 1 << 20, (m,), device=dev, generator=g))
    for c in range(13):
        cols[f"I{c}"] = DeviceColumn(torch.randn(m, device=dev, generator=g))
    cols["label"] = DeviceColumn(torch.randint(0, 2, (m,), device=dev, generator=g))
    frame = DeviceFrame(cols)
    index = torch.randperm(m, device=dev, generator=g)
    cats, conts = [f"C{c}" for c in range(26)], [f"I{c}" for c in range(13)]
    out = []

    def kernel_dict():
        bufs = {n: torch.empty(m, dtype=frame[n].data.dtype, device=dev) for n in cats + conts}
        y = torch.empty(m, dtype=torch.float32, device=dev)
        KD.take_frame(frame, index, [KD.Take(n, bufs[n]) for n in cats + conts] + [KD.Take("label", y)])
        return bufs, y

    def torch_dict():
        t = frame.take_rows(index)
        return {n: t[n].data for n in cats + conts}, t["label"].data.to(torch.float32)

    def kernel_stacked():
        xc = torch.empty((m, 26), dtype=torch.int64, device=dev)
        xf = torch.empty((m, 13), dtype=torch.float32, device=dev)
        y = torch.empty(m, dtype=torch.float32, device=dev)
        KD.take_frame(frame, index, [KD.Take(n, xc, column=c) for c, n in enumerate(cats)] +
                      [KD.Take(n, xf, column=c) for c, n in enumerate(conts)] + [KD.Take("label", y)])
        return {"cats": xc, "conts": xf}, y

    def torch_stacked():
        t = frame.take_rows(index)
        return {"cats": torch.stack([t[n].data.to(torch.int64) for n in cats], dim=1),
                "conts": torch.stack([t[n].data.to(torch.float32) for n in conts], dim=1)}, \
            t["label"].data.to(torch.float32)

    src_bytes = m * (26 * 8 + 13 * 4 + 8)
    for mode, kern, base in (("dict", kernel_dict, torch_dict), ("stacked", kernel_stacked, torch_stacked)):
        (xa, ya), (xb, yb) = kern(), base()
        assert same(ya, yb) and all(same(xa[k], xb[k]) for k in xa), mode
        del xa, ya, xb, yb
        moved = m * 8 + src_bytes + m * (26 * 8 + 13 * 4 + 4)
        k_ms, b_ms = median_ms(kern), median_ms(base)
        out.append({"workload": "criteo", "mode": mode, "rows_per_chunk": m, "kernel_ms": round(k_ms, 3),
                    "baseline_ms": round(b_ms, 3), "speedup": round(b_ms / k_ms, 3), "bytes_moved": moved,
                    "kernel_frac_of_8TBs": round(moved / (k_ms * 1e-3) / PEAK, 4),
                    "baseline_frac_of_8TBs": round(moved / (b_ms * 1e-3) / PEAK, 4)})
    return out


def list_workload(rows, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    lens = torch.randint(0, 17, (rows,), device=dev, generator=g)          # 8 leaves per row on average
    offsets = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offsets[1:])
    leaves = int(offsets[-1].item())
    frame = DeviceFrame({"s": DeviceColumn(torch.randint(0, 1 << 20, (leaves,), device=dev, generator=g), None,
                                           offsets)})
    index = torch.randperm(rows, device=dev, generator=g)

    def kern():
        got, _ = KD.take_lists(frame, ["s"], index)
        return got["s"][0], got["s"][1]

    def base():
        t = frame.take_rows(index)["s"]
        return t.data, t.offsets

    (va, oa), (vb, ob) = kern(), base()
    assert same(va, vb) and same(oa, ob)
    del va, oa, vb, ob
    moved = rows * 8 + rows * 16 + rows * 8 + leaves * 16
    k_ms, b_ms = median_ms(kern), median_ms(base)
    return [{"workload": "list", "mode": "ragged", "rows_per_chunk": rows, "leaves": leaves,
             "kernel_ms": round(k_ms, 3), "baseline_ms": round(b_ms, 3), "speedup": round(b_ms / k_ms, 3),
             "bytes_moved": moved, "kernel_frac_of_8TBs": round(moved / (k_ms * 1e-3) / PEAK, 4),
             "baseline_frac_of_8TBs": round(moved / (b_ms * 1e-3) / PEAK, 4)}]


def runs_of(fn, runs):
    """`runs` repeated runs of a median of 10: (median of the runs, lowest run, highest run) in ms."""
    meds = sorted(median_ms(fn, reps=10, warm=2) for _ in range(runs))
    return round(meds[len(meds) // 2], 3), round(meds[0], 3), round(meds[-1], 3)


def loader_workload(rows, list_rows, runs, dev):
    import pandas as pd

    import nvtabular_amd as nvt
    from nvtabular_amd.loader.torch import TorchAsyncItr

    g = torch.Generator(device=dev)
    g.manual_seed(3)
    cats, conts = [f"C{c}" for c in range(26)], [f"I{c}" for c in range(13)]

    def scalar_frames(k):
        out = []
        for _ in range(k):
            m = rows // k
            cols = {n: DeviceColumn(torch.randint(0, 1 << 20, (m,), device=dev, generator=g)) for n in cats}
            cols.update({n: DeviceColumn(torch.randn(m, device=dev, generator=g)) for n in conts})
            cols["label"] = DeviceColumn(torch.randint(0, 2, (m,), device=dev, generator=g))
            out.append(DeviceFrame(cols))
        return out

    def list_frames(k):
        out = []
        for _ in range(k):
            m = list_rows // k
            lens = torch.randint(0, 17, (m,), device=dev, generator=g)
            offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lens, 0, out=offsets[1:])
            leaves = int(offsets[-1].item())
            out.append(DeviceFrame({"s": DeviceColumn(torch.randint(0, 1 << 20, (leaves,), device=dev, generator=g),
                                                      None, offsets),
                                    "label": DeviceColumn(torch.randint(0, 2, (m,), device=dev, generator=g))}))
        return out

    # a small dataset of the same columns gives the loader its schema; the chunks it gathers are the
    # device frames above
    tiny = {n: [1, 2] for n in cats}
    tiny.update({n: [0.5, 1.5] for n in conts})
    tiny["label"] = [0, 1]
    small = nvt.Dataset(pd.DataFrame(tiny))
    small_list = nvt.Dataset(pd.DataFrame({"s": [[1], [2, 3]], "label": [0, 1]}))
    res = []
    for ppc in (1, 4):
        for layout in ("dict", "stacked", "list"):
            if layout == "list":
                frames = list_frames(ppc)
                it = TorchAsyncItr(small_list, cats=["s"], labels=["label"], batch_size=65536, shuffle=True,
                                   parts_per_chunk=ppc)
            else:
                frames = scalar_frames(ppc)
                it = TorchAsyncItr(small, cats=cats, conts=conts, labels=["label"], batch_size=65536, shuffle=True,
                                   parts_per_chunk=ppc, stacked=layout == "stacked")
            it._layout(frames[0])
            gen = torch.Generator(device=dev)
            gen.manual_seed(5)
            med, lo, hi = runs_of(lambda: it._gather(frames, None, gen), runs)
            res.append({"workload": "loader_gather", "layout": layout, "parts_per_chunk": ppc,
                        "rows_per_chunk": sum(len(f) for f in frames), "ms": med, "ms_lowest_run": lo,
                        "ms_highest_run": hi, "runs": runs})
            if layout == "dict" and ppc > 1 and hasattr(KD, "take_frames"):
                m = sum(len(f) for f in frames)
                index = torch.randperm(m, device=dev, generator=gen)
                bufs = {n: torch.empty(m, dtype=frames[0][n].data.dtype, device=dev) for n in cats + conts}

                def by_kernel():
                    KD.take_frames(frames, index, [KD.Take(n, bufs[n]) for n in cats + conts])

                def by_cat():
                    for n in cats + conts:
                        torch.index_select(torch.cat([f[n].data for f in frames]), 0, index, out=bufs[n])

                for name, fn in (("multi_source_kernel", by_kernel), ("cat_index_select", by_cat)):
                    med, lo, hi = runs_of(fn, runs)
                    res.append({"workload": "dict_plain_columns", "path": name, "parts_per_chunk": ppc,
                                "rows_per_chunk": m, "ms": med, "ms_lowest_run": lo, "ms_highest_run": hi,
                                "runs": runs})
                del bufs, index
            del frames, it
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45_000_000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--list-rows", type=int, default=20_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loader", action="store_true", help="time TorchAsyncItr._gather instead of the kernels")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.loader:
        res = loader_workload(a.rows // a.parts, a.list_rows // a.parts, a.runs, dev)
    else:
        res = scalar_workload(a.rows // a.parts, dev)
        torch.cuda.empty_cache()
        res += list_workload(a.list_rows // a.parts, dev)
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
