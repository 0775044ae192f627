"""Rates of the session operators against torch compositions that produce the same tensors.

Builds 4 list columns (2 x int64, 1 x int32, 1 x float32 with a validity bitmap) that share one
offsets tensor -- 20 M rows with geometric lengths of mean 8, and the skewed frame (one row of
10 M leaves, 1 M empty rows, 1 M rows of 1-30 leaves) -- and times, with HIP events after a
warm-up, the median of ``--reps`` runs of
  list_slice        ops.ListSlice(-20)            vs  repeat_interleave / cumsum / index gather
  list_slice_pad    ops.ListSlice(-20, pad=True)  vs  arange // 20 / where / index gather
  value_count       ops.ValueCount fit            vs  torch.diff(offsets).aminmax()
  difference_lag    ops.DifferenceLag(["user"], shift=[1, -1]) on 2 columns of 45 M rows
                                                  vs  the torch expression of the same formula
asserts inside the tool that both sides are bit-equal, and prints one JSON line per case: ms of
both sides (the same number of runs), algorithmic bytes (source leaves that are taken read once,
output leaves written once -- padded leaves are written, never read --, bitmaps and offsets included), GB/s
and the fraction of 8 TB/s.  Kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/session_rate.py --reps 3``.

    python tools/session_rate.py [--rows 20000000] [--lag-rows 45000000] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
WIDTH = 20


def timed(fn, reps, warmup=2):
    import torch

    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], out


def list_frame(lens, dev, seed):
    import torch

    from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap_device

    g = torch.Generator(device=dev).manual_seed(seed)
    off = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=off[1:])
    nl = int(off[-1].item())
    ok = torch.rand(nl, device=dev, generator=g) < 0.9
    return DeviceFrame({
        "a": DeviceColumn(torch.randint(0, 1 << 40, (nl,), device=dev, generator=g), None, off),
        "b": DeviceColumn(torch.randint(0, 1 << 40, (nl,), device=dev, generator=g), None, off),
        "c": DeviceColumn(torch.randint(0, 1 << 30, (nl,), device=dev, generator=g, dtype=torch.int32), None, off),
        "d": DeviceColumn(torch.rand(nl, device=dev, generator=g), pack_bitmap_device(ok), off),
    })


def torch_slice(frame, pad):
    """The last WIDTH leaves of every row with torch ops, the way DeviceFrame.take_rows handles
    lists; pad=True extends every row to WIDTH leaves of 0 (valid)."""
    import torch

    from nvtabular_amd.device import pack_bitmap_device

    off = frame["a"].offsets
    n = off.numel() - 1
    L = off[1:] - off[:-1]
    cnt = L.clamp(max=WIDTH)
    first = off[1:] - cnt
    if pad:
        idx = torch.arange(n * WIDTH, device=off.device)
        row = idx // WIDTH
        k = idx - row * WIDTH
        take = k < cnt[row]
        src = torch.where(take, first[row] + k, torch.zeros_like(k))
        new_off = torch.arange(0, (n + 1) * WIDTH, WIDTH, device=off.device)
    else:
        new_off = torch.zeros(n + 1, dtype=torch.int64, device=off.device)
        torch.cumsum(cnt, 0, out=new_off[1:])
        total = int(new_off[-1].item())
        src = torch.repeat_interleave(first - new_off[:-1], cnt) + torch.arange(total, device=off.device)
        take = None
    out = {}
    for name, col in frame.items():
        data = col.data[src] if col.data.numel() else col.data.new_zeros(src.numel())
        if take is not None:
            data = torch.where(take, data, torch.zeros_like(data))
        valid = None
        if col.valid is not None:
            bits = ((col.valid[src >> 3] >> (src & 7).to(torch.uint8)) & 1).to(torch.bool)
            if take is not None:
                bits = bits | ~take
            valid = pack_bitmap_device(bits)
        out[name] = (data, valid, new_off)
    return out


def same_lists(got, ref):
    import torch

    for name, (data, valid, off) in ref.items():
        c = got[name]
        if not (c.offsets.equal(off) and c.data.view(torch.uint8).equal(data.view(torch.uint8))):
            return False
        if (c.valid is None) != (valid is None) or (valid is not None and not c.valid.equal(valid)):
            return False
    return True


def slice_bytes(frame, out, pad):
    """What the algorithm reads and writes: the taken source leaves (the sum of the sliced row
    lengths) are read, every output leaf is written (padded leaves are written, never read), the
    bitmaps likewise; the old offsets are read, and the ragged path writes new ones."""
    n = len(frame)
    off = frame["a"].offsets
    taken = int((off[1:] - off[:-1]).clamp(max=WIDTH).sum().item())
    total = (n + 1) * 8 * (1 if pad else 2)
    for name in frame.columns:
        m = out[name].data.numel()
        assert m == (n * WIDTH if pad else taken)
        total += (taken + m) * out[name].data.element_size()
        if out[name].valid is not None:
            total += (taken + m) // 8
    return total


def torch_lag(x, user, shift):
    import torch

    n = x.numel()
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=x.device)
    s = abs(shift)
    if s == 0 or s >= n:
        return out
    hi, lo = slice(s, None), slice(None, n - s)
    i, j = (hi, lo) if shift > 0 else (lo, hi)
    if x.dtype == torch.float32:
        d = x[i] - x[j]
    else:
        d = (x[i].to(torch.float64) - x[j].to(torch.float64)).to(torch.float32)
    out[i] = torch.where(user[i] == user[j], d, out[i])
    return out


def report(case, t_new, t_ref, nbytes, equal, **extra):
    assert equal, f"{case}: the HIP path and the torch composition differ"
    print(json.dumps({
        "case": case, **extra, "bit_equal": bool(equal), "hip_ms": round(t_new, 3), "torch_ms": round(t_ref, 3),
        "speedup": round(t_ref / t_new, 2), "algorithmic_bytes": int(nbytes),
        "hip_GBps": round(nbytes / t_new / 1e6, 1), "frac_of_8TBps": round(nbytes / (t_new * 1e-3) / PEAK, 4),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--lag-rows", type=int, default=45_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()

    import torch

    import nvtabular_amd as nvt
    from nvtabular_amd import _lib, ops
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(20261016)
    # geometric on {0, 1, ...} with mean 8: floor(log(u) / log(1 - p)), p = 1 / 9
    u = torch.rand(args.rows, device=dev, generator=g).clamp_min(1e-12)
    uniform = torch.floor(torch.log(u) / torch.log(torch.tensor(8.0 / 9.0, device=dev))).to(torch.int64)
    skewed = torch.cat([torch.tensor([10_000_000], device=dev), torch.zeros(1_000_000, dtype=torch.int64, device=dev),
                        torch.randint(1, 31, (1_000_000,), device=dev, generator=g)])
    names = nvt.ColumnSelector(["a", "b", "c", "d"])
    for label, lens in (("uniform", uniform), ("skewed", skewed)):
        frame = list_frame(lens, dev, 7)
        n, nl = len(frame), int(frame["a"].data.numel())
        for pad in (False, True):
            op = ops.ListSlice(-WIDTH, pad=pad)
            t_new, out = timed(lambda: op.transform(names, frame), args.reps)
            t_ref, ref = timed(lambda: torch_slice(frame, pad), args.reps)
            report("list_slice_pad" if pad else "list_slice", t_new, t_ref, slice_bytes(frame, out, pad),
                   same_lists(out, ref), frame=label, rows=n, leaves=nl, out_leaves=int(out["a"].data.numel()))
            del out, ref
        vc = ops.ValueCount()

        def fit():
            st = vc.fit_begin(names)
            vc.fit_partition(st, names, frame)
            return vc.fit_end(st, names)

        def torch_fit():
            mn, mx = torch.diff(frame["a"].offsets).aminmax()
            return int(mn.item()), int(mx.item())

        t_new, stats = timed(fit, args.reps)
        t_ref, (mn, mx) = timed(torch_fit, args.reps)
        equal = all(stats[c]["value_count"] == {"min": mn, "max": mx} for c in names.names)
        report("value_count", t_new, t_ref, (n + 1) * 8, equal, frame=label, rows=n, min=mn, max=mx)
        del frame
        torch.cuda.empty_cache()

    n = args.lag_rows
    user = torch.cumsum((torch.rand(n, device=dev, generator=g) < 0.125).to(torch.int64), 0)
    ts = torch.cumsum(torch.randint(0, 1000, (n,), device=dev, generator=g), 0) + (1 << 58)
    v = torch.rand(n, device=dev, generator=g)
    frame = DeviceFrame({"user": DeviceColumn(user), "ts": DeviceColumn(ts), "v": DeviceColumn(v)})
    op = ops.DifferenceLag(["user"], shift=[1, -1])
    sel = nvt.ColumnSelector(["ts", "v"])
    t_new, out = timed(lambda: op.transform(sel, frame), args.reps)
    t_ref, ref = timed(lambda: {f"{c}_difference_lag_{s}": torch_lag(frame[c].data, user, s)
                                for c in ("ts", "v") for s in (1, -1)}, args.reps)
    equal = True
    for name, r in ref.items():
        got = out[name].data
        nan = torch.isnan(r)
        equal &= bool(torch.isnan(got).equal(nan)) and bool(got[~nan].view(torch.int32).equal(r[~nan].view(torch.int32)))
    report("difference_lag", t_new, t_ref, n * (8 + 8 + 4 + 4 * 4), equal, rows=n, outputs=4)


if __name__ == "__main__":
    main()
