"""Rates of the column-profile and narrowing-cast kernels against what the engine had before them.

One frame of 13 float32 columns x 2**24 rows with 10 % nulls, resident in HBM, and, with HIP events
after a warm-up, ``--reps`` runs of each side, the two sides of a comparison ALTERNATING in the same
process:
  profile          K.col_profile_many (rows, valid rows, min, max, sum, sum of squares: one read)
               vs  K.moments_many + per-column K.minmax_accumulate + per-column nvt_popcount
                   (the same numbers from three passes; the popcount is enqueued without its
                   read-back, which would add a host synchronisation per column)
  cast_i64_i16     K.cast_many int64 -> int16     vs  tensor.to(torch.int16)
  cast_f64_f32     K.cast_many float64 -> float32 vs  tensor.to(torch.float32)
asserts inside the tool that both sides agree (counts and extrema exactly, the sums bit for bit
with moments_many, the casts bit for bit), and prints one JSON line per case: median, minimum and
maximum ms of both sides, the ratio of the medians, algorithmic bytes (every column and bitmap read
once, every output written once), GB/s and the fraction of 8 TB/s.

    python tools/profile_rate.py [--rows 16777216] [--cols 13] [--reps 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def alternate(fa, fb, reps, warmup=3):
    """ms of ``reps`` runs of each of two functions, run in turns (a b a b ...)."""
    import torch

    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, sink in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            sink.append(a.elapsed_time(b))
    return sorted(ta), sorted(tb)


def report(case, new, old, nbytes, **extra):
    med = lambda t: t[len(t) // 2]   # noqa: E731
    line = dict(case=case, ms=round(med(new), 4), ms_min=round(new[0], 4), ms_max=round(new[-1], 4),
                baseline_ms=round(med(old), 4), baseline_ms_min=round(old[0], 4), baseline_ms_max=round(old[-1], 4),
                baseline_over_new=round(med(old) / med(new), 3), bytes=nbytes,
                gbps=round(nbytes / med(new) / 1e6, 1), frac_of_8tbps=round(nbytes / (med(new) * 1e-3) / PEAK, 4),
                baseline_gbps=round(nbytes / med(old) / 1e6, 1), reps=len(new), **extra)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--cols", type=int, default=13)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()

    import torch

    from nvtabular_amd import _lib
    from nvtabular_amd import kernels as K
    from nvtabular_amd.device import pack_bitmap_device

    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(1)
    n, k = args.rows, args.cols
    cols = []
    for _ in range(k):
        x = torch.randn(n, device=dev, generator=g) * 50
        cols.append((x, pack_bitmap_device(torch.rand(n, device=dev, generator=g) < 0.9)))

    # ---- profile ------------------------------------------------------------------------------
    acc = K.new_profile_acc([torch.float32] * k, dev)
    mom = torch.zeros(k, 3, dtype=torch.float64, device=dev)
    mm = torch.full((k, 2), float("nan"), dtype=torch.float64, device=dev)
    pc = torch.zeros(k, dtype=torch.int64, device=dev)
    lib = _lib.load()

    def fused():
        K.col_profile_many([(x, v, acc[i]) for i, (x, v) in enumerate(cols)])

    def three_passes():
        K.moments_many([(x, v, None, mom[i]) for i, (x, v) in enumerate(cols)])
        for i, (x, v) in enumerate(cols):
            K.minmax_accumulate(x, v, mm[i], first=False)
            _lib.check(lib.nvt_popcount(v.data_ptr(), n, pc[i:].data_ptr(), K.stream_ptr()), "nvt_popcount")

    fused()
    three_passes()
    rows = K.profile_rows(acc.cpu().numpy(), [torch.float32] * k)
    hm, hmm, hpc = mom.cpu().tolist(), mm.cpu().tolist(), pc.cpu().tolist()
    for r, m3, m2, p in zip(rows, hm, hmm, hpc):
        assert r["rows"] == n and r["valid"] == int(m3[0]) == p, (r, m3, p)     # (no NaN in the data)
        assert (r["min"], r["max"]) == (m2[0], m2[1]), (r, m2)
        assert (r["sum"], r["sumsq"]) == (m3[1], m3[2]), (r, m3)                   # bit for bit
    new, old = alternate(fused, three_passes, args.reps)
    report("profile", new, old, k * (n * 4 + n // 8), rows=n, cols=k, dtype="float32",
           baseline="moments_many + minmax_accumulate x cols + popcount x cols")

    # ---- casts --------------------------------------------------------------------------------
    del cols
    for case, src, dst, make in (
            ("cast_i64_i16", torch.int64, torch.int16,
             lambda: torch.randint(-40000, 40000, (n,), device=dev, generator=g, dtype=torch.int64)),
            ("cast_f64_f32", torch.float64, torch.float32,
             lambda: torch.randn(n, device=dev, generator=g, dtype=torch.float64) * 1e3)):
        xs = [make() for _ in range(k)]
        outs = [torch.empty(n, dtype=dst, device=dev) for _ in range(k)]
        keep = {}

        def ours():
            K.cast_many([(x, dst, o) for x, o in zip(xs, outs)])

        def torch_to():
            keep["t"] = [x.to(dst) for x in xs]

        ours()
        torch_to()
        for o, t in zip(outs, keep["t"]):
            assert torch.equal(o.view(torch.uint8), t.view(torch.uint8)), case
        new, old = alternate(ours, torch_to, args.reps)
        width = torch.empty(0, dtype=src).element_size() + torch.empty(0, dtype=dst).element_size()
        report(case, new, old, k * n * width, rows=n, cols=k, baseline="tensor.to(dtype) per column")
        del xs, outs, keep


if __name__ == "__main__":
    main()
