"""Times the fused embedding layers against the torch route the reference runs (torch.nn.Embedding +
torch.cat, torch.nn.EmbeddingBag; dense and sparse=True) and prints the figures of
profiles/embedding_notes.md.  Not a test and not bench.py: run it by hand on the GPU.

Shapes: B = 65 536; the 26 Criteo cardinalities of bench.py with _emb_sz_rule dims, ids drawn from a
bounded power law; and one multi-hot column (1 M ids, 0..8 values per row, as bench.py's cfg5).
Cardinalities are capped at --max-rows (default 2^20) so that the 512-wide tables, their dense
gradients and the torch twin fit on one device together.  Method: both routes in one process,
alternating, every shape warmed, device events around windows of at least --window seconds, --pairs
repeats; the spread of the repeats is printed with the medians.  ``--profile``: a few steps of each
fused path and nothing else, for a separate ``rocprofv3 --kernel-trace --stats`` run."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import CRITEO_CARDS  # noqa: E402
from nvtabular_amd.framework_utils.torch.layers import ConcatenatedEmbeddings, MultiHotEmbeddings  # noqa: E402
from nvtabular_amd.ops.categorify import _emb_sz_rule  # noqa: E402

DEV = "cuda"


def power_law(n, card, s, gen):
    u = torch.rand(n, device=DEV, dtype=torch.float64, generator=gen)
    x = (((card ** (1.0 - s) - 1.0) * u + 1.0) ** (1.0 / (1.0 - s))).floor().clamp_(1, card)
    return (x.to(torch.int64) * 2654435761) % card


class TorchCat(torch.nn.Module):
    def __init__(self, shapes, sparse):
        super().__init__()
        self.embedding_layers = torch.nn.ModuleList(torch.nn.Embedding(r, d, sparse=sparse) for r, d in shapes.values())

    def forward(self, x):
        return torch.cat([layer(x[:, i]) for i, layer in enumerate(self.embedding_layers)], 1)


class TorchBag(torch.nn.Module):
    def __init__(self, shapes, sparse):
        super().__init__()
        (r, d), = shapes.values()
        self.embedding_layers = torch.nn.ModuleList([torch.nn.EmbeddingBag(r, d, mode="sum", sparse=sparse)])

    def forward(self, x):
        values, offsets = x
        return self.embedding_layers[0](values, offsets[:-1])


def window(step, seconds):
    """ms per step over a window of at least `seconds`, by device events."""
    step()
    torch.cuda.synchronize()
    n, start, end = 4, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        start.record()
        for _ in range(n):
            step()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        if ms >= seconds * 1000:
            return ms / n
        n = max(n * 2, int(n * seconds * 1200 / max(ms, 1e-3)))


def compare(name, routes, x, grad, args, traffic):
    def fwd(m):
        with torch.no_grad():
            m(x)

    def fwd_bwd(m):
        for p in m.parameters():
            p.grad = None
        m(x).backward(grad)

    out = {}
    for what, fn in (("forward", fwd), ("forward_backward", fwd_bwd)):
        times = {k: [] for k in routes}
        for _ in range(args.pairs):          # alternate the routes inside every repeat
            for k, m in routes.items():
                times[k].append(window(lambda: fn(m), args.window))
        out[what] = {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
    print(json.dumps({"case": name, "bytes_from_shapes": traffic, **out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--max-rows", type=int, default=1 << 20)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(1)
    B = args.batch
    shapes = {f"C{j + 1}": (min(c, args.max_rows), _emb_sz_rule(c)[1]) for j, c in enumerate(CRITEO_CARDS)}
    D = sum(d for _, d in shapes.values())
    x = torch.stack([power_law(B, r, 1.05 + 0.05 * (j % 4), gen) for j, (r, _) in enumerate(shapes.values())], 1)
    grad = torch.randn(B, D, device=DEV, generator=gen)
    mh_shapes = {"tags": (1_000_000, 512)}
    lens = torch.randint(0, 9, (B,), device=DEV, generator=gen)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), lens.cumsum(0)])
    values = power_law(int(offsets[-1]), 1_000_000, 1.15, gen)
    mh_grad = torch.randn(B, 512, device=DEV, generator=gen)
    W = 4 * B * D   # output bytes; the single-hot gather reads as many table bytes
    torch.set_default_device(DEV)   # (the tables are initialised on the device)
    single = {"fused_dense": ConcatenatedEmbeddings(shapes),
              "fused_sparse": ConcatenatedEmbeddings(shapes, sparse_columns=list(shapes))}
    bag = {"fused_dense": MultiHotEmbeddings(mh_shapes)}
    mh_x = {"tags__values": values, "tags__offsets": offsets}
    if args.profile:
        for m, inp, g in ((single["fused_dense"], x, grad), (single["fused_sparse"], x, grad), (bag["fused_dense"], mh_x, mh_grad)):
            for _ in range(3):
                m(inp).backward(g)
        torch.cuda.synchronize()
        return
    single.update(torch_dense=TorchCat(shapes, False).to(DEV), torch_sparse=TorchCat(shapes, True).to(DEV))
    compare("criteo26_single_hot", single, x, grad, args,
            {"D": D, "ids": 8 * B * len(shapes), "fused_forward": 2 * W, "torch_forward": 4 * W,
             "dense_grad_fill": 4 * sum(r * d for r, d in shapes.values())})
    mh_routes = {"fused_dense": (bag["fused_dense"], mh_x), "torch_dense": (TorchBag(mh_shapes, False).to(DEV), (values, offsets)),
                 "torch_sparse": (TorchBag(mh_shapes, True).to(DEV), (values, offsets))}

    class Bound(torch.nn.Module):   # (every route of `compare` takes the same x)
        def __init__(self, m, inp):
            super().__init__()
            self.m, self.inp = m, inp

        def forward(self, _):
            return self.m(self.inp)

    compare("cfg5_multi_hot", {k: Bound(m, inp) for k, (m, inp) in mh_routes.items()}, None, mh_grad, args,
            {"values": int(values.numel()), "table_reads": 4 * 512 * int(values.numel()), "output": 4 * B * 512})


if __name__ == "__main__":
    main()
