"""2 ranks (one GPU, gloo): each rank fits FillMedian on its OWN 3 000-row frame; both must end
with the medians pandas computes on the union of the two frames, bit for bit."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pandas as pd
import torch
import torch.distributed as td

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
td.init_process_group("gloo", rank=rank, world_size=world)
import nvtabular_amd as nvt
from nvtabular_amd import ops


def make(r, n=3000):
    rng = np.random.default_rng(700 + r)
    df = pd.DataFrame({
        "x": rng.normal(3.0 + 5 * r, 2.0, n),                       # the ranks' rows barely overlap
        "y": rng.normal(0.0, 1e3, n).astype(np.float32),
        "k": rng.integers(-1000, 1000, n).astype(np.int64),
        "z": rng.integers(0, 3, n).astype(np.int32) * (1 - r)})      # heavy repeats, rank 1 all zero
    df.loc[rng.random(n) < 0.1, "x"] = np.nan
    df.loc[rng.random(n) < 0.1, "y"] = np.nan
    return df


cols = ["x", "y", "k", "z"]
wf = nvt.Workflow(cols >> ops.FillMedian())
wf.fit(nvt.Dataset(make(rank), npartitions=2))
op = next(n.op for n in nvt.workflow.iter_nodes(wf.output_node) if isinstance(n.op, ops.FillMedian))
union = pd.concat([make(r) for r in range(world)], ignore_index=True)
for c in cols:
    exp = float(union[c].dropna().quantile(0.5, interpolation="linear"))
    assert op.medians[c] == exp, (rank, c, float.hex(op.medians[c]), float.hex(exp))
out = wf.transform(nvt.Dataset(make(rank))).to_ddf().compute()
np.testing.assert_array_equal(out["x"].to_numpy(), make(rank)["x"].fillna(op.medians["x"]).to_numpy())
td.barrier()
print(f"rank {rank}: FillMedian medians == pandas on the union ({len(union)} rows)", flush=True)
td.destroy_process_group()
