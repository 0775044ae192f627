"""The cross-rank fold of a column profile (ops/_profile.merge_ranks: what ReduceDtypeSize.fit_end
and DataStats.fit_end reduce), with world_size = 2 over gloo on CPU tensors: counts and sums add,
extrema fold by MIN / MAX as int64 keys -- integer extrema exact beyond 2**53, a rank that saw no
valid row contributes nothing."""
import os
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IS_FLOAT = [False, False, False, True, True, True]


def _acc(rank):
    f = lambda *v: np.array(v, dtype=np.float64).view(np.int64).tolist()   # noqa: E731
    i64max, i64min = 2**63 - 1, -(2**63)
    rows = [
        # rows, valid, min, max, sum, sumsq
        [[10, 9, -(2**53) - 1, 5, *f(1.5, 2.5)], [7, 7, -3, 2**53 + 1, *f(0.25, 4.0)]],
        [[4, 0, i64max, i64min, *f(0.0, 0.0)], [6, 6, 2**62 + 1, 2**63 - 1, *f(8.0, 64.0)]],      # rank 0 saw nothing
        [[3, 0, i64max, i64min, *f(0.0, 0.0)], [2, 0, i64max, i64min, *f(0.0, 0.0)]],              # nobody did
        [[5, 5, *f(-0.0, 1.0), *f(1.0, 1.0)], [5, 5, *f(0.0, np.inf), *f(2.0, 3.0)]],              # zeros, +inf as a value
        [[5, 0, *f(np.nan, np.nan), *f(0.0, 0.0)], [5, 2, *f(-np.inf, -5e-324), *f(-1.0, 1.0)]],    # rank 0 saw nothing
        [[1, 0, *f(np.nan, np.nan), *f(0.0, 0.0)], [1, 0, *f(np.nan, np.nan), *f(0.0, 0.0)]],
    ]
    return torch.tensor([r[rank] for r in rows], dtype=torch.int64)


def _fit_acc(rank):
    f = lambda *v: np.array(v, dtype=np.float64).view(np.int64).tolist()   # noqa: E731
    return torch.tensor([[8 + rank, 6, -(2**53) - 1 - rank, 2**53 + 1 + rank, *f(2.0, 8.0)],
                         [8 + rank, 5, *f(-0.0, 1.5 + rank), *f(0.5, 0.75)],
                         [8 + rank, 8, 0, 200 + rank, *f(16.0, 64.0)]], dtype=torch.int64)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as td

    td.init_process_group("gloo", rank=rank, world_size=world)
    from nvtabular_amd.ops import _profile as P

    out = P.merge_ranks(_acc(rank), IS_FLOAT)
    q.put((rank, out.numpy()))
    # through ProfileFit: the LAST rank received no partition -- it has seen no column and holds no
    # accumulator, and must still join the same reductions
    names = ["a", "skipped", "b", "c"]
    fit = P.ProfileFit(names, device=torch.device("cpu"))
    if rank != world - 1:
        fit.dtypes.update(a=torch.int64, b=torch.float32, c=torch.uint8)   # what _begin takes from a partition
        fit._allocate()
        fit.acc.copy_(_fit_acc(rank))
    live, dts, acc = fit.reduced()
    q.put((rank, live, [str(d) for d in dts], acc.numpy()))
    td.barrier()
    td.destroy_process_group()


def test_profile_merge_ranks_world2_gloo():
    from nvtabular_amd import kernels as K

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    items = [q.get(timeout=150) for _ in range(2 * len(procs))]
    got = dict(t for t in items if len(t) == 2)
    fits = sorted(t for t in items if len(t) == 4)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    np.testing.assert_array_equal(got[0], got[1])                      # every rank holds the same fold
    dts = [torch.int64] * 3 + [torch.float64] * 3
    r = K.profile_rows(got[0], dts)
    assert r[0] == dict(rows=17, valid=16, min=-(2**53) - 1, max=2**53 + 1, sum=1.75, sumsq=6.5)
    assert r[1] == dict(rows=10, valid=6, min=2**62 + 1, max=2**63 - 1, sum=8.0, sumsq=64.0)
    assert r[2] == dict(rows=5, valid=0, min=None, max=None, sum=0.0, sumsq=0.0)
    assert got[0][2, 2:4].tolist() == [2**63 - 1, -(2**63)]            # the empty markers survive
    assert (r[3]["rows"], r[3]["valid"], r[3]["max"], r[3]["sum"]) == (10, 10, np.inf, 3.0)
    assert r[3]["min"] == 0 and np.signbit(r[3]["min"])                # -0.0 orders below +0.0
    assert (r[4]["valid"], r[4]["min"], r[4]["max"]) == (2, -np.inf, -5e-324)
    assert r[5]["min"] is None and np.isnan(got[0][5, 2:4].view(np.float64)).all()
    # ProfileFit.reduced: rank 1 had no partition; both ranks end with rank 0's profile
    for rank, live, dts, acc in fits:
        assert live == ["a", "b", "c"] and dts == ["torch.int64", "torch.float32", "torch.int64"], (rank, live, dts)
        np.testing.assert_array_equal(acc, _fit_acc(0).numpy(), err_msg=f"rank {rank}")
    assert [t[0] for t in fits] == [0, 1]
