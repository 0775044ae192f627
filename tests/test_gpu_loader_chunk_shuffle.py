"""TorchAsyncItr(shuffle=True, parts_per_chunk=k): a chunk is shuffled across its partitions, in the
documented order.  3 partitions x 400 rows; ``part`` names each row's partition."""
import numpy as np
import pandas as pd
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import kernels as K
from nvtabular_amd.loader.torch import TorchAsyncItr, epoch_row_order

pytestmark = pytest.mark.gpu

PARTS, PER = 3, 400
ROWS = PARTS * PER
SEED = 20240607


def host_frame(rows=ROWS):
    i = np.arange(rows, dtype=np.int64)
    x = pd.array(i / 3.0, dtype="Float64")
    x[i % 11 == 5] = pd.NA
    return pd.DataFrame({"id": i, "part": (i // PER).astype(np.int32), "x": x, "label": i % 2,
                         "s": [[int(k)] * int(k % 4) for k in i], "t": [[int(k)] * int(k % 3) for k in i]})


@pytest.fixture(scope="module")
def frame():
    return host_frame()


def dataset(df, cuts=None):
    cuts = cuts or list(range(0, ROWS + 1, PER))
    return nvt.Dataset([df.iloc[a:b].reset_index(drop=True) for a, b in zip(cuts[:-1], cuts[1:])])


def loader(df, cuts=None, **kw):
    args = dict(cats=["id", "part", "s", "t"], conts=["x"], labels=["label"], batch_size=100, shuffle=True,
                seed_fn=lambda: SEED)
    args.update(kw)
    return TorchAsyncItr(dataset(df, cuts), **args)


def collect(it):
    out = {"n": []}
    for x, y in it:
        out["n"].append(len(y))
        for k, v in x.items():
            out.setdefault(k, []).append(v.cpu().numpy())
        out.setdefault("y", []).append(y.cpu().numpy())
    return out


def want_x(i):
    v = i / 3.0
    v[i % 11 == 5] = np.nan
    return v


def check_rows(got, ids):
    """Scalar, list and label columns of every row agree with the row's id."""
    np.testing.assert_array_equal(np.concatenate(got["part"]), (ids // PER).astype(np.int32))
    np.testing.assert_array_equal(np.concatenate(got["x"]), want_x(ids))
    np.testing.assert_array_equal(np.concatenate(got["y"]), (ids % 2).astype(np.float32))
    at = 0
    for k, n in enumerate(got["n"]):
        rows = ids[at: at + n]
        for name, mod, dt in (("s", 4, np.int64), ("t", 3, np.int64)):
            vals, offs = got[name + "__values"][k], got[name + "__offsets"][k]
            assert offs.dtype == np.int64 and len(offs) == n + 1 and offs[0] == 0
            np.testing.assert_array_equal(np.diff(offs), rows % mod)
            np.testing.assert_array_equal(vals, np.repeat(rows, rows % mod).astype(dt))
        at += n


def model_ids(cuts, parts, seed, ppc):
    """The documented order, written out independently of the package: host generator for the
    partitions, one device draw per chunk over the chunk's rows in the order it holds them."""
    host = torch.Generator()
    host.manual_seed(seed)
    order = [parts[i] for i in torch.randperm(len(parts), generator=host).tolist()]
    order = [p for p in order if cuts[p + 1] > cuts[p]]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    out = []
    for k in range(0, len(order), ppc):
        rows = np.concatenate([np.arange(cuts[p], cuts[p + 1]) for p in order[k:k + ppc]])
        out.append(rows[torch.randperm(len(rows), device="cuda", generator=gen).cpu().numpy()])
    return np.concatenate(out)


def test_first_batch_mixes_all_partitions_of_the_chunk(frame):
    x, _ = next(iter(loader(frame, parts_per_chunk=3)))
    parts = x["part"].cpu().numpy()
    assert len(parts) == 100 and set(parts.tolist()) == {0, 1, 2}


@pytest.mark.parametrize("ppc", [1, 2, 3])
@pytest.mark.parametrize("batch_size", [100, 333])
def test_epoch_is_the_documented_order(frame, ppc, batch_size):
    got = collect(loader(frame, parts_per_chunk=ppc, batch_size=batch_size))
    ids = np.concatenate(got["id"])
    cuts = list(range(0, ROWS + 1, PER))
    np.testing.assert_array_equal(ids, model_ids(cuts, [0, 1, 2], SEED, ppc))
    pairs = epoch_row_order([PER] * PARTS, [0, 1, 2], SEED, ppc, "cuda").cpu().numpy()
    np.testing.assert_array_equal(ids, pairs[:, 0] * PER + pairs[:, 1])
    np.testing.assert_array_equal(np.sort(ids), np.arange(ROWS))
    assert all(n == batch_size for n in got["n"][:-1]) and sum(got["n"]) == ROWS
    check_rows(got, ids)


def test_two_epochs_differ_and_a_seed_repeats(frame):
    it = loader(frame, parts_per_chunk=3, seed_fn=None)
    a, b = np.concatenate(collect(it)["id"]), np.concatenate(collect(it)["id"])
    for ids in (a, b):
        np.testing.assert_array_equal(np.sort(ids), np.arange(ROWS))
    assert (a != b).any()
    one, two = (np.concatenate(collect(loader(frame, parts_per_chunk=3))["id"]) for _ in range(2))
    np.testing.assert_array_equal(one, two)
    other = np.concatenate(collect(loader(frame, parts_per_chunk=3, seed_fn=lambda: SEED + 1))["id"])
    assert (one != other).any()


@pytest.mark.parametrize("ppc", [2, 3])
def test_stacked_and_dict_mode_give_the_same_rows(frame, ppc):
    d = collect(loader(frame, parts_per_chunk=ppc))
    s = collect(loader(frame, parts_per_chunk=ppc, stacked=True))
    ids = np.concatenate(d["id"])
    cats, conts = np.concatenate(s["cats"]), np.concatenate(s["conts"])
    assert cats.dtype == np.int64 and cats.shape == (ROWS, 2) and conts.dtype == np.float32 and conts.shape == (ROWS, 1)
    np.testing.assert_array_equal(cats[:, 0], ids)
    np.testing.assert_array_equal(cats[:, 1], ids // PER)
    np.testing.assert_array_equal(conts[:, 0], want_x(ids).astype(np.float32))
    np.testing.assert_array_equal(np.concatenate(s["y"]), np.concatenate(d["y"]))
    for name in ("s", "t"):
        for key in ("__values", "__offsets"):
            for p, q in zip(d[name + key], s[name + key]):
                np.testing.assert_array_equal(p, q)


@pytest.mark.parametrize("dense", [True, False])
def test_sparse_max_pads_or_truncates_like_a_host_model(frame, dense):
    got = collect(loader(frame, parts_per_chunk=3, batch_size=333, sparse_names=["s", "t"],
                         sparse_max={"s": 2, "t": 4}, sparse_as_dense=dense))
    ids = np.concatenate(got["id"])
    np.testing.assert_array_equal(np.sort(ids), np.arange(ROWS))
    at = 0
    for k, n in enumerate(got["n"]):
        rows = ids[at: at + n]
        for name, mod, width in (("s", 4, 2), ("t", 3, 4)):
            lens = np.minimum(rows % mod, width)
            if dense:
                want = np.zeros((n, width))
                for r, (i, ln) in enumerate(zip(rows, lens)):
                    want[r, :ln] = i
                assert got[name][k].shape == (n, width)
                np.testing.assert_array_equal(got[name][k], want)
            else:
                np.testing.assert_array_equal(np.diff(got[name + "__offsets"][k]), lens)
                np.testing.assert_array_equal(got[name + "__values"][k], np.repeat(rows, lens))
        at += n


@pytest.mark.parametrize("batch_size", [333, 1001])
@pytest.mark.parametrize("drop_last", [False, True])
def test_spill_and_drop_last_still_partition_the_rows(frame, batch_size, drop_last):
    it = loader(frame, parts_per_chunk=2, batch_size=batch_size, drop_last=drop_last)
    got = collect(it)
    keep = ROWS - ROWS % batch_size if drop_last else ROWS
    if keep == 0:                                   # one batch would be larger than the epoch
        assert got == {"n": []} and len(it) == 0
        return
    ids = np.concatenate(got["id"])
    assert len(got["n"]) == len(it) and all(n == batch_size for n in got["n"][:-1]) and len(ids) == keep
    assert len(np.unique(ids)) == keep
    np.testing.assert_array_equal(ids, model_ids(list(range(0, ROWS + 1, PER)), [0, 1, 2], SEED, 2)[:keep])
    check_rows(got, ids)


def test_two_ranks_share_the_partitions(frame):
    cuts = [0, 200, 400, 700, 800, 1200]
    ids = []
    for rank in (0, 1):
        got = collect(loader(frame, cuts, parts_per_chunk=2, global_size=2, global_rank=rank))
        ids.append(np.concatenate(got["id"]))
        np.testing.assert_array_equal(ids[-1], model_ids(cuts, [p for p in range(5) if p % 2 == rank], SEED, 2))
        check_rows(got, ids[-1])
    assert not set(ids[0]) & set(ids[1])
    np.testing.assert_array_equal(np.sort(np.concatenate(ids)), np.arange(ROWS))


def test_unequal_partitions_and_an_empty_one_inside_a_chunk():
    i = np.arange(700, dtype=np.int64)
    df = pd.DataFrame({"id": i, "c": (i * 7 % 13).astype(np.int32), "label": i % 2})
    cuts = [0, 1, 258, 258, 700]                  # 1, 257, 0 and 442 rows
    ds = nvt.Dataset([df.iloc[a:b].reset_index(drop=True) for a, b in zip(cuts[:-1], cuts[1:])])
    for stacked in (False, True):
        it = TorchAsyncItr(ds, cats=["id", "c"], labels=["label"], batch_size=64, shuffle=True, seed_fn=lambda: SEED,
                           parts_per_chunk=4, stacked=stacked)
        rows = [(x["cats"][:, 0], x["cats"][:, 1], y) if stacked else (x["id"], x["c"], y) for x, y in it]
        ids = torch.cat([r[0] for r in rows]).cpu().numpy()
        np.testing.assert_array_equal(ids, model_ids(cuts, [0, 1, 2, 3], SEED, 4))
        np.testing.assert_array_equal(torch.cat([r[1] for r in rows]).cpu().numpy(), ids * 7 % 13)
        np.testing.assert_array_equal(torch.cat([r[2] for r in rows]).cpu().numpy(), (ids % 2).astype(np.float32))
        assert len({int(p) for p in np.searchsorted(cuts, ids[:64], side="right")}) > 1


@pytest.mark.parametrize("ppc, batch_size, chunks", [(3, 100, 1), (2, 100, 2), (2, 333, 2), (1, 333, 3)])
def test_lists_cost_one_read_back_per_chunk(frame, ppc, batch_size, chunks):
    """``s`` alone: one group of list columns, so one read-back per chunk, spill or not."""
    it = loader(frame, cats=["id", "s"], conts=[], parts_per_chunk=ppc, batch_size=batch_size)
    before = K.STATS.get("loader_list_readback", 0)
    n = sum(len(y) for _, y in it)
    assert n == ROWS
    assert K.STATS.get("loader_list_readback", 0) - before == chunks
