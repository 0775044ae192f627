"""TorchAsyncItr end to end on a 1000-row frame in partitions of 333 / 400 / 267."""
import numpy as np
import pandas as pd
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd.loader.torch import DLDataLoader, TorchAsyncItr

pytestmark = pytest.mark.gpu

ROWS = 1000
CUTS = [0, 333, 733, 1000]


def host_frame():
    i = np.arange(ROWS, dtype=np.int64)
    x = pd.array(i / 3.0, dtype="Float64")
    x[i % 11 == 5] = pd.NA
    return pd.DataFrame({"id": i, "c1": (i * 7 % 13).astype(np.int32), "x": x, "label": i % 2, "label2": i % 3,
                         "s": [[int(k)] * int(k % 4) for k in i]})


@pytest.fixture(scope="module")
def frame():
    return host_frame()


def dataset(df):
    return nvt.Dataset([df.iloc[a:b].reset_index(drop=True) for a, b in zip(CUTS[:-1], CUTS[1:])])


def loader(df, **kw):
    args = dict(cats=["id", "c1", "s"], conts=["x"], labels=["label"], batch_size=64)
    args.update(kw)
    return TorchAsyncItr(dataset(df), **args)


def want_x(i):
    v = i / 3.0
    v[i % 11 == 5] = np.nan
    return v


def collect(it):
    out = {"n": []}
    for x, y in it:
        out["n"].append(len(x["id"]))
        for k, v in x.items():
            out.setdefault(k, []).append(v.cpu().numpy())
        out.setdefault("y", []).append(None if y is None else y.cpu().numpy())
    return out


def check_rows(got, ids):
    """Every column agrees with the ids of its rows."""
    np.testing.assert_array_equal(np.concatenate(got["c1"]), (ids * 7 % 13).astype(np.int32))
    np.testing.assert_array_equal(np.concatenate(got["x"]), want_x(ids))
    np.testing.assert_array_equal(np.concatenate(got["y"]), (ids % 2).astype(np.float32))
    at = 0
    for vals, offs, n in zip(got["s__values"], got["s__offsets"], got["n"]):
        assert offs.dtype == np.int64 and len(offs) == n + 1 and offs[0] == 0
        rows = ids[at: at + n]
        np.testing.assert_array_equal(np.diff(offs), rows % 4)
        np.testing.assert_array_equal(vals, np.repeat(rows, rows % 4))
        at += n


@pytest.mark.parametrize("batch_size", [64, 333, 334, 1000, 1001])
@pytest.mark.parametrize("parts_per_chunk", [1, 2, 3])
def test_unshuffled_epoch_is_the_frame(frame, batch_size, parts_per_chunk):
    it = loader(frame, batch_size=batch_size, parts_per_chunk=parts_per_chunk)
    got = collect(it)
    assert len(it) == len(got["n"]) == -(-ROWS // batch_size)
    assert all(n == batch_size for n in got["n"][:-1]) and sum(got["n"]) == ROWS
    ids = np.concatenate(got["id"])
    np.testing.assert_array_equal(ids, np.arange(ROWS))
    assert got["id"][0].dtype == np.int64 and got["c1"][0].dtype == np.int32 and got["x"][0].dtype == np.float64
    assert got["y"][0].dtype == np.float32 and got["y"][0].ndim == 1
    check_rows(got, ids)


@pytest.mark.parametrize("batch_size", [10, 9, 8])
@pytest.mark.parametrize("drop_last", [True, False])
def test_drop_last_and_reset(frame, batch_size, drop_last):
    df = frame.iloc[:100]
    it = TorchAsyncItr(nvt.Dataset(df, npartitions=1), cats=["id"], labels=["label"], batch_size=batch_size,
                       drop_last=drop_last)
    want = 100 // batch_size if drop_last else -(-100 // batch_size)
    for _ in range(2):           # a second epoch starts over
        sizes = [len(x["id"]) for x, _ in it]
        assert len(sizes) == want == len(it)
        assert all(s == batch_size for s in sizes[:-1])
        if drop_last:
            assert sizes[-1] == batch_size


def test_shuffling(frame):
    it = loader(frame, shuffle=True, batch_size=100)
    a, b = collect(it), collect(it)
    ids_a, ids_b = np.concatenate(a["id"]), np.concatenate(b["id"])
    np.testing.assert_array_equal(np.sort(ids_a), np.arange(ROWS))
    np.testing.assert_array_equal(np.sort(ids_b), np.arange(ROWS))
    check_rows(a, ids_a)
    assert (np.diff(a["id"][0]) != 1).any()          # the first batch is not in order
    assert (ids_a != ids_b).any()                    # two epochs differ
    assert all(n == 100 for n in a["n"])
    one, two = (collect(loader(frame, shuffle=True, batch_size=100, seed_fn=lambda: 1234)) for _ in range(2))
    for p, q in zip(one["id"], two["id"]):
        np.testing.assert_array_equal(p, q)
    assert (np.concatenate(one["id"]) != ids_a).any() or (np.concatenate(one["id"]) != ids_b).any()


def test_keys_and_schema_roles(frame):
    """test_mh_support / test_dataloader_schema: the keys of a batch, roles from the schema's tags."""
    it = loader(frame, cats=["id", "s"], conts=["x"], labels=["label"])
    x, y = next(iter(it))
    assert sorted(x) == ["id", "s__offsets", "s__values", "x"] and y.shape == (64,)
    tagged = TorchAsyncItr(it.dataset, batch_size=64)      # the dataset's schema now carries the roles
    assert (tagged.cat_names, tagged.cont_names, tagged.label_names) == (["id", "s"], ["x"], ["label"])
    x2, y2 = next(iter(tagged))
    assert sorted(x2) == sorted(x) and torch.equal(y2, y)
    n = sum(1 for _ in DLDataLoader(it, batch_size=None, collate_fn=lambda b: b))
    assert n == len(it)


def test_two_ranks_share_the_partitions(frame):
    ids = [np.concatenate(collect(loader(frame, global_size=2, global_rank=r))["id"]) for r in (0, 1)]
    assert not set(ids[0]) & set(ids[1])
    np.testing.assert_array_equal(np.sort(np.concatenate(ids)), np.arange(ROWS))
    assert len(ids[0]) == 333 + 267 and len(ids[1]) == 400


@pytest.mark.parametrize("shuffle", [False, True])
def test_stacked(frame, shuffle):
    it = loader(frame, cats=["c1", "id", "s"], conts=["x", "label2"], labels=["label"],
                stacked=True, shuffle=shuffle, batch_size=300)
    n = 0
    for x, y in it:
        B = x["cats"].shape[0]
        assert x["cats"].dtype == torch.int64 and x["cats"].shape == (B, 2) and x["cats"].is_contiguous()
        assert x["conts"].dtype == torch.float32 and x["conts"].shape == (B, 2)
        assert y.dtype == torch.float32 and y.shape == (B,)
        ids = x["cats"][:, 1].cpu().numpy()
        np.testing.assert_array_equal(x["cats"][:, 0].cpu().numpy(), ids * 7 % 13)
        np.testing.assert_array_equal(x["conts"][:, 0].cpu().numpy(), want_x(ids).astype(np.float32))
        np.testing.assert_array_equal(x["conts"][:, 1].cpu().numpy(), (ids % 3).astype(np.float32))
        np.testing.assert_array_equal(y.cpu().numpy(), (ids % 2).astype(np.float32))
        np.testing.assert_array_equal(np.diff(x["s__offsets"].cpu().numpy()), ids % 4)
        n += B
    assert n == ROWS
    x, y = next(iter(loader(frame, cats=["id"], conts=[], labels=["label", "label2"], stacked=True)))
    ids = x["cats"][:, 0].cpu().numpy()
    assert y.shape == (64, 2) and "conts" not in x
    np.testing.assert_array_equal(y.cpu().numpy(), np.stack([ids % 2, ids % 3], axis=1).astype(np.float32))


def test_sparse_as_dense_and_truncation(frame):
    it = loader(frame, sparse_names=["s"], sparse_max={"s": 2}, sparse_as_dense=True, batch_size=300)
    for x, _ in it:
        ids = x["id"].cpu().numpy()
        want = np.zeros((len(ids), 2), np.int64)
        for r, k in enumerate(ids):
            want[r, : min(k % 4, 2)] = k
        assert x["s"].shape == (len(ids), 2)
        np.testing.assert_array_equal(x["s"].cpu().numpy(), want)
    for x, _ in loader(frame, sparse_names=["s"], sparse_max={"s": 2}, batch_size=300):
        ids = x["id"].cpu().numpy()
        np.testing.assert_array_equal(np.diff(x["s__offsets"].cpu().numpy()), np.minimum(ids % 4, 2))
        np.testing.assert_array_equal(x["s__values"].cpu().numpy(), np.repeat(ids, np.minimum(ids % 4, 2)))


def test_a_kept_batch_survives_the_epoch(frame):
    it = iter(loader(frame, shuffle=True, batch_size=100, stacked=True))
    x0, y0 = next(it)
    snap = {k: v.clone() for k, v in x0.items()}
    ysnap = y0.clone()
    for _ in it:
        pass
    junk = [torch.zeros(1 << 20, device="cuda") for _ in range(4)]     # the allocator hands blocks out again
    torch.cuda.synchronize()
    def same(a, b):          # bit-equal: the continuous matrix holds NaN
        return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))

    assert all(same(x0[k], snap[k]) for k in snap) and same(y0, ysnap)
    del junk


def test_string_column_raises(frame):
    df = frame.iloc[:50].copy()
    df["name"] = ["n%d" % (k % 5) for k in range(50)]
    it = TorchAsyncItr(nvt.Dataset(df), cats=["name"], labels=["label"], batch_size=10)
    with pytest.raises(TypeError, match="Categorify"):
        next(iter(it))
