"""Parquet list columns on the way in, device half: nvt_pqlist_unpack against the numpy reference
(tests/pq_levels_reference.py), then whole files through Dataset with the hand-written reader on
and off, the sharing of offsets between columns with equal level streams, and the reader under
ListSlice and the dataloader.  All comparisons are exact."""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import pq_levels_reference as R
from pq_list_files import WRITES, write_session_file, write_session_file_plain_writer

pytestmark = pytest.mark.gpu

GUARD = 64
TILE = 2048


def dev():
    return torch.device("cuda:0")


# ---- the kernel ---------------------------------------------------------------------------------
# (outer optional, leaf optional, fraction of null leaves, null lists mixed in)
CONFIGS = [(False, False, 0.0, False),    # max_def 1: definition levels at 1 bit
           (True, True, 0.0, False), (True, True, 0.3, False), (True, True, 0.3, True),
           (False, True, 0.3, False), (True, False, 0.0, True)]

CASES = {
    "one_empty": [0], "one_leaf": [1], "seven": [7], "eight": [8], "nine": [9], "mixed": [3, 0, 3],
    "nine_empty": [0] * 9,
    "63_one_row": [63], "64_one_row": [64], "65_one_row": [65],
    "63_rows": [1] * 63, "64_rows": [1] * 64, "65_rows": [1] * 65, "63_mixed": [30, 0, 32],
    "2047_one_row": [2047], "2048_one_row": [2048], "2049_one_row": [2049],
    "2047_rows": [1, 0] * 1023 + [1], "2048_rows": [1, 0] * 1024, "2049_rows": [1, 0] * 1024 + [1],
    "start_on_tile_boundary": [2048, 5, 0, 2040, 3],            # rows start at slots 2048 and 4096
    "row_over_three_tiles": [3, 5000, 2],
    "empty_tiles": [5] * 3 + [0] * 3000 + [7, 1, 2] + [0] * 2100 + [64] * 3,   # leaf base 15 behind leafless tiles
    "only_empty_rows": [0] * 100, "only_empty_rows_tiles": [0] * 4100,
    "no_rows": [],
}


def _unpack(rep, dfn, leaf_level, max_def, want_valid):
    from nvtabular_amd import kernels_parquet_list as KPL

    width = 1 if max_def == 1 else 2
    n = len(rep)
    exp_off, exp_valid = R.levels_to_offsets(rep, dfn, leaf_level, max_def)
    rows, leaves = len(exp_off) - 1, int(exp_off[-1])
    # (both streams a whole number of 64-bit words; an empty stream is still a buffer)
    d_rep = torch.from_numpy(R.pack_levels(rep, 1, max(8, -(-n // 64) * 8))).to(dev())
    d_def = torch.from_numpy(R.pack_levels(dfn, width, max(8, -(-n * width // 64) * 8))).to(dev())
    offsets, valid, (off_raw, valid_raw) = KPL.unpack_levels(d_rep, d_def, width, n, leaf_level, max_def, rows, leaves,
                                                             want_valid, guard=GUARD)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(offsets.cpu().numpy(), exp_off)
    raw = off_raw.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + (rows + 1) * 8:] == 0xA5).all()
    if want_valid:
        words = -(-leaves // 64)
        got = valid.cpu().numpy()
        assert len(got) == words * 8
        bits = np.unpackbits(got, bitorder="little")
        np.testing.assert_array_equal(bits[:leaves].astype(bool), exp_valid)
        assert not bits[leaves:].any()                       # bits past the last leaf
        raw = valid_raw.cpu().numpy()
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + words * 8:] == 0xA5).all()
    else:
        assert valid is None
    return exp_off, exp_valid


@pytest.mark.parametrize("case", sorted(CASES))
def test_unpack_equals_the_reference(case):
    lengths = CASES[case]
    rng = np.random.default_rng(len(lengths) + sum(lengths))
    for outer, elem, null_frac, null_lists in CONFIGS:
        leaf_null = rng.random(sum(lengths)) < null_frac if null_frac else None
        list_null = np.array([L == 0 and rng.random() < 0.5 for L in lengths]) if null_lists else None
        rep, dfn, leaf_level, max_def = R.levels_of_rows(lengths, leaf_null, list_null, outer, elem)
        assert len(rep) == sum(max(L, 1) for L in lengths)
        _unpack(rep, dfn, leaf_level, max_def, want_valid=True)
        if not null_frac:
            _unpack(rep, dfn, leaf_level, max_def, want_valid=False)


def test_unpack_is_deterministic_and_leaves_no_stale_bits():
    """Boundary words are merged with atomicOr into a bitmap the entry point zeroes itself: the same
    call on a dirty allocation gives the same bits."""
    rng = np.random.default_rng(5)
    lengths = list(rng.integers(0, 9, 3000))
    leaf_null = rng.random(sum(lengths)) < 0.3
    rep, dfn, leaf_level, max_def = R.levels_of_rows(lengths, leaf_null, None, True, True)
    for _ in range(2):
        torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=dev())   # (dirty what the allocator hands out next)
        _unpack(rep, dfn, leaf_level, max_def, want_valid=True)


def test_unpack_refuses_bad_arguments():
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev())
    p = buf.data_ptr()
    need = C.c_uint64()
    assert lib.nvt_pqlist_unpack_ws_bytes(100, C.byref(need)) == 0 and 0 < need.value <= 2048

    def call(width=2, n=100, leaf_level=2, max_def=3, rows=10, leaves=50, ws_bytes=2048, rep=p):
        return lib.nvt_pqlist_unpack(rep, p + 512, width, n, leaf_level, max_def, rows, leaves, p + 1024, p + 1536, p + 2048,
                                     ws_bytes, None)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(n=1 << 32), dict(width=3), dict(width=1), dict(max_def=4), dict(leaf_level=3), dict(rows=101),
               dict(leaves=101), dict(ws_bytes=8), dict(rep=p + 4), dict(rep=None)):
        assert call(**kw) == _lib.NVT_EINVAL, kw
    torch.cuda.synchronize()


# ---- whole files, both paths --------------------------------------------------------------------
def _read(path, on, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio

    monkeypatch.setattr(nio, "PLAIN_PARQUET_READ", on)
    frames = list(nvt.Dataset(path).to_iter())
    torch.cuda.synchronize()
    return frames


def _bits(valid, n):
    return np.unpackbits(valid.cpu().numpy(), bitorder="little")[:n].astype(bool)


def _assert_frames_equal(got, exp):
    """Column by column: dtype, offsets, validity present or absent and its bits, logical type, and the
    values (under a null the two readers hold whatever their buffers held: not compared)."""
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
        for name in b.columns:
            x, y = a[name], b[name]
            assert x.data.dtype == y.data.dtype and x.data.numel() == y.data.numel(), name
            assert x.logical == y.logical and x.strings is None and y.strings is None, name
            assert (x.offsets is None) == (y.offsets is None), name
            if y.offsets is not None:
                assert x.offsets.dtype == torch.int64
                np.testing.assert_array_equal(x.offsets.cpu().numpy(), y.offsets.cpu().numpy(), err_msg=name)
            assert (x.valid is None) == (y.valid is None), name
            n = y.data.numel()
            ok = np.ones(n, dtype=bool)
            if y.valid is not None:
                ok = _bits(y.valid, n)
                np.testing.assert_array_equal(_bits(x.valid, n), ok, err_msg=name)
            u = f"u{y.data.element_size()}"
            np.testing.assert_array_equal(x.data.cpu().numpy().view(u)[ok], y.data.cpu().numpy().view(u)[ok], err_msg=name)


def _groupby_file(tmp_path, monkeypatch, rows=5000):
    """Sessions written by Dataset.to_parquet from Groupby's "list" aggregates, in row groups of 400."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import ops

    rng = np.random.default_rng(23)
    df = pd.DataFrame({"user": rng.integers(0, 900, rows).astype(np.int64),
                       "item": rng.integers(0, 5000, rows).astype(np.int64),
                       "ts": rng.integers(0, 1_000_000, rows).astype(np.int64)})
    df = df.sort_values(["user", "ts"], kind="stable").reset_index(drop=True)
    feats = ["user", "item", "ts"] >> ops.Groupby(groupby_cols=["user"], sort_cols=["ts"],
                                                  aggs={"item": "list", "ts": "list"})
    wf = nvt.Workflow(feats)
    ds = nvt.Dataset(df)
    wf.fit(ds)
    out = str(tmp_path / "sessions")
    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 400)
    wf.transform(ds).to_parquet(out)
    (name,) = [f for f in os.listdir(out) if f.endswith(".parquet")]
    path = os.path.join(out, name)
    md = pq.read_metadata(path)
    assert md.created_by == "nvtabular_amd plain writer" and md.num_row_groups >= 2
    return path


@pytest.fixture
def files(tmp_path, monkeypatch):
    paths = {how: write_session_file(tmp_path, how) for how in WRITES}
    paths["plain_writer"] = write_session_file_plain_writer(str(tmp_path / "plain_writer.parquet"))
    paths["groupby"] = _groupby_file(tmp_path, monkeypatch)
    return paths


def test_files_equal_on_both_paths(files, monkeypatch):
    from nvtabular_amd import parquet_plain as PP

    for how, path in files.items():
        md = pq.read_metadata(path)
        top_level = len(pq.read_schema(path).names)
        before = dict(PP.READER_CHUNKS)
        got = _read(path, True, monkeypatch)
        # every chunk through the hand-written reader, none left to pyarrow
        assert PP.READER_CHUNKS["pyarrow"] == before["pyarrow"], how
        assert PP.READER_CHUNKS["plain"] == before["plain"] + top_level * md.num_row_groups, how
        mid = dict(PP.READER_CHUNKS)
        exp = _read(path, False, monkeypatch)
        assert PP.READER_CHUNKS["plain"] == mid["plain"] and PP.READER_CHUNKS["pyarrow"] > mid["pyarrow"], how
        assert len(got) == md.num_row_groups
        _assert_frames_equal(got, exp)
        assert any(got[0][name].offsets is not None for name in got[0].columns)


def test_equal_level_streams_share_one_unpack(tmp_path, monkeypatch):
    from nvtabular_amd import kernels as K

    path = _groupby_file(tmp_path, monkeypatch)
    before = K.STATS.get("pqlist_unpack", 0)
    frames = _read(path, True, monkeypatch)
    assert K.STATS.get("pqlist_unpack", 0) - before == len(frames)       # one per partition, two list columns
    for f in frames:
        assert f["item_list"].offsets.data_ptr() == f["ts_list"].offsets.data_ptr()
        assert f["item_list"].data.data_ptr() != f["ts_list"].data.data_ptr()
    _assert_frames_equal(frames, _read(path, False, monkeypatch))

    # one null leaf of difference: two unpacks, the same offsets values
    rng = np.random.default_rng(2)
    rows = [[int(v) for v in rng.integers(0, 9, int(rng.integers(0, 5)))] for _ in range(700)]
    other = [list(r) for r in rows]
    k = next(i for i, r in enumerate(other) if len(r) > 2)
    other[k][2] = None
    path = str(tmp_path / "differ.parquet")
    pq.write_table(pa.table({"a": pa.array(rows, type=pa.list_(pa.int64())),
                             "b": pa.array(other, type=pa.list_(pa.int64()))}), path)
    before = K.STATS.get("pqlist_unpack", 0)
    (f,) = _read(path, True, monkeypatch)
    assert K.STATS.get("pqlist_unpack", 0) - before == 2
    assert f["a"].offsets.data_ptr() != f["b"].offsets.data_ptr()
    np.testing.assert_array_equal(f["a"].offsets.cpu().numpy(), f["b"].offsets.cpu().numpy())
    assert f["a"].valid is None and f["b"].valid is not None
    _assert_frames_equal([f], _read(path, False, monkeypatch))


def test_reader_under_list_slice_and_the_dataloader(tmp_path, monkeypatch):
    """Groupby file -> Dataset(path) -> ListSlice(-3) -> TorchAsyncItr(batch_size=64): the batches of
    the same pipeline on the frame held in memory."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import ops
    from nvtabular_amd.loader.torch import TorchAsyncItr

    path = _groupby_file(tmp_path, monkeypatch)
    table = pq.read_table(path)

    def batches(ds):
        wf = nvt.Workflow((["item_list", "ts_list"] >> ops.ListSlice(-3)) + ["user"])
        wf.fit(ds)
        it = TorchAsyncItr(wf.transform(ds), cats=["user", "item_list", "ts_list"], batch_size=64)
        return [{k: v.cpu().numpy() for k, v in x.items()} for x, _ in it]

    monkeypatch.setattr(nio, "PLAIN_PARQUET_READ", True)
    got = batches(nvt.Dataset(path))
    exp = batches(nvt.Dataset(table, npartitions=1))
    assert len(got) == len(exp) == -(-table.num_rows // 64)
    for g, e in zip(got, exp):
        assert sorted(g) == sorted(e) == ["item_list__offsets", "item_list__values", "ts_list__offsets",
                                           "ts_list__values", "user"]
        for k in e:
            assert g[k].dtype == e[k].dtype
            np.testing.assert_array_equal(g[k], e[k], err_msg=k)
    assert max(np.diff(g["item_list__offsets"]).max() for g in got) == 3
