"""Dataset.to_parquet(use_dictionary=...) end to end on the device: dictionary pages of the PLAIN
writer read back with pyarrow and with this package, the chunk rule, the counters and the files'
sizes."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from test_gpu_parquet_list import _assert_same, _bitmap, _columns, _offsets

pytestmark = pytest.mark.gpu

PLAIN = "nvtabular_amd plain writer"
OFFERED = ["id", "i32", "i64", "when", "la", "lb"]


def dev():
    return torch.device("cuda:0")


def t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _frame(rows=5000, seed=3):
    """int32, int64 with nulls, a datetime, float32 and two list columns that share their offsets (one
    with null leaves); "id" orders the rows (its chunks have as many distinct values as rows: PLAIN)."""
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, rows)
    lens[0] = lens[-1] = 0
    lens[rows // 2] = 300
    off = _offsets(lens)
    leaves = int(off[-1])
    d_off = t(off)
    when = (rng.integers(0, 50, rows) * 86_400_000 + 1_600_000_000_000).astype(np.int64)
    return DeviceFrame({
        "id": DeviceColumn(t(rng.permutation(rows).astype(np.int64))),
        "i32": DeviceColumn(t(rng.integers(-20, 20, rows).astype(np.int32))),
        "i64": DeviceColumn(t(rng.choice(np.array([-2**63, -1, 0, 2**63 - 1, 77], dtype=np.int64), rows)),
                            _bitmap(rng.random(rows) >= 0.2)),
        "when": DeviceColumn(t(when), logical=np.dtype("datetime64[ms]")),
        "x": DeviceColumn(t((rng.integers(0, 4, rows) / 4).astype(np.float32))),
        "la": DeviceColumn(t(rng.integers(0, 300, leaves).astype(np.int64)), _bitmap(rng.random(leaves) >= 0.1), d_off),
        "lb": DeviceColumn(t(rng.integers(-5, 5, leaves).astype(np.int32)), None, d_off),
    })


def _parts(out):
    files = [f for f in os.listdir(out) if f.endswith(".parquet")]
    return [os.path.join(out, f) for f in sorted(files, key=lambda f: int(f.split("_")[1].split(".")[0]))]


def _chunks(path):
    """[(top-level column name, row group, ColumnChunkMetaData)]"""
    md = pq.read_metadata(path)
    return [(md.schema.column(j).path.split(".")[0], g, md.row_group(g).column(j))
            for g in range(md.num_row_groups) for j in range(md.num_columns)]


def _stats():
    from nvtabular_amd import kernels as K

    return {k: K.STATS.get(k, 0) for k in ("pqdict_build", "pqdict_pack", "pqdict_readback")}


def test_round_trip_and_encodings(tmp_path, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(PP, "PAGE_VALUES", 512)           # several pages per chunk
    frame = _frame()
    exp = _columns(frame.to_arrow())
    out = str(tmp_path / "out")
    before = _stats()
    nvt.Dataset(frame).to_parquet(out, use_dictionary=True)
    after = _stats()
    path, = _parts(out)
    assert pq.read_metadata(path).created_by == PLAIN
    for name, g, cm in _chunks(path):
        if name in ("i32", "i64", "when", "la", "lb"):
            assert "RLE_DICTIONARY" in cm.encodings and cm.has_dictionary_page, name
            assert cm.dictionary_page_offset < cm.data_page_offset
        else:                                            # the float column; "id": 5000 distinct values of 5000
            assert "RLE_DICTIONARY" not in cm.encodings and not cm.has_dictionary_page, name
    # every int column was offered ("id" too), in one read-back for the one row group
    assert {k: after[k] - before[k] for k in after} == dict(pqdict_build=6, pqdict_pack=6, pqdict_readback=1)
    table = pq.read_table(path)
    assert table.schema.field("when").type == pa.timestamp("ms")
    assert table.schema.field("i32").type == pa.int32() and table.schema.field("x").type == pa.float32()
    _assert_same(_columns(table), exp)
    reader = dict(PP.READER_CHUNKS)
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(out).to_iter()])
    assert PP.READER_CHUNKS["pyarrow"] == reader["pyarrow"] and PP.READER_CHUNKS["plain"] > reader["plain"]
    assert back.schema.field("when").type == pa.timestamp("ms")
    _assert_same(_columns(back), exp)


def test_a_list_of_names_offers_only_those(tmp_path):
    import nvtabular_amd as nvt

    frame = _frame(rows=1200)
    out = str(tmp_path / "out")
    nvt.Dataset(frame).to_parquet(out, use_dictionary=["i32", "lb"])
    path, = _parts(out)
    for name, g, cm in _chunks(path):
        assert ("RLE_DICTIONARY" in cm.encodings) == (name in ("i32", "lb")), name
    _assert_same(_columns(pq.read_table(path)), _columns(frame.to_arrow()))


@pytest.mark.parametrize("names", [["nope"], ["i32", "x"], "i32"])
def test_bad_names_raise_before_any_file(tmp_path, names):
    import nvtabular_amd as nvt

    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="use_dictionary"):
        nvt.Dataset(_frame(rows=100)).to_parquet(out, use_dictionary=names)
    assert not os.path.exists(out) or not [f for f in os.listdir(out) if f.startswith("part_")]


def test_as_many_distinct_values_as_rows_stay_plain(tmp_path):
    """4096 distinct int64 values in 4096 rows: the dictionary alone is the plain size."""
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(1)
    frame = DeviceFrame({"a": DeviceColumn(t(rng.permutation(4096).astype(np.int64) * 3)),
                         "b": DeviceColumn(t((np.arange(4096) % 3).astype(np.int64)))})
    out = str(tmp_path / "out")
    before = _stats()
    nvt.Dataset(frame).to_parquet(out, use_dictionary=True)
    assert _stats()["pqdict_build"] - before["pqdict_build"] == 2
    (_, _, ca), (_, _, cb) = _chunks(_parts(out)[0])
    assert ca.encodings == ("PLAIN", "RLE") and not ca.has_dictionary_page
    assert "RLE_DICTIONARY" in cb.encodings
    _assert_same(_columns(pq.read_table(_parts(out)[0])), _columns(frame.to_arrow()))


def test_size(tmp_path):
    """10 000 rows of int64 over 100 distinct values, no nulls: plain >= 80 000 bytes of values; with
    the option 800 bytes of dictionary + 8 750 bytes of 7-bit indices + headers < 10 000 bytes.  The
    bound comes from the layout: the file must be smaller than a quarter of the plain one."""
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(2)
    values = rng.integers(0, 100, 10_000).astype(np.int64) * 1_000_003
    values[:100] = np.arange(100) * 1_000_003
    frame = DeviceFrame({"a": DeviceColumn(t(values))})
    plain, small = str(tmp_path / "plain"), str(tmp_path / "dict")
    nvt.Dataset(frame).to_parquet(plain)
    nvt.Dataset(frame).to_parquet(small, use_dictionary=True)
    (_, _, cp), = _chunks(_parts(plain)[0])
    (_, _, cd), = _chunks(_parts(small)[0])
    print("chunk bytes: plain", cp.total_compressed_size, "dictionary", cd.total_compressed_size,
          "file bytes:", os.path.getsize(_parts(plain)[0]), os.path.getsize(_parts(small)[0]))
    assert cp.total_compressed_size >= 80_000
    assert 800 + 8_750 <= cd.total_compressed_size < 10_000
    assert os.path.getsize(_parts(small)[0]) * 4 < os.path.getsize(_parts(plain)[0])
    assert np.array_equal(np.asarray(pq.read_table(_parts(small)[0]).column("a")), values)


def test_row_groups_of_one_file_differ_in_encoding(tmp_path, monkeypatch):
    """Row groups of 1000 rows: "a" repeats in the first three and is a permutation in the last two,
    "f" is never offered.  One read-back per row group that had an offered column."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 1000)
    rng = np.random.default_rng(4)
    a = np.concatenate([rng.integers(0, 9, 3000), rng.permutation(2000) + 100]).astype(np.int64)
    frame = DeviceFrame({"a": DeviceColumn(t(a)), "f": DeviceColumn(t(rng.random(5000).astype(np.float32)))})
    out = str(tmp_path / "out")
    before = _stats()
    nvt.Dataset(frame).to_parquet(out, use_dictionary=True)
    after = _stats()
    path, = _parts(out)
    enc = {(name, g): "RLE_DICTIONARY" in cm.encodings for name, g, cm in _chunks(path)}
    assert [enc[("a", g)] for g in range(5)] == [True, True, True, False, False]
    assert not any(enc[("f", g)] for g in range(5))
    assert {k: after[k] - before[k] for k in after} == dict(pqdict_build=5, pqdict_pack=5, pqdict_readback=5)
    _assert_same(_columns(pq.read_table(path)), _columns(frame.to_arrow()))
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(out).to_iter()])
    _assert_same(_columns(back), _columns(frame.to_arrow()))
    # a frame without an offered column: no read-back at all
    before = _stats()
    nvt.Dataset(DeviceFrame({"f": frame["f"]})).to_parquet(str(tmp_path / "f"), use_dictionary=True)
    assert _stats() == before


@pytest.mark.parametrize("value", [None, False])
def test_without_the_option_nothing_changes(tmp_path, value):
    import nvtabular_amd as nvt

    frame = _frame(rows=1500)
    out, ref = str(tmp_path / "out"), str(tmp_path / "ref")
    before = _stats()
    nvt.Dataset(frame).to_parquet(out, use_dictionary=value)
    assert _stats() == before
    for name, g, cm in _chunks(_parts(out)[0]):
        assert not cm.has_dictionary_page and cm.encodings == ("PLAIN", "RLE"), name
    nvt.Dataset(frame).to_parquet(ref)                    # the call without the argument: the same bytes
    assert open(_parts(out)[0], "rb").read() == open(_parts(ref)[0], "rb").read()


def test_files_per_proc_and_shuffle(tmp_path, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import parquet_plain as PP
    from nvtabular_amd.io import Shuffle

    monkeypatch.setattr(PP, "PAGE_VALUES", 512)
    frame = _frame(rows=3000, seed=6)
    exp = _columns(frame.to_arrow(), by="id")
    out = str(tmp_path / "out")
    nvt.Dataset(frame).to_parquet(out, out_files_per_proc=2, shuffle=Shuffle.PER_PARTITION, use_dictionary=True)
    files = _parts(out)
    assert len(files) == 2
    for f in files:
        assert pq.read_metadata(f).created_by == PLAIN
        assert any("RLE_DICTIONARY" in cm.encodings for _, _, cm in _chunks(f))
    table = pa.concat_tables([pq.read_table(f) for f in files])
    assert not np.array_equal(np.asarray(table.column("id")), frame["id"].data.cpu().numpy())
    _assert_same(_columns(table, by="id"), exp)
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(out).to_iter()])
    _assert_same(_columns(back, by="id"), exp)


def test_pyarrow_gets_the_argument_when_it_writes(tmp_path):
    """A codec sends the frame to pyarrow's writer, which takes use_dictionary as its own."""
    import nvtabular_amd as nvt

    frame = _frame(rows=800)
    for value, expect in ((False, False), (["i32"], True)):
        out = str(tmp_path / f"out_{expect}")
        nvt.Dataset(frame).to_parquet(out, compression="snappy", use_dictionary=value)
        path, = _parts(out)
        assert pq.read_metadata(path).created_by != PLAIN
        has = {name: cm.has_dictionary_page for name, g, cm in _chunks(path)}
        assert has["i32"] == expect and not has["i64"] and not has["x"]
