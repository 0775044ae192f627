"""Dataset.to_parquet(column_encoding=...) end to end: DELTA_BINARY_PACKED pages of the PLAIN writer read
back with pyarrow and with this package, the chunk rule, the counters, the files' sizes and the errors."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import delta_reference as R
from test_gpu_parquet_dict import _chunks, _parts
from test_gpu_parquet_list import _assert_same, _bitmap, _columns

gpu = pytest.mark.gpu
DELTA = "DELTA_BINARY_PACKED"
SORTED = ["ts", "when", "n32", "n16"]
PAGE = 1 << 20


def _frame(rows, seed=11):
    """An ascending int64 timestamp with nulls, a datetime, an int32 counter, an int16 column, a random
    full-range int64 id (its chunks stay PLAIN) and a float column."""
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0")

    def t(v):
        return torch.from_numpy(np.ascontiguousarray(v)).to(dev)

    ts = 1_700_000_000 + np.cumsum(rng.integers(0, 30, rows)).astype(np.int64)
    when = (1_600_000_000_000 + np.arange(rows) * 1000 + rng.integers(0, 900, rows)).astype(np.int64)
    info = np.iinfo(np.int64)
    return DeviceFrame({
        "ts": DeviceColumn(t(ts), _bitmap(rng.random(rows) >= 0.1)),
        "when": DeviceColumn(t(when), logical=np.dtype("datetime64[ms]")),
        "n32": DeviceColumn(t((np.arange(rows) * 3 - 1000).astype(np.int32))),
        "n16": DeviceColumn(t((np.arange(rows) // 40 % 30000).astype(np.int16))),
        "id": DeviceColumn(t(rng.integers(info.min, info.max, rows, dtype=np.int64))),
        "x": DeviceColumn(t(rng.random(rows).astype(np.float32))),
    })


def _size(out):
    return sum(os.path.getsize(p) for p in _parts(out))


def _stats():
    from nvtabular_amd import kernels as K

    return {k: K.STATS.get(k, 0) for k in ("pqdelta_size", "pqdelta_pack", "pqdict_readback")}


@gpu
@pytest.mark.parametrize("rows, page", [(5000, 512), (PAGE + 7, PAGE)])
def test_round_trip_encodings_and_sizes(tmp_path, monkeypatch, rows, page):
    import nvtabular_amd as nvt
    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(PP, "PAGE_VALUES", page)
    frame = _frame(rows)
    exp = _columns(frame.to_arrow())
    plain, out, only_id = (str(tmp_path / d) for d in ("plain", "out", "only_id"))
    nvt.Dataset(frame).to_parquet(plain, statistics=True)
    nvt.Dataset(frame).to_parquet(out, statistics=True, column_encoding={c: DELTA for c in SORTED + ["id"]})
    nvt.Dataset(frame).to_parquet(only_id, statistics=True, column_encoding={"id": DELTA, "x": "PLAIN"})
    path, = _parts(out)
    for name, g, cm in _chunks(path):
        # the sorted columns are delta chunks; the random id falls back to PLAIN, the float was never offered
        assert (DELTA in cm.encodings) == (name in SORTED), (name, cm.encodings)
        assert cm.compression == "UNCOMPRESSED" and not cm.has_dictionary_page
    assert _size(out) < _size(plain) and _size(only_id) <= _size(plain)
    table = pq.read_table(path)
    assert table.schema.field("when").type == pa.timestamp("ms") and table.schema.field("n16").type == pa.int16()
    _assert_same(_columns(table), exp)
    for (_, _, cm), (_, _, cp) in zip(_chunks(path), _chunks(_parts(plain)[0])):   # min / max / nulls come from the values
        assert (cm.statistics.min, cm.statistics.max, cm.statistics.null_count) == \
            (cp.statistics.min, cp.statistics.max, cp.statistics.null_count)
    reader = dict(PP.READER_CHUNKS)
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(out).to_iter()])
    assert PP.READER_CHUNKS["pyarrow"] == reader["pyarrow"] and PP.READER_CHUNKS["plain"] > reader["plain"]
    _assert_same(_columns(back), exp)


@gpu
def test_bare_string_next_to_dictionary_and_snappy(tmp_path):
    """The bare string offers what use_dictionary does not take; a row group still costs ONE read-back; under
    device snappy a delta chunk is written uncompressed."""
    import nvtabular_amd as nvt

    frame = _frame(5000)
    out = str(tmp_path / "out")
    before = _stats()
    nvt.Dataset(frame).to_parquet(out, use_dictionary=["n16"], column_encoding=DELTA, device_compression="snappy")
    after = _stats()
    assert {k: after[k] - before[k] for k in after} == dict(pqdelta_size=4, pqdelta_pack=4, pqdict_readback=1)
    path, = _parts(out)
    for name, g, cm in _chunks(path):
        assert (DELTA in cm.encodings) == (name in ("ts", "when", "n32")), (name, cm.encodings)
        assert ("RLE_DICTIONARY" in cm.encodings) == (name == "n16"), (name, cm.encodings)
        if DELTA in cm.encodings:
            assert cm.compression == "UNCOMPRESSED"
    _assert_same(_columns(pq.read_table(path)), _columns(frame.to_arrow()))


@gpu
@pytest.mark.parametrize("kw", [
    dict(column_encoding={"nope": DELTA}),                           # no column
    dict(column_encoding={"x": DELTA}),                              # a float column is not eligible
    dict(column_encoding={"ts": "RLE"}),                             # another encoding
    dict(column_encoding="BYTE_STREAM_SPLIT"),
    dict(column_encoding={"ts": DELTA}, use_dictionary=["ts", "n32"]),   # offered to both
], ids=["no-column", "float", "encoding", "bare-encoding", "both"])
def test_errors_raise_before_anything_is_created(tmp_path, kw):
    import nvtabular_amd as nvt

    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="column_encoding"):
        nvt.Dataset(_frame(100)).to_parquet(out, **kw)
    assert not os.path.exists(out)


def test_delta_pages_layout_on_the_host(tmp_path, monkeypatch):
    """DeltaPages / PlainParquetWriter with regions made by the reference encoder, read by pyarrow: three
    pages (the last without a non-null value), nulls, an int32 column without."""
    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(PP, "PAGE_VALUES", 400)
    rng = np.random.default_rng(2)
    n = 1000
    ok = rng.random(n) >= 0.3
    ok[800:] = False
    a = np.cumsum(rng.integers(-3, 90, n)).astype(np.int64)
    b = (np.arange(n) * -7).astype(np.int32)

    def pages(vals, valid, bits):
        regs = [R.encode(vals[s: s + 400][valid[s: s + 400]], bits) for s in range(0, n, 400)]
        at = np.cumsum([0] + [16 * -(-len(r) // 16) for r in regs])
        packed = np.full(at[-1], 0xA5, dtype=np.uint8)
        for o, r in zip(at, regs):
            packed[o: o + len(r)] = np.frombuffer(r, dtype=np.uint8)
        nv = [int(valid[s: s + 400].sum()) for s in range(0, n, 400)]
        assert PP.delta_pays([len(r) for r in regs], nv, bits // 8)
        return PP.DeltaPages(vals.dtype, packed, at[:-1], [len(r) for r in regs], nv)

    path = str(tmp_path / "f.parquet")
    w = PP.PlainParquetWriter(path, ["a", "b"], ["int64", "int32"])
    w.write_row_group([(pages(a, ok, 64), np.packbits(ok, bitorder="little")), (pages(b, np.ones(n, bool), 32), None)], n)
    w.close()
    md = pq.read_metadata(path).row_group(0)
    assert set(md.column(0).encodings) == set(md.column(1).encodings) == {DELTA, "RLE"}
    table = pq.read_table(path)
    got = table["a"].to_numpy(zero_copy_only=False)
    np.testing.assert_array_equal(np.isnan(got), ~ok)
    np.testing.assert_array_equal(got[ok].astype(np.int64), a[ok])
    np.testing.assert_array_equal(table["b"].to_numpy(), b)
    assert PP.PlainParquetFile(path).decodable
    assert not PP.delta_pays([5], [0], 8) and not PP.delta_pays([800], [100], 8) and PP.delta_pays([799], [100], 8)
