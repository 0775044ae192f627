"""Dataset.to_parquet(device_compression="snappy") end to end on the device: the PLAIN writer's files
with SNAPPY chunks read back with pyarrow and with this package, the chunk rule, the sizes in the
footer against a default write of the same frame, argument errors and routing."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from test_gpu_parquet_list import _bitmap, _offsets
from test_gpu_parquet_string_out import _assert_tables_equal, _parts, _str_col

pytestmark = pytest.mark.gpu

PLAIN = "nvtabular_amd plain writer"
ROWS = 5000
COMPRESSIBLE = ["i32", "i32n", "i64", "i64n", "f32", "f32n", "f64", "f64n", "when", "la", "lb", "s"]
COMPRESSIBLE_WITH_DICTIONARIES = ["f32", "f32n", "f64", "f64n", "i64"]


def dev():
    return torch.device("cuda:0")


def t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _frame(rows=ROWS, seed=5):
    """int32 / int64 / float32 / float64 with and without nulls, a datetime, a ``rng.random`` float64
    column (incompressible), two list columns that share their offsets (one with null leaves) and a
    flat string column; "id" orders the rows."""
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    lab = np.minimum(rng.zipf(1.3, rows), 50000)
    lens = rng.integers(0, 6, rows)
    off = _offsets(lens)
    leaves = int(off[-1])
    d_off = t(off)
    words = ["", "a", "abc", "session-%d" % seed, "x" * 15, "häß", "日本語"]
    s = [None if rng.random() < 0.2 else words[i] for i in rng.integers(0, len(words), rows)]
    when = (rng.integers(0, 50, rows) * 86_400_000 + 1_600_000_000_000).astype(np.int64)

    def nulls():
        return _bitmap(rng.random(rows) >= 0.2)

    return DeviceFrame({
        "id": DeviceColumn(t(np.arange(rows, dtype=np.int64) + 10_000 * seed)),
        "i32": DeviceColumn(t(lab.astype(np.int32))),
        "i32n": DeviceColumn(t(rng.integers(-20, 20, rows).astype(np.int32)), nulls()),
        "i64": DeviceColumn(t(lab.astype(np.int64))),
        "i64n": DeviceColumn(t(rng.integers(0, 1000, rows).astype(np.int64)), nulls()),
        "f32": DeviceColumn(t((rng.integers(0, 4, rows) / 4).astype(np.float32))),
        "f32n": DeviceColumn(t((rng.integers(0, 8, rows) / 2).astype(np.float32)), nulls()),
        "f64": DeviceColumn(t((rng.integers(0, 100, rows) / 8).astype(np.float64))),
        "f64n": DeviceColumn(t(np.floor(rng.lognormal(2, 1, rows)).astype(np.float64)), nulls()),
        "when": DeviceColumn(t(when), logical=np.dtype("datetime64[ms]")),
        "rnd": DeviceColumn(t(rng.random(rows))),
        "la": DeviceColumn(t(rng.integers(0, 300, leaves).astype(np.int64)), _bitmap(rng.random(leaves) >= 0.1), d_off),
        "lb": DeviceColumn(t(rng.integers(-5, 5, leaves).astype(np.int32)), None, d_off),
        "s": _str_col(s),
    })


def _chunks(path):
    """{(top-level column name, row group): ColumnChunkMetaData}"""
    md = pq.read_metadata(path)
    return {(md.schema.column(j).path.split(".")[0], g): md.row_group(g).column(j)
            for g in range(md.num_row_groups) for j in range(md.num_columns)}


def _small(monkeypatch):
    from nvtabular_amd import io as nio
    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 2000)      # several row groups per partition
    monkeypatch.setattr(PP, "PAGE_VALUES", 512)            # several pages per chunk


@pytest.mark.parametrize("k, shuffle", [(None, None), (3, None), (None, "PER_PARTITION"), (2, "PER_PARTITION")])
@pytest.mark.parametrize("use_dictionary", [None, True])
def test_round_trip_sizes_and_codecs(tmp_path, monkeypatch, use_dictionary, k, shuffle):
    import nvtabular_amd as nvt
    from nvtabular_amd import parquet_plain as PP
    from nvtabular_amd.io import Shuffle

    _small(monkeypatch)
    frame = _frame()
    exp = frame.to_arrow()
    kw = dict(out_files_per_proc=k, use_dictionary=use_dictionary)
    out, ref = str(tmp_path / "snappy"), str(tmp_path / "default")
    nvt.Dataset(frame).to_parquet(out, device_compression="Snappy", shuffle=getattr(Shuffle, shuffle) if shuffle else None,
                                  **kw)
    files = _parts(out)
    assert len(files) == (k or 1)
    assert all(pq.read_metadata(f).created_by == PLAIN for f in files)
    by = "id" if shuffle else None
    _assert_tables_equal(pa.concat_tables([pq.read_table(f) for f in files]), exp, by=by)
    for f in files:
        plain = PP.PlainParquetFile(f)
        assert plain.decodable, plain.why_pyarrow
        for (name, g), cm in _chunks(f).items():
            # with dictionaries an offered chunk is SNAPPY only when its dictionary page shrinks by more
            # than the varints and tags of its pages cost: the float chunks and the labels' dictionary do
            if name in (COMPRESSIBLE_WITH_DICTIONARIES if use_dictionary else COMPRESSIBLE):
                assert cm.compression == "SNAPPY", (name, g)
            elif name == "rnd":
                assert cm.compression == "UNCOMPRESSED", (name, g)
            if cm.compression == "SNAPPY":
                assert cm.total_compressed_size < cm.total_uncompressed_size, (name, g)
            else:
                assert cm.compression == "UNCOMPRESSED" and cm.total_compressed_size == cm.total_uncompressed_size
            if use_dictionary and name in ("i32n", "i64", "when", "lb"):
                assert "RLE_DICTIONARY" in cm.encodings and cm.has_dictionary_page, name
    flat = nvt.Dataset(frame[[c for c in frame.columns if c not in ("la", "lb", "s")]])
    flat.to_parquet(str(tmp_path / "flat"), device_compression="snappy", **kw)
    assert all(PP.PlainParquetFile(f).eligible for f in _parts(str(tmp_path / "flat")))
    # this package's reader takes the files (no chunk goes to pyarrow)
    before = dict(PP.READER_CHUNKS)
    back = list(nvt.Dataset(out).to_iter())
    assert PP.READER_CHUNKS["pyarrow"] == before["pyarrow"] and PP.READER_CHUNKS["plain"] > before["plain"]
    _assert_tables_equal(pa.concat_tables([p.to_arrow() for p in back]), exp, by=by)
    assert pq.read_metadata(os.path.join(out, "_metadata")).num_rows == ROWS
    assert open(os.path.join(out, "_file_list.txt")).read().split() == [str(len(files))] + [os.path.basename(f) for f in files]
    if shuffle:
        return     # (a default write permutes the rows differently: its chunks are other chunks)
    # the same frame written without the codec: the same chunks, larger files
    nvt.Dataset(frame).to_parquet(ref, **kw)
    for f, r in zip(files, _parts(ref)):
        assert os.path.getsize(f) < os.path.getsize(r)
        cs, cr = _chunks(f), _chunks(r)
        assert list(cs) == list(cr)
        for key in cs:
            assert cs[key].total_uncompressed_size == cr[key].total_compressed_size == cr[key].total_uncompressed_size, key
            assert cs[key].encodings == cr[key].encodings and cs[key].num_values == cr[key].num_values, key


def test_counters_timing_and_the_default_is_untouched(tmp_path, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import kernels as K
    from nvtabular_amd import parquet_write as PW

    _small(monkeypatch)
    frame = _frame(rows=4500)
    names = ("snappy_plan", "snappy_compress", "snappy_gather", "snappy_readback")
    before = {k: K.STATS.get(k, 0) for k in names}
    nvt.Dataset(frame).to_parquet(str(tmp_path / "a"))
    assert {k: K.STATS.get(k, 0) for k in names} == before and PW.LAST_TIMING["snappy_s"] == 0.0
    assert all(cm.compression == "UNCOMPRESSED" for cm in _chunks(_parts(str(tmp_path / "a"))[0]).values())
    nvt.Dataset(frame).to_parquet(str(tmp_path / "b"), device_compression="snappy")
    after = {k: K.STATS.get(k, 0) - before[k] for k in names}
    # 3 row groups of 14 columns: one batched call of each kind (a launch per 16 columns) and one read-back each
    assert after == dict(snappy_plan=3, snappy_compress=3, snappy_gather=3, snappy_readback=3)
    assert PW.LAST_TIMING["snappy_s"] > 0 and nio.LAST_TIMING is PW.LAST_TIMING
    # two writes of the same frame give the same bytes
    nvt.Dataset(frame).to_parquet(str(tmp_path / "c"), device_compression="snappy")
    assert open(_parts(str(tmp_path / "b"))[0], "rb").read() == open(_parts(str(tmp_path / "c"))[0], "rb").read()


def test_argument_errors_leave_nothing_behind(tmp_path):
    import nvtabular_amd as nvt

    frame = _frame(rows=300)
    for name, kw in (("both", dict(compression="snappy", device_compression="snappy")),
                     ("none", dict(compression="none", device_compression="snappy")),
                     ("zstd", dict(device_compression="zstd")), ("true", dict(device_compression=True)),
                     ("empty", dict(device_compression=""))):
        out = tmp_path / name
        with pytest.raises(ValueError, match="device_compression"):
            nvt.Dataset(frame).to_parquet(str(out), **kw)
        assert not out.exists() or not os.listdir(out)


def test_frames_the_plain_writer_does_not_take_go_to_pyarrow_with_the_codec(tmp_path, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    keys = np.array([11, 22, 11, 33] * 50, dtype=np.int64)
    host = DeviceFrame({"id": DeviceColumn(torch.arange(200, dtype=torch.int64)),
                        "s": DeviceColumn(torch.from_numpy(keys), None, None, None, {11: "a", 22: "b", 33: "c"})})
    rows = [["a", "bb"], [], ["a"], ["ccc", "a", "a"]] * 50
    lists = DeviceFrame({"id": DeviceColumn(t(np.arange(200, dtype=np.int64))),
                         "ls": DeviceColumn.from_arrow(pa.array(rows, type=pa.list_(pa.string())), dev())})
    numbers = DeviceFrame({"id": DeviceColumn(torch.arange(200, dtype=torch.int64)),
                           "x": DeviceColumn(torch.from_numpy(keys.astype(np.float64)))})
    for name, frame in (("host", host), ("lists", lists), ("numbers", numbers)):
        out = str(tmp_path / name)
        nvt.Dataset(frame).to_parquet(out, device_compression="snappy")
        f, = _parts(out)
        assert pq.read_metadata(f).created_by != PLAIN
        assert all(cm.compression == "SNAPPY" for cm in _chunks(f).values())
        assert pq.read_table(f).to_pydict() == frame.to_arrow().to_pydict()
    monkeypatch.setattr(nio, "PLAIN_PARQUET", False)
    out = str(tmp_path / "switch")
    nvt.Dataset(_frame(rows=300)).to_parquet(out, device_compression="snappy")
    f, = _parts(out)
    assert pq.read_metadata(f).created_by != PLAIN and all(cm.compression == "SNAPPY" for cm in _chunks(f).values())
