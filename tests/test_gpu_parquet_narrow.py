"""Flat int8 / int16 / bool columns through the hand-written parquet writer and reader, end to end on
the device: to_parquet's files read back with pyarrow and with this package, pyarrow's files read
with this package, dictionaries, snappy, statistics and what stays with pyarrow."""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from test_gpu_parquet_list import _bitmap, _offsets
from test_gpu_parquet_string_out import _assert_tables_equal as _assert_other_columns_equal
from test_gpu_parquet_string_out import _parts, _str_col

pytestmark = pytest.mark.gpu

PLAIN = "nvtabular_amd plain writer"
ROWS = 5000
NARROW = {"i8": torch.int8, "i8n": torch.int8, "i16n": torch.int16, "b": torch.bool, "bn": torch.bool,
          "ball": torch.bool}


def dev():
    return torch.device("cuda:0")


def t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _frame(rows=ROWS, seed=2):
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, rows)
    off = _offsets(lens)
    words = ["", "a", "abc", "häß", "日本語"]
    s = [None if rng.random() < 0.2 else words[i] for i in rng.integers(0, len(words), rows)]
    i8 = rng.integers(-128, 128, rows).astype(np.int8)
    i8[:2] = [-128, 127]
    i16 = rng.integers(-32768, 32768, rows).astype(np.int16)
    i16[:2] = [-32768, 32767]
    return DeviceFrame({
        "i8": DeviceColumn(t(i8)),
        "i8n": DeviceColumn(t(rng.integers(0, 5, rows).astype(np.int8)), _bitmap(rng.random(rows) >= 0.2)),
        "i16n": DeviceColumn(t(i16), _bitmap(rng.random(rows) >= 0.2)),
        "b": DeviceColumn(t(rng.random(rows) < 0.5)),
        "bn": DeviceColumn(t(rng.random(rows) < 0.5), _bitmap(rng.random(rows) >= 0.3)),
        "ball": DeviceColumn(t(np.zeros(rows, dtype=bool)), _bitmap(np.zeros(rows, dtype=bool))),
        "i64": DeviceColumn(t(rng.integers(0, 1000, rows).astype(np.int64))),
        "f32": DeviceColumn(t(rng.random(rows).astype(np.float32))),
        "s": _str_col(s),
        "l": DeviceColumn(t(rng.integers(0, 300, int(off[-1])).astype(np.int64)), None, t(off)),
    })


def _assert_tables_equal(got, exp):
    """Types, values and nulls: the bool columns as Python lists, the rest bit for bit."""
    assert got.column_names == exp.column_names
    bools = [c for c in exp.column_names if pa.types.is_boolean(exp.schema.field(c).type)]
    for c in bools:
        assert pa.types.is_boolean(got.schema.field(c).type), c
        assert got.column(c).to_pylist() == exp.column(c).to_pylist(), c
    for c in exp.column_names:
        if pa.types.is_integer(exp.schema.field(c).type):
            assert got.schema.field(c).type == exp.schema.field(c).type, c
    _assert_other_columns_equal(got.drop(bools), exp.drop(bools))


def _small(monkeypatch):
    from nvtabular_amd import io as nio
    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 2000)      # three row groups
    monkeypatch.setattr(PP, "PAGE_VALUES", 512)            # several pages per chunk


def _chunks(path):
    md = pq.read_metadata(path)
    return {(md.schema.column(j).path.split(".")[0], g): md.row_group(g).column(j)
            for g in range(md.num_row_groups) for j in range(md.num_columns)}


def _read_back(path, **kw):
    """(the partitions of Dataset(path) as one Arrow table, their DeviceFrames, pyarrow chunks counted)"""
    import nvtabular_amd as nvt
    from nvtabular_amd.parquet_plain import READER_CHUNKS

    before = dict(READER_CHUNKS)
    frames = list(nvt.Dataset(path, engine="parquet", **kw).to_iter())
    assert READER_CHUNKS["plain"] > before["plain"]
    return pa.concat_tables([f.to_arrow() for f in frames]), frames, READER_CHUNKS["pyarrow"] - before["pyarrow"]


def test_round_trip(tmp_path, monkeypatch):
    """Fails on a writer / reader without narrow columns: the frame goes to pyarrow (created_by)."""
    import nvtabular_amd as nvt

    _small(monkeypatch)
    frame = _frame()
    exp = frame.to_arrow()
    assert [str(exp.schema.field(c).type) for c in NARROW] == ["int8", "int8", "int16", "bool", "bool", "bool"]
    out = str(tmp_path / "out")
    nvt.Dataset(frame).to_parquet(out)
    files = _parts(out)
    md = pq.read_metadata(files[0])
    assert md.created_by == PLAIN and md.num_row_groups >= 2
    got = pq.read_table(files[0])
    _assert_tables_equal(got, exp)
    back, frames, pyarrow_chunks = _read_back(out)
    assert pyarrow_chunks == 0
    for name, dt in NARROW.items():
        assert all(f[name].data.dtype == dt for f in frames), name
    _assert_tables_equal(back, exp)
    # a selection of columns goes the same way
    ds = nvt.Dataset(out, engine="parquet")
    some = pa.concat_tables([f.to_arrow() for f in ds.to_iter(columns=["bn", "i8n"])])
    _assert_tables_equal(some, exp.select(["bn", "i8n"]))
    assert [np.dtype(ds.schema[c].dtype) for c in ("i8", "i16n", "b")] == [np.dtype("int8"), np.dtype("int16"),
                                                                          np.dtype(bool)]


def test_workflow_labels_and_reduced_dtypes(tmp_path, monkeypatch):
    """Categorify >> ReduceDtypeSize and the reference's label idiom write PLAIN files."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    _small(monkeypatch)
    rng = np.random.default_rng(4)
    df = pd.DataFrame({"cat": rng.integers(0, 40, ROWS).astype(np.int64), "rating": rng.integers(1, 6, ROWS).astype(np.int64)})
    graph = (["cat"] >> ops.Categorify() >> ops.ReduceDtypeSize()) + \
        (["rating"] >> ops.LambdaOp(lambda c: (c > 3).astype("int8")))
    wf = nvt.Workflow(graph)
    res = wf.fit_transform(nvt.Dataset(df))
    exp = pa.concat_tables([f.to_arrow() for f in res.to_iter()])
    assert str(exp.schema.field("rating").type) == "int8" and str(exp.schema.field("cat").type) == "int8"
    np.testing.assert_array_equal(exp["rating"].to_numpy(), (df["rating"] > 3).astype("int8"))
    out = str(tmp_path / "wf")
    res.to_parquet(out)
    assert all(pq.read_metadata(f).created_by == PLAIN for f in _parts(out))
    _assert_tables_equal(pa.concat_tables([pq.read_table(f) for f in _parts(out)]), exp)
    back, _, pyarrow_chunks = _read_back(out)
    assert pyarrow_chunks == 0
    _assert_tables_equal(back, exp)


def test_use_dictionary(tmp_path, monkeypatch):
    import nvtabular_amd as nvt

    _small(monkeypatch)
    frame = _frame()
    exp = frame.to_arrow()
    out = str(tmp_path / "dict")
    nvt.Dataset(frame).to_parquet(out, use_dictionary=True)
    f = _parts(out)[0]
    assert pq.read_metadata(f).created_by == PLAIN
    for (name, g), cm in _chunks(f).items():
        if name == "i8n":   # five distinct values
            assert "RLE_DICTIONARY" in cm.encodings and cm.has_dictionary_page, g
        if name in ("b", "bn", "ball"):
            assert "RLE_DICTIONARY" not in cm.encodings and not cm.has_dictionary_page, (name, g)
    _assert_tables_equal(pq.read_table(f), exp)
    back, _, pyarrow_chunks = _read_back(out)
    assert pyarrow_chunks == 0
    _assert_tables_equal(back, exp)
    nvt.Dataset(frame).to_parquet(str(tmp_path / "named"), use_dictionary=["i8n", "i16n"])
    _assert_tables_equal(pq.read_table(_parts(str(tmp_path / "named"))[0]), exp)
    with pytest.raises(ValueError, match="use_dictionary names 'bn'"):
        nvt.Dataset(frame).to_parquet(str(tmp_path / "bad"), use_dictionary=["bn"])


def test_device_compression(tmp_path, monkeypatch):
    import nvtabular_amd as nvt

    _small(monkeypatch)
    frame = _frame()
    exp = frame.to_arrow()
    raw, out = str(tmp_path / "raw"), str(tmp_path / "snappy")
    nvt.Dataset(frame).to_parquet(raw)
    nvt.Dataset(frame).to_parquet(out, device_compression="snappy")
    f = _parts(out)[0]
    assert pq.read_metadata(f).created_by == PLAIN
    _assert_tables_equal(pq.read_table(f), exp)
    assert os.path.getsize(f) <= os.path.getsize(_parts(raw)[0])
    chunks = _chunks(f)
    assert all(chunks[name, 0].compression == "UNCOMPRESSED" for name in ("b", "bn", "ball"))
    assert chunks["i8n", 0].compression == "SNAPPY"
    back, _, pyarrow_chunks = _read_back(out)
    assert pyarrow_chunks == 0
    _assert_tables_equal(back, exp)


def test_statistics(tmp_path, monkeypatch):
    import nvtabular_amd as nvt

    _small(monkeypatch)
    frame = _frame()
    exp = frame.to_arrow()
    out = str(tmp_path / "stats")
    nvt.Dataset(frame).to_parquet(out, statistics=True)
    f = _parts(out)[0]
    md = pq.read_metadata(f)
    at = 0
    for g in range(md.num_row_groups):
        rows = md.row_group(g).num_rows
        for name in ("i8", "i8n", "i16n"):
            st = _chunks(f)[name, g].statistics
            col = exp[name].slice(at, rows).drop_null().to_numpy()
            assert st.has_min_max and (st.min, st.max) == (int(col.min()), int(col.max())), (name, g)
            assert st.null_count == rows - len(col)
        for name in ("b", "bn", "ball"):
            st = _chunks(f)[name, g].statistics
            assert st is not None and not st.has_min_max, (name, g)
            assert st.null_count == exp[name].slice(at, rows).null_count
        at += rows
    _assert_tables_equal(pq.read_table(f), exp)


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_pyarrow_files_are_read_by_the_reader(tmp_path, version):
    rng = np.random.default_rng(8)
    df = pd.DataFrame({"i8": rng.integers(-128, 128, ROWS).astype(np.int8),
                       "i16": rng.integers(-32768, 32768, ROWS).astype(np.int16),
                       "b": rng.random(ROWS) < 0.3,
                       "bn": pd.array(rng.random(ROWS) < 0.5, dtype="boolean"),
                       "i8n": pd.array(rng.integers(0, 3, ROWS), dtype="Int8"),
                       "x": rng.random(ROWS)})
    df.loc[rng.random(ROWS) < 0.3, ["bn", "i8n"]] = pd.NA
    path = str(tmp_path / "default.parquet")
    if version == "1.0":
        df.to_parquet(path)   # pyarrow's defaults
    else:
        df.to_parquet(path, data_page_version="2.0", row_group_size=2000, data_page_size=300)
    exp = pq.read_table(path).replace_schema_metadata(None)
    back, frames, pyarrow_chunks = _read_back(path)
    assert pyarrow_chunks == 0
    assert frames[0]["i8"].data.dtype == torch.int8 and frames[0]["i16"].data.dtype == torch.int16
    assert frames[0]["b"].data.dtype == torch.bool and frames[0]["bn"].data.dtype == torch.bool
    _assert_tables_equal(back, exp)


def test_uint8_and_narrow_list_leaves_stay_with_pyarrow(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(9)
    rows = 300
    off = _offsets(rng.integers(0, 4, rows))
    for name, frame in {
            "uint8": DeviceFrame({"u": DeviceColumn(t(rng.integers(0, 256, rows).astype(np.uint8))),
                                  "x": DeviceColumn(t(np.arange(rows, dtype=np.int64)))}),
            "list_of_int8": DeviceFrame({"l": DeviceColumn(t(rng.integers(-128, 128, int(off[-1])).astype(np.int8)), None,
                                                           t(off)),
                                         "x": DeviceColumn(t(np.arange(rows, dtype=np.int64)))})}.items():
        out = str(tmp_path / name)
        nvt.Dataset(frame).to_parquet(out)
        f = _parts(out)[0]
        assert pq.read_metadata(f).created_by != PLAIN, name
        _assert_tables_equal(pq.read_table(f).replace_schema_metadata(None), frame.to_arrow())
