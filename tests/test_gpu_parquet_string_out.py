"""Flat string columns through Dataset.to_parquet on the device: the hand-written PLAIN writer takes
them (BYTE_ARRAY pages filled on the device), pyarrow and this package read the files back, and what
the writer does not take still goes to pyarrow with the same content."""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from test_gpu_parquet_list import _assert_same, _bitmap, _columns, _offsets

pytestmark = pytest.mark.gpu

PLAIN = "nvtabular_amd plain writer"
WORDS = ["", "a", "abc", "abcd", "abcde", "x" * 15, "y" * 16, "z" * 17, "häß", "日本語", "🙂"]
STRINGS = ("s", "u")


def dev():
    return torch.device("cuda:0")


def t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _str_col(values):
    from nvtabular_amd.device import DeviceColumn

    return DeviceColumn.from_arrow(pa.array(values, pa.string()), dev())


def _frame(rows=3000, seed=1, words=WORDS, extra=None):
    """"s": strings with nulls, "u": five distinct strings without nulls, "id" orders the rows; an int64,
    a float32 with nulls, a datetime and a list-of-int64 column beside them.  ``extra``: {row: string}
    put into "s"."""
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    s = [None if rng.random() < 0.2 else words[i] for i in rng.integers(0, len(words), rows)]
    for row, v in (extra or {}).items():
        s[row] = v
    u = [f"u{i}-{seed}" for i in rng.integers(0, 5, rows)]
    lens = rng.integers(0, 4, rows)
    off = _offsets(lens)
    when = (rng.integers(0, 50, rows) * 86_400_000 + 1_600_000_000_000).astype(np.int64)
    return DeviceFrame({
        "id": DeviceColumn(t(rng.permutation(rows).astype(np.int64) + 10_000 * seed)),
        "s": _str_col(s),
        "x": DeviceColumn(t(rng.normal(size=rows).astype(np.float32)), _bitmap(rng.random(rows) >= 0.2)),
        "u": _str_col(u),
        "when": DeviceColumn(t(when), logical=np.dtype("datetime64[ms]")),
        "l": DeviceColumn(t(rng.integers(0, 9, int(off[-1])).astype(np.int64)), None, t(off)),
    })


def _parts(out):
    files = [f for f in os.listdir(out) if f.endswith(".parquet")]
    return [os.path.join(out, f) for f in sorted(files, key=lambda f: int(f.split("_")[1].split(".")[0]))]


def _assert_tables_equal(got, exp, by=None):
    """Arrow tables column by column: strings as Python lists, the rest bit for bit."""
    assert got.column_names == exp.column_names and got.num_rows == exp.num_rows
    if by is not None:
        got = got.take(pa.array(np.argsort(np.asarray(got.column(by)), kind="stable")))
        exp = exp.take(pa.array(np.argsort(np.asarray(exp.column(by)), kind="stable")))
    strs = [c for c in exp.column_names if pa.types.is_string(exp.schema.field(c).type) or
            pa.types.is_large_string(exp.schema.field(c).type)]
    for c in strs:
        assert pa.types.is_string(got.schema.field(c).type) or pa.types.is_large_string(got.schema.field(c).type), c
        assert got.column(c).to_pylist() == exp.column(c).to_pylist(), c
    _assert_same(_columns(got.drop(strs)), _columns(exp.drop(strs)))


def _assert_string_columns_equal(back, frame, names=STRINGS):
    """Surrogates (under the valid rows), bitmaps and dicts of the string columns of two frames."""
    for name in names:
        a, b = frame[name], back[name]
        ma, mb = a.valid_mask_host(), b.valid_mask_host()
        ma = np.ones(len(a), dtype=bool) if ma is None else ma
        mb = np.ones(len(b), dtype=bool) if mb is None else mb
        np.testing.assert_array_equal(ma, mb, err_msg=name)
        np.testing.assert_array_equal(a.data.cpu().numpy()[ma], b.data.cpu().numpy()[mb], err_msg=name)
        assert b.strings == a.strings, name


def _write(ds, out, **kw):
    ds.to_parquet(out, **kw)
    files = _parts(out)
    assert files
    return files, [pq.read_metadata(f).created_by for f in files], pa.concat_tables([pq.read_table(f) for f in files])


def test_round_trip(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd.parquet_plain import READER_CHUNKS

    frame = _frame()
    exp = frame.to_arrow()
    out = str(tmp_path / "out")
    files, made, table = _write(nvt.Dataset(frame), out)
    assert made == [PLAIN]
    assert nio.LAST_TIMING["strings_s"] > 0
    assert all(table.schema.field(c).type == pa.string() for c in STRINGS)
    _assert_tables_equal(table, exp)
    md = pq.read_metadata(files[0])
    for j in range(md.num_columns):
        cm = md.row_group(0).column(j)
        if cm.path_in_schema in STRINGS:
            assert cm.physical_type == "BYTE_ARRAY" and cm.encodings == ("PLAIN", "RLE")
            assert cm.statistics.null_count == exp.column(cm.path_in_schema).null_count
    before = dict(READER_CHUNKS)
    back, = list(nvt.Dataset(out).to_iter())
    assert READER_CHUNKS["pyarrow"] == before["pyarrow"] and READER_CHUNKS["plain"] > before["plain"]
    _assert_string_columns_equal(back, frame)
    _assert_tables_equal(back.to_arrow(), exp)


def test_row_groups_and_pages_with_a_long_entry(tmp_path, monkeypatch):
    """Row groups of 1000 rows; an entry of 2 MiB brings the page down to 504 rows, so every chunk of
    "s" has two pages; ONE read-back per row group."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import kernels as K
    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 1000)
    long = "L" * (2 << 20)
    assert PP.string_page_rows(len(long)) == 504
    frame = _frame(rows=2500, seed=2, extra={1700: long, 3: None, 4: None})
    exp = frame.to_arrow()
    before = K.STATS.get("pqdict_readback", 0)
    files, made, table = _write(nvt.Dataset(frame), str(tmp_path / "out"), statistics=True)
    assert made == [PLAIN] and pq.read_metadata(files[0]).num_row_groups == 3
    assert K.STATS.get("pqdict_readback", 0) - before == 3
    _assert_tables_equal(table, exp)
    md = pq.read_metadata(files[0])
    names = [md.schema.column(j).path.split(".")[0] for j in range(md.num_columns)]
    for g in range(3):
        assert not md.row_group(g).column(names.index("s")).statistics.has_min_max      # no min / max for strings
        assert md.row_group(g).column(names.index("id")).statistics.has_min_max
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(str(tmp_path / "out")).to_iter()])
    _assert_tables_equal(back, exp)


def test_one_file_for_three_partitions_with_their_own_dicts(tmp_path):
    import nvtabular_amd as nvt

    frames = [_frame(rows=700, seed=3, words=WORDS[:4]), _frame(rows=300, seed=4, words=WORDS[3:8]),
              _frame(rows=500, seed=5, words=WORDS[6:])]
    exp = pa.concat_tables([f.to_arrow() for f in frames])
    files, made, table = _write(nvt.Dataset(frames), str(tmp_path / "out"), out_files_per_proc=1)
    assert made == [PLAIN] and pq.read_metadata(files[0]).num_row_groups == 3
    _assert_tables_equal(table, exp)


def test_shuffle_per_partition(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd.io import Shuffle

    frame = _frame(rows=2000, seed=6)
    exp = frame.to_arrow()
    files, made, table = _write(nvt.Dataset(frame), str(tmp_path / "out"), shuffle=Shuffle.PER_PARTITION,
                                out_files_per_proc=2)
    assert made == [PLAIN, PLAIN]
    assert not np.array_equal(np.asarray(table.column("id")), np.asarray(exp.column("id")))
    _assert_tables_equal(table, exp, by="id")


def test_an_empty_partition(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    full = DeviceFrame({"id": DeviceColumn(t(np.arange(100, dtype=np.int64))),
                        "s": _str_col([None if i % 7 == 0 else WORDS[i % len(WORDS)] for i in range(100)])})
    none = torch.empty(0, dtype=torch.int64, device=dev())
    empty = DeviceFrame({"id": DeviceColumn(none), "s": DeviceColumn(none.clone(), None, None, None, {})})
    files, made, table = _write(nvt.Dataset([empty, full]), str(tmp_path / "out"))
    assert made == [PLAIN, PLAIN] and pq.read_metadata(files[0]).num_rows == 0
    assert pq.read_table(files[0]).schema.field("s").type == pa.string()
    _assert_tables_equal(table, full.to_arrow())


def test_all_null_and_no_null_row_groups(tmp_path, monkeypatch):
    """A row group whose strings are all null (no value reaches the kernels) between two that have values."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd.device import DeviceFrame

    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 64)
    values = ["a"] * 64 + [None] * 64 + ["bc", None] * 20
    frame = DeviceFrame({"s": _str_col(values)})
    files, made, table = _write(nvt.Dataset(frame), str(tmp_path / "out"))
    assert made == [PLAIN] and table.column("s").to_pylist() == values


def test_csv_to_parquet(tmp_path):
    """The first step of a Criteo-style pipeline: tab-separated text with a hex-id column."""
    import nvtabular_amd as nvt

    rng = np.random.default_rng(8)
    n = 600
    hexid = ["" if rng.random() < 0.1 else f"{v:08x}" for v in rng.integers(0, 2**32, n)]
    lines = ["label\thexid\tx"] + [f"{rng.integers(0, 2)}\t{h}\t{rng.normal():.6f}" for h in hexid]
    text = "\n".join(lines) + "\n"
    p = tmp_path / "day.tsv"
    p.write_text(text)
    dtypes = {"label": "int64", "hexid": "string", "x": "float64"}
    out = str(tmp_path / "pq")
    nvt.Dataset(str(p), engine="csv", sep="\t", dtypes=dtypes, part_size=len(text) // 2).to_parquet(out)
    files = _parts(out)
    assert len(files) >= 2 and all(pq.read_metadata(f).created_by == PLAIN for f in files)
    got = pd.concat([pd.read_parquet(f) for f in files], ignore_index=True)
    want = pd.read_csv(str(p), sep="\t", keep_default_na=False, na_values=[""], float_precision="round_trip",
                       dtype={"label": np.int64, "hexid": str, "x": np.float64})
    assert list(got.columns) == ["label", "hexid", "x"] and len(got) == n
    np.testing.assert_array_equal(got["label"].to_numpy(dtype=np.int64), want["label"].to_numpy())
    np.testing.assert_array_equal(got["x"].to_numpy(dtype=np.float64).view(np.uint64),
                                  want["x"].to_numpy().view(np.uint64))
    assert [None if pd.isna(v) else v for v in got["hexid"]] == [None if pd.isna(v) else v for v in want["hexid"]]


def test_what_still_goes_to_pyarrow(tmp_path, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    frame = _frame(rows=400, seed=9)
    exp = frame.to_arrow()
    for name, kw in (("cast", {"dtypes": {"s": "U"}}), ("codec", {"compression": "snappy"})):
        files, made, table = _write(nvt.Dataset(frame), str(tmp_path / name), **kw)
        assert all(m != PLAIN for m in made), name
        _assert_tables_equal(table, exp)
    # a dict value that is no str: the host fall-back of strings.py keys bytes too
    raw = DeviceFrame({"id": DeviceColumn(t(np.arange(4, dtype=np.int64))),
                       "b": DeviceColumn.from_pandas(pd.Series([b"ab", b"", None, b"ab"], dtype=object), dev())})
    assert raw["b"].strings is not None and raw["b"].data.is_cuda
    files, made, table = _write(nvt.Dataset(raw), str(tmp_path / "bytes"))
    assert all(m != PLAIN for m in made)
    assert table.column("b").to_pylist() == raw.to_arrow().column("b").to_pylist() == [b"ab", b"", None, b"ab"]
    # a frame on the host
    keys = np.array([11, 22, 11, 33], dtype=np.int64)
    host = DeviceFrame({"id": DeviceColumn(torch.arange(4, dtype=torch.int64)),
                        "s": DeviceColumn(torch.from_numpy(keys), None, None, None, {11: "a", 22: "b", 33: "c"})})
    files, made, table = _write(nvt.Dataset(host), str(tmp_path / "host"))
    assert all(m != PLAIN for m in made) and table.column("s").to_pylist() == ["a", "b", "a", "c"]
    # a later partition whose string column the writer does not take: the schema differs, no part file stays
    bad = DeviceFrame({"id": DeviceColumn(t(np.arange(4, dtype=np.int64))),
                       "b": DeviceColumn(t(keys), None, None, None, {11: "a", 22: "b", 33: "c"})})
    with pytest.raises(ValueError, match="partition schema differs"):
        nvt.Dataset([bad, raw]).to_parquet(str(tmp_path / "differs"))
    assert not _parts(str(tmp_path / "differs"))


def test_a_surrogate_outside_the_dict_raises_and_leaves_no_file(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    frame = DeviceFrame({"s": DeviceColumn(t(np.array([11, 22, 44, 11], dtype=np.int64)), None, None, None,
                                           {11: "a", 22: "b", 33: "c"})})
    with pytest.raises(ValueError, match="column 's'"):
        nvt.Dataset(frame).to_parquet(str(tmp_path / "out"))
    assert not _parts(str(tmp_path / "out"))


def test_use_dictionary(tmp_path):
    """"u" (5 distinct strings) gets a dictionary page, "s" too (11 words); a column of distinct ids
    stays PLAIN; the option never makes the file larger and never changes the content."""
    import nvtabular_amd as nvt
    from nvtabular_amd import kernels as K

    frame = _frame(rows=3000, seed=10)
    frame["h"] = _str_col([f"{i:08x}" for i in np.random.default_rng(0).permutation(3000)])
    exp = frame.to_arrow()
    plain_files, made, plain_table = _write(nvt.Dataset(frame), str(tmp_path / "plain"))
    before = {k: K.STATS.get(k, 0) for k in ("pqdict_readback", "pq_str_dict_readback")}
    files, made, table = _write(nvt.Dataset(frame), str(tmp_path / "dict"), use_dictionary=True)
    assert made == [PLAIN]
    # the states' read-back and ONE more for the sizes of the three string dictionary pages
    assert {k: K.STATS.get(k, 0) - v for k, v in before.items()} == dict(pqdict_readback=1, pq_str_dict_readback=1)
    md = pq.read_metadata(files[0])
    has = {md.schema.column(j).path.split(".")[0]: md.row_group(0).column(j).has_dictionary_page
           for j in range(md.num_columns)}
    assert has["u"] and has["s"] and not has["h"] and not has["x"]
    assert os.path.getsize(files[0]) < os.path.getsize(plain_files[0])
    _assert_tables_equal(table, exp)
    _assert_tables_equal(plain_table, exp)
    back, = list(nvt.Dataset(str(tmp_path / "dict")).to_iter())
    _assert_string_columns_equal(back, frame, names=("s", "u", "h"))
    # a list of names offers only those; all-distinct alone: the file is not larger than without
    files, made, table = _write(nvt.Dataset(frame), str(tmp_path / "named"), use_dictionary=["h", "u"])
    md = pq.read_metadata(files[0])
    has = {md.schema.column(j).path.split(".")[0]: md.row_group(0).column(j).has_dictionary_page
           for j in range(md.num_columns)}
    assert has["u"] and not has["h"] and not has["s"]
    assert os.path.getsize(files[0]) <= os.path.getsize(plain_files[0])
    _assert_tables_equal(table, exp)
