"""Flat string columns through ``PlainParquetWriter`` without a GPU: the ``ByteArrayPages`` are made by
tests/pq_str_out_reference.py (what the device makes) and pyarrow, pandas and the reader's own footer
verdict read the files back."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_str_out_reference as R
from nvtabular_amd import parquet_plain as PP

WORDS = ["", "a", "abc", "abcd", "abcde", "x" * 15, "y" * 16, "z" * 17, "häß", "日本語", "🙂"]


def _strings(rng, n, null_frac):
    values = [WORDS[i] for i in rng.integers(0, len(WORDS), n)]
    return [None if rng.random() < null_frac else v for v in values]


def _pages(values, page_rows=None):
    page_rows = page_rows or PP.PAGE_VALUES
    body, page_at, nv, bitmap = R.byte_array_pages(values, page_rows)
    return PP.ByteArrayPages(body, page_at, nv, page_rows), bitmap


def _write(path, columns, n, names=None, dtypes=None, **kw):
    names = names or [f"c{j}" for j in range(len(columns))]
    w = PP.PlainParquetWriter(path, names, dtypes or [PP.STRING_DTYPE] * len(columns), **kw)
    w.write_row_group(columns, n)
    w.close()


@pytest.mark.parametrize("n, null_frac", [(1, 0.0), (9, 0.5), (1000, 0.0), (1000, 0.3), (64, 1.0)])
def test_strings_read_back(tmp_path, n, null_frac):
    values = _strings(np.random.default_rng(n), n, null_frac)
    path = str(tmp_path / "s.parquet")
    _write(path, [_pages(values)], n, names=["s"])
    t = pq.read_table(path)
    assert t.schema.field("s").type == pa.string() and t.column("s").to_pylist() == values
    assert pd.read_parquet(path)["s"].tolist() == values
    cm = pq.read_metadata(path).row_group(0).column(0)
    assert cm.physical_type == "BYTE_ARRAY" and cm.encodings == ("PLAIN", "RLE") and not cm.has_dictionary_page
    assert cm.statistics.null_count == sum(v is None for v in values) and not cm.statistics.has_min_max
    assert pq.read_schema(path).field("s").type == pa.string()
    assert pq.ParquetFile(path).schema.column(0).logical_type.type == "STRING"
    pf = PP.PlainParquetFile(path)
    assert pf.decodable, pf.why_pyarrow
    assert pf.columns[0]["kind"] == "string" and pf.columns[0]["outer_optional"]


def test_several_pages_one_of_them_all_null(tmp_path):
    """R forced small: 5 rows per page, the second page without a value, the last one short."""
    values = ["a", None, "bc", "", "日本"] + [None] * 5 + ["x" * 17, None, "y", "zz", None] + ["last", None]
    pages, bitmap = _pages(values, page_rows=5)
    assert pages.nv == [4, 0, 3, 1] and pages.page_at[1] == pages.page_at[2]
    path = str(tmp_path / "p.parquet")
    _write(path, [(pages, bitmap)], len(values), names=["s"])
    assert pq.read_table(path).column("s").to_pylist() == values
    assert pq.read_metadata(path).row_group(0).column(0).statistics.null_count == values.count(None) == 9
    pf = pq.ParquetFile(path)
    assert pf.metadata.row_group(0).column(0).total_uncompressed_size == pf.metadata.row_group(0).total_byte_size


def test_page_rule():
    assert PP.string_page_rows(0) == PP.PAGE_VALUES and PP.string_page_rows(1020) == PP.PAGE_VALUES
    assert PP.string_page_rows(1021) == ((1 << 30) // 1025) & ~7 < PP.PAGE_VALUES
    assert PP.string_page_rows(PP.MAX_ENTRY_BYTES) == 1 and PP.string_page_rows((1 << 29) - 4) == 2
    for longest in (100, 5000, 1 << 20, PP.MAX_ENTRY_BYTES):
        assert PP.string_page_rows(longest) * (longest + 4) <= PP.MAX_PAGE_BYTES


def test_row_group_of_no_rows_and_several_row_groups(tmp_path):
    path = str(tmp_path / "e.parquet")
    w = PP.PlainParquetWriter(path, ["s", "x"], [PP.STRING_DTYPE, "int64"])
    rng = np.random.default_rng(2)
    exp = []
    for n in (0, 700, 0, 33):
        values = _strings(rng, n, 0.2)
        x = rng.integers(0, 100, n).astype("int64")
        w.write_row_group([_pages(values, page_rows=256), (x, None)], n)
        exp += values
    w.close()
    md = pq.read_metadata(path)
    assert md.num_row_groups == 4 and [md.row_group(g).num_rows for g in range(4)] == [0, 700, 0, 33]
    assert pq.read_table(path).column("s").to_pylist() == exp
    assert PP.PlainParquetFile(path).decodable


def test_beside_numbers_and_a_list_with_statistics(tmp_path):
    import pq_list_reference as LR

    rng = np.random.default_rng(4)
    n = 500
    values = _strings(rng, n, 0.25)
    a = rng.integers(-5, 5, n).astype("int64")
    f = rng.normal(size=n).astype("float32")
    lens = rng.integers(0, 4, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    leaves = rng.integers(0, 9, int(offsets[-1])).astype("int64")
    pages = LR.list_pages(offsets, None, 0, n, PP.PAGE_VALUES)
    levels = PP.ListLevels([p["slots"] for p in pages], [p["nonnull"] for p in pages],
                           np.frombuffer(b"".join(p["rep"] for p in pages), dtype=np.uint8),
                           np.cumsum([0] + [len(p["rep"]) for p in pages])[:-1],
                           np.frombuffer(b"".join(p["dfn"] for p in pages), dtype=np.uint8),
                           np.cumsum([0] + [len(p["dfn"]) for p in pages])[:-1])
    names, dtypes = ["s", "a", "f", "l"], [PP.STRING_DTYPE, "int64", "float32", "int64"]
    cols = [_pages(values), (a, None), (f, None), (leaves, levels)]
    stats = [None, np.array([a.min(), a.max()]), np.array([f.min(), f.max()]), None]
    lists = [False, False, False, True]
    path = str(tmp_path / "m.parquet")
    w = PP.PlainParquetWriter(path, names, dtypes, lists=lists)
    w.write_row_group(cols, n, stats=stats)
    w.close()
    t = pq.read_table(path)
    assert t.column("s").to_pylist() == values
    np.testing.assert_array_equal(np.asarray(t.column("a")), a)
    np.testing.assert_array_equal(np.asarray(t.column("f")), f)
    assert t.column("l").to_pylist() == [leaves[offsets[i]: offsets[i + 1]].tolist() for i in range(n)]
    rg = pq.read_metadata(path).row_group(0)
    assert not rg.column(0).statistics.has_min_max and rg.column(0).statistics.null_count == values.count(None)
    assert rg.column(1).statistics.has_min_max and rg.column(1).statistics.min == a.min()
    pf = PP.PlainParquetFile(path)
    assert pf.decodable and [c["kind"] for c in pf.columns] == ["string", "flat", "flat", "list"]


def test_dictionary_pages_of_strings(tmp_path):
    """A string chunk as DictPages: the dictionary page is the PLAIN BYTE_ARRAY body of the entries."""
    import pq_dict_reference as DR

    rng = np.random.default_rng(7)
    words = sorted(WORDS[:5])
    n = 300
    idx = rng.integers(0, 5, n).astype(np.int32)
    valid = rng.random(n) > 0.2
    values = [words[i] if ok else None for i, ok in zip(idx, valid)]
    keys, offsets, chars, _ = R.entry_table(dict(enumerate(words)))
    ps = R.page_start_of(valid, n, 128)
    dic, W, nv, packed = DR.encode(idx[valid], ps)
    pos, _ = R.plan(dic, offsets, [0, len(dic)])
    body = R.fill(dic, offsets, chars, pos, np.zeros(int(pos[-1]), dtype=np.uint8))
    dp = PP.DictPages(body, np.frombuffer(packed, dtype=np.uint8), W, nv, entries=len(dic), page_rows=128)
    path = str(tmp_path / "d.parquet")
    _write(path, [(dp, np.packbits(valid, bitorder="little"))], n, names=["s"])
    assert pq.read_table(path).column("s").to_pylist() == values
    cm = pq.read_metadata(path).row_group(0).column(0)
    assert cm.has_dictionary_page and "RLE_DICTIONARY" in cm.encodings
    assert PP.PlainParquetFile(path).decodable


def test_argument_errors(tmp_path):
    pages, bitmap = _pages(["a", "b", None], page_rows=2)
    w = PP.PlainParquetWriter(str(tmp_path / "x.parquet"), ["s", "x"], [PP.STRING_DTYPE, "int64"])
    with pytest.raises(TypeError, match="string"):
        w.write_row_group([(np.arange(3), None), (np.arange(3), None)], 3)
    with pytest.raises(TypeError):
        w.write_row_group([(pages, bitmap), (pages, bitmap)], 3)
    with pytest.raises(ValueError, match="non-null values"):
        w.write_row_group([(pages, None), (np.arange(3), None)], 3)     # the bitmap is missing
    with pytest.raises(ValueError):
        PP.ByteArrayPages(np.zeros(3, dtype=np.uint8), [0, 3], [1])      # a value takes 4 bytes or more
    with pytest.raises(ValueError):
        PP.ByteArrayPages(np.zeros(8, dtype=np.uint8), [0, 9], [1])      # behind the body
    with pytest.raises(TypeError, match="list columns of strings"):
        PP.PlainParquetWriter(str(tmp_path / "y.parquet"), ["s"], [PP.STRING_DTYPE], lists=[True])
    w.abort()
