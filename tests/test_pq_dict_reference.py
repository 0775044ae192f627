"""tests/pq_dict_reference.py pinned to pyarrow, without a GPU: the reference's dictionary and packed
indices go through ``PlainParquetWriter``'s dictionary column form (``DictPages``), pyarrow reads
the file back, and the footer says what DESIGN.md, "Dictionary pages in the PLAIN parquet writer",
says it must."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_dict_reference as R
import pq_list_reference as LR
from nvtabular_amd import parquet_plain as PP

I64 = np.iinfo(np.int64)
DICT_ENC = ("PLAIN", "RLE", "RLE_DICTIONARY")


@pytest.fixture
def page(monkeypatch):
    def set_page(rows):
        monkeypatch.setattr(PP, "PAGE_VALUES", rows)
        return rows
    return set_page


def flat_column(values, valid, page_rows, dictionary=True):
    """A flat column of len(values) rows in the writer's form: (values or DictPages, bitmap or None)."""
    nn = values[valid] if valid is not None else values
    bitmap = np.packbits(valid, bitorder="little") if valid is not None else None
    if not dictionary:
        return np.ascontiguousarray(nn), bitmap
    dic, W, nv, packed = R.encode(nn, R.flat_page_start(valid, len(values), page_rows))
    return PP.DictPages(dic, np.frombuffer(packed, dtype=np.uint8), W, nv), bitmap


def list_column(offsets, leaves, leaf_valid, page_slots, dictionary=True):
    """A list column in the writer's form: (non-null leaves or DictPages, ListLevels)."""
    pages = LR.list_pages(offsets, leaf_valid, 0, len(offsets) - 1, page_slots)
    rep, dfn = b"".join(p["rep"] for p in pages), b"".join(p["dfn"] for p in pages)
    rep_at = np.concatenate([[0], np.cumsum([len(p["rep"]) for p in pages])])[:-1]
    def_at = np.concatenate([[0], np.cumsum([len(p["dfn"]) for p in pages])])[:-1]
    nonnull = [p["nonnull"] for p in pages]
    levels = PP.ListLevels([p["slots"] for p in pages], nonnull, np.frombuffer(rep, dtype=np.uint8), rep_at,
                           np.frombuffer(dfn, dtype=np.uint8), def_at)
    nn = leaves[leaf_valid] if leaf_valid is not None else leaves
    if not dictionary:
        return np.ascontiguousarray(nn), levels
    dic, W, nv, packed = R.encode(nn, np.concatenate([[0], np.cumsum(nonnull)]).astype(np.int64))
    return PP.DictPages(dic, np.frombuffer(packed, dtype=np.uint8), W, nv), levels


def expect_flat(values, valid):
    return [int(v) if (valid is None or valid[i]) else None for i, v in enumerate(values)]


def expect_list(offsets, leaves, leaf_valid):
    return [[int(leaves[i]) if (leaf_valid is None or leaf_valid[i]) else None
             for i in range(offsets[r], offsets[r + 1])] for r in range(len(offsets) - 1)]


def check_dict_chunk(path, g, j, dt, d):
    cm = pq.ParquetFile(path).metadata.row_group(g).column(j)
    assert cm.encodings == DICT_ENC
    assert cm.has_dictionary_page
    head = len(PP._dict_page_header(d, d * dt.itemsize))
    assert cm.data_page_offset == cm.dictionary_page_offset + head + d * dt.itemsize
    assert cm.total_uncompressed_size == cm.total_compressed_size
    return cm


def distinct_values(d, dt, rng):
    """d distinct values of dt, spread over the type's range, in a random order with repeats."""
    info = np.iinfo(dt)
    base = np.unique(rng.integers(info.min, info.max, size=2 * d + 8, dtype=dt))[:d]
    assert len(base) == d
    return np.concatenate([base, rng.choice(base, size=max(3, d // 7))])[rng.permutation(d + max(3, d // 7))]


@pytest.mark.parametrize("dt", [np.dtype("int32"), np.dtype("int64")])
@pytest.mark.parametrize("d", [1, 2, 3, 256, 257, 65536, 65537])
def test_flat_widths(tmp_path, page, dt, d):
    rows = page(16 if d <= 3 else 4096)
    rng = np.random.default_rng(d)
    values = distinct_values(d, dt, rng)
    valid = rng.random(len(values)) > 0.2
    valid[np.unique(values, return_index=True)[1]] = True    # every distinct value stays
    path = str(tmp_path / "f.parquet")
    w = PP.PlainParquetWriter(path, ["a", "b"], [dt, dt])
    col_a, col_b = flat_column(values, valid, rows), flat_column(values, None, rows)
    assert col_a[0].W == col_b[0].W == max(1, (d - 1).bit_length())
    w.write_row_group([col_a, col_b], len(values))
    w.close()
    t = pq.read_table(path)
    assert t.schema.field("a").type == pa.from_numpy_dtype(dt)
    assert t["a"].to_pylist() == expect_flat(values, valid)
    assert t["b"].to_pylist() == expect_flat(values, None)
    first = check_dict_chunk(path, 0, 0, dt, d)
    assert first.dictionary_page_offset == 4
    second = check_dict_chunk(path, 0, 1, dt, d)
    assert second.dictionary_page_offset == 4 + first.total_compressed_size
    f = PP.PlainParquetFile(path)
    assert f.readable, f.why_not


def test_extreme_values(tmp_path, page):
    rows = page(16)
    values = np.array([I64.min, -1, 0, I64.max, I64.max, -1, I64.min, 0, 0] * 5, dtype=np.int64)
    path = str(tmp_path / "f.parquet")
    w = PP.PlainParquetWriter(path, ["a"], [np.int64])
    col = flat_column(values, None, rows)
    assert np.array_equal(col[0].dictionary, [I64.min, -1, 0, I64.max]) and col[0].W == 2
    w.write_row_group([col], len(values))
    w.close()
    assert pq.read_table(path)["a"].to_pylist() == expect_flat(values, None)
    check_dict_chunk(path, 0, 0, np.dtype("int64"), 4)
    assert PP.PlainParquetFile(path).readable


def test_pages_of_0_1_7_8_9_values(tmp_path, page):
    rows = page(16)
    counts = [0, 1, 7, 8, 9, 16, 0, 5]                       # non-null values of the pages; the last has 11 rows
    valid = np.concatenate([np.arange(16) < c for c in counts])[:7 * 16 + 11]
    rng = np.random.default_rng(5)
    valid[:7 * 16] = np.concatenate([rng.permutation(valid[p * 16:(p + 1) * 16]) for p in range(7)])
    values = rng.integers(-3, 4, size=len(valid)).astype(np.int64)
    path = str(tmp_path / "f.parquet")
    w = PP.PlainParquetWriter(path, ["a"], [np.int64])
    col = flat_column(values, valid, rows)
    assert col[0].nv == counts
    w.write_row_group([col], len(values))
    w.close()
    assert pq.read_table(path)["a"].to_pylist() == expect_flat(values, valid)
    check_dict_chunk(path, 0, 0, np.dtype("int64"), len(np.unique(values[valid])))
    assert PP.PlainParquetFile(path).readable


@pytest.mark.parametrize("dt", [np.dtype("int32"), np.dtype("int64")])
@pytest.mark.parametrize("d", [1, 5, 257])
def test_list_columns(tmp_path, dt, d):
    rng = np.random.default_rng(d)
    lens = rng.integers(0, 6, size=200)
    lens[10:30] = 0
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    leaves = rng.choice(distinct_values(d, dt, rng), size=int(offsets[-1])).astype(dt)
    leaf_valid = rng.random(len(leaves)) > 0.3
    leaf_valid[20:60] = False                                # a page of nothing but null leaves
    path = str(tmp_path / "l.parquet")
    w = PP.PlainParquetWriter(path, ["x", "y"], [dt, dt], lists=[True, True])
    cx = list_column(offsets, leaves, leaf_valid, 16)
    cy = list_column(offsets, leaves, None, 16)
    assert 0 in cx[0].nv
    w.write_row_group([cx, cy], len(lens))
    w.close()
    t = pq.read_table(path)
    assert t["x"].to_pylist() == expect_list(offsets, leaves, leaf_valid)
    assert t["y"].to_pylist() == expect_list(offsets, leaves, None)
    check_dict_chunk(path, 0, 0, dt, len(np.unique(leaves[leaf_valid])))
    check_dict_chunk(path, 0, 1, dt, len(np.unique(leaves)))
    f = PP.PlainParquetFile(path)
    assert f.readable, f.why_not


def test_row_groups_mix_dictionary_plain_and_empty(tmp_path, page):
    rows = page(16)
    rng = np.random.default_rng(9)
    a = [rng.integers(0, 5, size=40).astype(np.int64), np.zeros(0, dtype=np.int64),
         rng.integers(0, 1 << 40, size=33).astype(np.int64), rng.integers(-2, 2, size=50).astype(np.int64)]
    valid = [rng.random(len(x)) > 0.25 if len(x) else None for x in a]
    as_dict = [True, False, False, True]
    path = str(tmp_path / "m.parquet")
    w = PP.PlainParquetWriter(path, ["a", "b"], [np.int64, np.int32])
    for x, v, dic in zip(a, valid, as_dict):
        b = (x % 3).astype(np.int32)
        w.write_row_group([flat_column(x, v, rows, dictionary=dic),
                           flat_column(b, None, rows, dictionary=not dic and len(x) > 0)], len(x))
    w.close()
    t = pq.read_table(path)
    assert t["a"].to_pylist() == sum((expect_flat(x, v) for x, v in zip(a, valid)), [])
    assert t["b"].to_pylist() == sum((expect_flat(x % 3, None) for x in a), [])
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 4 and md.row_group(1).num_rows == 0
    for g, dic in enumerate(as_dict):
        ca, cb = md.row_group(g).column(0), md.row_group(g).column(1)
        assert ca.has_dictionary_page == dic and (ca.encodings == DICT_ENC) == dic
        assert cb.has_dictionary_page == (not dic and len(a[g]) > 0)
        if not dic:
            assert ca.encodings == ("PLAIN", "RLE") and ca.dictionary_page_offset is None
    f = PP.PlainParquetFile(path)
    assert f.readable, f.why_not


def test_chunk_rule():
    """A chunk is dictionary-encoded iff it has values, d <= DICT_MAX_ENTRIES and it gets smaller."""
    assert not PP.dict_pays(0, [0, 0], 8)
    assert PP.dict_pays(100, [10_000], 8)
    assert PP.dict_index_bytes([10_000], 7) == 1 + 2 + 7 * 1250
    assert not PP.dict_pays(4096, [4096], 8)                 # the dictionary alone is the plain size
    assert not PP.dict_pays(PP.DICT_MAX_ENTRIES + 1, [1 << 24], 8)
    assert PP.dict_pays(PP.DICT_MAX_ENTRIES, [1 << 20] * 16, 8)
    assert not PP.dict_pays(1, [1], 4) and PP.dict_pays(1, [2], 4)   # 4 + 3 bytes against 4 and against 8
    assert PP.dict_index_bytes([0, 8, 9], 3) == 1 + (1 + 1 + 3) + (1 + 1 + 6)


def test_writer_rejects_a_dictpages_that_does_not_match(tmp_path, page):
    rows = page(16)
    values = np.arange(40, dtype=np.int64) % 5
    col, _ = flat_column(values, None, rows)
    with pytest.raises(ValueError):
        PP.DictPages(col.dictionary, col.packed, col.W + 1, col.nv)
    with pytest.raises(ValueError):
        PP.DictPages(col.dictionary, col.packed[:8], col.W, col.nv)
    w = PP.PlainParquetWriter(str(tmp_path / "x.parquet"), ["a"], [np.int64])
    with pytest.raises(ValueError):
        w.write_row_group([(PP.DictPages(col.dictionary, col.packed, col.W, [16, 16, 7, 1]), None)], 40)
    with pytest.raises(TypeError):
        w.write_row_group([(PP.DictPages(col.dictionary.astype(np.int32), col.packed, col.W, col.nv), None)], 40)
    w.abort()
