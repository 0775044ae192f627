"""List columns in the hand-written PLAIN parquet writer (parquet_plain.PlainParquetWriter), driven
with the level streams of the numpy reference (pq_list_reference) and read back with pyarrow.  No
GPU: the device side is tests/test_gpu_parquet_list.py."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_list_reference as R
from nvtabular_amd.parquet_plain import ListLevels, PlainParquetWriter

PAGE = 64


def _frame(seed=0, rows=400):
    """Lengths 0..5, one row longer than three pages, empty rows first and last, 10 % null leaves."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, rows)
    lens[0] = lens[-1] = 0
    lens[rows // 3] = 3 * PAGE + 17
    lens[rows // 2: rows // 2 + 3] = 0
    off = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    leaves = int(off[-1])
    valid = rng.random(leaves) >= 0.1
    vi = rng.integers(-2**62, 2**62, leaves).astype(np.int64)
    vf = rng.normal(size=leaves).astype(np.float32)
    vf[rng.random(leaves) < 0.05] = np.nan          # NaN values that are NOT nulls
    flat = rng.integers(0, 1000, rows).astype(np.int32)
    return off, valid, vi, vf, flat


def _levels(off, valid, r0, r1, page=PAGE):
    pages = R.list_pages(off, valid, r0, r1, page)
    rep_at = np.cumsum([0] + [len(p["rep"]) for p in pages])[:-1]
    def_at = np.cumsum([0] + [len(p["dfn"]) for p in pages])[:-1]
    rep = np.frombuffer(b"".join(p["rep"] for p in pages), dtype=np.uint8)
    dfn = np.frombuffer(b"".join(p["dfn"] for p in pages), dtype=np.uint8)
    return ListLevels([p["slots"] for p in pages], [p["nonnull"] for p in pages], rep, rep_at, dfn, def_at), pages


def _leaves(off, valid, values, r0, r1):
    lo, hi = int(off[r0]), int(off[r1])
    return np.ascontiguousarray(values[lo:hi][valid[lo:hi]])


def _write(path, off, valid, vi, vf, flat, groups):
    w = PlainParquetWriter(str(path), ["l", "f", "x"], [np.int64, np.float32, np.int32], lists=[True, True, False])
    slots = []
    for r0, r1 in groups:
        lv, pages = _levels(off, valid, r0, r1)
        lv_all, _ = _levels(off, None, r0, r1)
        slots.append(sum(p["slots"] for p in pages))
        w.write_row_group([(_leaves(off, valid, vi, r0, r1), lv),
                           (np.ascontiguousarray(vf[off[r0]:off[r1]]), lv_all),
                           (np.ascontiguousarray(flat[r0:r1]), None)], r1 - r0)
    w.close()
    return slots


def test_list_columns_round_trip_through_pyarrow(tmp_path):
    off, valid, vi, vf, flat = _frame()
    rows = len(flat)
    groups = [(0, 250), (250, rows)]
    path = tmp_path / "lists.parquet"
    slots = _write(path, off, valid, vi, vf, flat, groups)

    t = pq.read_table(str(path))
    assert t.schema.field("l").type == pa.list_(pa.field("element", pa.int64()))
    assert t.schema.field("f").type == pa.list_(pa.field("element", pa.float32()))
    l, f = t.column("l").combine_chunks(), t.column("f").combine_chunks()
    assert l.null_count == 0 and f.null_count == 0           # empty lists, never null lists
    for arr in (l, f):
        got = np.asarray(arr.offsets, dtype=np.int64)
        np.testing.assert_array_equal(got - got[0], off)
    lv = l.flatten()
    got_valid = ~np.asarray(lv.is_null())
    np.testing.assert_array_equal(got_valid, valid)
    got = np.asarray(lv.fill_null(0))
    np.testing.assert_array_equal(got[valid], vi[valid])
    fv = f.flatten()
    assert fv.null_count == 0                                # NaN stays a value
    np.testing.assert_array_equal(np.asarray(fv).view(np.uint32), vf.view(np.uint32))
    np.testing.assert_array_equal(np.asarray(t.column("x")), flat)

    md = pq.read_metadata(str(path))
    assert md.created_by == "nvtabular_amd plain writer"
    assert md.num_rows == rows and md.num_row_groups == 2 and md.num_columns == 3
    for g, (r0, r1) in enumerate(groups):
        rg = md.row_group(g)
        assert rg.num_rows == r1 - r0
        for j, nonnull in ((0, int(valid[off[r0]:off[r1]].sum())), (1, int(off[r1] - off[r0]))):
            c = rg.column(j)
            assert c.path_in_schema == ("l", "f")[j] + ".list.element"
            assert c.num_values == slots[g]                  # slots: not leaves, not rows
            assert c.statistics.null_count == slots[g] - nonnull
        assert rg.column(2).path_in_schema == "x" and rg.column(2).num_values == r1 - r0
    # the footer is one pyarrow's _metadata writer accepts (Dataset.to_parquet collects them)
    md.set_file_path("lists.parquet")
    pq.write_metadata(pq.read_schema(str(path)), str(tmp_path / "_metadata"), metadata_collector=[md])
    assert pq.read_metadata(str(tmp_path / "_metadata")).num_row_groups == 2


def test_pages_follow_the_cut_rule(tmp_path):
    """No page is cut inside a row; the long row drops the nominal pages it covers."""
    off, valid, _, _, _ = _frame()
    rows = len(off) - 1
    _, pages = _levels(off, valid, 0, rows)
    S = R.slot_starts(off, 0, rows)
    assert sum(p["rows"] for p in pages) == rows and sum(p["slots"] for p in pages) == S[-1]
    assert len(pages) < -(-int(S[-1]) // PAGE)               # dropped pages
    at = 0
    for p in pages:
        assert p["row0"] == at and p["slot0"] == S[at] and p["rows"] > 0
        assert len(p["rep"]) == -(-p["slots"] // 8) and len(p["dfn"]) == 2 * len(p["rep"])
        assert p["rep"][0] & 1 == 0                          # a page starts at the first slot of a row
        at += p["rows"]


def test_zero_rows_and_flat_bytes_unchanged(tmp_path):
    """A row group without rows still gives a file pyarrow reads; a file of flat columns has the same
    bytes whether or not the writer is told that none of them is a list."""
    w = PlainParquetWriter(str(tmp_path / "empty.parquet"), ["l", "x"], [np.int64, np.float64], lists=[True, False])
    w.write_row_group([(np.empty(0, np.int64), ListLevels([], [], b"", [], b"", [])), (np.empty(0, np.float64), None)], 0)
    w.close()
    t = pq.read_table(str(tmp_path / "empty.parquet"))
    assert t.num_rows == 0 and t.schema.field("l").type == pa.list_(pa.field("element", pa.int64()))
    x = np.arange(100, dtype=np.int64)
    bitmap = np.packbits(x % 3 != 0, bitorder="little")
    for name, kw in (("a", {}), ("b", {"lists": [False, False]})):
        w = PlainParquetWriter(str(tmp_path / f"{name}.parquet"), ["p", "q"], [np.int64, np.int64], **kw)
        w.write_row_group([(x, None), (np.ascontiguousarray(x[x % 3 != 0]), bitmap)], 100)
        w.close()
    assert (tmp_path / "a.parquet").read_bytes() == (tmp_path / "b.parquet").read_bytes()


def test_argument_errors_come_before_anything_is_written(tmp_path):
    off, valid, vi, _, _ = _frame()
    rows = len(off) - 1
    lv, pages = _levels(off, valid, 0, rows)
    vals = _leaves(off, valid, vi, 0, rows)
    path = tmp_path / "bad.parquet"
    w = PlainParquetWriter(str(path), ["l"], [np.int64], lists=[True])

    def size():
        return path.stat().st_size

    before, pos = size(), w.pos
    # level bytes that do not match the page table
    short = ListLevels(lv.slots, lv.nonnull, lv.rep[:-1], lv.rep_at, lv.dfn, lv.def_at)
    with pytest.raises(ValueError, match="level bytes"):
        w.write_row_group([(vals, short)], rows)
    short = ListLevels(lv.slots, lv.nonnull, lv.rep, lv.rep_at, lv.dfn[:-1], lv.def_at)
    with pytest.raises(ValueError, match="level bytes"):
        w.write_row_group([(vals, short)], rows)
    with pytest.raises(ValueError, match="page table"):
        w.write_row_group([(vals, ListLevels(lv.slots, lv.nonnull[:-1], lv.rep, lv.rep_at, lv.dfn, lv.def_at))], rows)
    # value count != the sum of the non-null counts
    with pytest.raises(ValueError, match="values do not match"):
        w.write_row_group([(vals[:-1], lv)], rows)
    with pytest.raises(TypeError, match="int32"):
        w.write_row_group([(vals.astype(np.int32), lv)], rows)
    # a list column's description changing between row groups
    with pytest.raises(TypeError, match="list"):
        w.write_row_group([(vals, None)], rows)
    assert size() == before and w.pos == pos and w.row_groups == []
    w.write_row_group([(vals, lv)], rows)
    w.close()
    assert pq.read_table(str(path)).num_rows == rows
    w = PlainParquetWriter(str(tmp_path / "flat.parquet"), ["x"], [np.int64])
    with pytest.raises(TypeError, match="flat"):
        w.write_row_group([(vals, lv)], rows)
    w.abort()
    with pytest.raises(ValueError, match="differ in length"):
        PlainParquetWriter(str(tmp_path / "n.parquet"), ["x"], [np.int64], lists=[True, False])
