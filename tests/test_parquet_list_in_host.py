"""Parquet list columns on the way in, host half (no GPU): the footer's ``readable`` verdict, the
staged level streams and values of nvt_pq_decode_list_chunk against pyarrow's own reader, and the
decoder's refusals.  The level arithmetic is restated in tests/pq_levels_reference.py."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_levels_reference as R
from pq_list_files import WRITES, session_table, write_session_file, write_session_file_plain_writer
from nvtabular_amd import _lib
from nvtabular_amd import parquet_plain as PP


# ---- the footer ---------------------------------------------------------------------------------
def _list_table(outer_optional, elem_optional, n=50):
    rng = np.random.default_rng(3)
    rows = [[int(v) for v in rng.integers(0, 9, int(rng.integers(0, 4)))] for _ in range(n)]
    typ = pa.list_(pa.field("element", pa.int64(), nullable=elem_optional))
    return pa.Table.from_arrays([pa.array(rows, type=typ)],
                                schema=pa.schema([pa.field("l", typ, nullable=outer_optional)]))


@pytest.mark.parametrize("outer_optional, elem_optional, max_def", [(False, False, 1), (True, False, 2),
                                                                     (False, True, 2), (True, True, 3)])
def test_three_level_lists_are_readable(tmp_path, outer_optional, elem_optional, max_def):
    path = str(tmp_path / "l.parquet")
    pq.write_table(_list_table(outer_optional, elem_optional), path)
    pf = PP.PlainParquetFile(path)
    assert pf.readable, pf.why_not
    assert not pf.eligible and pf.why
    (col,) = pf.columns
    assert col["kind"] == "list" and col["outer_optional"] == outer_optional and col["elem_optional"] == elem_optional
    assert col["max_def"] == max_def and col["leaf_level"] == 1 + outer_optional
    assert col["leaf_dtype"] == np.dtype("int64")
    assert pf.names == ["l"] and pf.dtypes == [np.dtype("int64")] and pf.max_def == [max_def]


def test_non_compliant_names_are_readable(tmp_path):
    path = str(tmp_path / "l.parquet")
    t = pa.table({"x": pa.array(np.arange(3, dtype="int32")), "l": pa.array([[1.5], [], None], type=pa.list_(pa.float32()))})
    pq.write_table(t, path, use_compliant_nested_type=False)
    assert pq.ParquetFile(path).schema.column(1).path == "l.list.item"
    pf = PP.PlainParquetFile(path)
    assert pf.readable, pf.why_not
    assert not pf.eligible
    assert [c["kind"] for c in pf.columns] == ["flat", "list"] and pf.columns[1]["leaf_dtype"] == np.dtype("float32")
    assert pf.names == ["x", "l"]


@pytest.mark.parametrize("kind", ["list_of_lists", "struct", "map", "list_of_strings", "list_of_timestamps",
                                  "list_of_bool", "list_of_int8", "gzip"])
def test_nested_files_left_to_pyarrow(tmp_path, kind):
    kw = {}
    if kind == "list_of_lists":
        arr = pa.array([[[1, 2], [3]], [], [[4]]], type=pa.list_(pa.list_(pa.int64())))
    elif kind == "struct":
        arr = pa.array([{"a": 1, "b": 2.0}, {"a": 3, "b": 4.0}])
    elif kind == "map":
        arr = pa.array([[(1, 2)], [], [(3, 4), (5, 6)]], type=pa.map_(pa.int64(), pa.int64()))
    elif kind == "list_of_strings":
        arr = pa.array([["a", "b"], [], ["c"]])
    elif kind == "list_of_timestamps":
        arr = pa.array([[1, 2], [], [3]], type=pa.list_(pa.timestamp("us")))
    elif kind == "list_of_bool":
        arr = pa.array([[True], [], [False, True]])
    elif kind == "list_of_int8":
        arr = pa.array([[1], [], [2, 3]], type=pa.list_(pa.int8()))
    else:
        arr = pa.array([[1], [], [2, 3]], type=pa.list_(pa.int64()))
        kw["compression"] = "gzip"
        if not pa.Codec.is_available("gzip"):
            pytest.skip("pyarrow without gzip")
    path = str(tmp_path / "n.parquet")
    pq.write_table(pa.table({"x": pa.array(np.arange(len(arr), dtype="int32")), "c": arr}), path, **kw)
    pf = PP.PlainParquetFile(path)
    assert not pf.readable and pf.why_not
    assert not pf.eligible and pf.why
    # the first reason found stays: the column and what it is, or the codec of the first chunk
    assert ("codec 2" if kind == "gzip" else "'c'") in pf.why_not, pf.why_not


def test_flat_files_keep_both_verdicts(tmp_path):
    path = str(tmp_path / "f.parquet")
    pq.write_table(pa.table({"a": pa.array(np.arange(9, dtype="int64")), "b": pa.array(np.ones(9, dtype="float32"))}), path)
    pf = PP.PlainParquetFile(path)
    assert pf.eligible and pf.readable and [c["kind"] for c in pf.columns] == ["flat", "flat"]
    path = str(tmp_path / "s.parquet")
    pq.write_table(pa.table({"a": pa.array(["x", "y"])}), path)
    pf = PP.PlainParquetFile(path)
    assert not pf.eligible and not pf.readable and pf.why_not


# ---- staged streams against pyarrow -------------------------------------------------------------
def _staged_list_equals_arrow(sc, col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    rep = R.unpack_levels(sc.rep.numpy(), 1, sc.slots)
    dfn = R.unpack_levels(sc.dfn.numpy(), sc.width, sc.slots)
    offsets, valid = R.levels_to_offsets(rep, dfn, sc.leaf_level, sc.max_def)
    exp_off = np.asarray(col.offsets).astype(np.int64)
    np.testing.assert_array_equal(offsets, exp_off - exp_off[0])
    flat = col.flatten()
    np.testing.assert_array_equal(valid, np.asarray(flat.is_valid()))
    assert sc.rows == len(col) and sc.leaves == len(flat) and sc.nvalid == len(flat) - flat.null_count
    got, exp = sc.values.numpy()[:sc.nvalid], flat.drop_null().to_numpy()
    assert got.dtype == exp.dtype
    np.testing.assert_array_equal(got.view(np.uint8), exp.view(np.uint8))
    # nothing behind the last slot (the device reads whole words)
    assert not sc.rep.numpy()[(sc.slots + 7) // 8:].any() and not sc.dfn.numpy()[(sc.slots * sc.width + 7) // 8:].any()


@pytest.mark.parametrize("how", sorted(WRITES))
def test_staged_streams_equal_pyarrow(tmp_path, how):
    path = write_session_file(tmp_path, how)
    pf = PP.PlainParquetFile(path)
    assert pf.readable, pf.why_not
    assert pf.num_row_groups == 2
    before = dict(PP.READER_CHUNKS)
    staged = PP.read_row_groups_staged(pf, [0, 1], pin=False)
    assert PP.READER_CHUNKS["plain"] == before["plain"] + 6 and PP.READER_CHUNKS["pyarrow"] == before["pyarrow"]
    table = pq.read_table(path)
    for name in ("l", "f"):
        assert staged[name].is_list and staged[name].same_as is None
        _staged_list_equals_arrow(staged[name], table[name])
    x, ex = staged["x"], table["x"].combine_chunks()
    assert not x.is_list and x.rows == 1001 and x.nvalid == 1001 - ex.null_count
    np.testing.assert_array_equal(x.values.numpy()[:x.nvalid], ex.drop_null().to_numpy())
    # one row group alone, and a column subset
    staged = PP.read_row_groups_staged(pf, [1], columns=["l"], pin=False)
    assert set(staged) == {"l"}
    _staged_list_equals_arrow(staged["l"], pq.ParquetFile(path).read_row_groups([1])["l"])


def test_staged_streams_equal_pyarrow_on_the_plain_writers_file(tmp_path):
    path = write_session_file_plain_writer(str(tmp_path / "w.parquet"))
    pf = PP.PlainParquetFile(path)
    assert pf.readable, pf.why_not
    staged = PP.read_row_groups_staged(pf, [0, 1], pin=False)
    table = pq.read_table(path)
    for name in ("l", "f"):
        _staged_list_equals_arrow(staged[name], table[name])
    ref = session_table()   # (and the file holds the frame: None rows as empty ones)
    assert table["l"].combine_chunks().flatten().equals(ref["l"].combine_chunks().flatten())


def _level_runs(stream, width):
    """[(kind, count)] of one hybrid level stream."""
    runs, p = [], 0
    while p < len(stream):
        head = sh = 0
        while True:
            b = stream[p]
            p += 1
            head |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        if head & 1:
            runs.append(("bp", (head >> 1) * 8))
            p += (head >> 1) * width
        else:
            runs.append(("rle", head >> 1))
            p += 1
    return runs


def test_the_fixture_holds_both_run_kinds_and_several_pages(tmp_path):
    """What the comparison above rests on: the v1 file's list chunk has several pages, and its long
    page puts bit-packed AND RLE runs into both level streams (rep: bp 368, rle 601, rle 499 as
    pyarrow writes it), so page and row-group joins fall on bit positions that are no byte boundary."""
    path = write_session_file(tmp_path, "v1_plain")
    pf = PP.PlainParquetFile(path)
    raw = open(path, "rb").read()
    kinds = {"rep": set(), "def": set()}
    pages_per_chunk = []
    for g in range(2):
        cc = pf.row_groups[g]["columns"][1]
        p, end, pages = cc["offset"], cc["offset"] + cc["size"], 0
        while p < end:
            r = PP._TReader(raw, p)
            h = r.struct()
            body = r.p
            if h[1] == 0:
                pages += 1
                n1 = int.from_bytes(raw[body:body + 4], "little")
                rep = raw[body + 4: body + 4 + n1]
                n2 = int.from_bytes(raw[body + 4 + n1: body + 8 + n1], "little")
                dfn = raw[body + 8 + n1: body + 8 + n1 + n2]
                kinds["rep"] |= {k for k, _ in _level_runs(rep, 1)}
                kinds["def"] |= {k for k, _ in _level_runs(dfn, 2)}
            p = body + h[3]
        pages_per_chunk.append(pages)
    assert kinds == {"rep": {"bp", "rle"}, "def": {"bp", "rle"}}, kinds
    assert max(pages_per_chunk) > 1
    assert pf.row_groups[0]["columns"][1]["num_values"] % 8 != 0      # the second row group joins mid-byte


def test_equal_level_streams_are_found(tmp_path):
    """Two list columns with the same lengths and null leaves share their streams (same_as); one null
    leaf more and they do not."""
    rng = np.random.default_rng(1)
    rows = [[int(v) for v in rng.integers(0, 9, int(rng.integers(0, 5)))] for _ in range(300)]
    other = [[v + 1 for v in r] for r in rows]
    third = [list(r) for r in rows]
    k = next(i for i, r in enumerate(third) if len(r) > 1)
    third[k][1] = None
    path = str(tmp_path / "s.parquet")
    pq.write_table(pa.table({"a": pa.array(rows, type=pa.list_(pa.int64())), "b": pa.array(other, type=pa.list_(pa.int64())),
                             "c": pa.array(third, type=pa.list_(pa.int64()))}), path)
    staged = PP.read_row_groups_staged(PP.PlainParquetFile(path), [0], pin=False)
    assert staged["a"].same_as is None and staged["b"].same_as == "a" and staged["c"].same_as is None


# ---- the decoder's own checks -------------------------------------------------------------------
def _chunk(path, name="l", group=0):
    pf = PP.PlainParquetFile(path)
    j = pf.names.index(name)
    cc = pf.row_groups[group]["columns"][j]
    raw = open(path, "rb").read()[cc["offset"]: cc["offset"] + cc["size"]]
    return pf, pf.columns[j], cc, raw, pf.row_groups[group]["num_rows"]


class _Out:
    """Guarded output buffers of one call: 4096 bytes of 0xA5 around each."""
    G = 4096

    def __init__(self, slots, itemsize, sbytes):
        self.slots = slots
        self.sizes = (((slots + 63) // 64) * 8, ((slots * 2 + 63) // 64) * 8, slots * itemsize, sbytes)
        self.bufs = [np.full(n + 2 * self.G, 0xA5, dtype="uint8") for n in self.sizes]
        self.counts = (C.c_uint64 * 4)()

    def ptr(self, i):
        return self.bufs[i].ctypes.data + self.G

    def margins_untouched(self):
        return all((b[:self.G] == 0xA5).all() and (b[self.G + n:] == 0xA5).all() for b, n in zip(self.bufs, self.sizes))


def _decode(lib, buf, out, codec, itemsize, leaf_level, max_def, slots, rows):
    b = (C.c_uint8 * len(buf)).from_buffer_copy(bytes(buf)) if len(buf) else None
    return lib.nvt_pq_decode_list_chunk(b, len(buf), codec, itemsize, leaf_level, max_def, slots, rows, out.ptr(0),
                                        out.ptr(1), 0, out.slots, out.ptr(2), out.sizes[2], out.ptr(3), out.sizes[3],
                                        out.counts)


def test_decode_list_chunk_refusals(tmp_path):
    path = write_session_file(tmp_path, "v1_plain")
    pf, col, cc, raw, rows = _chunk(path)
    assert (col["leaf_level"], col["max_def"]) == (2, 3)
    lib = _lib.load()
    slots = cc["num_values"]
    out = _Out(slots, 8, 64)
    args = (0, 8, 2, 3)
    assert _decode(lib, raw, out, *args, slots, rows) == 0
    assert list(out.counts)[:2] == [slots, rows]
    assert _decode(lib, raw[: len(raw) // 2], out, *args, slots, rows) == _lib.NVT_EINVAL      # truncated
    assert _decode(lib, raw, out, *args, slots, rows - 1) == _lib.NVT_EINVAL                   # more row starts than rows
    assert _decode(lib, raw, out, *args, slots, rows + 1) == _lib.NVT_EINVAL                   # fewer
    assert b"row starts" in lib.nvt_last_error()
    assert _decode(lib, raw, out, *args, slots - 1, rows) == _lib.NVT_EINVAL                   # slots != num_values
    assert _decode(lib, raw, out, *args, slots + 1, rows) == _lib.NVT_EINVAL
    assert _decode(lib, raw, out, 0, 8, 2, 2, slots, rows) == _lib.NVT_EINVAL                  # max_def 3 offered as 2
    assert b"maximum" in lib.nvt_last_error()
    assert _decode(lib, raw, out, 0, 8, 1, 1, slots, rows) == _lib.NVT_EINVAL                  # ... as 1 (width 1)
    assert _decode(lib, raw, out, 0, 8, 2, 4, slots, rows) == _lib.NVT_EINVAL                  # no such column
    assert _decode(lib, raw, out, 2, 8, 2, 3, slots, rows) == _lib.NVT_EUNSUPPORTED            # gzip
    # the second row group's chunk does not start inside a row, a chunk cut at its second page does not
    # matter here: a chunk whose FIRST slot continues a row is refused
    assert out.margins_untouched()


def test_first_slot_must_start_a_row():
    """A hand-made v1 page whose first repetition level is 1."""
    from nvtabular_amd.parquet_plain import _Struct, _varint

    lib = _lib.load()

    def page(rep_levels):
        rep = _varint((1 << 1) | 1) + bytes([int(sum(b << i for i, b in enumerate(rep_levels)))])   # one bit-packed group
        dfn = _varint(len(rep_levels) << 1) + b"\x01"                                               # all def 1
        vals = np.arange(len(rep_levels), dtype="int64").tobytes()
        body = len(rep).to_bytes(4, "little") + rep + len(dfn).to_bytes(4, "little") + dfn + vals
        dph = _Struct().i32(1, len(rep_levels)).i32(2, 0).i32(3, 3).i32(4, 3).done()
        return _Struct().i32(1, 0).i32(2, len(body)).i32(3, len(body)).struct(5, dph).done() + body

    out = _Out(8, 8, 64)
    assert _decode(lib, page([0, 1, 1, 0, 1]), out, 0, 8, 1, 1, 5, 2) == 0
    assert list(out.counts) == [5, 2, 5, 5]
    assert _decode(lib, page([1, 1, 1, 0, 1]), out, 0, 8, 1, 1, 5, 1) == _lib.NVT_EINVAL
    assert b"first slot" in lib.nvt_last_error()


@pytest.mark.parametrize("how", ["v1_plain", "default", "v2"])
def test_decode_list_chunk_survives_corrupted_pages(tmp_path, how):
    """A list chunk with flipped / overwritten bytes is decoded or refused -- never read or written
    outside its buffers: both level streams, the values and the scratch sit inside 0xA5 margins."""
    path = write_session_file(tmp_path, how)
    pf, col, cc, raw, rows = _chunk(path)
    lib = _lib.load()
    slots = cc["num_values"]
    sbytes = 2 * max(cc["raw_size"], cc["size"]) + 64
    out = _Out(slots, 8, sbytes)
    rng = np.random.default_rng(17)
    seen = set()
    for it in range(400):
        buf = bytearray(raw)
        if it:
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, len(buf))) if rng.random() < 0.5 else int(rng.integers(0, min(64, len(buf))))
                buf[at] = int(rng.integers(0, 256)) if rng.random() < 0.7 else (0xFF if rng.random() < 0.5 else 0x80)
        rc = _decode(lib, buf, out, cc["codec"], 8, col["leaf_level"], col["max_def"], slots, rows)
        seen.add(rc)
        assert rc in (0, _lib.NVT_EINVAL, _lib.NVT_EUNSUPPORTED)
        assert out.margins_untouched(), it
        if rc == 0:
            assert out.counts[0] == slots and out.counts[1] == rows and out.counts[3] <= out.counts[2] <= slots
    assert 0 in seen and _lib.NVT_EINVAL in seen


def test_new_symbols_are_declared_and_bound():
    for name in ("nvt_pq_decode_list_chunk", "nvt_pqlist_unpack", "nvt_pqlist_unpack_ws_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
