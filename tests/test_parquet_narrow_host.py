"""Flat int8 / int16 / bool columns in the hand-written parquet reader and writer, host half: the
verdict on pyarrow's files and their staged values, PlainParquetWriter's files read with pyarrow,
nvt_pq_decode_bool_chunk against corrupt chunks, and what ``plain_eligible`` takes (no GPU)."""
import ctypes as C
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from nvtabular_amd import _lib
from nvtabular_amd import parquet_plain as PP
from nvtabular_amd.parquet_thrift import _Struct, _TReader, _varint

ROWS = 5000


def _table(nullable, rows=ROWS, seed=0):
    rng = np.random.default_rng(seed)
    i8 = rng.integers(-128, 128, rows).astype(np.int8)
    i8[:2] = [-128, 127]
    i16 = rng.integers(-32768, 32768, rows).astype(np.int16)
    i16[:2] = [-32768, 32767]
    few = rng.integers(0, 4, rows).astype(np.int8)   # (a dictionary pays)
    b = rng.random(rows) < 0.5
    runs = np.repeat(rng.random(rows // 50 + 1) < 0.5, 50)[:rows]   # (long runs: RLE runs under v2)
    cols = {"i8": i8, "i16": i16, "few": few, "b": b, "runs": runs, "i64": rng.integers(0, 1000, rows),
            "f32": rng.random(rows).astype(np.float32)}

    def arr(v):
        return pa.array(v, mask=(rng.random(rows) < 0.25) if nullable else None)

    fields = [pa.field(n, pa.from_numpy_dtype(v.dtype), nullable=nullable) for n, v in cols.items()]
    arrays = [arr(v) for v in cols.values()]
    if nullable:
        fields += [pa.field("nothing8", pa.int8()), pa.field("nothing", pa.bool_())]
        arrays += [pa.array([None] * rows, pa.int8()), pa.array([None] * rows, pa.bool_())]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def _staged_equals(path, table):
    pf = PP.PlainParquetFile(path)
    assert pf.eligible, pf.why
    want = {"i8": "int8", "i16": "int16", "few": "int8", "b": "bool", "runs": "bool", "i64": "int64", "f32": "float32",
            "nothing8": "int8", "nothing": "bool"}
    assert [str(d) for d in pf.dtypes] == [want[n] for n in table.column_names]
    before = PP.READER_CHUNKS["plain"]
    staged = PP.read_row_groups_staged(pf, list(range(pf.num_row_groups)), pin=False)
    assert PP.READER_CHUNKS["plain"] - before == table.num_columns * pf.num_row_groups
    for name in table.column_names:
        sc, col = staged[name], table.column(name).combine_chunks()
        mask = np.asarray(col.is_valid())
        assert sc.rows == table.num_rows and sc.nvalid == int(mask.sum()), name
        assert str(sc.dtype) == want[name]
        if mask.all():
            assert sc.valid is None, name
        else:
            bits = np.unpackbits(sc.valid.numpy(), bitorder="little")[:sc.rows].astype(bool)
            np.testing.assert_array_equal(bits, mask, err_msg=name)
        vals = sc.values[:sc.nvalid].numpy()
        # staged: int32 for int8 / int16, one byte per bool -- narrowed here as the device does
        assert vals.dtype == {"int8": np.int32, "int16": np.int32, "bool": np.uint8}.get(want[name], vals.dtype)
        np.testing.assert_array_equal(vals.astype(np.dtype(want[name])), col.drop_null().to_numpy(zero_copy_only=False),
                                      err_msg=name)


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("use_dictionary", [True, False])
@pytest.mark.parametrize("compression", ["snappy", "none"])
def test_pyarrow_files_are_staged_as_pyarrow_reads_them(tmp_path, compression, use_dictionary, version, nullable):
    table = _table(nullable)
    path = str(tmp_path / "f.parquet")
    pq.write_table(table, path, compression=compression, use_dictionary=use_dictionary, data_page_version=version,
                   data_page_size=700, row_group_size=3000)
    md = pq.read_metadata(path)
    assert md.num_row_groups == 2
    _staged_equals(path, table)


def _pack_pages(vals, mask, rows, page):
    out = [np.zeros(0, np.uint8)]
    for s in range(0, rows, page):
        m = mask[s: s + page] if mask is not None else np.ones(min(page, rows - s), bool)
        out.append(np.packbits(vals[s: s + page][m], bitorder="little"))
    return np.concatenate(out)


@pytest.mark.parametrize("page", [None, 16])
@pytest.mark.parametrize("rows", [0, 1, 7, 8, 9, 1000])
def test_writer_files_read_by_pyarrow(tmp_path, monkeypatch, rows, page):
    """int8 / int16 as sign-extended int32 buffers, bool as BoolPages: pyarrow reads int8 / int16 /
    bool with the same values and nulls, over one page and over several."""
    if page is not None:
        monkeypatch.setattr(PP, "PAGE_VALUES", page)
    page = page or PP.PAGE_VALUES
    rng = np.random.default_rng(rows)
    i8 = rng.integers(-128, 128, rows).astype(np.int8)
    i16 = rng.integers(-32768, 32768, rows).astype(np.int16)
    b = rng.random(rows) < 0.5
    mask = rng.random(rows) < 0.7
    bitmap = np.packbits(mask, bitorder="little")
    path = str(tmp_path / "w.parquet")
    w = PP.PlainParquetWriter(path, ["i8", "i16n", "b", "bn", "x"], ["int8", "int16", "bool", "bool", "int64"])
    stats = [np.array([i8.min(), i8.max()], np.int32) if rows else None, None, None, None, None]
    w.write_row_group([(i8.astype(np.int32), None), (i16[mask].astype(np.int32), bitmap),
                       (PP.BoolPages(_pack_pages(b, None, rows, page), rows), None),
                       (PP.BoolPages(_pack_pages(b, mask, rows, page), int(mask.sum())), bitmap),
                       (np.arange(rows, dtype=np.int64), None)], rows, stats=stats)
    w.close()
    got = pq.read_table(path)
    assert [str(x) for x in got.schema.types] == ["int8", "int16", "bool", "bool", "int64"]
    np.testing.assert_array_equal(got["i8"].to_numpy(), i8)
    assert got["i16n"].to_pylist() == [int(v) if k else None for v, k in zip(i16, mask)]
    assert got["b"].to_pylist() == [bool(v) for v in b]
    assert got["bn"].to_pylist() == [bool(v) if k else None for v, k in zip(b, mask)]
    md = pq.read_metadata(path)
    el = md.schema.column(0)
    assert el.physical_type == "INT32" and el.converted_type == "INT_8"
    assert str(el.logical_type) == "Int(bitWidth=8, isSigned=true)"
    assert md.schema.column(1).converted_type == "INT_16" and md.schema.column(2).physical_type == "BOOLEAN"
    st = md.row_group(0).column(0).statistics
    if rows:
        assert (st.min, st.max) == (int(i8.min()), int(i8.max()))
    assert md.row_group(0).column(3).statistics.null_count == rows - int(mask.sum())
    assert not md.row_group(0).column(3).statistics.has_min_max
    # our own reader takes the file, and the _metadata summary accepts the footer
    pf = PP.PlainParquetFile(path)
    assert pf.eligible and [str(d) for d in pf.dtypes] == ["int8", "int16", "bool", "bool", "int64"]
    md.set_file_path("w.parquet")
    pq.write_metadata(got.schema, str(tmp_path / "_metadata"), metadata_collector=[md])
    assert pq.read_metadata(str(tmp_path / "_metadata")).num_rows == rows
    if rows:
        _staged = PP.read_row_groups_staged(pf, [0], pin=False)
        np.testing.assert_array_equal(_staged["bn"].values[:_staged["bn"].nvalid].numpy().astype(bool), b[mask])
        np.testing.assert_array_equal(_staged["i16n"].values[:_staged["i16n"].nvalid].numpy(), i16[mask].astype(np.int32))


def test_writer_refuses_other_types_and_mismatched_buffers(tmp_path):
    with pytest.raises(TypeError, match="unsupported dtype uint8"):
        PP.PlainParquetWriter(str(tmp_path / "u.parquet"), ["u"], ["uint8"])
    for dt in ("int8", "bool"):
        with pytest.raises(TypeError, match="list columns of bool / int8 / int16"):
            PP.PlainParquetWriter(str(tmp_path / "l.parquet"), ["l"], [dt], lists=[True])
    w = PP.PlainParquetWriter(str(tmp_path / "m.parquet"), ["a", "b"], ["int8", "bool"])
    with pytest.raises(TypeError, match="column buffer is int8"):   # (int8 values travel as int32)
        w.write_row_group([(np.zeros(4, np.int8), None), (PP.BoolPages(np.zeros(1, np.uint8), 4), None)], 4)
    with pytest.raises(TypeError):
        w.write_row_group([(np.zeros(4, np.int32), None), (np.zeros(4, bool), None)], 4)
    with pytest.raises(ValueError, match="do not match the validity bitmap"):
        w.write_row_group([(np.zeros(4, np.int32), None), (PP.BoolPages(np.zeros(1, np.uint8), 3), None)], 4)
    with pytest.raises(ValueError, match="packed bytes"):
        PP.BoolPages(np.zeros(1, np.uint8), 9)
    w.abort()


# ---- the verdict on annotations ---------------------------------------------------------------------
def _rewrite_schema(src, dst, edit):
    """A copy of parquet file ``src`` whose footer went through ``edit(schema elements)`` -- the
    elements as {field id: value} dicts of a flat file; only fields 1, 3, 4, 5, 6 and 10 are kept."""
    raw = open(src, "rb").read()
    flen = int.from_bytes(raw[-8:-4], "little")
    start = len(raw) - 8 - flen
    meta = _TReader(raw[start: start + flen]).struct()
    els = meta[2]
    edit(els)
    # the footer is re-encoded from its first byte up to the end of the schema list, the rest is kept:
    # fields 1 (version) and 2 (schema) come first in every writer's footer
    r = _TReader(raw[start: start + flen])
    assert r.b[r.p] == 0x15                    # field 1, i32
    r.p += 1
    version = r.zigzag()
    assert r.b[r.p] == 0x19                    # field 2, list
    r.p += 1
    r.value(9)
    tail = raw[start + r.p: start + flen]
    items = []
    for e in els:
        st = _Struct()
        if 1 in e:
            st.i32(1, e[1])
        if 3 in e:
            st.i32(3, e[3])
        st.binary(4, e[4])
        if 5 in e:
            st.i32(5, e[5])
        if 6 in e:
            st.i32(6, e[6])
        if 10 in e:   # (as the file had it: an INTEGER annotation decoded to {10: {1: bits, 2: signed}})
            st.struct(10, e[10] if isinstance(e[10], bytes) else _int_annotation(e[10][10][1], e[10][10][2]))
        items.append(st.done())
    head = _Struct().i32(1, version).list(2, 12, items).done()[:-1]   # (without the stop byte: `tail` goes on)
    # `tail` starts with a field header relative to field 2: kept as it is
    footer = head + tail
    with open(dst, "wb") as f:
        f.write(raw[:start] + footer + len(footer).to_bytes(4, "little") + b"PAR1")


def _int_annotation(bits, signed):
    return _Struct().struct(10, _Struct().byte(1, bits).bool(2, signed).done()).done()


def test_legacy_converted_types_and_unsigned(tmp_path):
    rows = 100
    rng = np.random.default_rng(1)
    i8, i16 = rng.integers(-128, 128, rows).astype(np.int8), rng.integers(-32768, 32768, rows).astype(np.int16)
    src = str(tmp_path / "src.parquet")
    pq.write_table(pa.table({"a": i8, "b": i16}), src, use_dictionary=False, compression="none")
    assert PP.PlainParquetFile(src).eligible

    def legacy(els):   # converted types 15 / 16 alone, no LogicalType
        for e in els[1:]:
            e.pop(10, None)

    def only_logical(els):
        for e, bits in zip(els[1:], (8, 16)):
            e.pop(6, None)
            e[10] = _int_annotation(bits, True)

    def unsigned(els):
        els[1][10] = _int_annotation(8, False)
        els[1][6] = 11   # UINT_8

    def unsigned_logical_only(els):
        els[1].pop(6, None)
        els[1][10] = _int_annotation(8, False)

    def mismatch(els):   # INTEGER{8} beside INT_16
        els[1][10] = _int_annotation(8, True)
        els[1][6] = 16

    for name, edit, ok in [("legacy", legacy, True), ("only_logical", only_logical, True), ("unsigned", unsigned, False),
                           ("unsigned_logical_only", unsigned_logical_only, False), ("mismatch", mismatch, False)]:
        dst = str(tmp_path / f"{name}.parquet")
        _rewrite_schema(src, dst, edit)
        pf = PP.PlainParquetFile(dst)
        assert pf.eligible == ok, (name, pf.why)
        if ok:
            assert [str(d) for d in pf.dtypes] == ["int8", "int16"], name
            assert [str(x) for x in pq.read_schema(dst).types] == ["int8", "int16"], name
            st = PP.read_row_groups_staged(pf, [0], pin=False)
            np.testing.assert_array_equal(st["a"].values.numpy(), i8.astype(np.int32))
        else:
            assert "logical type" in pf.why or "converted type" in pf.why, (name, pf.why)


def test_narrow_and_bool_list_leaves_stay_with_pyarrow(tmp_path):
    for name, typ in [("i8", pa.int8()), ("i16", pa.int16()), ("b", pa.bool_())]:
        path = str(tmp_path / f"{name}.parquet")
        one, zero = (True, False) if name == "b" else (1, 0)
        pq.write_table(pa.table({"l": pa.array([[one, zero], [], None, [one]], pa.list_(typ))}), path)
        pf = PP.PlainParquetFile(path)
        assert not pf.decodable and "list leaves" in pf.why_pyarrow, name


# ---- nvt_pq_decode_bool_chunk against corrupt chunks ---------------------------------------------------
GUARD = 64


def _page_v1(num_values, body, encoding=0, claim=None):
    dph = _Struct().i32(1, num_values).i32(2, encoding).i32(3, 3).i32(4, 3).done()
    size = len(body) if claim is None else claim
    return _Struct().i32(1, 0).i32(2, size).i32(3, size).struct(5, dph).done() + body


def _levels(mask):
    groups = (len(mask) + 7) // 8
    run = _varint((groups << 1) | 1) + np.packbits(mask, bitorder="little").tobytes()
    return len(run).to_bytes(4, "little") + run


def _decode(chunk, rows, nbytes=None, max_def=1):
    """-> (rc, values, bitmap) with the guard bytes around both outputs checked."""
    lib = _lib.load()
    nbytes = len(chunk) if nbytes is None else nbytes
    buf = (C.c_uint8 * max(len(chunk), 1)).from_buffer_copy(chunk if chunk else b"\0")
    vals = np.full(rows + 2 * GUARD, 0xA5, np.uint8)
    valid = np.full((rows + 7) // 8 + 8 + 2 * GUARD, 0xA5, np.uint8)
    valid[GUARD:-GUARD] = 0
    r, v = C.c_uint64(), C.c_uint64()
    rc = lib.nvt_pq_decode_bool_chunk(buf, nbytes, 0, max_def, rows, valid.ctypes.data + GUARD, 0,
                                      vals.ctypes.data + GUARD, rows, None, 0, C.byref(r), C.byref(v))
    assert (vals[:GUARD] == 0xA5).all() and (vals[-GUARD:] == 0xA5).all()
    assert (valid[:GUARD] == 0xA5).all() and (valid[-GUARD:] == 0xA5).all()
    return rc, vals[GUARD: GUARD + int(v.value)] if rc == 0 else None, valid[GUARD:-GUARD]


def _rle_values(runs):
    body = b"".join(runs)
    return len(body).to_bytes(4, "little") + body


def test_bool_chunk_plain_and_rle_pages_decode():
    rng = np.random.default_rng(5)
    rows = 1000
    mask, b = rng.random(rows) < 0.7, rng.random(rows) < 0.5
    nv = int(mask.sum())
    plain = _page_v1(rows, _levels(mask) + np.packbits(b[mask], bitorder="little").tobytes())
    rc, vals, valid = _decode(plain, rows)
    assert rc == 0
    np.testing.assert_array_equal(vals.astype(bool), b[mask])
    np.testing.assert_array_equal(np.unpackbits(valid, bitorder="little")[:rows].astype(bool), mask)
    # RLE: a repeat run of 100 ones, then a bit-packed run for the rest
    want = np.concatenate([np.ones(100, bool), b[mask][100:]])
    rest = want[100:]
    groups = (len(rest) + 7) // 8
    rle = _page_v1(rows, _levels(mask) + _rle_values([_varint(100 << 1) + b"\x01", _varint((groups << 1) | 1) +
                                                    np.packbits(rest, bitorder="little").tobytes()]), encoding=3)
    rc, vals, _ = _decode(rle, rows)
    assert rc == 0 and len(vals) == nv
    np.testing.assert_array_equal(vals.astype(bool), want)


def test_bool_chunk_truncated_and_lying_headers_are_refused():
    """Every corruption returns an error code; nothing is written outside the outputs (the guard
    bytes are checked by ``_decode``)."""
    rng = np.random.default_rng(6)
    rows = 1000
    mask, b = rng.random(rows) < 0.7, rng.random(rows) < 0.5
    nv = int(mask.sum())
    packed = np.packbits(b[mask], bitorder="little").tobytes()
    groups = (nv + 7) // 8
    good_rle = _rle_values([_varint((groups << 1) | 1) + packed])
    chunks = {"plain": _page_v1(rows, _levels(mask) + packed),
              "rle": _page_v1(rows, _levels(mask) + good_rle, encoding=3)}
    for name, chunk in chunks.items():
        assert _decode(chunk, rows)[0] == 0, name
        for cut in np.unique(np.linspace(0, len(chunk) - 1, 64).astype(int)):   # truncated at 64 lengths
            rc, _, _ = _decode(chunk[:cut], rows, nbytes=int(cut))
            assert rc in (_lib.NVT_EINVAL, _lib.NVT_EUNSUPPORTED), (name, cut, rc)
    # num_values of the header
    for claim in (0, 2**31 - 1, 2**61):
        rc, _, _ = _decode(_page_v1(claim, _levels(mask) + packed), rows)
        assert rc == _lib.NVT_EINVAL, claim
    # the RLE length prefix (a u32: 2^61 does not fit one, its low 32 bits and the largest u32 stand in)
    for claim in (0, 2**31 - 1, (2**61) & 0xFFFFFFFF, 2**32 - 1):
        body = _levels(mask) + claim.to_bytes(4, "little") + good_rle[4:]
        rc, _, _ = _decode(_page_v1(rows, body, encoding=3), rows)
        assert rc == _lib.NVT_EINVAL, claim
    # runs that claim more values than the page holds: a repeat run, a bit-packed run, 2^61 groups
    for run in (_varint((nv + 1) << 1) + b"\x01", _varint(((groups + 1) << 1) | 1) + packed + b"\0",
                _varint((2**61 << 1) | 1) + packed, _varint(2**61 << 1) + b"\x01"):
        rc, _, _ = _decode(_page_v1(rows, _levels(mask) + _rle_values([run]), encoding=3), rows)
        assert rc == _lib.NVT_EINVAL, run[:4]
    # page sizes that run past the chunk, a value above 1 in a repeat run, another encoding
    assert _decode(_page_v1(rows, _levels(mask) + packed, claim=2**31 - 1), rows)[0] == _lib.NVT_EINVAL
    bad = _rle_values([_varint(nv << 1) + b"\x02"])
    assert _decode(_page_v1(rows, _levels(mask) + bad, encoding=3), rows)[0] == _lib.NVT_EINVAL
    assert _decode(_page_v1(rows, _levels(mask) + packed, encoding=8), rows)[0] == _lib.NVT_EUNSUPPORTED


# ---- what the PLAIN write driver takes -----------------------------------------------------------------
class _Col:
    """What ``plain_eligible`` looks at, with ``is_cuda`` as on the device (no GPU here)."""

    class _Data:
        def __init__(self, dtype, is_cuda):
            self.dtype, self.is_cuda = dtype, is_cuda

    def __init__(self, dtype, is_cuda=True, offsets=None, logical=None):
        self.data, self.offsets, self.logical, self.strings = self._Data(dtype, is_cuda), offsets, logical, None


class _Frame(dict):
    @property
    def columns(self):
        return list(self)


def test_plain_eligible():
    from nvtabular_amd.parquet_write import dictionary_columns, plain_eligible

    frame = _Frame(a=_Col(torch.int8), b=_Col(torch.bool), c=_Col(torch.int16), x=_Col(torch.int64))
    assert plain_eligible(frame, None)
    assert plain_eligible(frame, {"x": "int32"})
    assert not plain_eligible(_Frame(u=_Col(torch.uint8)), None)
    assert not plain_eligible(_Frame(x=_Col(torch.int64)), {"x": "int8"})       # a cast to int8: pyarrow's
    assert not plain_eligible(_Frame(x=_Col(torch.int64)), {"x": "bool"})
    assert not plain_eligible(_Frame(a=_Col(torch.int8)), {"a": "int8"})        # a dtypes= entry of its own
    assert not plain_eligible(_Frame(l=_Col(torch.int8, offsets=object())), None)   # a list of int8
    assert not plain_eligible(_Frame(l=_Col(torch.bool, offsets=object())), None)
    assert not plain_eligible(_Frame(a=_Col(torch.int8, is_cuda=False)), None)  # a host column
    assert not plain_eligible(_Frame(b=_Col(torch.bool, is_cuda=False)), None)
    assert plain_eligible(_Frame(x=_Col(torch.int64, is_cuda=False)), None)     # (as before)
    # use_dictionary: int8 / int16 are offered like int32, bool stays PLAIN silently, named: ValueError
    assert dictionary_columns(frame, None, True) == frozenset({"a", "c", "x"})
    assert dictionary_columns(frame, None, ["a", "c"]) == frozenset({"a", "c"})
    with pytest.raises(ValueError, match="use_dictionary names 'b'"):
        dictionary_columns(frame, None, ["b"])
