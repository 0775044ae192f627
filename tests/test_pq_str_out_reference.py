"""tests/pq_str_out_reference.py against pyarrow: the body the reference makes is wrapped in one data
page of a REQUIRED string column by hand (thrift structs written here, not by the writer under test)
and pyarrow reads the strings back; the entry table is compared with pyarrow's large_string buffers
and with the one the product builds."""
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_str_out_reference as R
from nvtabular_amd.parquet_thrift import _CT_BINARY, _CT_I32, _CT_STRUCT, _Struct, _varint, _zigzag

WORDS = ["", "a", "abc", "abcd", "abcde", "x" * 15, "y" * 16, "z" * 17, "häß", "日本語", "🙂", "tab\there"]


def _one_page_file(path, body, n):
    """A parquet file of one required BYTE_ARRAY (UTF8) column "s" whose only data page holds ``body``."""
    dph = _Struct().i32(1, n).i32(2, 0).i32(3, 3).i32(4, 3).done()
    page = _Struct().i32(1, 0).i32(2, len(body)).i32(3, len(body)).struct(5, dph).done() + bytes(body)
    meta = (_Struct().i32(1, 6).list(2, _CT_I32, [_zigzag(0)])
            .list(3, _CT_BINARY, [_varint(1) + b"s"]).i32(4, 0).i64(5, n).i64(6, len(page)).i64(7, len(page))
            .i64(9, 4).done())
    chunk = _Struct().i64(2, 4).struct(3, meta).done()
    group = _Struct().list(1, _CT_STRUCT, [chunk]).i64(2, len(page)).i64(3, n).done()
    schema = [_Struct().binary(4, "schema").i32(5, 1).done(),
              _Struct().i32(1, 6).i32(3, 0).binary(4, "s").i32(6, 0).done()]
    footer = _Struct().i32(1, 1).list(2, _CT_STRUCT, schema).i64(3, n).list(4, _CT_STRUCT, [group]).done()
    with open(path, "wb") as f:
        f.write(b"PAR1" + page + footer + struct.pack("<I", len(footer)) + b"PAR1")


@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_body_is_plain_byte_array(tmp_path, n):
    rng = np.random.default_rng(n)
    values = [WORDS[i] for i in rng.integers(0, len(WORDS), n)]
    body, page_at, nv, bitmap = R.byte_array_pages(values, page_rows=1 << 20)
    assert bitmap is None and list(page_at) == [0, len(body)] and list(nv) == [n]
    assert len(body) == sum(4 + len(v.encode()) for v in values)
    path = str(tmp_path / "one.parquet")
    _one_page_file(path, body, n)
    assert pq.read_table(path).column("s").to_pylist() == values


def test_pages_and_nulls():
    values = [None, None, None, "a", None, "bcd", "", None, None]
    body, page_at, nv, bitmap = R.byte_array_pages(values, page_rows=3)
    assert list(nv) == [0, 2, 1] and list(page_at) == [0, 0, 4 + 1 + 4 + 3, 4 + 1 + 4 + 3 + 4]
    assert bytes(body) == b"\x01\0\0\0a\x03\0\0\0bcd\0\0\0\0"
    assert list(np.unpackbits(bitmap, bitorder="little")[:9]) == [0, 0, 0, 1, 0, 1, 1, 0, 0]
    assert list(R.page_start_of(None, 0, 4)) == [0, 0] and list(R.page_start_of(None, 9, 4)) == [0, 4, 8, 9]


def test_entry_table_is_arrow_layout():
    from nvtabular_amd import kernels_parquet_str_out as KSO

    rng = np.random.default_rng(5)
    ks = np.concatenate([[np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max],
                         rng.integers(-2**62, 2**62, len(WORDS) - 5)])
    strings = dict(zip(ks.tolist()[::-1], WORDS))   # (inserted in descending key order)
    keys, offsets, chars, longest = R.entry_table(strings)
    arr = pa.array([strings[k] for k in sorted(strings)], pa.large_string())
    assert list(keys) == sorted(strings) and longest == max(len(w.encode()) for w in WORDS)
    assert list(offsets) == list(np.frombuffer(arr.buffers()[1], dtype=np.int64)[:len(WORDS) + 1])
    assert bytes(chars[:offsets[-1]]) == arr.buffers()[2].to_pybytes()[:offsets[-1]]
    assert chars.size % 4 == 0 and not chars[offsets[-1]:].any()
    table = KSO.entry_table(strings)
    np.testing.assert_array_equal(table.keys, keys)
    np.testing.assert_array_equal(table.offsets, offsets)
    np.testing.assert_array_equal(table.chars, chars)
    assert table.longest == longest and table.entries == len(WORDS)
    for bad in ({1: "a", 2: b"b"}, {1: b"a"}, {1: "a", 2: None}, {1: "a", 2: 3}):
        assert KSO.entry_table(bad) is None
    assert KSO.entry_table({}).entries == 0


def test_entry_ids_and_absent_surrogates():
    keys = np.array([np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max], dtype=np.int64)
    ids, bad = R.entry_ids(keys, [1, np.iinfo(np.int64).max, 5, -1, np.iinfo(np.int64).min, -7])
    assert list(ids) == [3, 4, 0, 1, 0, 0] and bad == 2
    ids, bad = R.entry_ids(np.zeros(0, dtype=np.int64), [3, 4])
    assert list(ids) == [0, 0] and bad == 2


def test_fill_skips_what_does_not_fit():
    keys, offsets, chars, _ = R.entry_table({0: "ab", 1: "cde"})
    pos, _ = R.plan([0, 1], offsets, [0, 2])
    out = R.fill([0, 1], offsets, chars, pos, np.full(13, 0xA5, dtype=np.uint8), out_bytes=12)
    assert bytes(out) == b"\x02\0\0\0ab" + b"\xa5" * 7
