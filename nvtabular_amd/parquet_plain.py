"""PLAIN / uncompressed parquet files written straight from column buffers.

The output half of the parquet path (reference contract: ``Dataset.to_parquet``,
merlin-io via tests/unit/workflow/test_cpu_workflow.py:67-81 and
bench/datasets/tools/nvt_etl.py:154-171).  pyarrow's writer spent the time of a 45 M-row
Criteo partition set in dictionary building, statistics and compression (5 M rows/s); the
columns this engine produces are fixed-width numbers (int64 labels, float64 / float32
normalised values, int32 passthroughs) for which a PLAIN data page is the column buffer itself:

    page = thrift PageHeader | definition levels | values (non-null ones, little endian)

* no nulls: the definition levels are ONE RLE run ("n times 1": a varint and a byte);
* nulls: the hybrid encoding's bit-packed run at bit width 1 IS the Arrow validity bitmap
  (LSB first), so the bitmap bytes are written verbatim behind a run header, and the values are
  compacted on the device before they are copied out (the caller hands over non-null values).

The file layout (magic, row groups of column chunks of pages, thrift-compact FileMetaData
footer) is written by hand: parquet-format's PageHeader / FileMetaData structures in the
thrift compact protocol.  Readers: pyarrow / pandas / the reference's merlin-io read these
files like any other (tests/test_parquet_plain.py reads them back with pyarrow).
A datetime column (DeviceColumn.logical, unit ms / us / ns) is an INT64 column whose
SchemaElement carries the LogicalType TIMESTAMP (isAdjustedToUTC = false) and, for ms / us, the
converted type; parquet has no seconds unit.
A list column of such numbers is the standard three-level list: a page is

    thrift PageHeader | repetition levels | definition levels | non-null leaves

with both level streams ONE bit-packed run each (bit width 1 and 2), packed on the device
(kernels_parquet_list, csrc/nvt_parquet_list.hip) and handed over as ``ListLevels``; a row of L
leaves is max(L, 1) slots and every page starts at a row ("List columns in the PLAIN
parquet writer").  The reading half below takes such lists too, from any writer ("List
columns in the parquet reader"); other nested files are read with pyarrow.
A flat string column (int64 surrogates and a {surrogate -> str} dict) is a BYTE_ARRAY column annotated
UTF8 / STRING whose page is

    thrift PageHeader | definition levels | per non-null value: u32 length, UTF-8 bytes

The value sections of a chunk's pages are filled on the device (kernels_parquet_str_out,
csrc/nvt_parquet_str_out.hip) and handed over as ``ByteArrayPages``; the rows per page follow the
longest entry (``string_page_rows``) so that no page passes 2^30 bytes; string chunks carry a null
count and no min / max ("String columns in the PLAIN parquet writer").
A flat int8 / int16 column is an INT32 column of sign-extended values annotated INTEGER{8 | 16, signed}
(converted type INT_8 / INT_16): the writer takes its values as int32.  A flat bool column is a BOOLEAN
column whose page is

    thrift PageHeader | definition levels | ceil(nv / 8) bytes: the nv non-null values one per bit, LSB first

packed on the device (kernels_parquet_narrow, csrc/nvt_parquet_narrow.hip) and handed over as
``BoolPages`` ("Narrow and bool columns in the parquet path"); the reading half takes both.
Anything else (lists of strings or of bool / 8 / 16-bit leaves, unsigned integers, string columns on the
host or with bytes / mixed objects in their dict, casts of list or string columns) stays with pyarrow's writer.
With ``to_parquet(use_dictionary=...)`` an int32 / int64 column chunk (datetime counts and list leaves
too) may instead be a dictionary page -- its distinct non-null values, ascending -- followed by data
pages of the same cut whose values are ``W | ONE bit-packed run of indices`` (encoding
RLE_DICTIONARY), handed over as ``DictPages``: dictionary and indices are made on the device
(kernels_parquet_dict, csrc/nvt_parquet_dict.hip), and ``dict_pays`` keeps a chunk PLAIN unless
the dictionary makes it smaller ("Dictionary pages in the PLAIN parquet writer").  A string
chunk's dictionary page is the PLAIN BYTE_ARRAY encoding of its distinct entries.  Not
done: float and bool dictionaries, RLE runs inside the index stream, DELTA encodings.
With ``to_parquet(device_compression="snappy")`` a column chunk may be written SNAPPY (codec 1): the
same pages, every body the snappy raw stream ``varint(U) | one literal holding the level bytes | the
elements of the values region`` with the elements made on the device (kernels_snappy,
csrc/nvt_snappy.hip), handed over as ``SnappyPages``; ``snappy_pays`` keeps a chunk as it is written
today unless the codec makes it smaller ("Snappy pages in the PLAIN parquet writer").
The reading half also takes flat STRING columns (any writer's dictionary / PLAIN pages): their
dictionary entries and index runs are staged as the file holds them and expanded, hashed and
gathered on the device (``StagedStrings``, kernels_parquet_str.py; DESIGN.md, "String columns in
the parquet reader").  Binary columns, lists of strings and DELTA encodings stay with pyarrow.
parquet_thrift.py holds the thrift compact protocol, parquet_write.py the driver in front of the writer.
"""
from __future__ import annotations

import os
import struct
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .parquet_thrift import _CT_BINARY, _CT_I32, _CT_STRUCT, _Struct, _TReader, _varint, _zigzag

_PQ_TYPE = {np.dtype("int32"): 1, np.dtype("int64"): 2, np.dtype("float32"): 4, np.dtype("float64"): 5}   # physical types
PAGE_VALUES = 1 << 20          # values per data page (8 MiB of int64)
ROW_GROUP_ROWS = 1 << 23       # rows per row group
STRING_DTYPE = np.dtype("O")   # what a flat string column (BYTE_ARRAY, UTF8 / STRING) is in ``dtypes``
MAX_PAGE_BYTES = 1 << 30       # a string page's body (a thrift page size is an i32)
MAX_ENTRY_BYTES = MAX_PAGE_BYTES - 4   # the longest string the PLAIN writer takes


BOOL_DTYPE = np.dtype(bool)     # a flat bool column: physical BOOLEAN, ``BoolPages`` in the place of the values
# a flat int8 / int16 column: physical INT32 (the writer takes its values sign-extended to int32),
# annotated LogicalType INTEGER{bitWidth, signed} and the converted type INT_8 / INT_16
_NARROW = {np.dtype("int8"): (8, 15), np.dtype("int16"): (16, 16)}


def _ptype(dt) -> int:
    """Physical type of a column of the writer."""
    return 6 if dt == STRING_DTYPE else 0 if dt == BOOL_DTYPE else _PQ_TYPE[dt]


def physical_dtype(dt):
    """The dtype of the buffers the writer takes for a column of ``dt``: int32 for int8 / int16."""
    return np.dtype("int32") if dt in _NARROW else dt


def string_page_rows(longest: int) -> int:
    """Rows per data page of a string column whose longest entry has ``longest`` bytes:
    min(PAGE_VALUES, max(1, 2^30 // (longest + 4))), so that no page body passes 2^30 bytes -- rounded
    down to a multiple of 8 when it is 8 or more, so that every page starts at a byte of the validity
    bitmap and its definition levels are a slice of it (fewer than 8 rows per page: entries of 128 MiB
    and more; ``_flat_pages`` then re-packs the bits of a page)."""
    rows = min(PAGE_VALUES, max(1, MAX_PAGE_BYTES // (int(longest) + 4)))
    return rows if rows < 8 else rows & ~7


# datetime unit -> (TimeUnit union field of LogicalType TIMESTAMP, converted type or None)
_TS_UNIT = {"ms": (1, 9), "us": (2, 10), "ns": (3, None)}
_TS_BY_FIELD = {1: "ms", 2: "us", 3: "ns"}


def supported_dtype(dt) -> bool:
    return np.dtype(dt) in _PQ_TYPE


def timestamp_unit(logical) -> Optional[str]:
    """"ms" / "us" / "ns" of a datetime64 dtype the PLAIN writer takes, else None."""
    if logical is None:
        return None
    dt = np.dtype(logical)
    unit = np.datetime_data(dt)[0] if dt.kind == "M" else None
    return unit if unit in _TS_UNIT else None


def _page_header(num_values: int, page_bytes: int, encoding: int = 0, compressed: Optional[int] = None) -> bytes:
    """``compressed``: the bytes of the body as it is written (None: ``page_bytes``, no codec)."""
    dph = _Struct().i32(1, num_values).i32(2, encoding).i32(3, 3).i32(4, 3).done()  # PLAIN / RLE_DICTIONARY, RLE, RLE
    return (_Struct().i32(1, 0).i32(2, page_bytes).i32(3, page_bytes if compressed is None else compressed)
            .struct(5, dph).done())


def _dict_page_header(d: int, page_bytes: int, compressed: Optional[int] = None) -> bytes:
    """PageHeader of a DICTIONARY_PAGE (type 2) of d PLAIN values."""
    return (_Struct().i32(1, 2).i32(2, page_bytes).i32(3, page_bytes if compressed is None else compressed)
            .struct(7, _Struct().i32(1, d).i32(2, 0).done()).done())


def _def_levels(n: int, valid_bytes: Optional[memoryview]) -> Tuple[bytes, Optional[memoryview]]:
    """Definition levels of one page (max level 1): (prefix bytes, bitmap bytes or None)."""
    if valid_bytes is None:
        body = _varint(n << 1) + b"\x01"          # RLE run: n times the value 1
        return struct.pack("<I", len(body)) + body, None
    groups = (n + 7) // 8
    head = _varint((groups << 1) | 1)             # bit-packed run of `groups` groups of 8 levels
    return struct.pack("<I", len(head) + groups) + head, valid_bytes[:groups]


def _packed_levels(slots: int, width: int) -> bytes:
    """Prefix of one level stream of a list page: u32 length | header of ONE bit-packed run of
    ceil(slots / 8) groups; `width` bytes of payload per group follow (bit width 1 or 2)."""
    groups = (slots + 7) // 8
    head = _varint((groups << 1) | 1)
    return struct.pack("<I", len(head) + groups * width) + head


def _flat_pages(valid, n: int, page_rows: int):
    """(rows, bitmap bytes or None, non-null values) of the data pages a flat chunk of n rows is cut
    into, ``page_rows`` rows each (n = 0: one page without rows)."""
    vb = memoryview(np.ascontiguousarray(valid)).cast("B") if valid is not None else None
    done_rows = 0
    while True:
        rows = min(page_rows, n - done_rows)
        if vb is not None:
            page_valid = vb[done_rows // 8: (done_rows + rows + 7) // 8]
            bits = np.unpackbits(np.frombuffer(page_valid, dtype=np.uint8), bitorder="little")
            if done_rows % 8:   # (a page that starts inside a byte of the bitmap: its bits are re-packed)
                bits = bits[done_rows % 8:]
                page_valid = memoryview(np.packbits(bits[:rows], bitorder="little")).cast("B")
            nv = int(bits[:rows].sum()) if rows else 0
        else:
            page_valid, nv = None, rows
        yield rows, page_valid, nv
        done_rows += rows
        if done_rows >= n:
            return


class ListLevels:
    """Repetition / definition levels of one list column chunk, already bit-packed (the device
    packs them: kernels_parquet_list; tests/pq_list_reference.py restates the layout).

    Page p holds ``slots[p]`` slots (a row of L leaves is max(L, 1) slots) of which ``nonnull[p]``
    are non-null leaves; its repetition levels are the ceil(slots / 8) bytes at ``rep_at[p]`` of
    ``rep`` (bit width 1), its definition levels the 2 * ceil(slots / 8) bytes at ``def_at[p]`` of
    ``dfn`` (bit width 2), LSB first, pad bits 0.  ``rep`` / ``dfn`` are bytes-like (uint8 arrays);
    like the values they may still be in flight when the row group is laid out, the tables not."""

    __slots__ = ("slots", "nonnull", "rep", "rep_at", "dfn", "def_at")

    def __init__(self, slots, nonnull, rep, rep_at, dfn, def_at):
        self.slots = [int(x) for x in slots]
        self.nonnull = [int(x) for x in nonnull]
        self.rep_at = [int(x) for x in rep_at]
        self.def_at = [int(x) for x in def_at]
        self.rep, self.dfn = rep, dfn


DICT_MAX_ENTRIES = 1 << 20     # distinct values of a dictionary-encoded chunk (an 8 MiB int64 dictionary page)


def dict_index_width(d: int) -> int:
    """Bits per index of a dictionary of d entries: max(1, bit_length(d - 1))."""
    return max(1, (int(d) - 1).bit_length())


def dict_page_offsets(nv, W: int):
    """(byte offset of every page's indices in ``DictPages.packed``, total bytes): page p's
    ``W * ceil(nv[p] / 8)`` bytes start at ``16 * sum_{q<p} ceil(W * ceil(nv[q] / 8) / 16)``."""
    at, pos = [], 0
    for x in nv:
        at.append(pos)
        pos += 16 * (-(-(W * ((int(x) + 7) // 8)) // 16))
    return at, pos


def dict_index_bytes(nv, W: int) -> int:
    """Bytes the index streams of the data pages take: per page the width byte and, when the page
    has values, the header and the payload of ONE bit-packed run."""
    return sum(1 + (len(_varint((((int(x) + 7) // 8) << 1) | 1)) + W * ((int(x) + 7) // 8) if x else 0) for x in nv)


def dict_pays(d: int, nv, itemsize: int) -> bool:
    """The chunk rule: a chunk of sum(nv) non-null values with d distinct ones is dictionary-encoded
    iff it has values, d <= DICT_MAX_ENTRIES and dictionary + indices are SMALLER than the values."""
    m = sum(int(x) for x in nv)
    return m > 0 and d <= DICT_MAX_ENTRIES and \
        d * itemsize + dict_index_bytes(nv, dict_index_width(d)) < m * itemsize


class DictPages:
    """One dictionary-encoded column chunk, as ``write_row_group`` takes it in the place of the
    values: ``dictionary`` (the d distinct non-null values, ascending, the column's dtype),
    ``packed`` (bytes-like: page p's indices -- the payload of ONE bit-packed run at ``W`` bits, LSB
    first, pad bits 0 -- at ``dict_page_offsets(nv, W)[0][p]``) and ``nv[p]``, the non-null values of
    data page p (the pages are cut where a PLAIN chunk's are).  The device packs them
    (kernels_parquet_dict; tests/pq_dict_reference.py restates the layout).  Like the values,
    ``dictionary`` and ``packed`` may still be in flight when the row group is laid out.
    A string column's chunk: ``entries`` = d and ``dictionary`` the uint8 bytes of the dictionary page,
    the PLAIN BYTE_ARRAY encoding of the d entries; ``page_rows``: the rows per data page of the chunk."""

    __slots__ = ("dictionary", "packed", "W", "nv", "at", "entries", "page_rows")

    def __init__(self, dictionary, packed, W, nv, entries=None, page_rows=None):
        self.dictionary, self.packed, self.W = dictionary, packed, int(W)
        self.nv = [int(x) for x in nv]
        self.entries = int(entries) if entries is not None else None
        self.page_rows = int(page_rows) if page_rows is not None else None   # (None: PAGE_VALUES)
        d = int(np.asarray(dictionary).size) if entries is None else self.entries
        if d < 1 or self.W != dict_index_width(d):
            raise ValueError(f"DictPages: index width {self.W} for a dictionary of {d} entries")
        if entries is not None and not 4 * d <= len(dictionary) <= MAX_PAGE_BYTES:
            raise ValueError(f"DictPages: a dictionary page of {len(dictionary)} bytes for {d} strings")
        self.at, total = dict_page_offsets(self.nv, self.W)
        if len(packed) < total:
            raise ValueError(f"DictPages: {len(packed)} packed bytes, the pages take {total}")

    @property
    def dtype(self):
        return STRING_DTYPE if self.entries is not None else np.asarray(self.dictionary).dtype

    def prologue(self, dt, at):
        """([(offset, bytes-like)] of the dictionary page laid out from ``at``, the offset behind it)."""
        dic = np.asarray(self.dictionary)
        if self.dtype != dt or dic.ndim != 1 or not dic.flags.c_contiguous or \
                (self.entries is not None and dic.dtype != np.uint8):
            raise TypeError(f"PlainParquetWriter: dictionary is {self.dtype}, the file's column is {dt}")
        d, nbytes = (dic.size, dic.size * dt.itemsize) if self.entries is None else (self.entries, dic.size)
        head = _dict_page_header(d, nbytes)
        return [(at, head), (at + len(head), memoryview(dic).cast("B"))], at + len(head) + nbytes

    def indices(self, p, nv):
        """[bytes-like] of data page p's value section: the width byte, then the run."""
        if not 0 <= p < len(self.nv) or self.nv[p] != nv:
            raise ValueError(f"PlainParquetWriter: page {p} has {nv} non-null values, its DictPages say "
                             f"{self.nv[p] if 0 <= p < len(self.nv) else 'nothing'}")
        if nv == 0:
            return [bytes([self.W])]
        groups = (nv + 7) // 8
        return [bytes([self.W]) + _varint((groups << 1) | 1),
                memoryview(self.packed).cast("B")[self.at[p]: self.at[p] + groups * self.W]]


class ByteArrayPages:
    """One PLAIN column chunk of a flat string column, as ``write_row_group`` takes it in the place of
    the values: ``body`` (bytes-like, uint8) holds the value sections of all data pages of the chunk
    -- per non-null value its length as a little-endian u32, then its UTF-8 bytes -- page p's at
    ``body[page_at[p]: page_at[p + 1]]``; ``nv[p]`` is the number of non-null values of page p and
    ``page_rows`` the rows every page but the last holds (``string_page_rows`` of the column's
    longest entry).  The device fills the body (kernels_parquet_str_out; tests/pq_str_out_reference.py
    restates the layout); it may still be in flight when the row group is laid out, the tables not."""

    __slots__ = ("body", "page_at", "nv", "page_rows")

    def __init__(self, body, page_at, nv, page_rows=None):
        self.body, self.page_rows = body, int(page_rows if page_rows is not None else PAGE_VALUES)
        self.page_at = [int(x) for x in page_at]
        self.nv = [int(x) for x in nv]
        if self.page_rows < 1 or len(self.page_at) != len(self.nv) + 1 or len(self.nv) < 1:
            raise ValueError(f"ByteArrayPages: {len(self.page_at)} page starts for {len(self.nv)} pages "
                             f"of {self.page_rows} rows")
        if self.page_at[0] < 0 or self.page_at[-1] > len(body):
            raise ValueError(f"ByteArrayPages: pages at {self.page_at[0]} .. {self.page_at[-1]} of a body of "
                             f"{len(body)} bytes")
        for p, k in enumerate(self.nv):
            size = self.page_at[p + 1] - self.page_at[p]
            if k < 0 or size < 4 * k or (k == 0 and size) or size > MAX_PAGE_BYTES:
                raise ValueError(f"ByteArrayPages: page {p} holds {k} values in {size} bytes")

    @property
    def dtype(self):
        return STRING_DTYPE

    def page(self, p, nv):
        """The value section of data page p (bytes-like)."""
        if not 0 <= p < len(self.nv) or self.nv[p] != nv:
            raise ValueError(f"PlainParquetWriter: page {p} has {nv} non-null values, its ByteArrayPages say "
                             f"{self.nv[p] if 0 <= p < len(self.nv) else 'nothing'}")
        if self.page_at[p + 1] == self.page_at[p]:
            return memoryview(b"")
        return memoryview(self.body).cast("B")[self.page_at[p]: self.page_at[p + 1]]


class BoolPages:
    """One column chunk of a flat bool column, as ``write_row_group`` takes it in the place of the
    values: ``packed`` (bytes-like, uint8) holds the value sections of all data pages of the chunk
    one behind the other -- a page's ``nv`` non-null values one per bit, LSB first, in ceil(nv / 8)
    bytes, the unused high bits of the last byte 0, every page starting at a byte -- and ``nvalues``
    their number.  The pages are cut by rows like any flat column's, so their sizes follow from the
    validity bitmap.  The device packs the bits (kernels_parquet_narrow.bool_pack); ``packed`` may
    still be in flight when the row group is laid out."""

    __slots__ = ("packed", "nvalues")

    def __init__(self, packed, nvalues):
        self.packed, self.nvalues = packed, int(nvalues)
        if self.nvalues < 0 or len(packed) < (self.nvalues + 7) // 8:
            raise ValueError(f"BoolPages: {len(packed)} packed bytes for {self.nvalues} values")

    @property
    def dtype(self):
        return BOOL_DTYPE

    def page(self, at, nv):
        """The value section of a data page of nv values whose bytes start at ``at`` (bytes-like)."""
        size = (nv + 7) // 8
        if at + size > len(self.packed):
            raise ValueError(f"PlainParquetWriter: a page of {nv} values at byte {at} of {len(self.packed)} packed bytes")
        return memoryview(self.packed).cast("B")[at: at + size] if size else memoryview(b"")


def _snappy_literal_tag(n: int) -> bytes:
    """The tag of a snappy literal element of n >= 1 bytes: ``(n - 1) << 2`` up to 60 bytes, else
    ``(59 + k) << 2`` and n - 1 in k little-endian bytes."""
    if n <= 60:
        return bytes([(n - 1) << 2])
    k = ((n - 1).bit_length() + 7) // 8
    return bytes([(59 + k) << 2]) + (n - 1).to_bytes(k, "little")


def flat_level_bytes(rows: int, nulls: bool) -> int:
    """Bytes of the definition levels of a flat page of ``rows`` rows (``_def_levels``)."""
    if not nulls:
        return 4 + len(_varint(rows << 1)) + 1
    groups = (rows + 7) // 8
    return 4 + len(_varint((groups << 1) | 1)) + groups


def list_level_bytes(slots: int) -> int:
    """Bytes of the repetition and definition levels of a list page of ``slots`` slots."""
    return len(_packed_levels(slots, 1)) + len(_packed_levels(slots, 2)) + 3 * ((slots + 7) // 8)


def snappy_chunk_bytes(pages, dictionary=None):
    """(bytes of the chunk written SNAPPY, bytes of the same chunk as it is written today), page
    headers included.  ``pages``: per data page (num_values, literal, raw, elements, encoding) -- the
    bytes of its body that travel inside the literal element (levels, and the indices of a dictionary
    page), the bytes of its values region, the bytes of the region's element stream and 0 (PLAIN) or 8
    (RLE_DICTIONARY).  ``dictionary``: None, or (entries, raw, elements) of the dictionary page."""
    comp = plain = 0
    if dictionary is not None:
        d, raw, el = (int(x) for x in dictionary)
        c = len(_varint(raw)) + el
        comp += len(_dict_page_header(d, raw, c)) + c
        plain += len(_dict_page_header(d, raw)) + raw
    for num_values, literal, raw, el, encoding in pages:
        U = int(literal) + int(raw)
        c = len(_varint(U)) + (len(_snappy_literal_tag(literal)) + literal if literal else 0) + int(el)
        comp += len(_page_header(num_values, U, encoding, c)) + c
        plain += len(_page_header(num_values, U, encoding)) + U
    return comp, plain


def snappy_pays(compressed: int, plain: int) -> bool:
    """The chunk rule of ``device_compression``: a chunk is written SNAPPY iff that form, page headers
    included, is SMALLER than the chunk as it is written today (``snappy_chunk_bytes``).  Applied
    after ``dict_pays``, to whichever form the chunk takes; an incompressible chunk stays as it is."""
    return int(compressed) < int(plain)


class SnappyPages:
    """One SNAPPY column chunk, as ``write_row_group`` takes it in the place of the values.  The
    pages are the pages of the uncompressed chunk; a page body is the snappy raw stream

        varint(U) | ONE literal element { the level bytes as they are written today } | elements

    where the elements are those of the page's values region, made on the device (kernels_snappy;
    tests/snappy_reference.py restates the format).  ``dense`` (bytes-like, uint8) holds the element
    streams of all pages one behind the other, ``sizes[p]`` the bytes of page p's stream and
    ``raw[p]`` the bytes of its values region (a number column: non-null values x item size).
    ``dtype``: the column's (``STRING_DTYPE``: the regions are PLAIN BYTE_ARRAY bodies, and
    ``page_rows`` the rows per page as in ``ByteArrayPages``).
    A dictionary chunk: ``indices`` = (W, packed, nv, entries) as in ``DictPages`` (``entries``: the
    dictionary's), ``dense`` / ``sizes[0]`` / ``raw[0]`` the elements of the dictionary page alone;
    the width byte and the index run of a data page travel inside its literal.
    Like the values, ``dense`` and ``packed`` may still be in flight when the row group is laid out."""

    __slots__ = ("dtype", "dense", "sizes", "raw", "at", "page_rows", "W", "packed", "nv", "idx_at", "entries")

    def __init__(self, dtype, dense, sizes, raw, page_rows=None, indices=None):
        self.dtype = STRING_DTYPE if dtype == STRING_DTYPE else np.dtype(dtype)
        self.dense = dense
        self.sizes, self.raw = [int(x) for x in sizes], [int(x) for x in raw]
        self.page_rows = int(page_rows) if page_rows is not None else None
        if len(self.sizes) != len(self.raw) or len(self.sizes) < 1:
            raise ValueError(f"SnappyPages: {len(self.sizes)} stream sizes for {len(self.raw)} regions")
        if any(c < 0 or u < 0 or (u == 0) != (c == 0) or u > MAX_PAGE_BYTES for c, u in zip(self.sizes, self.raw)):
            raise ValueError("SnappyPages: a page's stream and its region must both be empty or both hold bytes")
        self.at = [0]
        for c in self.sizes:
            self.at.append(self.at[-1] + c)
        if len(dense) < self.at[-1]:
            raise ValueError(f"SnappyPages: {len(dense)} dense bytes, the pages take {self.at[-1]}")
        self.W = self.packed = self.nv = self.idx_at = self.entries = None
        if indices is not None:
            W, packed, nv, entries = indices
            self.W, self.packed, self.nv, self.entries = int(W), packed, [int(x) for x in nv], int(entries)
            if len(self.sizes) != 1 or self.entries < 1 or self.W != dict_index_width(self.entries):
                raise ValueError(f"SnappyPages: index width {self.W} for a dictionary of {self.entries} entries")
            self.idx_at, total = dict_page_offsets(self.nv, self.W)
            if len(packed) < total:
                raise ValueError(f"SnappyPages: {len(packed)} packed bytes, the pages take {total}")

    def indices(self, p, nv):
        """[bytes-like] of data page p's value section of a dictionary chunk: the width byte, then the run."""
        if not 0 <= p < len(self.nv) or self.nv[p] != nv:
            raise ValueError(f"PlainParquetWriter: page {p} has {nv} non-null values, its SnappyPages say "
                             f"{self.nv[p] if 0 <= p < len(self.nv) else 'nothing'}")
        if nv == 0:
            return [bytes([self.W])]
        groups = (nv + 7) // 8
        return [bytes([self.W]) + _varint((groups << 1) | 1),
                memoryview(self.packed).cast("B")[self.idx_at[p]: self.idx_at[p] + groups * self.W]]


class PlainParquetWriter:
    """One parquet file of int32 / int64 / float32 / float64 columns, flat or "list of" such leaves,
    flat int8 / int16 columns (their values passed as int32) and bool columns (``BoolPages``),
    and flat string columns (``STRING_DTYPE``: BYTE_ARRAY annotated UTF8 / STRING),
    every column OPTIONAL (like pyarrow writes nullable Arrow columns), PLAIN encoding, no
    compression.  A list column is the standard three-level list (optional group ``name`` (LIST) >
    repeated group ``list`` > optional ``element``); there are no null lists.

    With a thread ``pool`` a row group is written by a pool task: a PLAIN page's size is known
    before it is written, so the row group is laid out first and its pages go to their offsets
    with ``os.pwrite`` (which releases the GIL) while the caller stages the next row group or
    another file."""

    def __init__(self, path: str, names: Sequence[str], dtypes: Sequence, pool=None, logical=None, lists=None):
        """``logical[j]``: None, or datetime64[ms|us|ns] for an int64 column of such counts.
        ``lists[j]``: True for a list column whose leaves are ``dtypes[j]``."""
        self.path = path
        self.names = list(names)
        self.dtypes = [np.dtype(d) for d in dtypes]
        for d in self.dtypes:
            if d not in _PQ_TYPE and d != STRING_DTYPE and d != BOOL_DTYPE and d not in _NARROW:
                raise TypeError(f"PlainParquetWriter: unsupported dtype {d}")
        self.physical = [physical_dtype(d) for d in self.dtypes]   # what the columns' buffers hold
        self.logical = [np.dtype(x) if x is not None else None for x in (logical or [None] * len(self.names))]
        for d, x in zip(self.dtypes, self.logical):
            if x is not None and (timestamp_unit(x) is None or d != np.dtype("int64")):
                raise TypeError(f"PlainParquetWriter: logical type {x} on a {d} column (int64 counts in ms, us or ns)")
        self.lists = [bool(x) for x in (lists or [False] * len(self.names))]
        if len(self.lists) != len(self.names):
            raise ValueError("PlainParquetWriter: names and lists differ in length")
        if any(l and x is not None for l, x in zip(self.lists, self.logical)):
            raise TypeError("PlainParquetWriter: list columns of datetime leaves are not written")
        if any(l and d == STRING_DTYPE for l, d in zip(self.lists, self.dtypes)):
            raise TypeError("PlainParquetWriter: list columns of strings are not written")
        if any(l and (d == BOOL_DTYPE or d in _NARROW) for l, d in zip(self.lists, self.dtypes)):
            raise TypeError("PlainParquetWriter: list columns of bool / int8 / int16 leaves are not written")
        self.fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.pwrite(self.fd, b"PAR1", 0)
        self.pos = 4
        self.pool = pool
        self.row_groups: List[bytes] = []
        self.num_rows = 0
        self.pending = []

    def _plan_column(self, values, valid, n, dt, start):
        """[(offset, bytes-like)] of one column chunk laid out from `start`, its size and the
        offset of its first data page."""
        if isinstance(values, DictPages):
            return self._plan_dict_column(values, valid, n, dt, start)
        if isinstance(values, BoolPages) or dt == BOOL_DTYPE:
            return self._plan_bool_column(values, valid, n, dt, start)
        bp = values if isinstance(values, ByteArrayPages) else None
        if (bp is not None) != (dt == STRING_DTYPE):
            raise TypeError(f"PlainParquetWriter: column buffer is {getattr(values, 'dtype', type(values))}, "
                            f"the file's column is {'string' if dt == STRING_DTYPE else dt}")
        values = np.asarray(values) if bp is None else None
        if bp is None and (values.dtype != dt or not values.flags.c_contiguous):
            # never cast here: the buffer may still be the target of an asynchronous device-to-host
            # copy (`ready`), and a silent cast would hide a schema change between row groups
            raise TypeError(f"PlainParquetWriter: column buffer is {values.dtype} "
                            f"(contiguous={values.flags.c_contiguous}), the file's column is {dt}")
        vbytes = memoryview(values).cast("B") if (bp is None and values.size) else memoryview(b"")
        segs, at = [], start
        done_vals = 0
        for p, (rows, page_valid, nv) in enumerate(_flat_pages(valid, n, PAGE_VALUES if bp is None else bp.page_rows)):
            prefix, bitmap = _def_levels(rows, page_valid)
            payload = vbytes[done_vals * dt.itemsize: (done_vals + nv) * dt.itemsize] if bp is None else bp.page(p, nv)
            body = len(prefix) + (len(bitmap) if bitmap is not None else 0) + len(payload)
            head = _page_header(rows, body) + prefix
            segs.append((at, head))
            at += len(head)
            if bitmap is not None and len(bitmap):
                segs.append((at, bitmap))
                at += len(bitmap)
            if len(payload):
                segs.append((at, payload))
                at += len(payload)
            done_vals += nv
        if bp is not None and p + 1 != len(bp.nv):
            raise ValueError(f"PlainParquetWriter: {p + 1} data pages, the ByteArrayPages hold {len(bp.nv)}")
        if bp is None and done_vals != values.size:
            raise ValueError("PlainParquetWriter: the values do not match the validity bitmap "
                             f"({values.size} values, {done_vals} valid rows)")
        return segs, at - start, start

    def _plan_bool_column(self, bp, valid, n, dt, start):
        """A flat bool chunk: page = header | def levels | ceil(nv / 8) bytes of bits."""
        if not isinstance(bp, BoolPages) or dt != BOOL_DTYPE:
            raise TypeError(f"PlainParquetWriter: column buffer is {getattr(bp, 'dtype', type(bp))}, "
                            f"the file's column is {dt}")
        segs, at, byte_at, done_vals = [], start, 0, 0
        for rows, page_valid, nv in _flat_pages(valid, n, PAGE_VALUES):
            prefix, bitmap = _def_levels(rows, page_valid)
            payload = bp.page(byte_at, nv)
            body = len(prefix) + (len(bitmap) if bitmap is not None else 0) + len(payload)
            for buf in (_page_header(rows, body) + prefix, bitmap, payload):
                if buf is not None and len(buf):
                    segs.append((at, buf))
                    at += len(buf)
            byte_at += len(payload)
            done_vals += nv
        if done_vals != bp.nvalues:
            raise ValueError("PlainParquetWriter: the values do not match the validity bitmap "
                             f"({bp.nvalues} values, {done_vals} valid rows)")
        return segs, at - start, start

    def _plan_dict_column(self, dp, valid, n, dt, start):
        """A flat chunk of dictionary pages: dictionary page | data pages (header | def levels | W | run)."""
        segs, at = dp.prologue(dt, start)
        first = at
        p = 0
        for rows, page_valid, nv in _flat_pages(valid, n, dp.page_rows or PAGE_VALUES):
            prefix, bitmap = _def_levels(rows, page_valid)
            bufs = [bitmap] + dp.indices(p, nv)
            body = len(prefix) + sum(len(b) for b in bufs if b is not None)
            for buf in [_page_header(rows, body, 8) + prefix] + bufs:
                if buf is not None and len(buf):
                    segs.append((at, buf))
                    at += len(buf)
            p += 1
        if p != len(dp.nv):
            raise ValueError(f"PlainParquetWriter: {p} data pages, the DictPages hold {len(dp.nv)}")
        return segs, at - start, first

    def _plan_list_column(self, values, levels, dt, start):
        """The same for a list column: page = header | rep levels | def levels | non-null leaves
        (a DictPages in the place of the values: ... | W | run of indices)."""
        dp = values if isinstance(values, DictPages) else None
        values = np.asarray(values if dp is None else dp.dictionary)
        if values.dtype != dt or values.ndim != 1 or not values.flags.c_contiguous:
            raise TypeError(f"PlainParquetWriter: leaf buffer is {values.dtype} "
                            f"(contiguous={values.flags.c_contiguous}), the file's column is list of {dt}")
        vbytes = memoryview(values).cast("B") if values.size else memoryview(b"")
        npages = len(levels.slots)
        if not (len(levels.nonnull) == len(levels.rep_at) == len(levels.def_at) == npages):
            raise ValueError("PlainParquetWriter: the page table's columns differ in length")
        segs, at, done_vals = [], start, 0
        if dp is not None:
            segs, at = dp.prologue(dt, start)
            if len(dp.nv) != npages:
                raise ValueError(f"PlainParquetWriter: {npages} data pages, the DictPages hold {len(dp.nv)}")
        first = at
        for p, (slots, lev, nv) in enumerate(self._list_page_levels(levels)):
            payload = [vbytes[done_vals * dt.itemsize: (done_vals + nv) * dt.itemsize]] if dp is None else \
                dp.indices(p, nv)
            body = sum(len(b) for b in lev) + sum(len(b) for b in payload)
            for buf in [_page_header(slots, body, 0 if dp is None else 8) + lev[0]] + lev[1:] + payload:
                if len(buf):
                    segs.append((at, buf))
                    at += len(buf)
            done_vals += nv
        if npages == 0:
            # no rows: one page without slots (both level streams an RLE run of length 0)
            empty = _varint(0) + b"\x00"
            body = 2 * (struct.pack("<I", len(empty)) + empty)
            segs.append((at, _page_header(0, len(body)) + body))
            at += len(segs[-1][1])
        if dp is None and done_vals != values.size:
            raise ValueError("PlainParquetWriter: the values do not match the page table "
                             f"({values.size} values, {done_vals} non-null leaves)")
        return segs, at - start, first

    @staticmethod
    def _list_page_levels(levels):
        """(slots, [level buffers], non-null leaves) of every page of a list chunk, as
        ``_plan_list_column`` lays them out."""
        rep = memoryview(levels.rep).cast("B") if len(levels.rep) else memoryview(b"")
        dfn = memoryview(levels.dfn).cast("B") if len(levels.dfn) else memoryview(b"")
        npages = len(levels.slots)
        if not (len(levels.nonnull) == len(levels.rep_at) == len(levels.def_at) == npages):
            raise ValueError("PlainParquetWriter: the page table's columns differ in length")
        for p in range(npages):
            slots, nv = levels.slots[p], levels.nonnull[p]
            groups = (slots + 7) // 8
            r0, d0 = levels.rep_at[p], levels.def_at[p]
            if slots <= 0 or not 0 <= nv <= slots:
                raise ValueError(f"PlainParquetWriter: page {p} has {slots} slots and {nv} non-null leaves")
            if r0 < 0 or d0 < 0 or r0 + groups > len(rep) or d0 + 2 * groups > len(dfn):
                raise ValueError(f"PlainParquetWriter: the level bytes do not match the page table (page {p}: "
                                 f"{slots} slots at {r0} of {len(rep)} rep bytes, at {d0} of {len(dfn)} def bytes)")
            yield slots, [_packed_levels(slots, 1), rep[r0: r0 + groups], _packed_levels(slots, 2),
                          dfn[d0: d0 + 2 * groups]], nv

    def _plan_snappy_column(self, sp, valid, n, dt, start, is_list):
        """A SNAPPY chunk, flat or list: the pages of the uncompressed chunk, every body the raw stream
        varint(U) | literal { levels (dictionary chunk: and W | run) } | the region's elements.
        -> (segments, bytes written, offset of the first data page of a dictionary chunk or None, the
        bytes the chunk takes uncompressed, its non-null values)."""
        if sp.dtype != dt:
            raise TypeError(f"PlainParquetWriter: SnappyPages of {sp.dtype}, the file's column is "
                            f"{'string' if dt == STRING_DTYPE else dt}")
        dense = memoryview(sp.dense).cast("B") if len(sp.dense) else memoryview(b"")
        segs, at, raw_size, first = [], start, 0, None
        if sp.W is not None:
            U, c = sp.raw[0], sp.sizes[0]
            pre = _varint(U)
            for buf in (_dict_page_header(sp.entries, U, len(pre) + c) + pre, dense[:c]):
                segs.append((at, buf))
                at += len(buf)
            raw_size += len(_dict_page_header(sp.entries, U)) + U
            first = at
        if is_list:
            pages = self._list_page_levels(valid)
        else:
            pages = ((rows, list(_def_levels(rows, page_valid)), nv)
                     for rows, page_valid, nv in _flat_pages(valid, n, sp.page_rows or PAGE_VALUES))
        p = nvalid = 0
        for num_values, literal, nv in pages:
            if sp.W is None:
                if p >= len(sp.sizes):
                    raise ValueError(f"PlainParquetWriter: more than the {len(sp.sizes)} data pages the SnappyPages hold")
                region, elements = sp.raw[p], dense[sp.at[p]: sp.at[p + 1]]
                if (region != nv * dt.itemsize) if dt != STRING_DTYPE else (region < 4 * nv or (nv == 0 and region)):
                    raise ValueError(f"PlainParquetWriter: page {p} has {nv} non-null values, its SnappyPages "
                                     f"hold a region of {region} bytes")
            else:
                literal = literal + sp.indices(p, nv)
                region, elements = 0, memoryview(b"")
            literal = [b for b in literal if b is not None and len(b)]
            L = sum(len(b) for b in literal)
            U = L + region
            pre = _varint(U) + (_snappy_literal_tag(L) if L else b"")
            head = _page_header(num_values, U, 0 if sp.W is None else 8, len(pre) + L + len(elements)) + pre
            for buf in [head] + literal + [elements]:
                if len(buf):
                    segs.append((at, buf))
                    at += len(buf)
            raw_size += len(_page_header(num_values, U, 0 if sp.W is None else 8)) + U
            nvalid += nv
            p += 1
        if p != (len(sp.nv) if sp.W is not None else len(sp.sizes)):
            raise ValueError(f"PlainParquetWriter: {p} data pages, the SnappyPages hold "
                             f"{len(sp.nv) if sp.W is not None else len(sp.sizes)}")
        return segs, at - start, first, raw_size, nvalid

    def _run(self, segs, ready=None):
        if ready is not None:
            ready()   # (e.g. the event behind the device-to-host copy of these buffers)
        for off, buf in segs:
            mv = memoryview(buf)
            while len(mv):          # (pwrite may write less than asked for)
                k = os.pwrite(self.fd, mv, off)
                mv, off = mv[k:], off + k

    def write_row_group(self, columns, n: int, wait: bool = True, ready=None, stats=None):
        """columns[j] = (values, valid): `values` a 1-D numpy array of the column's dtype holding
        the NON-NULL values in row order, `valid` None or the Arrow validity bitmap (uint8, LSB
        first, >= ceil(n / 8) bytes) of the n rows.  A list column: (values, levels) with the
        non-null LEAVES of the n rows in order and their ``ListLevels``.  A string column: a
        ``ByteArrayPages`` in the place of ``values``, a bool column: a ``BoolPages``; an int8 / int16
        column: its values sign-extended to int32.  A dictionary-encoded chunk
        (of any kind): a ``DictPages`` in the place of ``values``.  A SNAPPY chunk (of any kind, also
        a dictionary chunk): a ``SnappyPages`` in the place of ``values``.  Argument errors raise
        before anything of the row group is written.  wait=False (with a pool): returns the
        futures of the column writes instead of waiting for them -- the layout is fixed, so later
        row groups (of this or of other files) can be written meanwhile; the caller keeps the
        buffers alive until the futures are done, close() waits for whatever is left.
        ready: called by every column task before it touches its buffers (the VALUES may still
        be in flight when this returns; validity bitmaps must be complete: pages are laid out
        from their popcounts).
        stats[j]: None, or a 2-element numpy array of the column's dtype that holds {min, max} of
        the non-null values by the time close() runs (it may still be in flight now): written as
        the chunk's min / max statistics (NaN / empty chunks: omitted; string columns take None:
        they get no min / max).  The null count of every chunk is always written."""
        chunks, plans = [], []
        total = 0
        if len(columns) != len(self.names):
            raise ValueError(f"PlainParquetWriter: {len(columns)} columns for a file of {len(self.names)}")
        pos = self.pos
        for j, ((values, valid), name, dt) in enumerate(zip(columns, self.names, self.physical)):
            start = pos
            if self.lists[j] != isinstance(valid, ListLevels):
                raise TypeError(f"PlainParquetWriter: column '{name}' is a {'list' if self.lists[j] else 'flat'} "
                                f"column of the file, this row group passes it as the other kind")
            raw_size = None
            if isinstance(values, SnappyPages):
                segs, size, first, raw_size, nvalid = self._plan_snappy_column(values, valid, n, dt, start, self.lists[j])
                nv = sum(valid.slots) if self.lists[j] else n
            elif self.lists[j]:
                segs, size, first = self._plan_list_column(values, valid, dt, start)
                nv = sum(valid.slots)   # (num_values of a list chunk counts slots, not leaves or rows)
            else:
                segs, size, first = self._plan_column(values, valid, n, dt, start)
                nv = n
            plans.append(segs)
            pos += size
            is_dict = isinstance(values, DictPages) or (raw_size is not None and values.W is not None)
            if raw_size is None:
                nvalid = sum(values.nv) if isinstance(values, (DictPages, ByteArrayPages)) else \
                    values.nvalues if isinstance(values, BoolPages) else int(np.asarray(values).size)
            chunks.append(dict(name=name, dt=dt, n=nv, size=size, start=start, nulls=nv - nvalid,
                               minmax=stats[j] if (stats is not None and nvalid > 0) else None,
                               is_list=self.lists[j], first_data=first if is_dict else None,
                               raw_size=size if raw_size is None else raw_size, codec=0 if raw_size is None else 1))
            total += chunks[-1]["raw_size"]   # (a row group's total_byte_size counts uncompressed bytes)
        self.pos = pos
        futures = []
        if self.pool is not None:
            # ONE task per row group: buffered writes to one file serialise on its inode lock
            # (11 GB/s on the GPU box whatever the thread count, tools/write_probe.py), so
            # threads are spent on DIFFERENT files (6 files: 58 GB/s), not on one file's columns
            futures = [self.pool.submit(self._run, [sg for segs in plans for sg in segs], ready)]
            if wait:
                for f in futures:
                    f.result()
                futures = []
            else:
                self.pending += futures
        else:
            for segs in plans:
                self._run(segs, ready)
        self.row_groups.append((chunks, total, n))   # (thrift structs are built by close(): statistics)
        self.num_rows += n
        return futures

    @staticmethod
    def _chunk_struct(c) -> bytes:
        dt, name = c["dt"], c["name"]
        st = _Struct()
        mm = c["minmax"]
        lo = hi = None
        if mm is not None:
            mm = np.asarray(mm)
            if mm.dtype == dt and mm.size == 2 and not (mm.dtype.kind == "f" and not np.isfinite(mm).all()):
                lo, hi = mm[0:1].tobytes(), mm[1:2].tobytes()
        if hi is not None:
            st.binary(1, hi).binary(2, lo)               # (deprecated pair: signed order, same bytes)
        st.i64(3, c["nulls"])
        if hi is not None:
            st.binary(5, hi).binary(6, lo)               # max_value / min_value
        path = [name, "list", "element"] if c.get("is_list") else [name]
        # a dictionary chunk: encodings PLAIN, RLE, RLE_DICTIONARY; data_page_offset (9) is its first
        # data page, dictionary_page_offset (11) the chunk's start; the sizes include the dictionary
        first = c.get("first_data")
        meta = (_Struct().i32(1, _ptype(dt))
                .list(2, _CT_I32, [_zigzag(0), _zigzag(3)] + ([_zigzag(8)] if first is not None else []))
                .list(3, _CT_BINARY, [_varint(len(x.encode())) + x.encode() for x in path])
                .i32(4, c.get("codec", 0)).i64(5, c["n"]).i64(6, c.get("raw_size", c["size"])).i64(7, c["size"])
                .i64(9, c["start"] if first is None else first))
        if first is not None:
            meta.i64(11, c["start"])
        meta = meta.struct(12, st.done()).done()
        return _Struct().i64(2, c["start"]).struct(3, meta).done()

    def close(self):
        for f in self.pending:
            f.result()
        self.pending = []
        schema = [_Struct().binary(4, "schema").i32(5, len(self.names)).done()]
        for name, dt, logical, is_list in zip(self.names, self.dtypes, self.logical, self.lists):
            if is_list:
                # optional group <name> (LIST) { repeated group list { optional <T> element } }
                schema.append(_Struct().i32(3, 1).binary(4, name).i32(5, 1).i32(6, 3)
                              .struct(10, _Struct().struct(3, _Struct().done()).done()).done())
                schema.append(_Struct().i32(3, 2).binary(4, "list").i32(5, 1).done())
                schema.append(_Struct().i32(1, _PQ_TYPE[dt]).i32(3, 1).binary(4, "element").done())
                continue
            el = _Struct().i32(1, _ptype(physical_dtype(dt))).i32(3, 1).binary(4, name)
            if dt == STRING_DTYPE:
                # BYTE_ARRAY, converted type UTF8 (0), LogicalType STRING (union field 1, an empty struct)
                el.i32(6, 0).struct(10, _Struct().struct(1, _Struct().done()).done())
            if dt in _NARROW:
                # INT32, converted type INT_8 / INT_16, LogicalType INTEGER (union field 10) {bitWidth, isSigned}
                bits, conv = _NARROW[dt]
                el.i32(6, conv).struct(10, _Struct().struct(10, _Struct().byte(1, bits).bool(2, True).done()).done())
            if logical is not None:
                field, conv = _TS_UNIT[timestamp_unit(logical)]
                if conv is not None:
                    el.i32(6, conv)
                unit = _Struct().struct(field, _Struct().done()).done()
                el.struct(10, _Struct().struct(8, _Struct().bool(1, False).struct(2, unit).done()).done())
            schema.append(el.done())
        groups = [_Struct().list(1, _CT_STRUCT, [self._chunk_struct(c) for c in chunks]).i64(2, total).i64(3, n).done()
                  for chunks, total, n in self.row_groups]
        # column_orders: TYPE_ORDER for every column (min_value / max_value are only defined with it)
        type_order = _Struct().struct(1, _Struct().done()).done()
        footer = (_Struct().i32(1, 1).list(2, _CT_STRUCT, schema).i64(3, self.num_rows)
                  .list(4, _CT_STRUCT, groups)
                  .binary(6, "nvtabular_amd plain writer")
                  .list(7, _CT_STRUCT, [type_order] * len(self.names)).done())
        self._run([(self.pos, footer + struct.pack("<I", len(footer)) + b"PAR1")])
        os.close(self.fd)
        self.fd = -1

    def abort(self):
        """A failed write: wait for what is in flight, close the descriptor and remove the
        footer-less file (a truncated part file must not be left behind as if it were output)."""
        for f in self.pending:
            try:
                f.result()
            except Exception:
                pass
        self.pending = []
        if self.fd >= 0:
            os.close(self.fd)
            self.fd = -1
        try:
            os.unlink(self.path)
        except OSError:
            pass


# ================================================================================================
# reading side: footer (thrift compact FileMetaData) + column chunks of PLAIN / uncompressed pages
# ================================================================================================
_PQ_NP = {1: np.dtype("int32"), 2: np.dtype("int64"), 4: np.dtype("float32"), 5: np.dtype("float64")}


def _judge_leaf(e, narrow=False):
    """(dtype, unit, reason or None) of a primitive SchemaElement (1 physical type, 3 repetition
    {0 required, 1 optional, 2 repeated}, 4 name, 6 converted type, 10 LogicalType): the rule for
    flat columns (``narrow``: bool / int8 / int16 too) and for list leaves.  ``unit``: "ms" / "us" /
    "ns" of an INT64 TIMESTAMP."""
    ptype, conv, logical = e.get(1), e.get(6), e.get(10)
    dt, who = _PQ_NP.get(ptype), f"column {e.get(4)!r}"
    # an INT64 TIMESTAMP (LogicalType union field 8 {1: isAdjustedToUTC, 2: unit}, or the
    # converted types 9 TIMESTAMP_MILLIS / 10 TIMESTAMP_MICROS of legacy writers) keeps its
    # bits: the counts are taken as they are and the unit is recorded
    unit = None
    if ptype == 2 and isinstance(logical, dict) and len(logical) == 1 and isinstance(logical.get(8), dict):
        tu = logical[8].get(2)
        unit = _TS_BY_FIELD.get(next(iter(tu))) if isinstance(tu, dict) and len(tu) == 1 else None
        if unit is not None and conv not in (None, _TS_UNIT[unit][1]):
            unit = None
    elif ptype == 2 and logical is None and conv in (9, 10):
        unit = "ms" if conv == 9 else "us"
    if unit is not None:
        conv = logical = None
    # the most specific annotation is the one reported.  LogicalType union: 10 = INTEGER
    # {1: bitWidth, 2: isSigned}.  Converted types that reinterpret the integer: DATE 6, TIME 7-8,
    # TIMESTAMP 9-10, UINT 11-14, DECIMAL 5; INT_8 / INT_16 (15 / 16) on a physical INT32 come back
    # as int8 / int16 from pyarrow (legacy writers without a LogicalType): only INT_32 (17) on INT32
    # and INT_64 (18) on INT64 keep dtype AND bits -- the same rule as for the LogicalType INTEGER;
    # everything else is left to the pyarrow reader
    integer = logical.get(10) if isinstance(logical, dict) else None
    if narrow:
        # a FLAT column may also be a BOOLEAN without an annotation (bool) or an INT32 annotated
        # INTEGER{8 | 16, signed} and / or with the legacy converted type INT_8 / INT_16 alone
        # (int8 / int16: the values are staged as int32 and narrowed on the device)
        if ptype == 0 and conv is None and logical is None and e.get(3, 0) != 2:
            return BOOL_DTYPE, None, None
        for ndt, (bits, nconv) in _NARROW.items():
            by_logical = (integer is not None and len(logical) == 1 and integer.get(1, 0) == bits and
                          integer.get(2, False) is True)
            if ptype == 1 and e.get(3, 0) != 2 and conv in ((None, nconv) if by_logical else (nconv,)) and \
                    (by_logical or logical is None):
                return ndt, None, None
    if logical is not None and not (integer is not None and integer.get(2, True) and len(logical) == 1 and
                                    integer.get(1, 0) == (32 if ptype == 1 else 64)):
        return dt, unit, f"{who}: logical type {logical}"
    if conv is not None and conv != {1: 17, 2: 18}.get(ptype):
        return dt, unit, f"{who}: converted type {conv}"
    if dt is None or e.get(3, 0) == 2:
        return dt, unit, f"{who}: physical type {ptype} / repetition {e.get(3, 0)}"
    return dt, unit, None


def _is_string_leaf(e):
    """A BYTE_ARRAY (physical type 6) annotated as a string: converted type UTF8 (0) and / or the
    LogicalType STRING (union field 1) -- what pyarrow writes for ``string`` and ``large_string``.
    Plain binary (no annotation), JSON / BSON / ENUM / DECIMAL byte arrays are not."""
    conv, logical = e.get(6), e.get(10)
    if e.get(1) != 6:
        return False
    if logical is not None:
        return isinstance(logical, dict) and list(logical) == [1] and conv in (None, 0)
    return conv == 0


def _judge_column(schema, at):
    """(``columns`` entry, reason or None) of the top-level column whose subtree starts at
    schema[at]: a flat number column, a flat string column, or the standard three-level list of
    number leaves."""
    e = schema[at]
    name, logical = e.get(4, b"").decode(), e.get(10)
    col = dict(name=name, kind="flat", outer_optional=False, elem_optional=False, max_def=0, leaf_level=0,
               leaf_dtype=None, unit=None)
    if not e.get(5) and _is_string_leaf(e):
        col.update(kind="string", outer_optional=e.get(3, 0) == 1, max_def=0 if e.get(3, 0) == 0 else 1)
        return col, (f"column {name!r}: a repeated string" if e.get(3, 0) == 2 else None)
    if not e.get(5):
        dt, unit, why = _judge_leaf(e, narrow=True)
        col.update(outer_optional=e.get(3, 0) == 1, max_def=0 if e.get(3, 0) == 0 else 1, leaf_dtype=dt, unit=unit)
        return col, why
    col["kind"] = "list"
    mid = schema[at + 1] if at + 1 < len(schema) else {}
    leaf = schema[at + 2] if at + 2 < len(schema) else {}
    if not (e.get(6) == 3 or (isinstance(logical, dict) and 3 in logical)):
        kind = "map" if (e.get(6) in (1, 2) or (isinstance(logical, dict) and 2 in logical)) else "struct"
        return col, f"column {name!r}: a {kind}"
    if e.get(3, 0) == 2 or int(e.get(5)) != 1 or mid.get(3, 0) != 2:
        return col, f"column {name!r}: not the standard three-level list"
    if not mid.get(5):
        return col, f"column {name!r}: legacy two-level list (a repeated primitive)"
    if int(mid.get(5)) != 1 or leaf.get(5):
        return col, f"column {name!r}: list of lists or of structs"
    if leaf.get(3, 0) == 2:
        return col, f"column {name!r}: a repeated leaf"
    dt, unit, why = _judge_leaf(leaf)
    if why is not None:
        return col, f"column {name!r}: list leaves: {why}"
    if unit is not None:
        return col, f"column {name!r}: list of TIMESTAMP leaves"
    O, E = int(e.get(3, 0) == 1), int(leaf.get(3, 0) == 1)
    col.update(outer_optional=bool(O), elem_optional=bool(E), max_def=O + 1 + E, leaf_level=O + 1, leaf_dtype=dt)
    return col, None


def _judge_chunk(cc, col, file_size):
    """(row_groups[g]["columns"] entry, reason or None) of one ColumnChunk that stands where
    top-level column ``col`` (None: there is no such column) has its chunk."""
    md = cc.get(3) or {}
    enc = set(md.get(2, []))
    first = int(md.get(9, 0))   # (the chunk starts at its dictionary page when it has one)
    dpo = md.get(11)
    if dpo is not None and 0 < int(dpo) < first:
        first = int(dpo)
    path = [x.decode() for x in md.get(3, [])]
    c = dict(offset=first, size=int(md.get(7, 0)), num_values=int(md.get(5, 0)), codec=int(md.get(4, 0)),
             raw_size=int(md.get(6, 0)), dictionary=bool(dpo is not None or (enc & {2, 8})), path=path)
    # codec 0 UNCOMPRESSED / 1 SNAPPY; encodings PLAIN 0, PLAIN_DICTIONARY 2, RLE 3, BIT_PACKED 4,
    # RLE_DICTIONARY 8 (nvt_pq_decode_chunk_codec)
    if not (md.get(4) in (0, 1) and enc <= {0, 2, 3, 4, 8} and cc.get(1) in (None, b"")):
        return c, f"chunk of {md.get(3)}: codec {md.get(4)}, encodings {sorted(enc)}"
    if len(path) > 1 and 4 in enc:
        return c, f"chunk of {md.get(3)}: BIT_PACKED level streams"
    if not (0 <= c["offset"] and 0 <= c["size"] and c["offset"] + c["size"] <= file_size):
        return c, f"chunk of {md.get(3)} lies outside the file"
    # the chunks follow the top-level columns, a list chunk's path has three parts
    if col is None or path[:1] != [col["name"]] or len(path) != (3 if col["kind"] == "list" else 1):
        return c, "column chunks do not follow the schema order"
    if col["kind"] == "string" and not 0 <= c["raw_size"] < (1 << 32):
        return c, f"chunk of {md.get(3)}: {c['raw_size']} uncompressed bytes"
    return c, None


class PlainParquetFile:
    """Footer of one parquet file and the verdict on whether the hand-written reader takes it.
    ``decodable``: every top-level column is a flat column (physical type INT32 / INT64 / FLOAT /
    DOUBLE without a converted / logical type that changes the meaning of the bits: dates, decimals,
    unsigned; BOOLEAN, and INT32 annotated INTEGER{8 | 16, signed} or INT_8 / INT_16: bool / int8 /
    int16), a flat string column (BYTE_ARRAY annotated UTF8 / STRING, ``kind`` "string": DESIGN.md,
    "String columns in the parquet reader") or the standard three-level list of such number leaves (a group annotated LIST, optional or
    required, holding one repeated group, holding one primitive leaf, optional or required; the two
    inner names are not looked at), and every column chunk follows its column, with codec
    UNCOMPRESSED or SNAPPY, values PLAIN or dictionary-encoded (what pandas / pyarrow / cuDF write by
    default), encodings within {PLAIN, PLAIN_DICTIONARY, RLE, BIT_PACKED, RLE_DICTIONARY} and no
    BIT_PACKED levels on a list chunk.  Otherwise ``why_pyarrow`` is the FIRST thing found that keeps
    the file with pyarrow (legacy two-level lists, lists of lists, maps, structs, binary / fixed-length
    binary columns, string / bool / narrow / TIMESTAMP list leaves, DELTA encodings, other codecs).
    ``readable`` / ``why_not`` keep the meaning they had before the reader knew strings: decodable
    AND no string column (number columns and lists of numbers only); a string column is their first
    reason like any other.  The reader goes by ``decodable``.
    ``eligible``: readable and all columns flat number columns.
    ``columns[j]`` describes top-level column j: ``kind`` ("flat" / "string" / "list"), ``outer_optional``,
    ``elem_optional``, ``max_def`` (lists: O + 1 + E), ``leaf_level`` (O + 1), ``leaf_dtype`` and
    ``unit``; ``names`` / ``dtypes`` / ``max_def`` / ``units`` are the same per top-level column."""

    def __init__(self, path: str):
        self.path = path
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            if size < 12:
                raise ValueError(f"{path}: not a parquet file")
            f.seek(size - 8)
            tail = f.read(8)
            if tail[4:] != b"PAR1":
                raise ValueError(f"{path}: no parquet magic")
            flen = struct.unpack("<I", tail[:4])[0]
            f.seek(size - 8 - flen)
            meta = _TReader(f.read(flen)).struct()
        schema = meta.get(2, [])
        self.num_rows = int(meta.get(3, 0))
        self.readable, self.why_not, self.columns = True, "", []
        self.decodable, self.why_pyarrow = True, ""

        def behind(i, depth=0):   # index behind the subtree at i of the depth-first schema list
            kids = int(schema[i].get(5) or 0) if (i < len(schema) and depth < 64) else 0
            i += 1
            for _ in range(kids):
                i = behind(i, depth + 1)
            return i

        at = 1
        for _ in range(int(schema[0].get(5, 0)) if schema else 0):
            if at >= len(schema):
                self._fail("schema shorter than its root says")
                break
            col, why = _judge_column(schema, at)
            self.columns.append(col)
            self._fail(why)
            if col["kind"] == "string":
                self._fail(f"column {col['name']!r}: a string column", strings=True)
            at = behind(at)
        else:   # (every column was there)
            self._fail("schema longer than its root says" if at != len(schema) else None)
        self.names = [c["name"] for c in self.columns]
        self.dtypes = [c["leaf_dtype"] for c in self.columns]
        self.max_def = [c["max_def"] for c in self.columns]
        self.units = [c["unit"] for c in self.columns]
        self.row_groups = []
        for rg in meta.get(4, []):
            cols = []
            for j, cc in enumerate(rg.get(1, [])):
                c, why = _judge_chunk(cc, self.columns[j] if j < len(self.columns) else None, size)
                cols.append(c)
                self._fail(why)
            if len(cols) != len(self.columns):
                self._fail("column chunks do not follow the schema order")
            self.row_groups.append(dict(num_rows=int(rg.get(3, 0)), columns=cols))

    def _fail(self, why, strings=False):
        """strings: a reason that keeps the file from ``readable`` only (the reader takes it)."""
        if why is not None and self.readable:   # (the first reason stays)
            self.readable, self.why_not = False, why
        if why is not None and self.decodable and not strings:
            self.decodable, self.why_pyarrow = False, why

    @property
    def eligible(self):
        return self.readable and all(c["kind"] == "flat" for c in self.columns)

    @property
    def why(self):
        """What keeps the file from being ``eligible``."""
        return self.why_not or next((f"column {c['name']!r}: a list column" for c in self.columns
                                     if c["kind"] == "list"), "")

    @property
    def num_row_groups(self):
        return len(self.row_groups)


class StagedColumn:
    """One column of a partition in pinned host memory: packed (non-null) values + validity
    bitmap, as nvt_pq_decode_chunk leaves them.

    A list column (``rep`` is not None) is staged as nvt_pq_decode_list_chunk leaves it: ``values``
    the ``nvalid`` non-null LEAVES, ``rep`` / ``dfn`` the level streams of its ``slots`` slots (1 and
    ``width`` bits per slot, continuous over the partition), ``leaves`` the leaf slots among them,
    ``leaf_level`` / ``max_def`` the level arithmetic; ``rows`` stays the row count.  ``same_as``: the
    name of an earlier list column of the partition whose level streams are byte-equal (they share
    one unpack and one offsets tensor on the device), else None.

    A string column (``strs`` is not None) has no ``values``: ``strs`` (StagedStrings) holds its
    entries, run table and packed index bytes, ``nvalid`` counts its non-null rows."""

    __slots__ = ("values", "valid", "rows", "nvalid", "dtype", "logical", "rep", "dfn", "width", "leaf_level",
                 "max_def", "slots", "leaves", "same_as", "strs")

    def __init__(self, values, valid, rows, nvalid, dtype, logical=None, rep=None, dfn=None, width=0, leaf_level=0,
                 max_def=0, slots=0, leaves=0):
        self.values, self.valid, self.rows, self.nvalid, self.dtype = values, valid, rows, nvalid, dtype
        self.logical = logical   # datetime64[ms|us|ns] of a TIMESTAMP column, else None
        self.rep, self.dfn, self.width, self.leaf_level, self.max_def = rep, dfn, width, leaf_level, max_def
        self.slots, self.leaves, self.same_as = slots, leaves, None
        self.strs = None

    @property
    def is_list(self):
        return self.rep is not None


_MAX_STR_CHARS = (1 << 32) - 2   # kernels_strings._MAX_CHARS: the dict's strings are gathered with 32-bit sums


class StagedStrings:
    """The staging buffers of one string column of a partition, as nvt_pq_decode_str_chunk fills them
    (include/nvt_hip.h, nvt_pq_str_stage): ``offsets`` (int64) / ``chars`` the entries, ``runs`` the run
    table (int32 words, 4 per record, the closing record behind the ``nruns`` runs), ``packed`` the
    bytes of the bit-packed runs.  Sized from the footer and enlarged when the decoder asks for it.
    ``where`` names file and column for error messages."""

    def __init__(self, entries_cap, chars_cap, runs_cap, packed_cap, pinned, where):
        import torch

        from . import _lib

        self.pinned, self.where = pinned, where
        self.offsets = torch.empty(entries_cap + 1, dtype=torch.int64, pin_memory=pinned)
        self.chars = torch.empty((chars_cap + 7) & ~7, dtype=torch.uint8, pin_memory=pinned)
        self.runs = torch.empty(4 * runs_cap, dtype=torch.int32, pin_memory=pinned)
        self.packed = torch.empty(((packed_cap + 7) & ~7) + 8, dtype=torch.uint8, pin_memory=pinned)
        self.offsets[0] = 0
        self.c = _lib.PqStrStage()
        self._bind()

    def _bind(self):
        c = self.c
        c.offsets, c.chars, c.runs, c.packed = (self.offsets.data_ptr(), self.chars.data_ptr(), self.runs.data_ptr(),
                                                self.packed.data_ptr())
        c.entries_cap, c.chars_cap = self.offsets.numel() - 1, self.chars.numel()
        c.runs_cap, c.packed_cap = self.runs.numel() // 4, self.packed.numel()

    def grow(self, need):
        """Enlarges the buffers named by ``need`` = (entries, chars, runs, packed), 0 = large enough,
        keeping what is filled."""
        import torch

        from . import _lib

        c = self.c
        for which, want in enumerate(need):
            if not want:
                continue
            name, used, unit, extra = (("offsets", c.entries + 1, 1, 1), ("chars", c.nchars, 8, 0),
                                       ("runs", 4 * (c.nruns + 1), 4, 0), ("packed", c.npacked + 8, 8, 0))[which]
            old = getattr(self, name)
            if which == 1 and want > _MAX_STR_CHARS + 2:
                raise _lib.NvtHipError(f"{self.where}: more than {_MAX_STR_CHARS} bytes of strings in one partition")
            size = max(int(want) * (4 if which == 2 else 1), 2 * old.numel())
            if which == 1:
                size = min(size, _MAX_STR_CHARS + 2)
            new = torch.empty(((size + unit - 1) // unit) * unit + extra, dtype=old.dtype, pin_memory=self.pinned)
            new[:used] = old[:used]
            setattr(self, name, new)
        self._bind()

    @property
    def entries(self):
        return int(self.c.entries)

    @property
    def nchars(self):
        return int(self.c.nchars)

    @property
    def nruns(self):
        return int(self.c.nruns)

    @property
    def npacked(self):
        return int(self.c.npacked)

    @property
    def nvalues(self):
        return int(self.c.nvalues)


class StagedPartition:
    """A partition as ``read_row_groups_staged`` leaves it on the host: {column: StagedColumn}.
    ``to_device`` enqueues the copies on the CURRENT stream (the prefetcher's side stream) and
    expands columns with nulls to one slot per row on the device (kernels.expand_valid)."""

    def __init__(self, columns):
        self.columns = columns

    @property
    def num_rows(self):
        return next(iter(self.columns.values())).rows if self.columns else 0

    def to_device(self, device=None):
        import torch

        from . import kernels as K
        from . import kernels_parquet_list as KPL
        from .device import DeviceColumn, DeviceFrame, default_device

        device = device or default_device()
        out = {}
        unpacked = {}   # list column -> (offsets, leaf bitmap): one unpack per distinct level streams
        for name, sc in self.columns.items():
            if device.type != "cuda":   # (host-only use: tests of the reader itself)
                raise K._lib.NvtHipError("StagedPartition.to_device needs a GPU")
            if sc.strs is not None:
                # entries, run table and packed index bytes travel as the file holds them: the ids are
                # expanded, the entries hashed and the dict built on the device
                from . import kernels_parquet_str as KPS

                out[name] = KPS.column_from_staged(sc, device)
                continue
            packed = sc.values[:sc.nvalid].to(device, non_blocking=True)
            if sc.is_list:
                # the level streams become offsets and the leaf bitmap on the device (columns with
                # byte-equal streams share both tensors); the non-null leaves are then expanded to
                # one slot per leaf like a flat column's rows
                key = sc.same_as if sc.same_as in unpacked else name
                if key not in unpacked:
                    rep = sc.rep[: ((sc.slots + 63) // 64) * 8].to(device, non_blocking=True)
                    dfn = sc.dfn[: ((sc.slots * sc.width + 63) // 64) * 8].to(device, non_blocking=True)
                    unpacked[key] = KPL.unpack_levels(rep, dfn, sc.width, sc.slots, sc.leaf_level, sc.max_def,
                                                      sc.rows, sc.leaves, sc.nvalid < sc.leaves)
                offsets, bitmap = unpacked[key]
                data = packed if bitmap is None else K.expand_valid(packed, bitmap, sc.leaves)
                out[name] = DeviceColumn(data, bitmap, offsets)
            elif sc.dtype == BOOL_DTYPE or sc.dtype in _NARROW:
                # staged as int32 values / one byte per bool: expanded and narrowed in one pass
                from . import kernels_parquet_narrow as KPN

                bitmap = None
                if sc.valid is not None:
                    bitmap = sc.valid[: ((sc.rows + 63) // 64) * 8].to(device, non_blocking=True)
                out[name] = DeviceColumn(KPN.expand_narrow(packed, getattr(torch, sc.dtype.name), bitmap, sc.rows),
                                         bitmap)
            elif sc.valid is None:
                out[name] = DeviceColumn(packed, logical=sc.logical)
            else:
                bitmap = sc.valid[: ((sc.rows + 63) // 64) * 8].to(device, non_blocking=True)
                out[name] = DeviceColumn(K.expand_valid(packed, bitmap, sc.rows), bitmap, logical=sc.logical)
        return DeviceFrame(out)


_TLS = threading.local()


def _scratch(slot: str, nbytes: int) -> bytearray:
    """This thread's buffer ``slot`` ("read": one column chunk as it is in the file; "codec": a
    dictionary + one decompressed page), grown in powers of two."""
    buf = getattr(_TLS, slot, None)
    if buf is None or len(buf) < nbytes:
        cap = 1 << 20
        while cap < nbytes:
            cap <<= 1
        buf = bytearray(cap)
        setattr(_TLS, slot, buf)
    return buf


# column chunks decoded by the hand-written reader / left to pyarrow since the process started
# (bench.py's end_to_end entry reports them: a fallback must not be silent)
READER_CHUNKS = {"plain": 0, "pyarrow": 0}


def read_row_groups_staged(pf: PlainParquetFile, groups, columns=None, pool=None, pin=True):
    """{column: StagedColumn} for the concatenation of `groups` (row-group indices) of a decodable
    file.  One task per column: pread of a chunk into a scratch buffer, then nvt_pq_decode_chunk
    (ctypes: GIL released) moves its values and validity bits to their place in the partition's
    (pinned) staging buffers; a list column's chunks go through nvt_pq_decode_list_chunk, which
    appends their levels to the column's two level streams instead, a string column's through
    nvt_pq_decode_str_chunk, which appends entries, index runs and packed bytes to a StagedStrings."""
    import ctypes as C

    import torch

    from . import _lib

    lib = _lib.load()
    names = [n for n in pf.names if columns is None or n in columns]
    total = sum(pf.row_groups[g]["num_rows"] for g in groups)
    pinned = bool(pin) and torch.cuda.is_available()   # (host-only processes stage in pageable memory)
    fd = os.open(pf.path, os.O_RDONLY)

    def chunks(n, j):
        """(row group, chunk, rows, chunk bytes, codec scratch, its size) of column j's chunks in
        the row groups that have rows, each read into this thread's buffers."""
        for g in groups:
            cc, rows = pf.row_groups[g]["columns"][j], pf.row_groups[g]["num_rows"]
            if rows == 0:
                continue
            buf = _scratch("read", cc["size"])   # (per thread, reused: a fresh 30 MB bytearray is
            got, mv = 0, memoryview(buf)         #  zero-filled and page-faulted in for every chunk)
            while got < cc["size"]:
                k = os.preadv(fd, [mv[got:cc["size"]]], cc["offset"] + got)
                if k <= 0:
                    raise IOError(f"{pf.path}: short read of column chunk {n}")
                got += k
            sbuf, sbytes = None, 0
            if cc.get("codec", 0) != 0 or cc.get("dictionary"):
                sbytes = 2 * max(cc.get("raw_size", 0), cc["size"]) + 64
                sraw = _scratch("codec", sbytes)
                sbuf = (C.c_uint8 * len(sraw)).from_buffer(sraw)
            yield g, cc, rows, (C.c_uint8 * len(buf)).from_buffer(buf), sbuf, sbytes

    def decoded(fn, rc, n, g):
        if rc != 0:
            raise _lib.NvtHipError(f"{fn}({pf.path}, {n}, row group {g}): {lib.nvt_last_error().decode()} (rc {rc})")
        READER_CHUNKS["plain"] += 1

    def list_task(n, j):
        """One list column: the non-null leaves of its chunks behind each other, their levels
        appended to ONE repetition and ONE definition stream (a thread per column: chunks share words)."""
        col, dt = pf.columns[j], pf.dtypes[j]
        width = 1 if col["max_def"] == 1 else 2
        slots = sum(pf.row_groups[g]["columns"][j]["num_values"] for g in groups if pf.row_groups[g]["num_rows"])
        vals = torch.empty(slots, dtype=getattr(torch, dt.name), pin_memory=pinned)
        rep = torch.zeros(((slots + 63) // 64) * 8 + 8, dtype=torch.uint8, pin_memory=pinned)
        dfn = torch.zeros(((slots * width + 63) // 64) * 8 + 8, dtype=torch.uint8, pin_memory=pinned)
        slot_at = val_at = leaves = 0
        counts = (C.c_uint64 * 4)()
        for g, cc, rows, cbuf, sbuf, sbytes in chunks(n, j):
            rc = lib.nvt_pq_decode_list_chunk(cbuf, cc["size"], cc.get("codec", 0), dt.itemsize, col["leaf_level"],
                                              col["max_def"], cc["num_values"], rows, rep.data_ptr(), dfn.data_ptr(),
                                              slot_at, slots, vals.data_ptr() + val_at * dt.itemsize,
                                              (slots - val_at) * dt.itemsize, sbuf, sbytes, counts)
            decoded("nvt_pq_decode_list_chunk", rc, n, g)
            slot_at += int(counts[0])
            leaves += int(counts[2])
            val_at += int(counts[3])
        return StagedColumn(vals, None, total, val_at, dt, None, rep=rep, dfn=dfn, width=width,
                            leaf_level=col["leaf_level"], max_def=col["max_def"], slots=slot_at, leaves=leaves)

    def str_task(n, j):
        """One string column: the chunks' entries, index runs and packed bytes appended to ONE
        StagedStrings (nvt_pq_decode_str_chunk), validity bits at the partition's row positions."""
        ccs = [pf.row_groups[g]["columns"][j] for g in groups if pf.row_groups[g]["num_rows"]]
        nv = sum(cc["num_values"] for cc in ccs)
        raw = sum(max(cc.get("raw_size", 0), cc["size"]) for cc in ccs)
        # from the footer: every entry holds a 4-byte length and every run 2 bytes or more of its
        # page, pyarrow's runs 8 values or more; a footer that understates them makes the decoder ask
        st = StagedStrings(min(nv, raw // 4) + 16, min(raw, _MAX_STR_CHARS) + 8, min(raw // 2, nv // 8) + 1024,
                           raw + nv // 64 + 4096, pinned, f"{pf.path}: column {n!r}")
        valid = None
        if pf.max_def[j]:
            valid = torch.zeros(((total + 63) // 64) * 8 + 8, dtype=torch.uint8, pin_memory=pinned)
        row_at = 0
        need = (C.c_uint64 * 4)()
        for g, cc, rows, cbuf, sbuf, sbytes in chunks(n, j):
            while True:
                rc = lib.nvt_pq_decode_str_chunk(cbuf, cc["size"], cc.get("codec", 0), pf.max_def[j], rows,
                                                 valid.data_ptr() if valid is not None else None, row_at,
                                                 C.addressof(st.c), sbuf, sbytes, need)
                if rc != _lib.PQ_STR_GROW:
                    break
                st.grow(tuple(int(x) for x in need))
            decoded("nvt_pq_decode_str_chunk", rc, n, g)
            if st.nchars > _MAX_STR_CHARS:
                raise _lib.NvtHipError(f"{st.where}: more than {_MAX_STR_CHARS} bytes of strings in one partition")
            row_at += rows
        sc = StagedColumn(None, valid if (valid is not None and st.nvalues < total) else None, total, st.nvalues, None)
        sc.strs = st
        return sc

    def task(n):
        """One column: its chunks of the row groups one after the other -- packed values behind
        each other, validity bits at the partition's row positions (a thread per COLUMN: two row
        groups may share a bitmap byte)."""
        j = pf.names.index(n)
        if pf.columns[j]["kind"] == "list":
            return list_task(n, j)
        if pf.columns[j]["kind"] == "string":
            return str_task(n, j)
        dt = pf.dtypes[j]
        # an int8 / int16 column is staged as the INT32 values the file holds, a bool column one byte
        # per non-null value: the device narrows them (StagedPartition.to_device)
        st = np.dtype("uint8") if dt == BOOL_DTYPE else physical_dtype(dt)
        vals = torch.empty(total, dtype=getattr(torch, st.name), pin_memory=pinned)
        valid = None
        if pf.max_def[j]:
            valid = torch.zeros(((total + 63) // 64) * 8 + 8, dtype=torch.uint8, pin_memory=pinned)
        row_at = val_at = 0
        for g, cc, rows, cbuf, sbuf, sbytes in chunks(n, j):
            r, v = C.c_uint64(), C.c_uint64()
            if dt == BOOL_DTYPE:
                fn = "nvt_pq_decode_bool_chunk"
                rc = lib.nvt_pq_decode_bool_chunk(cbuf, cc["size"], cc.get("codec", 0), pf.max_def[j], rows,
                                                  valid.data_ptr() if valid is not None else None, row_at,
                                                  vals.data_ptr() + val_at, total - val_at, sbuf, sbytes,
                                                  C.byref(r), C.byref(v))
            else:
                fn = "nvt_pq_decode_chunk_codec"
                rc = lib.nvt_pq_decode_chunk_codec(cbuf, cc["size"], cc.get("codec", 0), st.itemsize, pf.max_def[j],
                                                   rows, valid.data_ptr() if valid is not None else None, row_at,
                                                   vals.data_ptr() + val_at * st.itemsize,
                                                   (total - val_at) * st.itemsize, sbuf, sbytes,
                                                   C.byref(r), C.byref(v))
            decoded(fn, rc, n, g)
            row_at += rows
            val_at += int(v.value)
        logical = np.dtype(f"datetime64[{pf.units[j]}]") if pf.units[j] is not None else None
        return StagedColumn(vals, valid if (valid is not None and val_at < total) else None, total, val_at, dt,
                            logical)

    futs = []
    try:
        if pool is not None and len(names) > 1:
            futs = [pool.submit(task, n) for n in names]
            cols = [f.result() for f in futs]
        else:
            cols = [task(n) for n in names]
    finally:
        # (after a failed column the others may still be reading: the descriptor is closed -- and
        # its number free for the next open -- only when none of them uses it any more)
        for f in futs:
            f.cancel()
        for f in futs:
            if not f.cancelled():
                f.exception()
        os.close(fd)
    # list columns whose level streams are byte-equal (what ops.Groupby's "list" aggregates of one
    # frame are) share one unpack on the device: 3 bits per slot to compare
    lists = []
    for n, sc in zip(names, cols):
        if not sc.is_list:
            continue
        key = (sc.slots, sc.width, sc.leaf_level, sc.max_def)
        for m, other in lists:
            if key == (other.slots, other.width, other.leaf_level, other.max_def) and \
                    torch.equal(sc.rep, other.rep) and torch.equal(sc.dfn, other.dfn):
                sc.same_as = m
                break
        else:
            lists.append((n, sc))
    return dict(zip(names, cols))
