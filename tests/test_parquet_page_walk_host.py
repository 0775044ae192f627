"""The page walk of the parquet reader, host half: every nvt_pq_decode_* entry point goes through ONE
walk over the pages of a column chunk, so every entry point must judge a defect in the page structure
the same way.  Hand-built chunks of three data pages (14 rows), one defect each, fed to all eight entry
points through ctypes: the return code per entry point is tabled below, and no call may write past the
capacities it was given (guard bytes behind every output and staging buffer)."""
import ctypes as C
import struct

import numpy as np
import pytest

from nvtabular_amd import _lib
from nvtabular_amd import parquet_plain as PP
from nvtabular_amd.parquet_plain import _Struct, _varint

OK, EINVAL, EUNSUP = 0, _lib.NVT_EINVAL, _lib.NVT_EUNSUPPORTED
GUARD, ROOM = 64, 4096
PAGE_ROWS = (5, 5, 4)
ROWS = sum(PAGE_ROWS)

ENTRIES = ("nvt_pq_decode_chunk", "nvt_pq_decode_chunk_codec", "nvt_pq_decode_list_chunk",
           "nvt_pq_decode_chunk_delta", "nvt_pq_decode_chunk_dict", "nvt_pq_decode_chunk_inflate",
           "nvt_pq_decode_str_chunk", "nvt_pq_decode_bool_chunk")
FILL_STATE = ("entries", "nchars", "nruns", "npacked", "nvalues", "nbytes", "npages", "nmbs", "ndict_bytes")
KIND = {"nvt_pq_decode_list_chunk": "list", "nvt_pq_decode_str_chunk": "string", "nvt_pq_decode_bool_chunk": "bool"}


# ---- chunks: pages are dicts {type, num_values, encoding, body, ...}, turned into bytes by `chunk_bytes` ----
def _rle(count, value):
    return _varint(count << 1) + bytes([value])


def _values(kind, at, n, by_dict):
    """The values region of a page holding values [at, at + n) of the column."""
    if by_dict:   # indices into a dictionary of 4 entries: bit width 2, one repeat run of entry 1
        return b"\x02" + _rle(n, 1)
    if kind == "string":
        return b"".join(struct.pack("<I", 1 + i % 3) + b"xyz"[: 1 + i % 3] for i in range(at, at + n))
    if kind == "bool":
        return np.packbits(np.arange(at, at + n) % 3 == 0, bitorder="little").tobytes()
    return np.arange(at, at + n, dtype="int64").tobytes()


def data_pages(kind, by_dict=False):
    """Three v1 data pages of a required column; a list column has one row per page (required list of
    required int64 leaves: repetition 0, 1, 1, ..., definition 1 throughout)."""
    pages, at = [], 0
    for n in PAGE_ROWS:
        levels = b""
        if kind == "list":
            rep, dfn = _rle(1, 0) + _rle(n - 1, 1), _rle(n, 1)
            levels = struct.pack("<I", len(rep)) + rep + struct.pack("<I", len(dfn)) + dfn
        pages.append({"type": 0, "num_values": n, "encoding": 8 if by_dict else 0,
                      "body": levels + _values(kind, at, n, by_dict)})
        at += n
    return pages


def dictionary_page(kind):
    body = _values(kind, 0, 4, False) if kind == "string" else np.arange(4, dtype="int64").tobytes()
    return {"type": 2, "dict_values": 4, "body": body}


def _snappy(raw):
    """A snappy block of literals only."""
    return _varint(len(raw)) + (PP._snappy_literal_tag(len(raw)) + raw if raw else b"")


def chunk_bytes(pages, codec):
    out = b""
    for p in pages:
        body, lead = p["body"], p.get("def_bytes_true", 0)   # (v2: the levels in front stay uncompressed)
        stored = body[:lead] + _snappy(body[lead:]) if codec == 1 else body
        head = (_Struct().i32(1, p["type"]).i32(2, p.get("uncompressed", len(body)))
                .i32(3, p.get("compressed", len(stored))))
        if "v2_def_bytes" in p:
            dph = (_Struct().i32(1, p["num_values"]).i32(2, 0).i32(3, p["num_values"]).i32(4, p["encoding"])
                   .i32(5, p["v2_def_bytes"]).i32(6, 0).done())
            head = head.struct(8, dph)
        elif "dict_values" in p:
            head = head.struct(7, _Struct().i32(1, p["dict_values"]).i32(2, 0).done())
        else:
            dph = _Struct().i32(1, p["num_values"]).i32(2, p["encoding"]).i32(3, 3).i32(4, 3).done()
            head = head.struct(5, dph)
        out += head.done() + stored
    return out


# ---- the defects: (kind, codec) -> (chunk, codec argument, rows / slots the caller expects) ----
def _edit(page, **fields):
    def build(kind, codec):
        pages = data_pages(kind)
        pages[page].update(fields)
        return chunk_bytes(pages, codec), codec, ROWS
    return build


def _cut_header(kind, codec):
    pages = data_pages(kind)
    return chunk_bytes(pages[:1], codec) + chunk_bytes(pages[1:2], codec)[:3], codec, ROWS


def _v2_levels_past_page(kind, codec):
    pages = data_pages(kind)
    pages[1].update(type=3, v2_def_bytes=len(pages[1]["body"]) + (8 if codec == 1 else 1))
    return chunk_bytes(pages, codec), codec, ROWS


def _two_dictionaries(kind, codec):
    return chunk_bytes([dictionary_page(kind)] * 2 + data_pages(kind, by_dict=True), codec), codec, ROWS


DEFECTS = {
    "none": lambda kind, codec: (chunk_bytes(data_pages(kind), codec), codec, ROWS),
    "one dictionary page": lambda kind, codec: (
        chunk_bytes([dictionary_page(kind)] + data_pages(kind, by_dict=True), codec), codec, ROWS),
    "header cut short": _cut_header,
    "compressed_page_size past the chunk": _edit(2, compressed=1 << 20),
    "negative size": _edit(1, compressed=-5),
    "page type 4": _edit(1, type=4),
    "codec 2": lambda kind, codec: (chunk_bytes(data_pages(kind), 0), 2, ROWS),
    "v2 def_bytes larger than the page": _v2_levels_past_page,
    "num_values above the rows still owed": _edit(2, num_values=PAGE_ROWS[2] + 1),
    "pages ending one row short": lambda kind, codec: (chunk_bytes(data_pages(kind), codec), codec, ROWS + 1),
    "a second dictionary page": _two_dictionaries,
    "dictionary indices with no dictionary page": lambda kind, codec: (
        chunk_bytes(data_pages(kind, by_dict=True), codec), codec, ROWS),
}

# The return code of every entry point, and where an entry point differs by design.
EXPECT = {
    "none": (OK, {}),
    # parquet has no bool dictionaries: the bool route refuses the dictionary page itself
    "one dictionary page": (OK, {"nvt_pq_decode_bool_chunk": EUNSUP}),
    "header cut short": (EINVAL, {}),
    "compressed_page_size past the chunk": (EINVAL, {}),
    "negative size": (EINVAL, {}),
    "page type 4": (EUNSUP, {}),
    # nvt_pq_decode_chunk has no codec argument: it reads the (uncompressed) chunk
    "codec 2": (EUNSUP, {"nvt_pq_decode_chunk": OK}),
    "v2 def_bytes larger than the page": (EINVAL, {}),
    "num_values above the rows still owed": (EINVAL, {}),
    "pages ending one row short": (EINVAL, {}),
    # (bool: the FIRST dictionary page is refused already, with the same code)
    "a second dictionary page": (EUNSUP, {}),
    # bool: encoding 8 is no bool encoding (PLAIN and RLE are), refused before the dictionary is missed
    "dictionary indices with no dictionary page": (EINVAL, {"nvt_pq_decode_bool_chunk": EUNSUP}),
}


# ---- the calls: every output and staging buffer is ROOM bytes of capacity in front of GUARD bytes ----
class Buffers:
    def __init__(self):
        self.all = []

    def new(self):
        a = np.full(ROOM + GUARD, 0xA5, dtype=np.uint8)
        a[:ROOM] = 0
        self.all.append(a)
        return a

    def guards_intact(self):
        return all(bool((a[ROOM:] == 0xA5).all()) for a in self.all)


def call(lib, entry, chunk, codec, expect):
    """-> (rc, {name: bytes of an output or staging buffer, or a tuple of counts}, guards intact).
    ``expect``: the rows the caller expects (list: the slots; its rows are the pages)."""
    b = Buffers()
    cbuf = (C.c_uint8 * max(1, len(chunk))).from_buffer_copy(chunk or b"\0")
    vals, valid, scratch = b.new(), b.new(), b.new()
    r, v = C.c_uint64(), C.c_uint64()
    need = (C.c_uint64 * 4)()
    flat = (0, expect, valid.ctypes.data, 0)   # max_def_level, rows, validity bitmap, its bit offset
    tail = (scratch.ctypes.data, ROOM, C.byref(r), C.byref(v))
    out, stage = {}, None
    if entry == "nvt_pq_decode_chunk":
        rc = lib.nvt_pq_decode_chunk(cbuf, len(chunk), 8, *flat, vals.ctypes.data, ROOM, C.byref(r), C.byref(v))
    elif entry == "nvt_pq_decode_chunk_codec":
        rc = lib.nvt_pq_decode_chunk_codec(cbuf, len(chunk), codec, 8, *flat, vals.ctypes.data, ROOM, *tail)
    elif entry == "nvt_pq_decode_bool_chunk":
        rc = lib.nvt_pq_decode_bool_chunk(cbuf, len(chunk), codec, *flat, vals.ctypes.data, ROOM, *tail)
    elif entry == "nvt_pq_decode_list_chunk":
        rep, dfn, counts = b.new(), b.new(), (C.c_uint64 * 4)()
        rc = lib.nvt_pq_decode_list_chunk(cbuf, len(chunk), codec, 8, 1, 1, expect, len(PAGE_ROWS), rep.ctypes.data,
                                          dfn.ctypes.data, 0, ROOM * 4, vals.ctypes.data, ROOM, scratch.ctypes.data,
                                          ROOM, counts)
        out = {"rep": rep, "dfn": dfn}
        r.value, v.value = counts[0], counts[3]
        out["counts"] = tuple(counts) if rc == OK else ()
    elif entry == "nvt_pq_decode_str_chunk":
        bufs = [b.new() for _ in range(4)]
        stage = _lib.PqStrStage(*(x.ctypes.data for x in bufs), ROOM // 8 - 1, ROOM, ROOM // 16, ROOM, 0, 0, 0, 0, 0)
        rc = lib.nvt_pq_decode_str_chunk(cbuf, len(chunk), codec, *flat, C.addressof(stage), scratch.ctypes.data, ROOM,
                                         need)
        out = dict(zip(("offsets", "chars", "runs", "packed"), bufs))
        r.value, v.value = (expect, stage.nvalues) if rc == OK else (0, 0)
    else:
        bufs = [b.new() for _ in range(3)]
        ptrs = [x.ctypes.data for x in bufs]
        if entry == "nvt_pq_decode_chunk_delta":
            stage = _lib.PqDeltaStage(*ptrs, ROOM, ROOM // (8 * _lib.PQ_DELTA_RECORD_WORDS), ROOM // 16, 0, 0, 0)
            args = (2, *flat, vals.ctypes.data, ROOM, 0, C.byref(stage))   # physical type INT64
        elif entry == "nvt_pq_decode_chunk_dict":
            stage = _lib.PqDictStage(*ptrs, ROOM, ROOM // 16, ROOM, 0, 0, 0)
            args = (8, *flat, vals.ctypes.data, ROOM, 0, C.byref(stage))
        else:
            stage = _lib.PqInflateStage(*ptrs[:2], ROOM, ROOM // (8 * _lib.INFLATE_PAGE_WORDS), 0, 0)
            args = (8, *flat, vals.ctypes.data, ROOM, 0, 0, C.byref(stage))   # the footer says: no nulls
        rc = getattr(lib, entry)(cbuf, len(chunk), codec, *args, *tail, need)
        out = dict(zip("abc", bufs))
    out.update(values=vals, valid=valid)
    out["counts"] = out.get("counts", (r.value, v.value) if rc == OK else ())
    out["need"] = tuple(need) if rc == 1 else ()   # (every *_GROW is 1)
    if stage is not None:   # the fill state: the fields behind the capacities
        out["stage"] = tuple(getattr(stage, f) for f, _ in stage._fields_ if f in FILL_STATE)
    return rc, {k: (x[:ROOM].tobytes() if isinstance(x, np.ndarray) else x) for k, x in out.items()}, b.guards_intact()


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_every_entry_point_judges_a_page_defect_alike(defect, codec):
    lib = _lib.load()
    default, differs = EXPECT[defect]
    assert set(differs) <= set(ENTRIES)
    for entry in ENTRIES:
        if entry == "nvt_pq_decode_chunk" and codec == 1:
            continue   # (no codec argument)
        chunk, codec_arg, expect = DEFECTS[defect](KIND.get(entry, "number"), codec)
        rc, out, intact = call(lib, entry, chunk, codec_arg, expect)
        assert rc == differs.get(entry, default), (entry, rc, lib.nvt_last_error().decode())
        assert intact, entry
        if rc == OK:
            assert out["counts"][0] == ROWS and out["counts"][-1] == ROWS, (entry, out["counts"])
        elif "stage" in out:   # nothing is committed to a stage but on NVT_OK
            assert not any(out["stage"]), (entry, out["stage"])


def test_a_decoded_chunk_holds_the_column():
    """The walk's products for the chunk without a defect, both codecs: values, levels, entries."""
    lib = _lib.load()
    want = np.arange(ROWS, dtype="int64").tobytes()
    for codec in (0, 1):
        for entry in ENTRIES[1:6]:
            rc, out, _ = call(lib, entry, chunk_bytes(data_pages(KIND.get(entry, "number")), codec), codec, ROWS)
            staged = entry == "nvt_pq_decode_chunk_inflate" and codec == 1   # (holes: the device fills them)
            assert rc == OK and (staged or out["values"][: len(want)] == want), entry
            if staged:
                bodies = [len(_snappy(p["body"])) for p in data_pages("number")]   # each on a 16-byte boundary
                assert out["stage"] == (sum((n + 15) & ~15 for n in bodies[:2]) + bodies[2], 3)
        rc, out, _ = call(lib, "nvt_pq_decode_list_chunk", chunk_bytes(data_pages("list"), codec), codec, ROWS)
        assert out["counts"] == (ROWS, 3, ROWS, ROWS)   # slots, row starts, leaves, non-null leaves
        starts = np.unpackbits(np.frombuffer(out["rep"][:2], np.uint8), bitorder="little")[:ROWS] == 0
        assert np.flatnonzero(starts).tolist() == [0, 5, 10]
        rc, out, _ = call(lib, "nvt_pq_decode_bool_chunk", chunk_bytes(data_pages("bool"), codec), codec, ROWS)
        assert rc == OK and out["values"][:ROWS] == bytes(int(i % 3 == 0) for i in range(ROWS))
        rc, out, _ = call(lib, "nvt_pq_decode_str_chunk", chunk_bytes(data_pages("string"), codec), codec, ROWS)
        chars = b"".join(b"xyz"[: 1 + i % 3] for i in range(ROWS))
        assert rc == OK and out["stage"] == (ROWS, len(chars), 1, 0, ROWS) and out["chars"][: len(chars)] == chars
