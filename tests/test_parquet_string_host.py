"""String columns in the hand-written parquet reader, host side: the file verdict, the host decoder
(nvt_pq_decode_str_chunk: entries + run table + packed bytes) against pyarrow through the numpy run
expansion of pq_runs_reference.py, and its bounds under corrupted chunks.  No GPU."""
import ctypes as C
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_runs_reference as R
import pq_str_files as F
from nvtabular_amd import _lib
from nvtabular_amd import parquet_plain as PP
from nvtabular_amd.parquet_thrift import _Struct

OK, EINVAL, EUNSUPPORTED = 0, _lib.NVT_EINVAL, _lib.NVT_EUNSUPPORTED


# ---- verdicts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", ["string", "large_string"])
@pytest.mark.parametrize("nullable", [True, False])
def test_string_columns_are_decodable_and_not_eligible(tmp_path, typ, nullable):
    path = str(tmp_path / "s.parquet")
    t = F.table(["a", "b", "c"] * 10, typ=getattr(pa, typ)(), nullable=nullable)
    pq.write_table(t, path)
    pf = PP.PlainParquetFile(path)
    assert pf.decodable, pf.why_pyarrow
    # (`readable` keeps its earlier meaning, numbers and lists of numbers only: the string column is its reason)
    assert not pf.readable and "'s'" in pf.why_not and "string" in pf.why_not
    col = pf.columns[pf.names.index("s")]
    assert col["kind"] == "string" and col["max_def"] == int(nullable) and col["leaf_dtype"] is None
    assert not pf.eligible and "'s'" in pf.why and "string" in pf.why


@pytest.mark.parametrize("kind", ["binary", "fixed", "DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY", "list_of_strings"])
def test_byte_arrays_that_stay_with_pyarrow(tmp_path, kind):
    path = str(tmp_path / "b.parquet")
    kw = {}
    if kind == "binary":
        t = pa.table({"s": pa.array([b"a", b"bc"] * 20, type=pa.binary())})
    elif kind == "fixed":
        t = pa.table({"s": pa.array([b"abcd", b"efgh"] * 20, type=pa.binary(4))})
    elif kind == "list_of_strings":
        t = pa.table({"s": pa.array([["a", "b"], []] * 20)})
    else:
        t = pa.table({"s": pa.array(["a", "bc"] * 20)})
        kw = dict(use_dictionary=False, column_encoding={"s": kind})
    pq.write_table(t, path, **kw)
    pf = PP.PlainParquetFile(path)
    assert not pf.decodable and pf.why_pyarrow and not pf.readable and pf.why_not
    assert "string column" not in pf.why_pyarrow     # (a string column keeps no file with pyarrow)


def test_a_string_column_beside_number_and_list_columns_is_decodable(tmp_path):
    path = str(tmp_path / "m.parquet")
    t = pa.table({"x": pa.array(range(40), type=pa.int32()), "s": pa.array(["u", None] * 20),
                  "l": pa.array([[1, 2], []] * 20, type=pa.list_(pa.int64()))})
    pq.write_table(t, path)
    pf = PP.PlainParquetFile(path)
    assert pf.decodable, pf.why_pyarrow
    assert [c["kind"] for c in pf.columns] == ["flat", "string", "list"] and not pf.eligible


# ---- decode --------------------------------------------------------------------------------------
def staged_strings(sc):
    """StagedColumn of a string column -> (list of str / None per row, run kinds by run)."""
    st = sc.strs
    runs = st.runs[: 4 * (st.nruns + 1)].numpy().view(np.uint32).reshape(-1, 4)
    assert int(runs[-1, 0]) == st.nvalues == sc.nvalid and (runs[-1, 1] & 0xFF) == R.END
    assert (np.diff(runs[:, 0].astype(np.int64)) > 0).all()          # no empty run
    packed = st.packed[: st.npacked + 8].numpy()
    assert not packed[st.npacked:].any()                              # the 8 pad bytes
    ids, bad = R.expand(runs, packed, st.entries)
    assert bad == 0
    off = st.offsets[: st.entries + 1].numpy()
    chars = st.chars[: st.nchars].numpy().tobytes()
    assert off[0] == 0 and (int(off[-1]) if st.entries else 0) == st.nchars
    entries = [chars[off[i]:off[i + 1]].decode() for i in range(st.entries)]
    vals = [entries[i] for i in ids]
    if sc.valid is None:
        assert sc.nvalid == sc.rows
        return vals, runs
    bits = np.unpackbits(sc.valid.numpy(), bitorder="little")[: sc.rows].astype(bool)
    assert int(bits.sum()) == sc.nvalid
    it = iter(vals)
    return [next(it) if b else None for b in bits], runs


def check_against_pyarrow(path, groups, columns=None):
    pf = PP.PlainParquetFile(path)
    assert pf.decodable, pf.why_pyarrow
    before = dict(PP.READER_CHUNKS)
    staged = PP.read_row_groups_staged(pf, groups, columns, pin=False)
    ncols = len(columns) if columns is not None else len(pf.names)
    live = [g for g in groups if pf.row_groups[g]["num_rows"]]
    assert PP.READER_CHUNKS["plain"] - before["plain"] == ncols * len(live)
    assert PP.READER_CHUNKS["pyarrow"] == before["pyarrow"]
    want = pq.ParquetFile(path).read_row_groups(groups, columns=columns)
    assert list(staged) == want.column_names
    got, runs = staged_strings(staged["s"])
    assert got == want["s"].to_pylist()
    if want["s"].null_count == 0:
        assert staged["s"].valid is None
    for n in ("x", "f"):
        if n in staged:
            assert staged[n].nvalid == len(want) - want[n].null_count
    return runs


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_decode_equals_pyarrow(tmp_path, name):
    path = str(tmp_path / f"{name}.parquet")
    F.write(name, path)
    ng = pq.ParquetFile(path).num_row_groups
    for g in range(ng):
        runs = check_against_pyarrow(path, [g])
        kinds = set(int(k) & 0xFF for k in runs[:-1, 1])
        if name.startswith("small_dict") and g == 0:
            # a dictionary page, index pages and then PLAIN pages in ONE chunk (the writer looks at
            # the dictionary's size every 1024 values: the 2500-row groups fall back, the last does not)
            assert R.SEQUENCE in kinds and kinds & {R.PACKED, R.REPEAT}, kinds
        if name == "constant":
            assert kinds == {R.REPEAT} and len(runs) == 2           # bit width 0: one run of entry 0
        if name == "plain_uncompressed":
            assert kinds == {R.SEQUENCE}
    check_against_pyarrow(path, list(range(ng)))                       # every row group in one partition


def test_two_row_groups_and_projection(tmp_path):
    path = str(tmp_path / "p.parquet")
    F.write("small_dict_v2", path)
    check_against_pyarrow(path, [0, 1], columns=["s"])
    check_against_pyarrow(path, [1, 2], columns=["s", "f"])


def test_empty_row_group(tmp_path):
    path = str(tmp_path / "e.parquet")
    t, _ = F.CASES["default"]
    with pq.ParquetWriter(path, t.schema) as w:
        w.write_table(t.slice(0, 1000))
        w.write_table(t.slice(0, 0))
        w.write_table(t.slice(1000, 500))
    pf = PP.PlainParquetFile(path)
    groups = list(range(pf.num_row_groups))
    got, _ = staged_strings(PP.read_row_groups_staged(pf, groups, pin=False)["s"])
    assert got == t["s"].to_pylist()[:1500]


def test_staging_buffers_grow_when_the_footer_understates(tmp_path, monkeypatch):
    """Capacities of almost nothing: the decoder asks (NVT_PQ_STR_GROW), the stage is enlarged with
    its filled part kept, and the result is the same."""
    path = str(tmp_path / "g.parquet")
    F.write("small_dict_v2", path)
    real = PP.StagedStrings

    def tiny(entries_cap, chars_cap, runs_cap, packed_cap, pinned, where):
        return real(1, 8, 1, 8, pinned, where)

    monkeypatch.setattr(PP, "StagedStrings", tiny)
    check_against_pyarrow(path, [0, 1, 2])


def test_the_run_reference_against_a_bit_loop():
    """pq_runs_reference.expand (what the kernel is tested against) against the plainest reading of
    the layout: one bit at a time."""
    rng = np.random.default_rng(0)
    runs, packed = R.random_table(rng, 3000, 70_000)
    ids, bad = R.expand(runs, packed, 70_000)
    bits = np.unpackbits(packed, bitorder="little")
    assert bad == 0 and len(ids) == 3000
    for r in range(len(runs) - 1):
        start, word1, a, b = (int(x) for x in runs[r])
        kind, width = word1 & 0xFF, word1 >> 8
        for k in range(int(runs[r + 1, 0]) - start):
            if kind == R.PACKED:
                at = 32 * b + k * width
                want = a + sum(int(bits[at + j]) << j for j in range(width))
            else:
                want = a + (k if kind == R.SEQUENCE else 0)
            assert ids[start + k] == want, (r, k)


# ---- corruption ----------------------------------------------------------------------------------
GUARD = 64


class Guarded:
    """A buffer of exactly `nbytes` between two guard blocks of 0xA5."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.raw = np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8)

    @property
    def ptr(self):
        return self.raw.ctypes.data + GUARD

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all() and (self.raw[GUARD + self.n:] == 0xA5).all())


class Harness:
    """One chunk and output buffers of exactly the documented sizes, each between guards."""

    def __init__(self, chunk, codec, max_def, rows, raw_size, caps=None):
        self.codec, self.max_def, self.rows = codec, max_def, rows
        bound = 2 * max(raw_size, len(chunk)) + 64
        self.caps = caps or (bound // 4 + 16, (bound + 3) & ~3, bound + 2, 4 * bound + 64)
        e, c, r, p = self.caps
        self.offsets, self.chars, self.runs, self.packed = Guarded(8 * (e + 1)), Guarded(c), Guarded(16 * r), Guarded(p)
        self.valid = Guarded((rows + 7) // 8 + 8)
        self.scratch = Guarded(bound)
        self.stage = _lib.PqStrStage()
        self.need = (C.c_uint64 * 4)()
        self.lib = _lib.load()

    def decode(self, data):
        st = self.stage
        st.offsets, st.chars, st.runs, st.packed = self.offsets.ptr, self.chars.ptr, self.runs.ptr, self.packed.ptr
        st.entries_cap, st.chars_cap, st.runs_cap, st.packed_cap = self.caps
        st.entries = st.nchars = st.nruns = st.npacked = st.nvalues = 0
        buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
        rc = self.lib.nvt_pq_decode_str_chunk(buf.ctypes.data, len(data), self.codec, self.max_def, self.rows,
                                              self.valid.ptr, 0, C.addressof(st), self.scratch.ptr, self.scratch.n,
                                              self.need)
        assert all(g.intact() for g in (self.offsets, self.chars, self.runs, self.packed, self.valid, self.scratch))
        return rc


def _small_chunk(tmp_path, compression):
    rng = np.random.default_rng(3)
    vals = [None if i % 7 == 3 else f"id{int(v):05d}" for i, v in enumerate(rng.integers(0, 150, 900))]
    path = str(tmp_path / f"c_{compression}.parquet")
    pq.write_table(pa.table({"s": pa.array(vals)}), path, compression=compression, data_page_version="1.0",
                   data_page_size=600, write_statistics=False)
    pf = PP.PlainParquetFile(path)
    cc = pf.row_groups[0]["columns"][0]
    data = open(path, "rb").read()[cc["offset"]: cc["offset"] + cc["size"]]
    assert 1000 < len(data) < 4000
    return data, cc, len(vals)


@pytest.mark.parametrize("compression", ["none", "snappy"])
def test_corrupted_chunks_stay_inside_their_buffers(tmp_path, compression):
    data, cc, rows = _small_chunk(tmp_path, compression)
    h = Harness(data, cc["codec"], 1, rows, cc["raw_size"])
    assert h.decode(data) == OK and h.stage.nvalues == rows - len(range(3, rows, 7))
    seen = set()
    for at in range(len(data)):
        for v in (0x00, 0xFF, data[at] ^ 0xFF):
            bad = bytearray(data)
            bad[at] = v
            seen.add(h.decode(bad))
        seen.add(h.decode(data[:at]))
    assert seen <= {OK, EINVAL, EUNSUPPORTED}, seen
    assert OK in seen and EINVAL in seen


def _page(header: bytes, body: bytes) -> bytes:
    return header + body


def _dict_page(count, body):
    dph = _Struct().i32(1, count).i32(2, 0).done()
    return _Struct().i32(1, 2).i32(2, len(body)).i32(3, len(body)).struct(7, dph).done() + body


def _index_page(nvalues, body):
    dph = _Struct().i32(1, nvalues).i32(2, 8).i32(3, 3).i32(4, 3).done()   # RLE_DICTIONARY, RLE levels
    return _Struct().i32(1, 0).i32(2, len(body)).i32(3, len(body)).struct(5, dph).done() + body


def _plain(values):
    return b"".join(struct.pack("<I", len(v)) + v for v in values)


def test_forged_page_headers():
    entries = _plain([b"aa", b"b"])
    # 16 values: one RLE run of 16 x index 1 at bit width 1 (required column: no levels)
    good = _dict_page(2, entries) + _index_page(16, bytes([1, 16 << 1, 1]))
    h = Harness(good, 0, 0, 16, len(good))
    assert h.decode(good) == OK and h.stage.entries == 2 and h.stage.nvalues == 16
    # a dictionary count that does not fit its page: 2^61 * 4 wraps to 0 in 64 bits
    for count in (2**61, 2**62 + 1, 3, 2**31 - 1, -1):
        forged = _dict_page(count, entries) + _index_page(16, bytes([1, 16 << 1, 1]))
        assert h.decode(forged) == EINVAL, count
    # bit width 33 (and 255)
    for bw in (33, 64, 255):
        forged = _dict_page(2, entries) + _index_page(16, bytes([bw, 16 << 1, 1, 0, 0, 0, 0]))
        assert h.decode(forged) == EINVAL, bw
    # a length prefix past its page; a run longer than the page is clipped to the page's values
    assert h.decode(_dict_page(2, _plain([b"aa"]) + struct.pack("<I", 999) + b"b") +
                    _index_page(16, bytes([1, 16 << 1, 1]))) == EINVAL
    assert h.decode(_dict_page(2, entries) + _index_page(16, bytes([1, 0x80, 0x80, 0x01, 1]))) == OK
    assert h.stage.nvalues == 16
    # a bit-packed run whose bytes are not there
    assert h.decode(_dict_page(2, entries) + _index_page(16, bytes([1, (2 << 1) | 1, 0xFF]))) == EINVAL
    # an index past the dictionary in a repeat run: staged as the id no partition has
    assert h.decode(_dict_page(2, entries) + _index_page(16, bytes([2, 16 << 1, 3]))) == OK
    runs = np.frombuffer(h.runs.raw[GUARD: GUARD + 32].tobytes(), dtype=np.uint32).reshape(2, 4)
    assert runs[0, 2] == 0xFFFFFFFF and R.expand(runs, np.zeros(8, np.uint8), 2)[1] == 16
