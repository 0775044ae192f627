"""Kernel-level matrix for the delimited-text reader (nvtabular_amd/csrc/nvt_csv.hip, nvt_csv_parse.hpp,
nvt_csv_field.hpp and the CSV half of nvt_datetime.hip): the nvt_csv_* entries called directly through
``_lib.load()`` on torch tensors and compared with csv_reference.py (which test_csv_reference.py pins to
csv.reader, pandas, float(), int() and numpy on the CPU).  Every comparison is exact: bit patterns for
floats, integers elsewhere.  Every output buffer is filled with 0xA5 bytes first and carries spare
elements behind the documented output, which must still hold 0xA5 afterwards.

Route -> entry point -> kernels, and the test that reaches it on purpose.

  nvt_csv_count        count_kernel (one workgroup per 4096-byte tile, grid-stride beyond 2048 tiles),
                       tile_scan_kernel (one workgroup, 256 tile records a step)
    classify()         the `live` mask of the last 16 bytes                    test_index_sizes (the bytes past nbytes
                                                                               hold quote, separator, newline),
                                                                               test_bytes_past_the_end_are_no_bytes
    inside_mask()      lane -> wave -> tile parity                             test_quote_on_an_edge[15 / 1023 / 4095-*]
    tile_scan_kernel   tile -> tile, step -> step parity and counts            test_quote_on_an_edge[1048575-*],
                                                                               test_index_sizes[1048575 .. 1052972]
    second grid trip   tiles 2048 ..                                           test_index_second_grid_trip
    state words        BAD_ROW / QUOTE_ROW / BAD_FIELD = 2^64 - 1, SLOW = word 7 = 0
                                                                               every check_index call
  nvt_csv_index        index_kernel
    field_end          every separator at its rank                             every check_index call
    rank < nfields     fewer slots than separators                             test_fewer_slots_than_separators
    BAD_ROW            atomicMin over tiles                                    test_bad_rows_in_three_tiles,
                                                                               test_totals_balance
    QUOTE_ROW, PARITY                                                          test_newlines_inside_quotes,
                                                                               test_quote_that_never_closes
    sep / quote bytes  -1, ', tab, |, 0xFE; ncols 1 and 200                    test_separator_and_quote_variants
    a quoted field of separators over two whole tiles                          test_quoted_field_covers_two_tiles
  nvt_csv_parse_many   parse_kernel (one lane per row, 64 descriptors a launch, grid-stride beyond 2048 * 256 rows)
    csv_parse_f64      Clinger / Eisel-Lemire (second product, subnormal, halfway, carry) / declined /
                       specials / invalid, as float64 and float32               test_float_corpus
    csv_parse_i64      limits, overflow, invalid, as int64 and int32            test_int_corpus
    validity words     rows 1 .. 257, quoted and empty fields, CRLF             test_parse_rows
    second grid trip   524 289 rows                                             test_parse_second_grid_trip
    descriptor batches 1, 64, 65, 130; one k under two dtypes                   test_descriptor_batches
    BAD_FIELD          atomicMin over rows, columns, launches and calls         test_bad_field_is_the_least
  nvt_csv_str_offsets  str_len_kernel + exclusive_scan_u32                      test_strings, test_undoubled_quote
  nvt_csv_str_copy     str_copy_kernel; the clamp to chars_bytes                test_strings, test_chars_clamp
  nvt_csv_parse_datetime  parse_kernel of nvt_datetime.hip                      test_datetime_corpus (65 descriptors)

Left out, by name: text of 2^31 bytes and more (refused by the entries: test_csv_cabi.py); field_end beyond
2^32 (cannot exist below 2^31 bytes); the host half of kernels_csv.parse_text (test_gpu_csv.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import csv_reference as R
from nvtabular_amd import _lib

pytestmark = pytest.mark.gpu

NONE = R.NONE
SENT = 0xA5
SENT64 = 0xA5A5A5A5A5A5A5A5
GUARD = 4                      # spare 64-bit words behind the state block
TILE, STEP = _lib.CSV_TILE, _lib.CSV_SCAN_STEP
COMMA, QUOTE, TAB = ord(","), ord('"'), ord("\t")
HOT_TAIL = b'",\n'             # what the bytes between nbytes and the next multiple of 16 hold
CODE = {"float32": _lib.NVT_F32, "float64": _lib.NVT_F64, "int32": _lib.NVT_I32, "int64": _lib.NVT_I64}
M = bytes([R.MARK])
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _free_shared():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sentinel(nbytes):
    return torch.full((max(8, (nbytes + 7) // 8 * 8),), SENT, dtype=torch.uint8, device="cuda")


def host(t):
    return t.cpu().numpy()


def device_text(raw, tail=HOT_TAIL):
    """The bytes on the device, readable to the next multiple of 16; the bytes past the end hold `tail`."""
    n = len(raw)
    buf = np.zeros(max(16, (n + 15) // 16 * 16), dtype=np.uint8)
    buf[:n] = np.frombuffer(raw, dtype=np.uint8)
    if tail:
        buf[n:] = np.resize(np.frombuffer(tail, dtype=np.uint8), len(buf) - n)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def fresh_state():
    """The state block as nvt_csv_count leaves it for text without rows, and GUARD words behind it."""
    st = np.array([0, 0, 0, NONE, NONE, NONE, 0, 0] + [SENT64] * GUARD, dtype=np.uint64)
    return torch.from_numpy(st.view(np.int64)).cuda()


def read_state(state):
    st = host(state).view(np.uint64)
    assert (st[_lib.CSV_STATE_WORDS:] == SENT64).all()
    return [int(v) for v in st[:_lib.CSV_STATE_WORDS]]


# ---- index ----------------------------------------------------------------------------------------------
def run_index(lib, raw, sep, quote, ncols, tail=HOT_TAIL, short=0):
    """(state after nvt_csv_count, state after nvt_csv_index, field_end with 16 spare slots)."""
    text, n = device_text(raw, tail), len(raw)
    need = C.c_uint64()
    assert lib.nvt_csv_ws_bytes(n, C.byref(need)) == 0
    ws = sentinel(need.value)
    state = sentinel(8 * (_lib.CSV_STATE_WORDS + GUARD))
    rc = lib.nvt_csv_count(text.data_ptr(), n, sep, quote, ws.data_ptr(), need.value, state.data_ptr(), stream())
    assert rc == 0, lib.nvt_last_error()
    counted = read_state(state)
    slots = counted[_lib.CSV_ST_FIELDS] - short
    assert 0 <= slots <= n
    field_end = sentinel(4 * (slots + 16))
    rc = lib.nvt_csv_index(text.data_ptr(), n, sep, quote, ncols, ws.data_ptr(), need.value, field_end.data_ptr(),
                           slots, state.data_ptr(), stream())
    assert rc == 0, lib.nvt_last_error()
    return counted, read_state(state), host(field_end).view(np.uint32)[:slots + 16], slots


def check_index(lib, raw, sep=COMMA, quote=QUOTE, ncols=2, tail=HOT_TAIL, short=0):
    want = R.index(raw, len(raw), sep, quote, ncols)
    counted, indexed, fe, slots = run_index(lib, raw, sep, quote, ncols, tail, short)
    assert counted == [want["nfields"], want["nrows"], want["parity"], NONE, NONE, NONE, 0, 0]
    assert indexed == [want["nfields"], want["nrows"], want["parity"], want["bad_row"], want["quote_row"], NONE, 0, 0]
    np.testing.assert_array_equal(fe[:slots], want["field_end"][:slots])
    assert (fe[slots:] == 0xA5A5A5A5).all()
    return want


def tiled_text(size, seed):
    """Well-formed text of `size` bytes with quoted fields in it: a block of 65 521 bytes (a prime: the
    block edges fall on every offset of a lane) repeated, then filled to the size."""
    block = R.structured_text([], 65521, seed=seed)
    reps = max(0, (size - 200) // len(block))
    return block * reps + R.structured_text([], size - reps * len(block), seed=seed + 1)


SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, STEP * TILE - 1, STEP * TILE, STEP * TILE + 1,
         (STEP + 1) * TILE + 300]


@pytest.mark.parametrize("size", SIZES)
def test_index_sizes(lib, size):
    if size == 1:
        want = check_index(lib, b"\n", ncols=1)
        assert (want["nrows"], want["nfields"]) == (1, 1)
        return
    raw = tiled_text(size, seed=size % 89)
    want = check_index(lib, raw)
    assert len(raw) == size and want["nrows"] > 0 and want["bad_row"] == NONE and want["parity"] == 0
    assert size < 1000 or (raw.count(b'"') > 0 and want["nfields"] < raw.count(b",") + raw.count(b"\n"))


def test_index_second_grid_trip(lib):
    # 2049 tiles and 17 bytes: the launch has 2048 workgroups, tiles 2048 and 2049 are second trips
    raw = tiled_text(2049 * TILE + 17, seed=3)
    want = check_index(lib, raw)
    assert want["bad_row"] == NONE and want["field_end"][-1] == len(raw) - 1 > 2048 * TILE


@pytest.mark.parametrize("size", [1, 15, 17, 4097])
def test_bytes_past_the_end_are_no_bytes(lib, size):
    raw = b"\n" if size == 1 else R.structured_text([], size, seed=size)
    ncols = 1 if size == 1 else 2
    for tail in (None, HOT_TAIL, b"\n\n\n", b'"'):
        check_index(lib, raw, ncols=ncols, tail=tail)


EDGE_ROWS = {"open": b"12," + M + b'"ab,cd"\n', "close": b'12,"ab,cd' + M + b'"\n', "doubled": b'12,"ab' + M + b'""cd,"\n',
             "separator": b'12,"ab' + M + b',cd"\n', "newline": b'12,"ab,cd"' + M + b"\n"}


@pytest.mark.parametrize("kind", list(EDGE_ROWS))
@pytest.mark.parametrize("position", [15, 16 + 15, 1023, 4095, 3 * 4096 - 1, (1 << 20) - 1])
def test_quote_on_an_edge(lib, position, kind):
    # the marked byte is the last one of a lane (16 bytes), a wave (1024), a tile (4096) or a scan step (2^20)
    raw = R.structured_text([(EDGE_ROWS[kind], position)], position + 2 * TILE + 7, seed=position % 97)
    assert raw[position:position + 1] == {"separator": b",", "newline": b"\n"}.get(kind, b'"')
    assert kind != "doubled" or raw[position:position + 2] == b'""'
    want = check_index(lib, raw)
    assert want["bad_row"] == NONE and want["quote_row"] == NONE and want["parity"] == 0
    assert want["nfields"] == 2 * want["nrows"]


def test_quoted_field_covers_two_tiles(lib):
    row = b"5," + M + b'"' + b"," * (3 * TILE) + b'"\n'            # opens 7 bytes before a tile edge
    raw = R.structured_text([(row, TILE - 7)], 6 * TILE + 5, seed=1)
    assert set(raw[TILE:4 * TILE - 7]) == {COMMA}
    want = check_index(lib, raw)
    assert want["bad_row"] == NONE and want["nfields"] == 2 * want["nrows"]


def variant_text(size, ncols, sep, quote, seed):
    return R.structured_text([], size, ncols=ncols, sep=bytes([sep]), quote=bytes([quote]), seed=seed)


def test_separator_and_quote_variants(lib):
    raw = R.structured_text([], 3 * TILE + 11, seed=2)
    assert raw.count(b'"') > 100
    want = check_index(lib, raw, quote=-1)                   # quoting off: every comma counts
    assert want["nfields"] == raw.count(b",") + raw.count(b"\n") and want["bad_row"] != NONE and want["parity"] == 0
    want = check_index(lib, variant_text(3 * TILE + 11, 2, COMMA, ord("'"), 4), quote=ord("'"))
    assert want["bad_row"] == NONE
    raw = variant_text(3 * TILE + 11, 2, COMMA, ord("'"), 4).replace(b"y", b'"')    # the other quote is text now
    assert check_index(lib, raw, quote=ord("'"))["bad_row"] == NONE
    for sep in (TAB, ord("|"), 0xFE):
        raw = variant_text(2 * TILE + 3, 3, sep, QUOTE, sep)
        want = check_index(lib, raw, sep=sep, ncols=3)
        assert want["bad_row"] == NONE and want["nfields"] == 3 * want["nrows"]
        assert check_index(lib, raw, sep=COMMA, ncols=3)["bad_row"] == 0          # (no comma in it: one field a row)
    raw = variant_text(2 * TILE + 3, 1, COMMA, QUOTE, 5)
    want = check_index(lib, raw, ncols=1)
    assert want["bad_row"] == NONE and want["nfields"] == want["nrows"] > 10
    raw = variant_text(5 * TILE + 3, 200, COMMA, QUOTE, 6)
    want = check_index(lib, raw, ncols=200)
    assert want["bad_row"] == NONE and want["nfields"] == 200 * want["nrows"] and want["nrows"] >= 3
    assert check_index(lib, raw, ncols=199)["bad_row"] == 0


@pytest.mark.parametrize("order", ["short_long_short", "long_short_short", "short_short_long"])
def test_bad_rows_in_three_tiles(lib, order):
    rows = {"short": M + b"7\n", "long": M + b"1,2,3\n"}
    spec = [(rows[w], at) for w, at in zip(order.split("_"), (TILE + 900, 2 * TILE + 900, 4 * TILE + 900))]
    raw = R.structured_text(spec, 6 * TILE + 1, seed=7)
    want = check_index(lib, raw)
    first = raw[:TILE + 900].count(b"\n")
    assert want["bad_row"] == first and want["quote_row"] == NONE


def test_totals_balance(lib):
    want = check_index(lib, b"a,b,c\nd\n")
    assert (want["nfields"], want["nrows"], want["bad_row"]) == (4, 2, 0)
    raw = R.structured_text([(M + b"1,2,3\n", TILE + 5), (M + b"4\n", 3 * TILE + 5)], 5 * TILE, seed=8)
    want = check_index(lib, raw)
    assert want["nfields"] == 2 * want["nrows"] and want["bad_row"] == raw[:TILE + 5].count(b"\n")


def test_newlines_inside_quotes(lib):
    row = b'1,"x' + M + b'\ny"\n'
    raw = R.structured_text([(row, TILE + 77), (row, 3 * TILE + 78)], 5 * TILE + 9, seed=9)
    want = check_index(lib, raw)
    assert want["quote_row"] == raw[:TILE + 77].count(b"\n") and want["parity"] == 0


def test_quote_that_never_closes(lib):
    raw = R.structured_text([], 2 * TILE + 40, seed=10) + b'9,"abc\n'
    want = check_index(lib, raw)
    assert want["parity"] == 1 and want["quote_row"] == want["nrows"] == raw.count(b"\n") - 1
    raw = b'9,"abc\n' + R.structured_text([], 2 * TILE + 40, seed=10)
    want = check_index(lib, raw)
    assert want["parity"] == 1 and want["quote_row"] == 0


def test_fewer_slots_than_separators(lib):
    raw = R.structured_text([], 2 * TILE + 100, seed=11)
    want = check_index(lib, raw, short=3)
    assert want["nfields"] > TILE // 16


# ---- numbers --------------------------------------------------------------------------------------------
def run_parse(lib, entry, raw, field_end, nrows, ncols, quote, descs, state=None):
    """One call of nvt_csv_parse_many / nvt_csv_parse_datetime with the descriptors (k, dtype) ->
    (list of dict(values, valid, slow), state words).  The spare elements of every buffer are checked."""
    text = _CACHE.get(("text", id(raw))) if len(raw) > (1 << 20) else None
    if text is None:
        text = device_text(raw)
        if len(raw) > (1 << 20):
            _CACHE[("text", id(raw))] = text
            _CACHE[("keep", id(raw))] = raw
    fe = torch.from_numpy(np.ascontiguousarray(field_end, dtype=np.uint32).view(np.int32)).cuda()
    assert len(field_end) >= nrows * ncols
    words = max(1, (nrows + 63) // 64)
    state = fresh_state() if state is None else state
    cols = (_lib.CsvCol * len(descs))()
    bufs = []
    for c, (k, dtype) in zip(cols, descs):
        size = np.dtype(dtype).itemsize
        out, valid = sentinel(size * (nrows + 8)), sentinel(8 * (words + 2))
        slow = sentinel(8 * (words + 2)) if np.dtype(dtype).kind == "f" and entry == "nvt_csv_parse_many" else None
        c.out, c.out_valid, c.k, c.dtype = out.data_ptr(), valid.data_ptr(), k, CODE[dtype]
        c.slow = slow.data_ptr() if slow is not None else None
        bufs.append((out, valid, slow))
    rc = getattr(lib, entry)(text.data_ptr(), len(raw), fe.data_ptr(), nrows, ncols, quote, cols, len(descs),
                             state.data_ptr(), stream())
    assert rc == 0, lib.nvt_last_error()
    st = read_state(state)
    outs = []
    for (out, valid, slow), (k, dtype) in zip(bufs, descs):
        size = np.dtype(dtype).itemsize
        o, v = host(out), host(valid).view(np.uint64)
        assert (o[size * nrows:] == SENT).all() and (v[words:] == SENT64).all()
        s = None
        if slow is not None:
            s = host(slow).view(np.uint64)
            assert (s[words:] == SENT64).all()
            s = s[:words]
        outs.append(dict(values=o[:size * nrows].view(dtype), valid=v[:words], slow=s))
    return outs, st


def bits_of(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_column(got, want, label=""):
    np.testing.assert_array_equal(bits_of(got["values"]), bits_of(want["values"]), err_msg=f"values {label}")
    np.testing.assert_array_equal(got["valid"], want["valid"], err_msg=f"valid {label}")
    if want["slow"] is None:
        assert got["slow"] is None
    else:
        np.testing.assert_array_equal(got["slow"], want["slow"], err_msg=f"slow {label}")
        assert int(sum(bin(int(w)).count("1") for w in got["slow"])) == want["nslow"]
        assert not (got["slow"] & ~got["valid"]).any()              # a declined field carries validity 1 and slow 1


def assert_state(st, wants):
    """Nothing but BAD_FIELD and SLOW moves; they are the least word and the sum over the descriptors."""
    assert st == [0, 0, 0, NONE, NONE, min(w["bad"] for w in wants), sum(w["nslow"] for w in wants), 0]


def corpus_column(name):
    """(raw text, field_end, field bytes) of a corpus laid out as column 1 of 3, tab-separated."""
    if ("column", name) not in _CACHE:
        cells = [s.encode("utf-8") for s in getattr(R, name)()]
        assert not any(b"\t" in c or b"\n" in c or b'"' in c for c in cells)
        raw = R.column_text(cells)
        ix = R.index(raw, len(raw), TAB, QUOTE, 3)
        assert (ix["nrows"], ix["bad_row"], ix["parity"]) == (len(cells), NONE, 0)
        raws, _ = R.field_bytes(raw, ix["field_end"], 3, 1, QUOTE)
        assert raws == cells
        _CACHE[("column", name)] = raw, ix["field_end"], cells
    return _CACHE[("column", name)]


def float_reference():
    if "float64" not in _CACHE:
        _CACHE["float64"] = R.parse_texts(corpus_column("float_corpus")[2], "float64")
    return _CACHE["float64"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_float_corpus(lib, dtype):
    raw, fe, cells = corpus_column("float_corpus")
    vals, codes = float_reference()
    with np.errstate(over="ignore"):
        want = R.parse_outputs(vals.astype(dtype), codes, 1, True)      # float32: the double rounded once more
    assert want["nslow"] >= 20 and want["bad"] != NONE
    (got,), st = run_parse(lib, "nvt_csv_parse_many", raw, fe, len(cells), 3, QUOTE, [(1, dtype)])
    assert_column(got, want, dtype)
    assert_state(st, [want])


@pytest.mark.parametrize("dtype", ["int64", "int32"])
def test_int_corpus(lib, dtype):
    raw, fe, cells = corpus_column("int_corpus")
    vals, codes = R.parse_texts(cells, dtype)
    want = R.parse_outputs(vals, codes, 1, False)
    assert (codes == R.OVERFLOW).sum() >= 10 and (codes == R.INVALID).sum() >= 15
    (got,), st = run_parse(lib, "nvt_csv_parse_many", raw, fe, len(cells), 3, QUOTE, [(1, dtype)])
    assert_column(got, want, dtype)
    assert_state(st, [want])


INT_CELLS = [b"0", b"-1", b"", b'"5"', b'""', b"2147483647", b"-2147483648", b"+7", b"0012", b'"-3"']
BIG_CELLS = [b"9223372036854775807", b"-9223372036854775808", b"", b'"4294967296"', b"-0", b"17"]
FLOAT_CELLS = [b"1.5", b"", b'"2.5"', b'""', b"1e23", b"9007199254740993", b"12345678901234567890123", b"nan", b"-inf",
               b"4.9e-324", b"1e-40", b"9495784171365944765e-329", b'"0.1234567890123456789012"', b"-0.0", b"1e400",
               b"3.4028235677973366e38", b"7.006492321624085e-46"]
MIXED = [(0, "int64", BIG_CELLS), (1, "int32", INT_CELLS), (2, "float64", FLOAT_CELLS), (3, "float32", FLOAT_CELLS),
         (4, "float64", FLOAT_CELLS)]


def mixed_table(n, seed=0, bad=()):
    """n rows of 5 comma-separated columns ending in CRLF (the last column's '\\r' is dropped) ->
    (raw, field_end).  bad: (row, column, bytes) cells put in afterwards."""
    key = ("mixed", n, seed, tuple(bad))
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        rows = [[cells[int(rng.integers(len(cells)))] for _, _, cells in MIXED] for _ in range(n)]
        for r, k, cell in bad:
            rows[r][k] = cell
        raw = b"".join(b",".join(row) + b"\r\n" for row in rows)
        ix = R.index(raw, len(raw), COMMA, QUOTE, 5)
        assert (ix["nrows"], ix["nfields"], ix["bad_row"]) == (n, 5 * n, NONE)
        _CACHE[key] = raw, ix["field_end"]
    return _CACHE[key]


def mixed_reference(n, k, dtype, seed=0, bad=()):
    key = ("mixed_ref", n, seed, tuple(bad), k, dtype)
    if key not in _CACHE:
        raw, fe = mixed_table(n, seed, bad)
        _CACHE[key] = R.parse(raw, len(raw), fe, n, 5, k, QUOTE, dtype)
    return _CACHE[key]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_parse_rows(lib, n):
    raw, fe = mixed_table(n, seed=n)
    descs = [(k, dtype) for k, dtype, _ in MIXED]
    wants = [mixed_reference(n, k, dtype, seed=n) for k, dtype in descs]
    outs, st = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 5, QUOTE, descs)
    for got, want, d in zip(outs, wants, descs):
        assert_column(got, want, str(d))
        assert want["bad"] == NONE
    assert_state(st, wants)
    if n >= 63:
        assert sum(w["nslow"] for w in wants) > 0 and not all(int(w["valid"][0]) == NONE for w in wants)


def test_parse_second_grid_trip(lib):
    # 2048 workgroups of 256 rows, and one row more: one column, ncols = 1, every row end a field end
    n = 2048 * 256 + 1
    rng = np.random.default_rng(5)
    corpus = corpus_column("float_corpus")[2]
    base = [corpus[int(i)] for i in rng.integers(0, len(corpus), 4096)]
    base[0] = b"2.5"
    block = b"".join(c + b"\n" for c in base)
    raw = block * (n // 4096) + base[0] + b"\n"
    ends = np.cumsum([len(c) + 1 for c in base]) - 1
    fe = np.concatenate([(ends[None, :] + len(block) * np.arange(n // 4096)[:, None]).reshape(-1), [len(raw) - 1]])
    assert len(fe) == n and raw[int(fe[-2])] == 10
    wants = []
    for dtype in ("float64", "int32"):
        vals, codes = R.parse_texts(base, dtype)
        vals, codes = np.concatenate([np.tile(vals, n // 4096), vals[:1]]), np.concatenate([np.tile(codes, n // 4096), codes[:1]])
        wants.append(R.parse_outputs(vals, codes, 0, dtype == "float64"))
    assert wants[0]["values"][-1] == 2.5 and wants[1]["bad"] == (0 << 24 | 0 << 2 | R.INVALID)
    outs, st = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 1, QUOTE, [(0, "float64"), (0, "int32")])
    for got, want in zip(outs, wants):
        assert_column(got, want)
    assert_state(st, wants)


COMBOS = [(0, "int64"), (0, "float64"), (1, "int32"), (1, "int64"), (2, "float64"), (2, "float32"), (3, "float32"),
          (4, "float64"), (4, "float32"), (1, "float32"), (0, "int32")]      # (0, "int32"): some cells overflow


@pytest.mark.parametrize("ndesc", [1, 64, 65, 130])
def test_descriptor_batches(lib, ndesc):
    n = 257
    raw, fe = mixed_table(n, seed=n)
    descs = [COMBOS[(i * 7 + i // len(COMBOS)) % len(COMBOS)] for i in range(ndesc)]
    wants = [mixed_reference(n, k, dtype, seed=n) for k, dtype in descs]
    outs, st = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 5, QUOTE, descs)
    for i, (got, want) in enumerate(zip(outs, wants)):
        assert_column(got, want, f"descriptor {i} {descs[i]}")
    assert_state(st, wants)
    if ndesc > _lib.CSV_MAX_COLS:
        assert {(0, "int64"), (0, "float64")} <= set(descs) and (ndesc == 65 or len(set(descs[_lib.CSV_MAX_COLS:])) > 1)
        # a later launch of the call writes what a call of its own writes
        for i in (_lib.CSV_MAX_COLS, ndesc - 1):
            (alone,), _ = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 5, QUOTE, [descs[i]])
            for part in ("values", "valid", "slow"):
                assert (outs[i][part] is None) == (alone[part] is None)
                if alone[part] is not None:
                    np.testing.assert_array_equal(bits_of(outs[i][part]), bits_of(alone[part]), err_msg=f"{part} of {i}")


def test_bad_field_is_the_least(lib):
    n = 300
    bad = ((200, 0, b"x"), (150, 2, b"1.5x"), (250, 2, b"--1"), (150, 1, b"2147483648"), (100, 1, b"99999999999"),
           (299, 1, b"1.0"), (100, 4, b"abc"))
    raw, fe = mixed_table(n, seed=1, bad=bad)
    descs = [(2, "float64")] * 64 + [(0, "int64")] * 5 + [(1, "int32")] + [(1, "int64")] + [(4, "float32")]
    wants = [mixed_reference(n, k, dtype, seed=1, bad=bad) for k, dtype in descs]
    word = lambda r, k, code: r << 24 | k << 2 | code
    assert wants[0]["bad"] == word(150, 2, R.INVALID) and wants[64]["bad"] == word(200, 0, R.INVALID)
    assert wants[69]["bad"] == word(100, 1, R.OVERFLOW) and wants[70]["bad"] == word(299, 1, R.INVALID)
    assert wants[71]["bad"] == word(100, 4, R.INVALID)
    state = fresh_state()
    outs, st = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 5, QUOTE, descs, state)
    for got, want in zip(outs, wants):
        assert_column(got, want)
    assert st[_lib.CSV_ST_BAD_FIELD] == word(100, 1, R.OVERFLOW)      # from the 70th descriptor, the second launch
    assert_state(st, wants)
    # the first 64 alone: the least of one launch
    _, st = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 5, QUOTE, descs[:64])
    assert st[_lib.CSV_ST_BAD_FIELD] == word(150, 2, R.INVALID)
    # a second call on the state of the first keeps the earlier, smaller word, and adds its slow fields
    _, st2 = run_parse(lib, "nvt_csv_parse_many", raw, fe, n, 5, QUOTE, [(0, "int64"), (2, "float64")], state)
    assert st2[_lib.CSV_ST_BAD_FIELD] == word(100, 1, R.OVERFLOW)
    assert st2[_lib.CSV_ST_SLOW] == sum(w["nslow"] for w in wants) + wants[0]["nslow"] > 64


# ---- strings --------------------------------------------------------------------------------------------
def run_strings(lib, raw, field_end, nrows, ncols, k, quote, short=0):
    """nvt_csv_str_offsets + nvt_csv_str_copy -> dict(offsets, valid, chars, total), state words."""
    text = device_text(raw)
    fe = torch.from_numpy(np.ascontiguousarray(field_end, dtype=np.uint32).view(np.int32)).cuda()
    words = max(1, (nrows + 63) // 64)
    need = C.c_uint64()
    assert lib.nvt_csv_str_ws_bytes(nrows, C.byref(need)) == 0
    ws, offsets, valid, state = sentinel(need.value), sentinel(4 * (nrows + 1 + 4)), sentinel(8 * (words + 2)), fresh_state()
    rc = lib.nvt_csv_str_offsets(text.data_ptr(), len(raw), fe.data_ptr(), nrows, ncols, k, quote, offsets.data_ptr(),
                                 valid.data_ptr(), ws.data_ptr(), need.value, state.data_ptr(), stream())
    assert rc == 0, lib.nvt_last_error()
    off, v = host(offsets).view(np.int32), host(valid).view(np.uint64)
    assert (off[nrows + 1:] == np.int32(-0x5A5A5A5B)).all() and (v[words:] == SENT64).all()
    total = int(off[nrows])
    chars = sentinel(total + 16)
    rc = lib.nvt_csv_str_copy(text.data_ptr(), len(raw), fe.data_ptr(), nrows, ncols, k, quote, offsets.data_ptr(),
                              chars.data_ptr(), total - short, stream())
    assert rc == 0, lib.nvt_last_error()
    ch = host(chars)
    assert (ch[total - short:] == SENT).all()                  # nothing at or past chars_bytes
    return dict(offsets=off[:nrows + 1], valid=v[:words], chars=ch[:total - short], total=total), read_state(state)


def check_strings(lib, raw, ncols, k, quote, sep=COMMA, short=0):
    ix = R.index(raw, len(raw), sep, quote, ncols)
    assert ix["bad_row"] == NONE and ix["parity"] == 0 and ix["nfields"] == ix["nrows"] * ncols
    n = ix["nrows"]
    want = R.str_buffers(raw, len(raw), ix["field_end"], n, ncols, k, quote)
    got, st = run_strings(lib, raw, ix["field_end"], n, ncols, k, quote, short)
    np.testing.assert_array_equal(got["offsets"], want["offsets"])
    np.testing.assert_array_equal(got["valid"], want["valid"])
    np.testing.assert_array_equal(got["chars"], want["chars"][:len(want["chars"]) - short])
    assert st == [0, 0, 0, NONE, NONE, want["bad"], 0, 0]
    return want


STRING_CELLS = [b'""', b'""""', b'"a""b"', b'"""a"""', b'"a,b"', b"plain", b"", "naïve ✓ 日本".encode(), b'"' + "ü,ß".encode() + b'"',
                b'"x"', b"x", b'","', b'""""""', b'"a""""b"', b"NA", b'"tail"""', b'"""head"']


def string_table(n, seed, eol=b"\n", cells=STRING_CELLS):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        row = [str(i).encode()] + [cells[int(rng.integers(len(cells)))] for _ in range(2)]
        if i == 1:
            row[1] = b'"' + b'long ""field"", ' * 313 + b'"'        # 5 008 bytes in the file
        rows.append(b",".join(row) + eol)
    return b"".join(rows)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_strings(lib, n):
    raw = string_table(n, seed=n, eol=b"\r\n" if n % 2 else b"\n")
    seen = set()
    for k in (1, 2):
        want = check_strings(lib, raw, 3, k, QUOTE)
        assert want["bad"] == NONE
        seen |= set(want["strings"])
        if n > 1 and k == 1:
            assert want["strings"][1] == b'long "field", ' * 313
    if n >= 63:
        assert {b"", b'"', b'a"b', b'"a"', b"a,b", b'""', "ü,ß".encode()} <= seen


def test_strings_with_quoting_off(lib):
    cells = [c for c in STRING_CELLS if b"," not in c]
    raw = string_table(200, seed=3, eol=b"\r\n", cells=cells).replace(b'long ""field"", ', b'long ""field""; ')
    for k in (1, 2):
        want = check_strings(lib, raw, 3, k, -1)
    assert b'"a""b"' in want["strings"] and b'""' in want["strings"]      # the quotes are kept


def test_undoubled_quote(lib):
    raw = string_table(257, seed=4)
    rows = raw.split(b"\n")
    for r in (70, 200):
        rows[r] = str(r).encode() + b',"a"b"c",ok'
    rows[130] = b'130,fine,"p"q"r"'
    raw = b"\n".join(rows)
    assert check_strings(lib, raw, 3, 1, QUOTE)["bad"] == (70 << 24 | 1 << 2 | R.INVALID)
    assert check_strings(lib, raw, 3, 2, QUOTE)["bad"] == (130 << 24 | 2 << 2 | R.INVALID)
    assert check_strings(lib, raw, 3, 0, QUOTE)["bad"] == NONE


def test_chars_clamp(lib):
    for n in (1, 64, 257):
        raw = string_table(n, seed=n + 1) + b'9,"tail""s",lastcell\n'
        check_strings(lib, raw, 3, 1, QUOTE, short=5)
        check_strings(lib, raw, 3, 2, QUOTE, short=5)


# ---- datetimes ------------------------------------------------------------------------------------------
def test_datetime_corpus(lib):
    raw, fe, cells = corpus_column("datetime_corpus")
    n = len(cells)
    want = R.parse_datetime(raw, len(raw), fe, n, 3, 1, QUOTE)
    vals, codes = R.parse_datetime_texts(cells)
    assert (codes == R.OK).sum() > 2400 and (codes == R.OVERFLOW).sum() >= 6 and (codes == R.INVALID).sum() >= 25
    first = int(np.flatnonzero(codes >= R.INVALID)[0])
    assert want["bad"] == (first << 24 | 1 << 2 | int(codes[first]))
    outs, st = run_parse(lib, "nvt_csv_parse_datetime", raw, fe, n, 3, QUOTE, [(1, "int64")] * 65)
    for i, got in enumerate(outs):
        np.testing.assert_array_equal(got["values"], want["values"], err_msg=f"descriptor {i}")
        np.testing.assert_array_equal(got["valid"], want["valid"], err_msg=f"descriptor {i}")
    assert st == [0, 0, 0, NONE, NONE, want["bad"], 0, 0]
    # quoted and empty fields, CRLF on the last column; the row numbers of column 0 are no dates
    cells = [b'"2024-01-05 10:00:00.5"', b"", b'""', b"2024-02-29T23:59", b'"2023-02-29"', b"1969-12-31"] * 30
    raw = R.column_text(cells, ncols=2, k=1, sep=b",", eol=b"\r\n")
    ix = R.index(raw, len(raw), COMMA, QUOTE, 2)
    wants = [R.parse_datetime(raw, len(raw), ix["field_end"], 180, 2, k, QUOTE) for k in (1, 0)]
    assert wants[0]["bad"] == (4 << 24 | 1 << 2 | R.INVALID) and wants[1]["bad"] == (0 << 24 | 0 << 2 | R.INVALID)
    outs, st = run_parse(lib, "nvt_csv_parse_datetime", raw, ix["field_end"], 180, 2, QUOTE, [(1, "int64"), (0, "int64")])
    for got, want in zip(outs, wants):
        np.testing.assert_array_equal(got["values"], want["values"])
        np.testing.assert_array_equal(got["valid"], want["valid"])
    assert st == [0, 0, 0, NONE, NONE, wants[1]["bad"], 0, 0]
