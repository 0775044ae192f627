"""Pins csv_reference.py -- the reference test_gpu_csv_kernels.py compares the nvt_csv_* kernels
with -- to csv.reader, pandas, float(), int() and numpy, and runs its corpora through the host
entries of the scalar parsers (nvt_csv_parse_f64_host, _i64_host, _datetime_host): every return
code, every DECLINED and every bit of every value.  Runs without a GPU.

The reference follows the kernels' parity rule: a quote toggles the inside-quotes state wherever it
stands.  On well-formed text (quotes only wrap whole fields, a quote inside is doubled) that is what
csv.reader and pandas do; on other text it is not, and test_parity_rule_on_malformed_text pins
three such strings by hand."""
import collections
import csv
import ctypes as C
import fractions
import io
import struct

import numpy as np
import pandas as pd
import pytest

import csv_reference as R
from nvtabular_amd import _lib

OK, DECLINED, INVALID, OVERFLOW, NULL = R.OK, R.DECLINED, R.INVALID, R.OVERFLOW, R.NULL


@pytest.fixture(scope="module")
def float_corpus():
    return R.float_corpus()


# ---- index, fields, strings against csv.reader and pandas -------------------------------------------
WORDS = ["plain", "with,comma", 'say "hi"', "", "naïve ✓ 日本", "NA", "x", ",", '"', '""', "tab\there", "a|b", "a" * 37,
         '"quoted"', 'end"', '"start', "12", "-3.5"]


def well_formed(n, sep, eol, quote, seed):
    """(text, rows): n rows of 4 fields; with quoting a field that holds the separator or a quote
    is wrapped (some others too), without it such fields are not drawn."""
    rng = np.random.default_rng(seed)
    rows, lines = [], []
    for _ in range(n):
        row, cells = [], []
        for _ in range(4):
            w = WORDS[int(rng.integers(len(WORDS)))]
            if quote is None:
                w = w.replace(sep, ";")
                cells.append(w)
            elif sep in w or '"' in w or (w and rng.random() < 0.2) or (w == "" and rng.random() < 0.5):
                cells.append('"' + w.replace('"', '""') + '"')
            else:
                cells.append(w)
            row.append(w)
        rows.append(row)
        lines.append(sep.join(cells) + eol)
    return "".join(lines).encode("utf-8"), rows


@pytest.mark.parametrize("eol", ["\n", "\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("sep", [",", "\t", "|"], ids=["comma", "tab", "bar"])
@pytest.mark.parametrize("quote", ['"', None], ids=["quoted", "noquote"])
def test_index_fields_strings_equal_csv_reader_and_pandas(sep, eol, quote):
    text, rows = well_formed(300, sep, eol, quote, seed=len(eol) * 7 + ord(sep))
    q = ord('"') if quote else -1
    ix = R.index(text, len(text), ord(sep), q, 4)
    assert (ix["nrows"], ix["nfields"], ix["parity"], ix["bad_row"], ix["quote_row"]) == (300, 1200, 0, R.NONE, R.NONE)
    kw = dict(quotechar='"') if quote else dict(quoting=csv.QUOTE_NONE)
    got = list(csv.reader(io.StringIO(text.decode("utf-8"), newline=""), delimiter=sep, **kw))
    assert got == rows
    frame = pd.read_csv(io.BytesIO(text), sep=sep, header=None, dtype=str, keep_default_na=False, na_values=[""],
                        quoting=csv.QUOTE_MINIMAL if quote else csv.QUOTE_NONE)
    for k in range(4):
        b = R.str_buffers(text, len(text), ix["field_end"], 300, 4, k, q)
        assert [s.decode("utf-8") for s in b["strings"]] == [r[k] for r in rows]
        assert b["bad"] == R.NONE and b["offsets"].dtype == np.int32 and b["offsets"][0] == 0
        chars = b["chars"].tobytes()
        assert [chars[a:e] for a, e in zip(b["offsets"][:-1], b["offsets"][1:])] == b["strings"]
        valid = np.unpackbits(b["valid"].view(np.uint8), bitorder="little")
        np.testing.assert_array_equal(valid[:300].astype(bool), frame[k].notna().to_numpy())
        assert not valid[300:].any()
        assert [s.decode("utf-8") for s, v in zip(b["strings"], valid) if v] == frame[k].dropna().tolist()


def test_parity_rule_on_malformed_text():
    q, c = ord('"'), ord(",")
    # a quote in the middle of a field opens a quoted stretch: one field, no error in the index
    t = b'ab"c,d"e\n'
    ix = R.index(t, len(t), c, q, 1)
    assert ix["field_end"].tolist() == [8] and (ix["nrows"], ix["parity"], ix["bad_row"]) == (1, 0, R.NONE)
    assert R.str_buffers(t, len(t), ix["field_end"], 1, 1, 0, q)["strings"] == [b'ab"c,d"e']    # not wrapped: kept
    # a stray quote swallows the line end: the next row's newline closes nothing, the text ends inside
    t = b'1,w"\n2,v\n'
    ix = R.index(t, len(t), c, q, 2)
    assert ix["field_end"].tolist() == [1] and (ix["nrows"], ix["parity"], ix["quote_row"]) == (0, 1, 0)
    # lone quotes inside a wrapped field: csv.reader ends the field at `"a"` and reads two fields; by
    # parity the comma follows three quotes and is inside, so this is one field, whose lone quotes the
    # string column keeps and posts as INVALID
    t = b'"a"b",c"\n'
    ix = R.index(t, len(t), c, q, 1)
    assert ix["field_end"].tolist() == [8] and (ix["nrows"], ix["parity"], ix["bad_row"]) == (1, 0, R.NONE)
    b = R.str_buffers(t, len(t), ix["field_end"], 1, 1, 0, q)
    assert b["strings"] == [b'a"b",c'] and b["bad"] == (0 << 24 | 0 << 2 | INVALID)
    assert len(next(csv.reader([t.decode()]))) == 2


def test_index_errors_and_crlf_by_hand():
    c, q = ord(","), ord('"')
    t = b"1,2\n3\n4,5,6\n7,8\n"
    ix = R.index(t, len(t), c, q, 2)
    assert (ix["nrows"], ix["nfields"], ix["bad_row"]) == (4, 8, 1)          # the totals balance
    t = b'1,"x\ny"\n2,"p\nq"\n'
    assert R.index(t, len(t), c, q, 2)["quote_row"] == 0
    t = b'1,u\n2,"x\ny"\n'
    ix = R.index(t, len(t), c, q, 2)
    assert (ix["quote_row"], ix["nrows"]) == (1, 2)
    t = b'1,"2"\r\n"3"\r,4\r\n'
    ix = R.index(t, len(t), c, q, 2)
    raws, quoted = R.field_bytes(t, ix["field_end"], 2, 1, q)
    assert raws == [b"2", b"4"] and quoted.tolist() == [True, False]
    assert R.field_bytes(t, ix["field_end"], 2, 0, q)[0] == [b"1", b'"3"\r']  # '\r' is dropped on the last column only
    assert R.index(b"a'b,c'\n", 7, c, -1, 2)["nfields"] == 2


def test_words_and_bad_word():
    w = R.pack_words(np.arange(70) % 3 == 0)
    assert w.dtype == np.dtype("<u8") and len(w) == 2
    assert int(w[0]) == sum(1 << i for i in range(0, 64, 3)) and int(w[1]) == (1 << 2 | 1 << 5)
    assert len(R.pack_words([])) == 1 and len(R.pack_words([True] * 64)) == 1
    codes = np.array([OK, NULL, DECLINED, OVERFLOW, INVALID], dtype=np.int8)
    assert R.bad_word(codes, 5) == (3 << 24 | 5 << 2 | OVERFLOW)
    assert R.bad_word(codes[:3], 5) == R.NONE


# ---- numbers ------------------------------------------------------------------------------------------
# what float() takes and the grammar does not: blanks, underscores, digits that are not ASCII
FLOAT_ONLY = {" 1", "1 ", "1_0", "١٢", "１２", "１"}
INT_ONLY = {" 1", "1 ", "1_0", "१२", "１２", "١"}


def python_float(s):
    try:
        return float(s)
    except ValueError:
        return None


def test_float_reference_equals_python_float(float_corpus):
    assert len(float_corpus) >= 200_000
    looser = set()
    raws = [s.encode("utf-8") for s in float_corpus]
    vals, codes = R.parse_texts(raws, "float64")
    v32, codes32 = R.parse_texts(raws[200_000:], "float32")
    np.testing.assert_array_equal(codes32, codes[200_000:])
    for s, raw, v, c in zip(float_corpus, raws, vals.tolist(), codes.tolist()):
        want = python_float(s) if "\x00" not in s else None
        if c == NULL:
            assert s == ""
        elif c == INVALID:
            if want is not None:
                looser.add(s)
        else:
            assert want is not None, s
            if c == OK:
                assert struct.pack("<d", v) == struct.pack("<d", want), s
            else:
                assert v == 0.0 and R.el_class(raw)[0] in ("many", "declined"), s
    assert looser == FLOAT_ONLY
    ok = codes[200_000:] == OK
    with np.errstate(over="ignore"):
        want32 = np.array([float(s) for s, o in zip(float_corpus[200_000:], ok) if o], dtype=np.float64).astype(np.float32)
    np.testing.assert_array_equal(v32[ok].view(np.uint32), want32.view(np.uint32))


def test_int_reference_equals_python_int():
    corpus = R.int_corpus()
    raws = [s.encode("utf-8") for s in corpus]
    looser = set()
    for dtype, lo, hi in (("int64", R.I64_MIN, R.I64_MAX), ("int32", R.I32_MIN, R.I32_MAX)):
        vals, codes = R.parse_texts(raws, dtype)
        assert vals.dtype == np.dtype(dtype)
        for s, v, c in zip(corpus, vals.tolist(), codes.tolist()):
            try:
                want = int(s) if "\x00" not in s else None
            except ValueError:
                want = None
            if c == NULL:
                assert s == ""
            elif c == INVALID:
                if want is not None:
                    looser.add(s)
            elif c == OVERFLOW:
                assert not lo <= want <= hi and v == 0, s
            else:
                assert c == OK and v == want and lo <= want <= hi, s
        for lim in (lo, hi):
            assert codes[corpus.index(str(lim))] == OK
        assert codes[corpus.index(str(lo - 1))] == OVERFLOW and codes[corpus.index(str(hi + 1))] == OVERFLOW
    assert looser == INT_ONLY


def test_halfway_points_are_halfway():
    half = R.halfway_points()
    for q in (-4, -3, -2, -1, 0, 23):
        assert len(half[q]) >= 50, q
    for q, texts in half.items():
        downs = 0
        for w, t in texts:
            assert 0 < w < 10 ** 19 and R.is_halfway(t)
            # the halfway rule is what rounds DOWN to the even neighbour (the plain rounding goes up)
            name, tags = R.el_class(t)
            down = fractions.Fraction(float(t)) < fractions.Fraction(w) * fractions.Fraction(10) ** q
            assert name == "el" and ("halfway" in tags) == down, t
            downs += down
            for other in (w - 1, w + 1):       # (at q = 23 the powers of two 1 and 2 are neighbours)
                assert not R.is_halfway("%de%d" % (other, q)) or (q == 23 and other & (other - 1) == 0)
        # both directions at every exponent but 23, where every string has the mantissa 5^23 of 1e23
        assert 0 < downs and (downs < len(texts) or q == 23), q
    assert not R.is_halfway("0.3") and R.is_halfway("9007199254740993") and R.is_halfway("1e23")


def test_el_class_reaches_every_branch(float_corpus):
    names, tags = collections.Counter(), collections.Counter()
    for s in float_corpus:
        raw = s.encode("utf-8")
        if R.parse_f64_text(raw)[0] == INVALID or not s or (raw[-1] | 0x20) in b"fyn":
            continue
        name, t = R.el_class(raw)
        names[name] += 1
        tags.update(t)
        if name == "el":       # the model itself is right: its bits are float()'s
            w, q, _ = R.decimal_parts(raw.lstrip(b"+-"))
            assert struct.pack("<Q", R.el_step(w, q)[1]) == struct.pack("<d", abs(float(s))), s
    print("el_class:", dict(names), "el tags:", dict(tags), "declined strings:", R.find_declined())
    for name in ("many", "zero", "clinger", "tiny", "huge", "el"):
        assert names[name] > 0, name
    for tag in ("second", "subnormal", "halfway", "carry"):
        assert tags[tag] > 0, tag
    assert names["declined"] == len(R.find_declined())          # (the search found some: see csv_reference.find_declined)
    assert R.el_class("1.7976931348623159e308") == ("el", frozenset({"carry"}))      # the carry to infinity
    assert R.el_class("2.2250738585072012e-308")[1] == {"subnormal"}                 # rounds up to 2^-1022


# ---- the host entries of the scalar parsers ---------------------------------------------------------------
def test_host_f64_equals_the_reference(float_corpus):
    lib = _lib.load()
    out = C.c_double()
    seen = collections.Counter()
    for s in float_corpus:
        raw = s.encode("utf-8")
        want_rc, want = R.parse_f64_text(raw) if raw else (INVALID, 0.0)
        out.value = -7.0
        rc = lib.nvt_csv_parse_f64_host(raw, len(raw), C.byref(out))
        assert rc == want_rc, (s, rc, want_rc)
        seen[rc] += 1
        if rc == OK:
            assert struct.pack("<d", out.value) == struct.pack("<d", want), s
        else:
            assert out.value == -7.0, s                           # nothing is written without OK
        if raw and want_rc != INVALID and (raw[-1] | 0x20) not in b"fyn":
            assert (rc == DECLINED) == (R.el_class(raw)[0] in ("many", "declined")), s
    assert seen[OK] > 200_000 and seen[DECLINED] >= 10 and seen[INVALID] >= 40 and seen[OVERFLOW] == 0


def test_host_i64_equals_the_reference():
    lib = _lib.load()
    out = C.c_int64()
    seen = collections.Counter()
    for s in R.int_corpus():
        raw = s.encode("utf-8")
        want_rc, want = R.parse_i64_text(raw) if raw else (INVALID, 0)
        out.value = -7
        rc = lib.nvt_csv_parse_i64_host(raw, len(raw), C.byref(out))
        assert rc == want_rc, (s, rc, want_rc)
        assert out.value == (want if rc == OK else -7), s
        seen[rc] += 1
    assert seen[OK] > 600 and seen[INVALID] >= 20 and seen[OVERFLOW] >= 10 and seen[DECLINED] == 0


def test_datetime_reference_equals_pandas_and_the_host_entry():
    corpus = R.datetime_corpus()
    lib = _lib.load()
    out = C.c_int64()
    codes = []
    valid = []
    for s in corpus:
        raw = s.encode("utf-8")
        want_rc, want = R.parse_datetime_text(raw)
        out.value = -7
        rc = lib.nvt_csv_parse_datetime_host(raw, len(raw), C.byref(out))
        assert rc == want_rc, (s, rc, want_rc)
        assert out.value == (want if rc == OK else -7), s
        codes.append(rc)
        if rc == OK:
            valid.append((s, want))
    assert {len(s) for s, _ in valid} == {10, 16, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29}
    assert len(valid) > 2400
    exp = pd.to_datetime(pd.Series([s for s, _ in valid]), format="ISO8601")
    assert exp.dtype == np.dtype("datetime64[ns]")
    np.testing.assert_array_equal(np.array([v for _, v in valid], dtype=np.int64), exp.to_numpy().view(np.int64))
    by_text = dict(zip(corpus, codes))
    assert all(by_text[s] == OK for s in R.VALID_DATETIMES)
    assert all(by_text[s] == INVALID for s in R.INVALID_DATETIMES)
    assert all(by_text[s] == OVERFLOW for s in R.OVERFLOW_DATETIMES)
    assert R.parse_datetime_text(R.FIRST_NS.encode()) == (OK, R.I64_MIN + 1)
    assert R.parse_datetime_text(R.LAST_NS.encode()) == (OK, R.I64_MAX)
    assert by_text["0000-01-01"] == INVALID and by_text["2262-04-11 23:47:17"] == OVERFLOW


# ---- the column and text builders ---------------------------------------------------------------------------
def test_parse_of_a_column():
    cells = [b"1.5", b"", b'"2.5"', b'""', b"x", b"12345678901234567890123", b"1e400", b"-0.0"]
    text = R.column_text(cells, ncols=3, k=2, sep=b",", eol=b"\r\n")
    ix = R.index(text, len(text), ord(","), ord('"'), 3)
    assert (ix["nrows"], ix["nfields"], ix["bad_row"]) == (8, 24, R.NONE)
    p = R.parse(text, len(text), ix["field_end"], 8, 3, 2, ord('"'), "float64")
    assert p["values"].tobytes() == struct.pack("<8d", 1.5, np.nan, 2.5, np.nan, 0, 0, np.inf, -0.0)
    assert p["valid"].tolist() == [0b11100101] and p["slow"].tolist() == [0b00100000] and p["nslow"] == 1
    assert p["bad"] == (4 << 24 | 2 << 2 | INVALID)
    p = R.parse(text, len(text), ix["field_end"], 8, 3, 0, ord('"'), "int32")
    assert p["values"].tolist() == list(range(8)) and p["valid"].tolist() == [255] and p["slow"] is None
    assert p["bad"] == R.NONE


@pytest.mark.parametrize("position", [15, 1023, 4095, (1 << 20) - 1])
def test_structured_text_places_the_marked_byte(position):
    m = bytes([R.MARK])
    for row, byte in ((b'12,' + m + b'"ab,cd"\n', b'"'), (b'12,"ab,cd' + m + b'"\n', b'"'), (b'12,"ab' + m + b'""cd"\n', b'"'),
                      (b'12,"ab' + m + b',cd"\n', b','), (b'12,abc' + m + b'\n', b'\n')):
        size = (position + 300 + 15) // 16 * 16 + 3
        text = R.structured_text([(row, position)], size)
        assert len(text) == size and text[position:position + 1] == byte and bytes([R.MARK]) not in text
        clean = row.replace(m, b"")
        at = position - row.index(m)
        assert text[at:at + len(clean)] == clean and (at == 0 or text[at - 1:at] == b"\n")
        ix = R.index(text, size, ord(","), ord('"'), 2)
        assert ix["bad_row"] == R.NONE and ix["quote_row"] == R.NONE and ix["parity"] == 0
        assert ix["nfields"] == 2 * ix["nrows"]
        assert len(list(csv.reader(io.StringIO(text.decode(), newline="")))) == ix["nrows"]
