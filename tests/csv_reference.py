"""The contract of the delimited-text reader (include/nvt_hip.h, the header comments of
nvtabular_amd/csrc/nvt_csv.hip, nvt_csv_parse.hpp and nvt_datetime.hpp) restated in numpy and plain
Python, plus the corpora that the CPU and GPU tests lay out as columns.  test_csv_reference.py pins
this module to csv.reader, pandas, float(), int() and numpy on the CPU; test_gpu_csv_kernels.py
compares the nvt_csv_* entries with it, bit for bit.

Choices where the header is silent (the kernels' current behaviour, kept):
  * the value slot of a field that does not parse (INVALID / OVERFLOW) and of a declined float is 0;
    only the empty field of a float column holds NaN;
  * ``5.`` is a number (the header's grammar line reads digits[.digits]; test_csv_host.py pins
    ``5.`` as one), ``.`` alone is not;
  * an integer column has no slow bitmap (the descriptor's ``slow`` is NULL);
  * a lone quote inside a quoted string field is copied as it stands (and posted as INVALID);
  * a datetime in year 0000 is INVALID (numpy has such a year, pandas' Timestamp does not);
  * text that is not well formed follows the parity rule and nothing else: a quote toggles the
    state wherever it stands, so ``ab"c,d"e`` is one field (test_csv_reference.py pins three such
    strings by hand).
"""
import fractions
import importlib.util
import itertools
import os
import re

import numpy as np

NONE = (1 << 64) - 1
OK, DECLINED, INVALID, OVERFLOW = 0, 1, 2, 3
NULL = -1                      # the "return code" of an empty field in this module
TILE, STEP, MAX_COLS = 4096, 256, 64
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NL, CR = 10, 13


# ---- index --------------------------------------------------------------------------------------
def as_bytes_array(text, nbytes=None):
    a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
    return a if nbytes is None else a[:nbytes]


def index(text, nbytes, sep, quote, ncols):
    """dict(field_end, nfields, nrows, parity, bad_row, quote_row) of text[:nbytes]."""
    t = as_bytes_array(text, nbytes)
    inside = (np.cumsum(t == quote) & 1).astype(bool) if quote >= 0 else np.zeros(len(t), bool)
    newline = t == NL
    ends = ((t == sep) | newline) & ~inside
    field_end = np.flatnonzero(ends).astype(np.uint32)
    row_end = np.flatnonzero(newline & ~inside)
    rank = np.searchsorted(field_end, row_end)                  # the separator rank of every row end
    rows = np.arange(len(row_end), dtype=np.int64)
    wrong = np.flatnonzero(rank != (rows + 1) * ncols - 1)
    quoted_nl = np.flatnonzero(newline & inside)
    return dict(field_end=field_end, nfields=len(field_end), nrows=len(row_end),
                parity=int(inside[-1]) if len(t) and quote >= 0 else 0,
                bad_row=int(wrong[0]) if len(wrong) else NONE,
                quote_row=int(np.searchsorted(row_end, quoted_nl[0])) if len(quoted_nl) else NONE)


def fields(text, field_end, ncols, k, quote, nrows=None):
    """(start, end, quoted) of field k of every row: the '\\r' of a CRLF end dropped on the last
    column, then the outer quotes dropped (quoted[r] tells where they were)."""
    t = as_bytes_array(text)
    fe = np.asarray(field_end, dtype=np.int64)
    n = len(fe) // ncols if nrows is None else nrows
    f = np.arange(n, dtype=np.int64) * ncols + k
    e = fe[f]
    s = np.where(f > 0, fe[np.maximum(f - 1, 0)] + 1, 0)
    if k == ncols - 1:
        e = e - ((e > s) & (t[np.maximum(e - 1, 0)] == CR))
    if quote >= 0 and n:
        q = (e - s >= 2) & (t[np.minimum(s, len(t) - 1)] == quote) & (t[np.maximum(e - 1, 0)] == quote)
    else:
        q = np.zeros(n, bool)
    return s + q, e - q, q


def field_bytes(text, field_end, ncols, k, quote, nrows=None):
    t = bytes(as_bytes_array(text))
    s, e, q = fields(text, field_end, ncols, k, quote, nrows)
    return [t[a:b] for a, b in zip(s.tolist(), e.tolist())], q


# ---- numbers --------------------------------------------------------------------------------------
_FLOAT = re.compile(rb"[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?"
                    rb"|[nN][aA][nN])")
_NUMBER = re.compile(rb"[+-]?([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?")
_INT = re.compile(rb"[+-]?[0-9]+")
_POW5 = {}


def pow5(q):
    """(hi, lo) of the 128-bit power of five that gen_csv_pow5.py writes for the exponent q."""
    if not _POW5:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nvtabular_amd", "csrc", "gen_csv_pow5.py")
        spec = importlib.util.spec_from_file_location("gen_csv_pow5", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        for e in range(mod.QMIN, mod.QMAX + 1):
            v = mod.entry(e)
            _POW5[e] = (v >> 64, v & NONE)
    return _POW5[q]


def decimal_parts(raw):
    """(w, q, digits) of a string of the float grammar that is no special: the significant digits as
    an integer, the decimal exponent of its last digit, and how many digits those are."""
    m = _NUMBER.fullmatch(raw)
    whole, frac, exp = m.group(1), m.group(2) or b"", int(m.group(3) or 0)
    digits = (whole + frac).lstrip(b"0")
    return int(digits or b"0"), exp - len(frac), len(digits)


def el_step(w, q):
    """The Eisel-Lemire step of nvt_csv_parse.hpp in Python integers for 0 < w < 2^64 and
    -342 <= q <= 308: (tags, bits) with bits None when the step declines."""
    lz = 64 - w.bit_length()
    w <<= lz
    hi, lo = pow5(q)
    first = w * hi
    upper, lower = first >> 64, first & NONE
    tags = set()
    if upper & 0x1FF == 0x1FF:
        tags.add("second")
        total = (upper << 64 | lower) + (w * lo >> 64)
        upper, lower = total >> 64, total & NONE
    if lower == NONE and not -27 <= q <= 55:
        return {"declined"}, None
    upperbit = upper >> 63
    shift = upperbit + 9
    m = upper >> shift
    power2 = ((217706 * q) >> 16) + 63 + upperbit - lz + 1023
    if power2 <= 0:
        tags.add("subnormal")
        if 1 - power2 >= 64:
            return tags, 0
        m >>= 1 - power2
        m = (m + (m & 1)) >> 1
        return tags, m            # (m = 2^52 is the smallest normal number: the pattern is the same)
    if lower <= 1 and -4 <= q <= 23 and m & 3 == 1 and m << shift == upper:
        tags.add("halfway")
        m &= ~1
    m = (m + (m & 1)) >> 1
    if m >= 2 << 52:
        tags.add("carry")
        m = 1 << 52
        power2 += 1
    if power2 >= 0x7FF:
        return tags, 0x7FF << 52
    return tags, (m & ~(1 << 52)) | power2 << 52


def el_class(text):
    """The route a string of the float grammar (no special) takes through csv_parse_f64:
    (name, tags) with name one of many, zero, clinger, tiny, huge, declined, el."""
    raw = text if isinstance(text, bytes) else text.encode()
    w, q, digits = decimal_parts(raw)
    none = frozenset()
    if digits > 19:
        return "many", none
    if w == 0:
        return "zero", none
    if w <= 1 << 53 and -22 <= q <= 22:
        return "clinger", none
    if q < -342:
        return "tiny", none
    if q > 308:
        return "huge", none
    tags, bits = el_step(w, q)
    return ("declined", none) if bits is None else ("el", frozenset(tags))


def parse_f64_text(raw):
    """(code, value) of one field: the grammar first, then float()."""
    if not _FLOAT.fullmatch(raw):
        return INVALID, 0.0
    if (raw[-1] | 0x20) in (0x66, 0x79, 0x6E):          # f, y, n: a special
        return OK, float(raw.decode())
    if el_class(raw)[0] in ("many", "declined"):
        return DECLINED, 0.0
    return OK, float(raw.decode())


def parse_i64_text(raw, lo=I64_MIN, hi=I64_MAX):
    if not _INT.fullmatch(raw):
        return INVALID, 0
    v = int(raw)
    return (OK, v) if lo <= v <= hi else (OVERFLOW, 0)


def pack_words(bits):
    """A bool array as whole little-endian 64-bit words, the bits past the end zero."""
    bits = np.asarray(bits, dtype=bool)
    words = max(1, (len(bits) + 63) // 64)
    padded = np.zeros(words * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view("<u8")


def bad_word(codes, k, row0=0):
    codes = np.asarray(codes)
    bad = np.flatnonzero(codes >= INVALID)
    if not len(bad):
        return NONE
    r = int(bad[0])
    return (r + row0) << 24 | k << 2 | int(codes[r])


def parse_texts(raws, dtype):
    """(values, codes) of a list of field bytes as a column of dtype (a numpy dtype name); an empty
    field has the code NULL.  float32 is the double cast by numpy, which rounds once more."""
    dtype = np.dtype(dtype)
    codes = np.empty(len(raws), dtype=np.int8)
    if dtype.kind == "f":
        vals = np.zeros(len(raws), dtype=np.float64)
        for i, raw in enumerate(raws):
            if not raw:
                codes[i], vals[i] = NULL, np.nan
            else:
                codes[i], vals[i] = parse_f64_text(raw)
        with np.errstate(over="ignore"):
            return vals.astype(dtype), codes
    lo, hi = (I32_MIN, I32_MAX) if dtype.itemsize == 4 else (I64_MIN, I64_MAX)
    vals = np.zeros(len(raws), dtype=dtype)
    for i, raw in enumerate(raws):
        if not raw:
            codes[i] = NULL
        else:
            codes[i], vals[i] = parse_i64_text(raw, lo, hi)
    return vals, codes


def parse_outputs(vals, codes, k, is_float):
    """What nvt_csv_parse_many leaves for one descriptor: dict(values, valid, slow, nslow, bad)."""
    valid = pack_words((codes == OK) | (codes == DECLINED))
    slow = pack_words(codes == DECLINED) if is_float else None
    return dict(values=vals, valid=valid, slow=slow, nslow=int((codes == DECLINED).sum()) if is_float else 0,
                bad=bad_word(codes, k))


def parse(text, nbytes, field_end, nrows, ncols, k, quote, dtype):
    raws, _ = field_bytes(as_bytes_array(text, nbytes), field_end, ncols, k, quote, nrows)
    vals, codes = parse_texts(raws, dtype)
    return parse_outputs(vals, codes, k, np.dtype(dtype).kind == "f")


# ---- strings ----------------------------------------------------------------------------------------
def unquote(inner, quote):
    """(bytes with doubled quotes undone, malformed) of the inside of a quoted field."""
    q = bytes([quote])
    if q not in inner:
        return inner, False
    out, i, bad = bytearray(), 0, False
    while i < len(inner):
        if inner[i] == quote:
            if i + 1 < len(inner) and inner[i + 1] == quote:
                i += 1
            else:
                bad = True
        out.append(inner[i])
        i += 1
    return bytes(out), bad


def str_buffers(text, nbytes, field_end, nrows, ncols, k, quote):
    """dict(offsets int32[nrows + 1], chars, valid words, bad, strings) of field k as a string column."""
    raws, quoted = field_bytes(as_bytes_array(text, nbytes), field_end, ncols, k, quote, nrows)
    out, codes = [], np.zeros(len(raws), dtype=np.int8)
    for i, (raw, q) in enumerate(zip(raws, quoted.tolist())):
        if q:
            raw, bad = unquote(raw, quote)
            codes[i] = INVALID if bad else OK
        out.append(raw)
    lengths = np.array([len(b) for b in out], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return dict(offsets=offsets, chars=np.frombuffer(b"".join(out), dtype=np.uint8), valid=pack_words(lengths > 0),
                bad=bad_word(codes, k), strings=out)


# ---- datetimes ----------------------------------------------------------------------------------------
_DATETIME = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})"
                       rb"(?:[T ]([0-9]{2}):([0-9]{2})(?::([0-9]{2})(?:\.([0-9]{1,9}))?)?)?")


def parse_datetime_text(raw):
    """(code, nanoseconds) of YYYY-MM-DD[(T| )HH:MM[:SS[.f{1,9}]]]: the calendar is numpy's."""
    m = _DATETIME.fullmatch(raw)
    if not m:
        return INVALID, 0
    y, mo, d, h, mi, s = (int(g or 0) for g in m.groups()[:6])
    frac = m.group(7) or b""
    if y < 1 or h > 23 or mi > 59 or s > 59:
        return INVALID, 0
    try:
        days = int(np.datetime64("%04d-%02d-%02d" % (y, mo, d), "D").astype(np.int64))
    except ValueError:
        return INVALID, 0
    ns = ((days * 24 + h) * 60 + mi) * 60 + s
    ns = ns * 10 ** 9 + int(frac.ljust(9, b"0") or 0)
    return (OK, ns) if I64_MIN < ns <= I64_MAX else (OVERFLOW, 0)       # INT64_MIN is NaT


def parse_datetime_texts(raws):
    vals, codes = np.zeros(len(raws), dtype=np.int64), np.empty(len(raws), dtype=np.int8)
    for i, raw in enumerate(raws):
        if not raw:
            codes[i] = NULL
        else:
            codes[i], vals[i] = parse_datetime_text(raw)
    return vals, codes


def parse_datetime(text, nbytes, field_end, nrows, ncols, k, quote):
    """dict(values, valid, bad) of field k as a datetime64[ns] column."""
    raws, _ = field_bytes(as_bytes_array(text, nbytes), field_end, ncols, k, quote, nrows)
    vals, codes = parse_datetime_texts(raws)
    return dict(values=vals, valid=pack_words(codes == OK), bad=bad_word(codes, k))


# ---- corpora ------------------------------------------------------------------------------------------
INVALID_FLOATS = ["", "-", "+", ".", "e5", "1e", "1e+", "1.2.3", "12a", " 1", "1 ", "0x10", "1_0", "in", "nanx", "--1",
                  "1,5"]            # test_csv_host.test_parse_f64_fixed_list
MORE_INVALID_FLOATS = ["1e5.5", "1.5e", "infinit", "infinityy", "nan0", "+-1", "1-", "0x1p3", "1d5", "1f", "١٢", "１２",
                       "1\x00", "+.", "-.e1", "inf1", "i", "n", "1e-", "1ee5", "１", "1.e", "e", "+e5", "nan(1)"]
INVALID_INTS = ["", "1.0", "12a", "-", "+", " 1", "1 ", "0x1", "1e3", "99999999999999999999999999x"]   # test_parse_i64
MORE_INVALID_INTS = ["1_0", "--1", "+-1", "1-", "१२", "１２", "1\x00", "1,5", "0b1", "١"]


def is_halfway(text):
    """Does the decimal string lie exactly between two neighbouring doubles?"""
    raw = text.encode()
    w, q, _ = decimal_parts(raw.lstrip(b"+-"))
    exact = fractions.Fraction(w) * fractions.Fraction(10) ** q
    d = abs(float(text))
    for other in (np.nextafter(d, np.inf), np.nextafter(d, -np.inf)):
        if np.isfinite(other) and (fractions.Fraction(d) + fractions.Fraction(float(other))) / 2 == exact:
            return True
    return False


def with_point(w, q):
    """w * 10^q (q < 0) written with a decimal point in place of the exponent."""
    s = str(w).rjust(1 - q, "0")
    return s[:q] + "." + s[q:]


def halfway_points(per_exponent=60, seed=5):
    """{q: [(w, text)]}: strings w * 10^q (0 < w < 10^19, not on the Clinger path) that lie exactly
    between two doubles.  w * 10^q = u * 2^j * 5^q * 2^q with u * 5^q (q >= 0) or u itself (q < 0,
    w = u * 5^-q) an odd integer of exactly 54 bits, whose last bit is then half a unit in the last
    place.  For q = 23 that leaves u = 1, and the 64 powers of two below 10^19 as w."""
    rng = np.random.default_rng(seed)
    out = {}
    for q in range(-4, 24):
        f = 5 ** abs(q)
        found = []
        if q < 0:       # u odd in [2^53, 2^54) with w = u * 5^-q below 10^19
            top = min(1 << 54, 10 ** 19 // f)
            for u in sorted({int(x) | 1 for x in rng.integers(1 << 53, top - 1, per_exponent)} | {(1 << 53) + 1, top - 1 | 1}):
                if u < top:
                    found.append(u * f)
        elif q == 0:
            found = sorted({int(x) | 1 for x in rng.integers(1 << 53, (1 << 54) - 1, per_exponent)}
                           | {(1 << 53) + 1, (1 << 54) - 1})
        else:           # u odd with u * 5^q in [2^53, 2^54), times every power of two that fits
            lo, hi = -(-(1 << 53) // f), ((1 << 54) - 1) // f
            first, count = lo | 1, (hi - (lo | 1)) // 2 + 1
            if count > per_exponent:
                us = sorted({first + 2 * int(i) for i in rng.integers(0, count, per_exponent)} | {first, first + 2 * (count - 1)})
            else:
                us = [first + 2 * i for i in range(count)]
            for u in us:
                for j in range(64):
                    w = u << j
                    if w < 10 ** 19 and (w > 1 << 53 or q > 22):
                        found.append(w)
            if len(found) > 2 * per_exponent:
                found = sorted({found[int(i)] for i in rng.integers(0, len(found), 2 * per_exponent)})
        texts = []
        for w in found:
            t = "%de%d" % (w, q) if q else str(w)
            assert is_halfway(t), t
            texts.append((w, t))
        out[q] = texts
    return out


def find_declined():
    """Every string w * 10^q whose first product's low word is all ones with q outside [-27, 55] and
    without the second product: w << lz must be -1 / hi modulo 2^64, which is odd, so lz = 0 and
    w >= 2^63; it exists for an odd hi only and must lie below 10^19.  The search is complete for
    that route (one candidate per exponent) and finds 15 strings.  Declines after the second product
    need the middle 64 bits of the 192-bit product all ones AND the low nine bits of the first
    product's high word all ones; a lattice search of the first condition (not kept here) met 150
    candidates over all exponents and none with the second, so none of that kind is in the corpus."""
    out = []
    for q in range(-342, 309):
        hi, _ = pow5(q)
        if -27 <= q <= 55 or hi % 2 == 0:
            continue
        w = -pow(hi, -1, 1 << 64) % (1 << 64)
        if 1 << 63 <= w < 10 ** 19 and el_step(w, q)[1] is None:
            out.append("%de%d" % (w, q))
    return out


def float_corpus():
    """The strings of the float tests, in a fixed order (see the issue list in each block)."""
    import test_csv_host

    out = [repr(v) for v in test_csv_host._random_doubles().tolist()]
    half = halfway_points()
    for q, texts in half.items():
        for w, t in texts:
            out += [t, "-" + t]
            out += ["%de%d" % (w + 1, q), "%de%d" % (w - 1, q)]             # one off in the last digit
            if q < 0:
                out += [with_point(w, q), with_point(w + 1, q), with_point(w - 1, q)]
    for w in ((1 << 53) - 1, 1 << 53, (1 << 53) + 1):                       # the Clinger boundaries
        out += ["%de%d" % (w, q) for q in (-23, -22, 22, 23)] + [str(w)]
    out += ["9007199254740991.5", "18014398509481983", "4503599627370495.75", "1.7976931348623159e308",       # carries
            "1.7976931348623157e308", "1.7976931348623158e308", "17976931348623158e292", "9007199254740993",
            "36028797018963967", "72057594037927935e3", "1.8e308", "179769313486231580793e288"]
    out += ["2.2250738585072014e-308", "2.225073858507201e-308", "2.2250738585072011e-308", "2.2250738585072012e-308",
            "2.2250738585072009e-308", "2.2250738585072016e-308", "22250738585072012e-324", "2.225073858507202e-308",
            "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.5e-324", "5e-324", "1e-323", "2e-324",
            "7.4e-324", "7.5e-324", "4.940656458412465e-324", "9.8813129168249309e-324"]
    assert float("2.2250738585072012e-308") == 2.0 ** -1022 > float("2.2250738585072011e-308")
    out += ["123e-345", "1e309", "1e-343", "9999999999999999999e-343", "1e-342", "9999999999999999999e-342", "1e308",
            "2e308", "1e-400", "1e400", "1e99999999", "1e-99999999", "0e99999", "0e-99999", "1e0000000000000000000001",
            "0." + "0" * 320 + "1e330", "1" + "0" * 18 + "e290", "1e+308", "1E-308", "17976931348623157e292"]
    out += ["12345678901234567890", "1.2345678901234567890", "0.00012345678901234567890", "10000000000000000000",
            "1000000000000000000", "9999999999999999999", "18446744073709551615", "18446744073709551616e5",
            "12345678901234567890123", "0.1234567890123456789", "0.12345678901234567890", "00000000000000000000001",
            "1.0000000000000000000", "1.00000000000000000000", "000001.5", "1.50000", "0000", "0.0", "-0.0", "00.00e5",
            ".5", "5.", "+.5", "-5.", "+5.e3", "-.5E-3", "0", "-0", "+0", "00012.50", "1e22", "1e-22", "1e23", "1E5", "+1.5",
            "9007199254740992e3", "2.5e-5", "123456789012345678e-40", "8.98846567431158e307", "0.3", "0.1", "1e-5"]
    for word in ("inf", "infinity", "nan"):
        for case in itertools.product(*[(c, c.upper()) for c in word]):
            out += [sign + "".join(case) for sign in ("", "+", "-")]
    out += INVALID_FLOATS + MORE_INVALID_FLOATS
    out += find_declined()
    return out


def int_corpus():
    out = []
    for lim in (I64_MIN, I64_MAX, I32_MIN, I32_MAX):
        out += [str(lim - 1), str(lim), str(lim + 1)]
    out += ["+" + str(I64_MAX), "+" + str(I64_MAX + 1), "+" + str(I32_MAX), "+" + str(I32_MAX + 1),
            "1000000000000000000", "9223372036854775799", "9223372036854775810", "9999999999999999999",
            "10000000000000000000", "18446744073709551615", "18446744073709551616", "18446744073709551621",
            "-9999999999999999999", "-10000000000000000000", "99999999999999999999999999",
            "0000123", "-000", "000000000000000000000000000007", "-00000000000000000000009223372036854775808",
            "00000000000000000000009223372036854775808", "+7", "-0", "+0", "0", "42", "-1", "4294967296", "-4294967296",
            "4294967295", "2147483650", "-2147483650"]
    rng = np.random.default_rng(11)
    out += [str(int(v)) for v in rng.integers(I64_MIN, I64_MAX, 300, endpoint=True)]
    out += [str(int(v)) for v in rng.integers(I32_MIN, I32_MAX, 300, endpoint=True)]
    out += INVALID_INTS + MORE_INVALID_INTS
    return out


FIRST_NS, LAST_NS = "1677-09-21 00:12:43.145224193", "2262-04-11 23:47:16.854775807"
VALID_DATETIMES = [FIRST_NS, LAST_NS, "2024-02-29", "2000-02-29T23:59", "1970-01-01 00:00:00",
                   "1969-12-31 23:59:59.999999999", "2024-01-05 10:00:00.1", "2024-01-05T10:00:00.123456789"]
INVALID_DATETIMES = ["2024-13-05", "2023-02-29", "2024-02-30", "2024-01-05 24:00:00", "2024-01-05 23:59:60", "2024-1-5",
                     "20240105", "2024-01-05 10", "2024-01-05 10:00:00Z", " 2024-01-05", "2024-01-05 10:00:00.1234567891",
                     "2024-00-05", "2024-01-00", "2024-04-31", "1900-02-29", "2024-01-05 10:60", "2024-01-05 ",
                     "2024-01-05 10:00:00.", "2024-01-05  10:00", "2024-01-05t10:00", "2024-01-05 10:00:00+01:00",
                     "2024/01/05", "-024-01-05", "2024-01-05 1o:00", ""]
OVERFLOW_DATETIMES = ["2262-04-11 23:47:16.854775808", "1677-09-21 00:12:43.145224192", "2262-04-12", "1677-09-20",
                      "9999-12-31 23:59:59.999999999", "0001-01-01"]


def datetime_corpus(n=2400, seed=7):
    """Random instants over the nanosecond range in every shape of the grammar (date, HH:MM, seconds,
    1 to 9 fraction digits; both separators), the two ends of the range and the lists of
    test_datetime_host.py."""
    rng = np.random.default_rng(seed)
    lo = int(np.datetime64("1677-09-22", "ns").astype(np.int64))     # (a shorter shape cuts the instant off)
    ns = rng.integers(lo, I64_MAX, n, endpoint=True)
    out = []
    for i, v in enumerate(ns.tolist()):
        t = str(np.datetime64(v, "ns"))                              # YYYY-MM-DDTHH:MM:SS.fffffffff
        assert len(t) == 29
        shape = i % 12                                               # 0 date, 1 minutes, 2 seconds, 3.. digits
        t = t[:10] if shape == 0 else t[:16] if shape == 1 else t[:19] if shape == 2 else t[:18 + shape]
        out.append(t.replace("T", " ") if (i // 12) % 2 else t)
    out += [FIRST_NS, LAST_NS, FIRST_NS.replace(" ", "T"), LAST_NS.replace(" ", "T")]
    out += ["0000-01-01", "1970-01-01", "1970-01-01T00:00", "1969-12-31 23:59:59.9", "2262-04-11 23:47:16.854775807",
            "2262-04-11 23:47:17", "1677-09-21 00:12:43.2", "1677-09-21 00:12:43.1", "1677-09-21 00:12:43", "1677-09-21",
            "2262-04-11", "2100-02-29", "2400-02-29", "2024-12-31T23:59:59.999999999", "2024-01-05 10:00:00.000000000",
            "2024-01-05x10:00", "2024-01-05 10:00:00,5", "2024-01-05 10:00:00.12a", "2024-01-05 10:00:00.1234567890123",
            "٢٠٢٤-01-05"]
    return out + VALID_DATETIMES + INVALID_DATETIMES + OVERFLOW_DATETIMES


# ---- text builders --------------------------------------------------------------------------------------
def column_text(cells, ncols=3, k=1, sep=b"\t", eol=b"\n", first=0):
    """One row per cell (bytes, written as they stand) in column k; the other columns hold the row
    number."""
    rows = []
    for i, c in enumerate(cells, start=first):
        num = str(i).encode()
        rows.append(sep.join([c if j == k else num for j in range(ncols)]) + eol)
    return b"".join(rows)


def filler(nbytes, ncols, sep, rng, first, quote=b'"'):
    """Rows of exactly nbytes bytes: a running integer, then ncols - 1 text fields, some of them
    quoted with separators and doubled quotes inside (none when quote is empty)."""
    least = ncols + 1
    if nbytes == 0:
        return b"", first
    if nbytes < least:
        raise ValueError(f"cannot fill {nbytes} bytes with rows of {ncols} fields")
    out, left, i = [], nbytes, first
    while True:
        cells = [str(i).encode()]
        for _ in range(ncols - 1):
            body = b"y" * int(rng.integers(0, 30))
            if quote and rng.random() < 0.3:
                body = quote + body + sep + quote + quote + sep + quote
            cells.append(body)
        row = sep.join(cells) + b"\n"
        if left - len(row) < least + 24:
            break
        out.append(row)
        left -= len(row)
        i += 1
    head = str(i).encode()[:max(1, left - ncols)]
    if ncols == 1:
        out.append(b"z" * (left - 1) + b"\n")
        return b"".join(out), i + 1
    out.append(head + sep + b"z" * (left - len(head) - ncols) + sep * (ncols - 2) + b"\n")
    return b"".join(out), i + 1


MARK = 1      # the byte structured_text takes out of a row: the byte after it lands on the position


def structured_text(rows, size, ncols=2, sep=b",", quote=b'"', seed=0):
    """Text of exactly ``size`` bytes that ends in a newline.  ``rows`` is a list of row
    specifications: bytes (a row as it stands, line end included), or (bytes with one MARK byte,
    position): that row is placed so that the byte which follows the mark -- an opening or closing
    quote, the first of a doubled quote, a separator inside quotes, the newline -- lies on the
    absolute byte ``position``.  Filler rows (filler()) pad in front of each placed row and
    behind the last one."""
    rng = np.random.default_rng(seed)
    out, at, nxt = [], 0, 10 ** 6
    for spec in rows:
        if isinstance(spec, tuple):
            row, position = spec
            off = row.index(bytes([MARK]))
            row = row[:off] + row[off + 1:]
            pad, nxt = filler(position - off - at, ncols, sep, rng, nxt, quote)
            out.append(pad)
            at += len(pad)
            assert at + off == position
        else:
            row = spec
        out.append(row)
        at += len(row)
    pad, _ = filler(size - at, ncols, sep, rng, nxt, quote)
    text = b"".join(out) + pad
    assert len(text) == size and text.endswith(b"\n")
    return text
