"""nvt_csv_*: every refusal is NVT_EINVAL, names its argument in nvt_last_error and comes before the
first launch (host buffers stand in for device memory: nothing is read through them).  Runs
without a GPU."""
import ctypes as C

from nvtabular_amd import _lib

F32, F64, I32, I64, U8 = 0, 1, 2, 3, 4
SEP, QUOTE = ord(","), ord('"')


def _setup():
    lib = _lib.load()
    raw = (C.c_uint8 * 16384)()
    base = (C.addressof(raw) + 63) & ~63
    return lib, raw, base


def _refused(lib, rc, *words):
    assert rc == _lib.NVT_EINVAL, (rc, lib.nvt_last_error())
    msg = lib.nvt_last_error()
    for w in words:
        assert w in msg, (w, msg)


def _col(base, **kw):
    d = (_lib.CsvCol * 1)()
    c = dict(out=base + 4096, out_valid=base + 6144, slow=base + 7168, k=0, dtype=F64)
    c.update(kw)
    for k, v in c.items():
        setattr(d[0], k, v)
    return d


def test_ws_bytes():
    lib, raw, base = _setup()
    a, b = C.c_uint64(), C.c_uint64()
    assert lib.nvt_csv_ws_bytes(100, C.byref(a)) == 0 and a.value >= 16
    assert lib.nvt_csv_ws_bytes(1 << 24, C.byref(b)) == 0 and b.value >= (1 << 12) * 16
    _refused(lib, lib.nvt_csv_ws_bytes(100, None), b"nvt_csv_ws_bytes", b"null output")
    _refused(lib, lib.nvt_csv_ws_bytes(1 << 31, C.byref(a)), b"nbytes", b"2^31")
    assert lib.nvt_csv_str_ws_bytes(100, C.byref(a)) == 0 and a.value >= 8
    _refused(lib, lib.nvt_csv_str_ws_bytes(100, None), b"null output")


def test_count_and_index_refuse_bad_arguments():
    lib, raw, base = _setup()
    text, ws, fe, state = base, base + 1024, base + 2048, base + 3072

    def count(text=text, nbytes=64, sep=SEP, quote=QUOTE, ws=ws, ws_bytes=64, state=state):
        return lib.nvt_csv_count(text, nbytes, sep, quote, ws, ws_bytes, state, None)

    def index(text=text, nbytes=64, sep=SEP, quote=QUOTE, ncols=2, ws=ws, ws_bytes=64, fe=fe, nfields=8, state=state):
        return lib.nvt_csv_index(text, nbytes, sep, quote, ncols, ws, ws_bytes, fe, nfields, state, None)

    for f, name in ((count, b"nvt_csv_count"), (index, b"nvt_csv_index")):
        _refused(lib, f(text=None), name, b"null text")
        _refused(lib, f(text=text + 8), b"text", b"16-byte aligned")
        _refused(lib, f(nbytes=1 << 31), b"nbytes", b"2^31")
        _refused(lib, f(sep=ord("\n")), b"sep")
        _refused(lib, f(sep=256), b"sep")
        _refused(lib, f(sep=-1), b"sep")
        _refused(lib, f(sep=QUOTE), b"sep")
        _refused(lib, f(quote=300), b"quote")
        _refused(lib, f(quote=-2), b"quote")
        _refused(lib, f(quote=ord("\n")), b"quote")
        _refused(lib, f(ws=None), b"null workspace")
        _refused(lib, f(ws=ws + 4), b"workspace", b"aligned")
        _refused(lib, f(ws_bytes=16), b"workspace smaller")
        _refused(lib, f(nbytes=8192, ws_bytes=32), b"workspace smaller")
        _refused(lib, f(state=None), b"null state")
        _refused(lib, f(state=state + 4), b"state", b"aligned")
        empty = dict(nbytes=0, nfields=0) if f is index else dict(nbytes=0)
        assert f(**empty) == 0
        assert f(text=None, **empty) == 0
    _refused(lib, index(ncols=0), b"ncols")
    _refused(lib, index(fe=None), b"null field_end")
    _refused(lib, index(fe=fe + 2), b"field_end", b"aligned")
    _refused(lib, index(nfields=65), b"nfields")


def test_parse_many_refuses_bad_arguments():
    lib, raw, base = _setup()
    text, fe, state = base, base + 2048, base + 3072

    def call(d, text=text, nbytes=64, fe=fe, nrows=8, ncols=2, quote=QUOTE, ndesc=1, state=state):
        return lib.nvt_csv_parse_many(text, nbytes, fe, nrows, ncols, quote, d, ndesc, state, None)

    _refused(lib, call(None), b"nvt_csv_parse_many", b"null descriptors")
    _refused(lib, call(_col(base), ndesc=-1), b"ndesc")
    _refused(lib, call(_col(base), text=None), b"null text")
    _refused(lib, call(_col(base), text=text + 4), b"text", b"aligned")
    _refused(lib, call(_col(base), nbytes=1 << 31), b"nbytes")
    _refused(lib, call(_col(base), quote=256), b"quote")
    _refused(lib, call(_col(base), ncols=0), b"ncols")
    _refused(lib, call(_col(base), fe=None), b"null field_end")
    _refused(lib, call(_col(base), fe=fe + 1), b"field_end", b"aligned")
    _refused(lib, call(_col(base), nrows=40), b"nrows * ncols")
    _refused(lib, call(_col(base), state=None), b"null state")
    for bad in (U8, 5, 6, 7, -1):
        _refused(lib, call(_col(base, dtype=bad)), b"dtype")
    _refused(lib, call(_col(base, k=2)), b"k must be below ncols")
    _refused(lib, call(_col(base, out=None)), b"null out")
    _refused(lib, call(_col(base, out_valid=None)), b"out_valid")
    _refused(lib, call(_col(base, out=base + 4100)), b"out", b"aligned")
    _refused(lib, call(_col(base, out=base + 4098, dtype=I32)), b"out", b"aligned")
    _refused(lib, call(_col(base, out_valid=base + 6148)), b"out_valid", b"aligned")
    _refused(lib, call(_col(base, slow=None)), b"slow")
    _refused(lib, call(_col(base, slow=None, dtype=F32)), b"slow")
    _refused(lib, call(_col(base, slow=base + 7172)), b"slow", b"aligned")
    # nothing to do
    assert call(_col(base), nrows=0) == 0
    assert call(_col(base, slow=None, dtype=I64), nrows=0, fe=None) == 0
    assert call(None, ndesc=0) == 0


def test_string_entries_refuse_bad_arguments():
    lib, raw, base = _setup()
    text, fe, off, valid, ws, chars = base, base + 2048, base + 3072, base + 4096, base + 5120, base + 6144

    def offsets(text=text, nbytes=64, fe=fe, nrows=8, ncols=2, k=1, quote=QUOTE, off=off, valid=valid, ws=ws,
                ws_bytes=64, state=base + 7168):
        return lib.nvt_csv_str_offsets(text, nbytes, fe, nrows, ncols, k, quote, off, valid, ws, ws_bytes, state,
                                       None)

    def copy(text=text, nbytes=64, fe=fe, nrows=8, ncols=2, k=1, quote=QUOTE, off=off, chars=chars, chars_bytes=32):
        return lib.nvt_csv_str_copy(text, nbytes, fe, nrows, ncols, k, quote, off, chars, chars_bytes, None)

    for f, name in ((offsets, b"nvt_csv_str_offsets"), (copy, b"nvt_csv_str_copy")):
        _refused(lib, f(text=None), name, b"null text")
        _refused(lib, f(text=text + 1), b"text", b"aligned")
        _refused(lib, f(nbytes=1 << 31), b"nbytes")
        _refused(lib, f(quote=-5), b"quote")
        _refused(lib, f(ncols=0), b"ncols")
        _refused(lib, f(k=2), b"k must be below ncols")
        _refused(lib, f(fe=None), b"null field_end")
        _refused(lib, f(fe=fe + 2), b"field_end", b"aligned")
        _refused(lib, f(nrows=33), b"nrows * ncols")
        _refused(lib, f(off=off + 2), b"offsets", b"aligned")
        _refused(lib, f(off=None), b"null offsets")
        assert f(nrows=0) == 0
    _refused(lib, offsets(valid=None), b"null out_valid")
    _refused(lib, offsets(valid=valid + 4), b"out_valid", b"aligned")
    _refused(lib, offsets(ws=None), b"null workspace")
    _refused(lib, offsets(ws=ws + 4), b"workspace", b"aligned")
    _refused(lib, offsets(ws_bytes=8), b"workspace smaller")
    _refused(lib, offsets(state=None), b"null state")
    _refused(lib, offsets(state=base + 7172), b"state", b"aligned")
    _refused(lib, copy(chars=None), b"null chars")
    assert copy(chars=None, chars_bytes=0) == 0


def test_host_parsers_refuse_null():
    lib, raw, base = _setup()
    out = C.c_double()
    _refused(lib, lib.nvt_csv_parse_f64_host(b"1", 1, None), b"nvt_csv_parse_f64_host", b"null output")
    _refused(lib, lib.nvt_csv_parse_f64_host(None, 1, C.byref(out)), b"null text")
    _refused(lib, lib.nvt_csv_parse_f64_host(b"1", -1, C.byref(out)), b"len")
    _refused(lib, lib.nvt_csv_parse_i64_host(b"1", 1, None), b"nvt_csv_parse_i64_host", b"null output")
