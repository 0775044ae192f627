"""nvt_batch_take_multi / nvt_take_list_*_multi: declared in the header, bound in _lib.py, exported
by the built library, and every refusal that needs no device is NVT_EINVAL with a message that names
its argument, before the first launch (host buffers stand in for device memory: nothing is read
through them).  Runs without a GPU."""
import ctypes as C
import os
import re

from nvtabular_amd import _lib

NEW = ["nvt_batch_take_multi", "nvt_take_list_offsets_multi", "nvt_take_list_multi"]
OLD = ["nvt_batch_take_many", "nvt_take_list_offsets", "nvt_take_list_many"]
F32, F64, I32, I64 = 0, 1, 2, 3
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvt_hip.h")


def _setup():
    lib = _lib.load()
    raw = (C.c_uint8 * 16384)()
    base = (C.addressof(raw) + 63) & ~63
    return lib, raw, base


def _col(base, **kw):
    d = (_lib.TakeCol * 1)()
    c = dict(src=base, src_valid=None, dst=base + 1024, dst_valid=base + 2048, dst_stride=1, src_dtype=0,
             dst_dtype=I64)
    c.update(kw)
    for k, v in c.items():
        setattr(d[0], k, v)
    return d


def _refused(lib, rc, *words):
    assert rc == _lib.NVT_EINVAL, (rc, lib.nvt_last_error())
    msg = lib.nvt_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_new_symbols_in_header_binding_and_library():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in NEW + OLD:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+NVT_TAKE_MAX_SOURCES\s+(\d+)", text).group(1) == str(_lib.TAKE_MAX_SOURCES)
    assert _lib.TAKE_MAX_SOURCES >= 4096
    # the record of the device table is three 8-byte words, as the driver packs it
    body = re.search(r"typedef struct nvt_take_src \{(.*?)\} nvt_take_src;", text, re.S).group(1)
    assert len(re.findall(r";", body)) == _lib.TAKE_SRC_WORDS
    # the single-source entries keep their signatures
    assert len(_lib.SIGNATURES["nvt_batch_take_many"]) == 6
    assert len(_lib.SIGNATURES["nvt_take_list_offsets"]) == 8
    assert len(_lib.SIGNATURES["nvt_take_list_many"]) == 8


def test_batch_take_multi_refuses_bad_arguments():
    lib, raw, base = _setup()
    idx, begin = base + 4096, base + 8192
    f = lib.nvt_batch_take_multi

    def call(d, m=8, n_total=8, index=idx, nsrc=2, src_begin=begin, ncols=1):
        return f(index, m, src_begin, nsrc, n_total, d, ncols, None)

    _refused(lib, f(idx, 8, begin, 2, 8, None, 1, None), b"nvt_batch_take_multi", b"null descriptors")
    _refused(lib, call(_col(base), src_begin=None), b"null src_begin")
    _refused(lib, call(_col(base), src_begin=begin + 4), b"src_begin", b"aligned")
    _refused(lib, call(_col(base, src=None)), b"null source table")
    _refused(lib, call(_col(base, src=base + 4)), b"source table", b"aligned")
    _refused(lib, call(_col(base, dst=None)), b"null")
    _refused(lib, call(_col(base), nsrc=0), b"nsrc")
    _refused(lib, call(_col(base), nsrc=-1), b"nsrc")
    limit = str(_lib.TAKE_MAX_SOURCES).encode()
    _refused(lib, call(_col(base), nsrc=_lib.TAKE_MAX_SOURCES + 1), b"nsrc", limit)
    _refused(lib, call(_col(base, dst_stride=0)), b"dst_stride")
    _refused(lib, call(_col(base, dst_stride=-2)), b"dst_stride")
    _refused(lib, call(_col(base, dst_dtype=9)), b"dst_dtype")
    _refused(lib, call(_col(base, dst=base + 1028)), b"dst", b"aligned")
    _refused(lib, call(_col(base, dst_valid=base + 2052)), b"dst_valid", b"aligned")
    _refused(lib, call(_col(base), m=9, n_total=8, index=None), b"index", b"m <= n_total")
    _refused(lib, call(_col(base), ncols=-1), b"ncols")
    # nothing to do: no launch, no device
    assert call(_col(base), m=0) == 0
    assert call(_col(base, src=None, dst=None), m=0) == 0
    assert f(None, 0, begin, 1, 0, None, 0, None) == 0
    assert call(_col(base), m=0, nsrc=_lib.TAKE_MAX_SOURCES) == 0


def test_take_list_multi_entries_refuse_bad_arguments():
    lib, raw, base = _setup()
    offs, idx, out, ws, begin = base + 512, base + 1024, base + 3072, base + 4096, base + 8192
    f = lib.nvt_take_list_offsets_multi
    _refused(lib, f(offs, begin, 2, 8, idx, 8, None, ws, 64, None), b"nvt_take_list_offsets_multi", b"out_offsets")
    _refused(lib, f(None, begin, 2, 8, idx, 8, out, ws, 64, None), b"null offsets table")
    _refused(lib, f(offs, None, 2, 8, idx, 8, out, ws, 64, None), b"null src_begin")
    _refused(lib, f(offs, begin, 0, 8, idx, 8, out, ws, 64, None), b"nsrc")
    _refused(lib, f(offs, begin, _lib.TAKE_MAX_SOURCES + 1, 8, idx, 8, out, ws, 64, None), b"nsrc",
             str(_lib.TAKE_MAX_SOURCES).encode())
    _refused(lib, f(offs, begin, 2, 8, None, 9, out, ws, 64, None), b"index", b"m <= n_total")
    _refused(lib, f(offs, begin, 2, 8, idx, 8, out, None, 64, None), b"null workspace")
    _refused(lib, f(offs, begin, 2, 8, idx, 8, out, ws + 4, 64, None), b"workspace", b"aligned")
    _refused(lib, f(offs, begin, 2, 8, idx, 8, out, ws, 8, None), b"workspace smaller")
    assert f(offs, begin, 2, 8, idx, 0, out, ws, 64, None) == 0
    g = lib.nvt_take_list_multi
    _refused(lib, g(None, 1, offs, begin, 2, idx, out, 8, 8, None), b"nvt_take_list_multi", b"null descriptors")
    _refused(lib, g(_col(base), 1, offs, None, 2, idx, out, 8, 8, None), b"null src_begin")
    _refused(lib, g(_col(base), 1, offs, begin, _lib.TAKE_MAX_SOURCES + 1, idx, out, 8, 8, None), b"nsrc")
    _refused(lib, g(_col(base, src=None), 1, offs, begin, 2, idx, out, 8, 8, None), b"null source table")
    _refused(lib, g(_col(base, dst_stride=2), 1, offs, begin, 2, idx, out, 8, 8, None), b"dst_stride")
    _refused(lib, g(_col(base, dst_stride=0), 1, offs, begin, 2, idx, out, 8, 8, None), b"dst_stride")
    _refused(lib, g(_col(base, dst_dtype=-1), 1, offs, begin, 2, idx, out, 8, 8, None), b"dst_dtype")
    _refused(lib, g(_col(base, dst=base + 1025), 1, offs, begin, 2, idx, out, 8, 8, None), b"dst", b"aligned")
    _refused(lib, g(_col(base), 1, None, begin, 2, idx, out, 8, 8, None), b"null offsets table")
    assert g(_col(base), 1, offs, begin, 2, idx, out, 8, 0, None) == 0       # no leaves
    assert g(_col(base), 1, offs, begin, 2, idx, out, 0, 0, None) == 0
