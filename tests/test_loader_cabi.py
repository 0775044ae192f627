"""nvt_batch_take_many / nvt_take_list_*: every refusal is NVT_EINVAL, names its argument in
nvt_last_error and comes before the first launch (host buffers stand in for device memory: nothing
is read through them).  Runs without a GPU."""
import ctypes as C

from nvtabular_amd import _lib

F32, F64, I32, I64, U8, I8, I16 = 0, 1, 2, 3, 4, 5, 6


def _setup():
    lib = _lib.load()
    raw = (C.c_uint8 * 8192)()
    base = (C.addressof(raw) + 63) & ~63
    return lib, raw, base


def _col(base, **kw):
    d = (_lib.TakeCol * 1)()
    c = dict(src=base, src_valid=None, dst=base + 1024, dst_valid=base + 2048, dst_stride=1, src_dtype=I32,
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


def test_batch_take_many_refuses_bad_arguments():
    lib, raw, base = _setup()
    idx = base + 4096

    def call(d, m=8, n_src=8, index=idx, ncols=1):
        return lib.nvt_batch_take_many(index, m, n_src, d, ncols, None)

    _refused(lib, lib.nvt_batch_take_many(idx, 8, 8, None, 1, None), b"nvt_batch_take_many", b"null descriptors")
    _refused(lib, call(_col(base, src_dtype=7)), b"src_dtype")
    _refused(lib, call(_col(base, src_dtype=-1)), b"src_dtype")
    _refused(lib, call(_col(base, dst_dtype=9)), b"dst_dtype")
    for s in (F32, F64):
        for d in (I32, I64, U8, I8, I16):
            _refused(lib, call(_col(base, src_dtype=s, dst_dtype=d)), b"dst_dtype", b"integer source")
    _refused(lib, call(_col(base, src_dtype=I64, dst_dtype=I32)), b"dst_dtype")     # narrowing is nvt_cast_many's
    _refused(lib, call(_col(base, dst_stride=0)), b"dst_stride")
    _refused(lib, call(_col(base, dst_stride=-3)), b"dst_stride")
    _refused(lib, call(_col(base, src=base + 2)), b"src", b"aligned")
    _refused(lib, call(_col(base, dst=base + 1028)), b"dst", b"aligned")
    _refused(lib, call(_col(base, dst_valid=base + 2052)), b"dst_valid", b"aligned")
    _refused(lib, call(_col(base, src=None)), b"null src")
    _refused(lib, call(_col(base), m=9, n_src=8, index=None), b"index", b"m <= n_src")
    # nothing to do
    assert call(_col(base), m=0) == 0
    assert lib.nvt_batch_take_many(None, 0, 0, None, 0, None) == 0


def test_take_list_entries_refuse_bad_arguments():
    lib, raw, base = _setup()
    off, idx, out, ws = base, base + 1024, base + 2048, base + 4096
    need, more = C.c_uint64(), C.c_uint64()
    assert lib.nvt_take_list_ws_bytes(100, C.byref(need)) == 0 and need.value >= 16
    assert lib.nvt_take_list_ws_bytes(1 << 20, C.byref(more)) == 0 and more.value > need.value
    _refused(lib, lib.nvt_take_list_ws_bytes(100, None), b"null output")
    f = lib.nvt_take_list_offsets
    _refused(lib, f(off, 8, idx, 8, None, ws, 64, None), b"out_offsets")
    _refused(lib, f(None, 8, idx, 8, out, ws, 64, None), b"null offsets")
    _refused(lib, f(off, 8, None, 9, out, ws, 64, None), b"index", b"m <= n_src")
    _refused(lib, f(off, 8, idx, 8, out, None, 64, None), b"null workspace")
    _refused(lib, f(off, 8, idx, 8, out, ws + 4, 64, None), b"workspace", b"aligned")
    _refused(lib, f(off, 8, idx, 8, out, ws, 8, None), b"workspace smaller")
    assert f(off, 8, idx, 0, out, ws, 64, None) == 0
    g = lib.nvt_take_list_many
    _refused(lib, g(None, 1, off, idx, out, 8, 8, None), b"nvt_take_list_many", b"null descriptors")
    _refused(lib, g(_col(base, src_dtype=8), 1, off, idx, out, 8, 8, None), b"src_dtype")
    _refused(lib, g(_col(base, src_dtype=F64, dst_dtype=I64), 1, off, idx, out, 8, 8, None), b"dst_dtype")
    _refused(lib, g(_col(base, dst_stride=2), 1, off, idx, out, 8, 8, None), b"dst_stride")
    _refused(lib, g(_col(base, dst_stride=0), 1, off, idx, out, 8, 8, None), b"dst_stride")
    _refused(lib, g(_col(base, src=base + 1), 1, off, idx, out, 8, 8, None), b"src", b"aligned")
    _refused(lib, g(_col(base, dst=base + 1025), 1, off, idx, out, 8, 8, None), b"dst", b"aligned")
    _refused(lib, g(_col(base, dst_valid=base + 2049), 1, off, idx, out, 8, 8, None), b"dst_valid")
    _refused(lib, g(_col(base), 1, None, idx, out, 8, 8, None), b"null offsets")
    assert g(_col(base), 1, off, idx, out, 8, 0, None) == 0       # no leaves
    assert g(_col(base), 1, off, idx, out, 0, 0, None) == 0
