"""Argument validation of nvt_compact_keep_terms without a GPU: every bad argument is rejected on the
host side with NVT_EINVAL (-1) and a message, before any launch; n = 0 is a no-op.  Host buffers
stand in for device memory: nothing is read through them."""
import ctypes as C


def _lib():
    import os

    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def _ws(lib, n):
    need = C.c_uint64()
    assert lib.nvt_compact_ws_bytes(n, C.byref(need)) == 0
    buf = (C.c_uint8 * (need.value + 512))()
    return buf, (C.addressof(buf) + 255) & ~255, need.value


def test_keep_terms_rejects_bad_arguments():
    from nvtabular_amd import _lib as L

    lib = _lib()
    n = 100
    x = (C.c_int64 * n)()
    sets = (C.c_int64 * 8)()
    buf, ws, nbytes = _ws(lib, n)
    assert L.FILTER_MAX_COLS == 16 and L.FILTER_MAX_TERMS == 64
    assert C.sizeof(L.FilterCol) == 24 and C.sizeof(L.FilterTerm) == 32

    def cols(k=2, **kw):
        arr = (L.FilterCol * max(k, 1))()
        for c in arr:
            c.x, c.dtype = C.addressof(x), L.NVT_I64
        for name, v in kw.items():
            setattr(arr[0], name, v)
        return arr

    def terms(k=3, **kw):
        arr = (L.FilterTerm * max(k, 1))()
        for i, t in enumerate(arr):
            t.col, t.op, t.conj = i % 2, L.FILTER_OPS["=="], i // 2
        for name, v in kw.items():
            setattr(arr[-1], name, v)
        return arr

    def call(c=None, nc=2, t=None, nt=3, s=sets, sw=8, rows=n, w=ws, wb=nbytes):
        return lib.nvt_compact_keep_terms(cols() if c is None else c, nc, terms() if t is None else t, nt,
                                          s, sw, rows, w, wb, None)

    def refused(rc, *words):
        assert rc == -1, rc
        msg = lib.nvt_last_error()
        assert b"nvt_compact_keep_terms" in msg or b"check_ws" in msg, msg
        for w in words:
            assert w in msg, (w, msg)

    # null pointers
    refused(lib.nvt_compact_keep_terms(None, 2, terms(), 3, sets, 8, n, ws, nbytes, None), b"null")
    refused(lib.nvt_compact_keep_terms(cols(), 2, None, 3, sets, 8, n, ws, nbytes, None), b"null")
    refused(call(s=None), b"null sets")
    refused(call(c=cols(x=None)), b"null x")
    refused(call(w=None), b"null workspace")
    # a misaligned or short workspace
    refused(call(w=ws + 8), b"aligned")
    refused(call(wb=nbytes - 1), b"workspace")
    # ncols / nterms out of range
    for nc in (0, -1, 17):
        refused(call(c=cols(17), nc=nc), b"ncols")
    for nt in (0, -2, 65):
        refused(call(t=terms(65), nt=nt), b"nterms")
    # a col index out of range, an unknown op, an unknown dtype, a misaligned x
    refused(call(t=terms(col=2)), b"col")
    refused(call(t=terms(col=-1)), b"col")
    refused(call(t=terms(op=8)), b"op")
    refused(call(t=terms(op=-1)), b"op")
    refused(call(c=cols(dtype=7)), b"dtype")
    refused(call(c=cols(x=C.addressof(x) + 4)), b"aligned")
    # unsorted conj
    bad = terms()
    bad[0].conj, bad[1].conj, bad[2].conj = 1, 0, 1
    refused(call(t=bad), b"sorted by conj")
    refused(call(t=terms(conj=-1)), b"conj")
    # set_off + set_len past set_words
    IN, NOT_IN = L.FILTER_OPS["in"], L.FILTER_OPS["not in"]
    refused(call(t=terms(op=IN, set_off=4, set_len=5)), b"set_words")
    refused(call(t=terms(op=NOT_IN, set_off=9, set_len=0)), b"set_words")
    refused(call(t=terms(op=IN, set_off=0, set_len=-1)), b"set_len")
    refused(call(t=terms(op=IN, set_off=(1 << 64) - 1, set_len=2)), b"set_words")
    refused(call(t=terms(op=IN, set_off=0, set_len=1), s=None, sw=0), b"set_words")
    refused(call(s=C.addressof(sets) + 4), b"aligned")
    # n >= 2^32 - 2048
    refused(call(rows=(1 << 32) - 2047), b"2^32")
    refused(call(rows=1 << 32), b"2^32")
    # the largest legal descriptors pass the checks up to the workspace
    refused(call(c=cols(16), nc=16, t=terms(64), nt=64, wb=0), b"workspace")
    refused(call(t=terms(op=IN, set_off=3, set_len=5), wb=0), b"workspace")
    refused(call(t=terms(op=IN, set_off=8, set_len=0), wb=0), b"workspace")


def test_keep_terms_without_rows_is_a_no_op():
    from nvtabular_amd import _lib as L

    lib = _lib()
    c = (L.FilterCol * 1)()
    c[0].dtype = L.NVT_F32                       # (x may be NULL when there are no rows)
    t = (L.FilterTerm * 1)()
    t[0].op = L.FILTER_OPS["in"]                 # an empty set without a sets buffer
    assert lib.nvt_compact_keep_terms(c, 1, t, 1, None, 0, 0, None, 0, None) == 0
