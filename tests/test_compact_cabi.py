"""Argument validation of the row-compaction entries (nvt_compact_*) without a GPU: bad arguments are
rejected on the host side with NVT_EINVAL (-1) and a message, before any launch; n = 0 is a no-op.
Also: ops.Filter / ops.Dropna exist under both package names."""
import ctypes as C

import pytest


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


def test_compact_ws_bytes():
    lib = _lib()
    need = C.c_uint64()
    assert lib.nvt_compact_ws_bytes(10, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_compact_ws_bytes(1 << 32, C.byref(need)) == -1
    assert b"2^32" in lib.nvt_last_error()
    assert lib.nvt_compact_ws_bytes(0, C.byref(need)) == 0
    # one tile: 32 mask words + the tile counts + the scan's chunk totals
    assert lib.nvt_compact_ws_bytes(2048, C.byref(need)) == 0 and need.value >= 256 + 8
    small = need.value
    assert lib.nvt_compact_ws_bytes(2049, C.byref(need)) == 0 and need.value >= small + 256


def test_keep_mask_rejects_bad_arguments():
    lib = _lib()
    n = 100
    mask = (C.c_uint8 * n)()
    buf, ws, nbytes = _ws(lib, n)
    assert lib.nvt_compact_keep_mask(None, n, ws, nbytes, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_compact_keep_mask(mask, n, None, nbytes, None) == -1
    assert lib.nvt_compact_keep_mask(mask, n, ws + 8, nbytes, None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_compact_keep_mask(mask, n, ws, nbytes - 1, None) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_compact_keep_mask(mask, 1 << 32, ws, nbytes, None) == -1
    assert lib.nvt_compact_keep_mask(None, 0, None, 0, None) == 0       # nothing to do


def test_keep_dropna_rejects_bad_arguments():
    from nvtabular_amd import _lib as L

    lib = _lib()
    n = 100
    x = (C.c_double * n)()
    buf, ws, nbytes = _ws(lib, n)
    cols = (L.DropnaCol * 2)()
    cols[0].x, cols[0].dtype = C.addressof(x), L.NVT_F64
    cols[1].x, cols[1].dtype = C.addressof(x), L.NVT_I64
    assert lib.nvt_compact_keep_dropna(cols, 0, n, ws, nbytes, None) == -1
    assert b"ncols" in lib.nvt_last_error()
    assert lib.nvt_compact_keep_dropna(cols, -1, n, ws, nbytes, None) == -1
    assert lib.nvt_compact_keep_dropna(None, 2, n, ws, nbytes, None) == -1
    cols[1].dtype = 9
    assert lib.nvt_compact_keep_dropna(cols, 2, n, ws, nbytes, None) == -1
    assert b"dtype" in lib.nvt_last_error()
    cols[1].dtype = L.NVT_F32
    cols[1].x = None
    assert lib.nvt_compact_keep_dropna(cols, 2, n, ws, nbytes, None) == -1
    assert b"null x" in lib.nvt_last_error()
    cols[1].x = C.addressof(x)
    assert lib.nvt_compact_keep_dropna(cols, 2, n, None, nbytes, None) == -1
    assert lib.nvt_compact_keep_dropna(cols, 2, n, ws, nbytes - 8, None) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_compact_keep_dropna(cols, 2, 0, None, 0, None) == 0    # nothing to do


def test_plan_and_list_entries_reject_bad_arguments():
    lib = _lib()
    n = 100
    buf, ws, nbytes = _ws(lib, n)
    lbuf, lws, lbytes = _ws(lib, 1000)
    off = (C.c_int64 * (n + 1))()
    out_off = (C.c_int64 * (n + 1))()
    assert lib.nvt_compact_plan(n, None, nbytes, None, None) == -1
    assert lib.nvt_compact_plan(n, ws, nbytes - 1, None, None) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_compact_plan(n, ws + 16, nbytes, None, None) == -1
    assert lib.nvt_compact_plan(0, None, 0, None, None) == 0
    assert lib.nvt_compact_list_keep(None, n, ws, 1000, lws, lbytes, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_compact_list_keep(off, n, None, 1000, lws, lbytes, None) == -1
    assert lib.nvt_compact_list_keep(off, n, ws + 8, 1000, lws, lbytes, None) == -1
    assert lib.nvt_compact_list_keep(off, n, ws, 1000, lws, lbytes - 1, None) == -1
    assert lib.nvt_compact_list_keep(off, 0, ws, 1000, lws, lbytes, None) == 0
    assert lib.nvt_compact_list_offsets(None, n, ws, lws, 1000, out_off, None) == -1
    assert lib.nvt_compact_list_offsets(off, n, ws, None, 1000, out_off, None) == -1
    assert lib.nvt_compact_list_offsets(off, n, ws, lws, 1000, None, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_compact_list_offsets(off, n, ws, lws + 8, 1000, out_off, None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_compact_list_offsets(off, 0, None, None, 0, None, None) == 0


def test_compact_many_rejects_bad_arguments():
    from nvtabular_amd import _lib as L

    lib = _lib()
    n = 100
    buf, ws, nbytes = _ws(lib, n)
    src = (C.c_int64 * n)()
    dst = (C.c_int64 * n)()
    vsrc = (C.c_uint8 * 16)()
    vdst = (C.c_uint32 * 4)()

    def cols(**kw):
        arr = (L.CompactCol * 1)()
        c = arr[0]
        c.src, c.dst, c.plan, c.n, c.width = C.addressof(src), C.addressof(dst), ws, n, 8
        for k, v in kw.items():
            setattr(c, k, v)
        return arr

    assert lib.nvt_compact_many(cols(), 0, None) == -1
    assert b"ncols" in lib.nvt_last_error()
    assert lib.nvt_compact_many(cols(), -3, None) == -1
    assert lib.nvt_compact_many(None, 1, None) == -1
    for width in (0, 2, 3, 16):
        assert lib.nvt_compact_many(cols(width=width), 1, None) == -1
        assert b"width" in lib.nvt_last_error()
    assert lib.nvt_compact_many(cols(src=None), 1, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_compact_many(cols(dst=None), 1, None) == -1
    assert lib.nvt_compact_many(cols(plan=None), 1, None) == -1
    assert lib.nvt_compact_many(cols(plan=ws + 8), 1, None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_compact_many(cols(src_valid=C.addressof(vsrc)), 1, None) == -1   # dst_valid missing
    assert b"together" in lib.nvt_last_error()
    assert lib.nvt_compact_many(cols(src_valid=C.addressof(vsrc), dst_valid=C.addressof(vdst) + 1), 1,
                                None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_compact_many(cols(n=1 << 32), 1, None) == -1
    # a descriptor with n = 0 launches nothing
    assert lib.nvt_compact_many(cols(n=0, src=None, dst=None, plan=None), 1, None) == 0


def test_filter_needs_a_function():
    from nvtabular_amd import ops

    with pytest.raises(ValueError, match="f cannot be None"):
        ops.Filter(None)
    with pytest.raises(ValueError):
        ops.Filter(f=None)


def test_filter_and_dropna_through_the_nvtabular_names():
    import nvtabular as nvt
    from nvtabular import ops
    from nvtabular.ops.dropna import Dropna
    from nvtabular.ops.filter import Filter

    import nvtabular_amd

    assert ops.Filter is Filter is nvtabular_amd.ops.Filter
    assert ops.Dropna is Dropna is nvtabular_amd.ops.Dropna
    node = ["a", "b"] >> ops.Dropna() >> ops.Filter(lambda df: df["a"] > 0)
    wf = nvt.Workflow(node)
    assert wf.output_node.op.__class__ is Filter
