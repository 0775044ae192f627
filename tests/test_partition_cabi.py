"""Argument validation of the partition entries (nvt_partition_*) without a GPU: bad arguments are
rejected on the host side with NVT_EINVAL (-1) and a message, before any launch; n = 0 is a no-op."""
import ctypes as C
import os
import re


def _lib():
    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_symbols_and_constants():
    from nvtabular_amd import _lib as L

    lib = _lib()
    for name in ("nvt_partition_ids", "nvt_partition_plan", "nvt_partition_gather_many",
                 "nvt_partition_plan_ws_bytes", "nvt_partition_tile_rows"):
        assert hasattr(lib, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nvt_hip.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert lib.nvt_partition_tile_rows() == define("NVT_PARTITION_TILE") > 0
    assert L.PARTITION_MAX == define("NVT_PARTITION_MAX") == 4096
    assert L.PARTITION_MAX_COLS == define("NVT_PARTITION_MAX_COLS") == 16
    assert L.PARTITION_MAX_SEGS == define("NVT_PARTITION_MAX_SEGS")
    assert C.sizeof(L.PartitionSeg) == 16 and C.sizeof(L.PartitionCol) == 40


def test_partition_ids_rejects_bad_arguments():
    lib = _lib()
    tags = (C.c_uint64 * 8)()
    pid = (C.c_uint32 * 8)()
    assert lib.nvt_partition_ids(tags, 8, 0, pid, None) == -1
    assert b"P must be" in lib.nvt_last_error()
    assert lib.nvt_partition_ids(tags, 8, 4097, pid, None) == -1
    assert lib.nvt_partition_ids(None, 8, 4, pid, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_partition_ids(tags, 8, 4, None, None) == -1
    assert lib.nvt_partition_ids(None, 0, 4, None, None) == 0        # nothing to do
    assert lib.nvt_partition_ids(None, 0, 0, None, None) == -1       # P is checked first


def test_partition_plan_rejects_bad_arguments():
    lib = _lib()
    need = C.c_uint64()
    assert lib.nvt_partition_plan_ws_bytes(100, 4, None) == -1
    assert lib.nvt_partition_plan_ws_bytes(100, 0, C.byref(need)) == -1
    assert lib.nvt_partition_plan_ws_bytes(100, 4097, C.byref(need)) == -1
    assert b"P must be" in lib.nvt_last_error()
    assert lib.nvt_partition_plan_ws_bytes(1 << 32, 4, C.byref(need)) == -1
    assert b"2^32" in lib.nvt_last_error()
    assert lib.nvt_partition_plan_ws_bytes(0, 4, C.byref(need)) == 0
    assert lib.nvt_partition_plan_ws_bytes(100, 4, C.byref(need)) == 0 and need.value >= 16
    one = need.value
    tile = lib.nvt_partition_tile_rows()
    assert lib.nvt_partition_plan_ws_bytes(tile + 1, 4, C.byref(need)) == 0 and need.value >= one + 16
    assert lib.nvt_partition_plan_ws_bytes(100, 4096, C.byref(need)) == 0 and need.value >= 4096 * 4

    n, P = 100, 4
    assert lib.nvt_partition_plan_ws_bytes(n, P, C.byref(need)) == 0
    buf = (C.c_uint8 * (need.value + 64))()
    ws = (C.addressof(buf) + 15) & ~15
    pid = (C.c_uint32 * n)()
    perm = (C.c_int64 * n)()
    counts = (C.c_uint64 * P)()
    assert lib.nvt_partition_plan(pid, n, 0, perm, counts, ws, need.value, None) == -1
    assert b"P must be" in lib.nvt_last_error()
    assert lib.nvt_partition_plan(pid, n, 4097, perm, counts, ws, need.value, None) == -1
    assert lib.nvt_partition_plan(pid, 1 << 32, P, perm, counts, ws, need.value, None) == -1
    assert lib.nvt_partition_plan(None, n, P, perm, counts, ws, need.value, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_partition_plan(pid, n, P, None, counts, ws, need.value, None) == -1
    assert lib.nvt_partition_plan(pid, n, P, perm, None, ws, need.value, None) == -1
    assert lib.nvt_partition_plan(pid, n, P, perm, counts, None, need.value, None) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_partition_plan(pid, n, P, perm, counts, ws + 8, need.value, None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_partition_plan(pid, n, P, perm, counts, ws, need.value - 1, None) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_partition_plan(None, 0, P, None, None, None, 0, None) == 0   # nothing to do


def test_partition_gather_rejects_bad_arguments():
    from nvtabular_amd import _lib as L

    lib = _lib()
    raw = (C.c_uint8 * 1024)()
    base = (C.addressof(raw) + 63) & ~63
    src_tab, valid_tab, dst, dst_valid, segs = (base + 128 * i for i in range(5))

    def cols(**kw):
        arr = (L.PartitionCol * 1)()
        c = arr[0]
        c.src, c.dst, c.width = src_tab, dst, 8
        for k, v in kw.items():
            setattr(c, k, v)
        return arr

    m = 10
    assert lib.nvt_partition_gather_many(None, 1, segs, 1, m, None) == -1
    assert b"null" in lib.nvt_last_error()
    for ncols in (0, -1, 17):
        assert lib.nvt_partition_gather_many(cols(), ncols, segs, 1, m, None) == -1
        assert b"ncols" in lib.nvt_last_error()
    for width in (0, 3, 5, 16):
        assert lib.nvt_partition_gather_many(cols(width=width), 1, segs, 1, m, None) == -1
        assert b"width" in lib.nvt_last_error()
    assert lib.nvt_partition_gather_many(cols(src=None), 1, segs, 1, m, None) == -1
    assert b"null column" in lib.nvt_last_error()
    assert lib.nvt_partition_gather_many(cols(dst=None), 1, segs, 1, m, None) == -1
    assert lib.nvt_partition_gather_many(cols(src_valid=valid_tab), 1, segs, 1, m, None) == -1   # dst_valid missing
    assert b"together" in lib.nvt_last_error()
    assert lib.nvt_partition_gather_many(cols(dst_valid=dst_valid), 1, segs, 1, m, None) == -1   # src_valid missing
    assert lib.nvt_partition_gather_many(cols(src_valid=valid_tab, dst_valid=dst_valid + 4), 1, segs, 1, m,
                                         None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_partition_gather_many(cols(), 1, None, 1, m, None) == -1
    assert b"segments" in lib.nvt_last_error()
    for nsegs in (0, -2, 1025):
        assert lib.nvt_partition_gather_many(cols(), 1, segs, nsegs, m, None) == -1
        assert b"nsegs" in lib.nvt_last_error()
    assert lib.nvt_partition_gather_many(cols(), 1, None, 0, 0, None) == 0                    # no rows
    assert lib.nvt_partition_gather_many(cols(src=None, dst=None), 1, None, 0, 0, None) == 0
