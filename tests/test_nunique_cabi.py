"""nvt_seg_nunique without a GPU: the symbol is exported and bound, bad arguments are rejected on
the host side with NVT_EINVAL (-1) and a message before any launch, n = 0 and ngroups = 0 are
no-ops."""
import ctypes as C
import os


def _lib():
    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def _args(n=16, ngroups=4, ncols=1, dtype=3):
    """Host buffers standing in for device memory: the calls below never get as far as a launch."""
    from nvtabular_amd import _lib as L

    keep = dict(words=(C.c_uint64 * 16)(), col=(C.c_int64 * 16)(), out=(C.c_uint64 * 64)(),
                ws=(C.c_uint8 * 64)())
    addr = lambda b: C.cast(b, C.c_void_p).value  # noqa: E731
    vals = L.ptr_array([addr(keep["col"])] * max(ncols, 1))
    valid = L.ptr_array([None] * max(ncols, 1))
    vd = (C.c_int * max(ncols, 1))(*([dtype] * max(ncols, 1)))
    a = [addr(keep["words"]), n, ngroups, vals, vd, valid, ncols, addr(keep["out"]), addr(keep["ws"]), None]
    return a, keep


def test_symbols_are_exported_and_bound():
    from nvtabular_amd import _lib as L

    lib = _lib()
    for name in ("nvt_seg_nunique", "nvt_seg_nunique_ws_bytes"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert len(L.SIGNATURES["nvt_seg_nunique"]) == 10


def test_ws_bytes():
    lib = _lib()
    need = C.c_uint64()
    assert lib.nvt_seg_nunique_ws_bytes(1000, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_seg_nunique_ws_bytes(0, C.byref(need)) == 0
    assert lib.nvt_seg_nunique_ws_bytes(1000, C.byref(need)) == 0 and need.value >= 1000 * 20
    small = need.value
    assert lib.nvt_seg_nunique_ws_bytes(100_000, C.byref(need)) == 0 and need.value > small


def test_rejects_bad_arguments():
    lib = _lib()
    for hole in (0, 3, 4, 7, 8):                      # words, vals, vdtypes, out, ws
        a, keep = _args()
        a[hole] = None
        assert lib.nvt_seg_nunique(*a) == -1, hole
        assert b"null" in lib.nvt_last_error()
    a, keep = _args()
    a[3][0] = None                                    # a null column in the table
    assert lib.nvt_seg_nunique(*a) == -1
    assert b"null value column" in lib.nvt_last_error()
    for ncols in (9, -1):
        a, keep = _args(ncols=ncols)
        assert lib.nvt_seg_nunique(*a) == -1
        assert b"ncols" in lib.nvt_last_error()
    for dtype in (5, 6, 7, -1):                       # NVT_I8 / NVT_I16 are cast outputs only
        a, keep = _args(dtype=dtype)
        assert lib.nvt_seg_nunique(*a) == -1
        assert b"dtype" in lib.nvt_last_error()
    a, keep = _args(n=1 << 30)
    assert lib.nvt_seg_nunique(*a) == -1
    assert b"rows" in lib.nvt_last_error()


def test_nothing_to_do_returns_ok():
    lib = _lib()
    assert lib.nvt_seg_nunique(None, 0, 4, None, None, None, 1, None, None, None) == 0
    assert lib.nvt_seg_nunique(None, 0, 0, None, None, None, 0, None, None, None) == 0
    a, keep = _args(ngroups=0)
    assert lib.nvt_seg_nunique(*a) == 0               # no groups: the output has no entries
    a, keep = _args(ncols=0)
    assert lib.nvt_seg_nunique(*a) == 0               # no columns
