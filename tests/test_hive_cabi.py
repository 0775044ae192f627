"""Argument validation of nvt_key_labels* without a GPU: bad arguments are rejected on the host side
with NVT_EINVAL (-1) and a message, before any launch; n = 0 is a no-op."""
import ctypes as C


def _lib():
    import os

    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_tile_rows_and_workspace():
    from nvtabular_amd import _lib as L

    lib = _lib()
    T = lib.nvt_key_labels_tile_rows()
    assert T > 0 and T % 64 == 0 and L.LABEL_MAX == L.PARTITION_MAX == 4096
    need = C.c_uint64()
    assert lib.nvt_key_labels_ws_bytes(10, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_key_labels_ws_bytes(1 << 32, C.byref(need)) == -1
    assert b"2^32" in lib.nvt_last_error()
    assert lib.nvt_key_labels_ws_bytes(0, C.byref(need)) == 0
    # the global table: 2 * NVT_LABEL_MAX tags with a first row and a label each
    assert lib.nvt_key_labels_ws_bytes((1 << 32) - 1, C.byref(need)) == 0
    assert need.value >= 2 * L.LABEL_MAX * (8 + 4 + 2) and need.value % 16 == 0


def test_key_labels_rejects_bad_arguments():
    lib = _lib()
    n = 100
    need = C.c_uint64()
    assert lib.nvt_key_labels_ws_bytes(n, C.byref(need)) == 0
    raw = (C.c_uint8 * (need.value + 512))()
    ws = (C.addressof(raw) + 255) & ~255
    tags, words = (C.c_uint64 * n)(), (C.c_uint64 * (2 * n))()
    nulls = (C.c_uint8 * n)()
    label, first, state = (C.c_uint32 * n)(), (C.c_uint32 * 4096)(), (C.c_uint64 * 2)()

    def call(tags=tags, nulls=nulls, words=None, nkeys=1, n=n, label=label, first=first, state=state, ws=ws,
             ws_bytes=need.value):
        return lib.nvt_key_labels(tags, nulls, words, nkeys, n, label, first, state, ws, ws_bytes, None)

    for kw in (dict(tags=None), dict(nulls=None), dict(label=None), dict(first=None), dict(state=None)):
        assert call(**kw) == -1, kw
        assert b"null pointer" in lib.nvt_last_error()
    for nkeys in (0, -1, 5):
        assert call(nkeys=nkeys, words=words) == -1
        assert b"nkeys" in lib.nvt_last_error()
    assert call(nkeys=2) == -1 and b"words" in lib.nvt_last_error()
    assert call(ws=None) == -1 and b"workspace" in lib.nvt_last_error()
    assert call(ws=ws + 8) == -1 and b"aligned" in lib.nvt_last_error()
    assert call(ws_bytes=need.value - 1) == -1 and b"workspace" in lib.nvt_last_error()
    assert call(n=1 << 32) == -1 and b"2^32" in lib.nvt_last_error()
    # no rows: nothing to do, nothing is read or written
    assert lib.nvt_key_labels(None, None, None, 1, 0, None, None, None, None, 0, None) == 0
    assert list(state) == [0, 0]
