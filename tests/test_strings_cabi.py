"""Argument validation of the string entries (nvt_str_*) without a GPU: bad arguments are
rejected on the host side with NVT_EINVAL (-1) and a message, before any launch."""
import ctypes as C


def _lib():
    import os

    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_str_hash_rejects_bad_arguments():
    lib = _lib()
    off = (C.c_int32 * 3)(0, 1, 2)
    chars = (C.c_uint64 * 1)(0)
    out = (C.c_int64 * 2)()
    assert lib.nvt_str_hash(None, 4, chars, None, 2, out, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_str_hash(off, 4, None, None, 2, out, None) == -1
    assert lib.nvt_str_hash(off, 4, chars, None, 2, None, None) == -1
    for width in (0, 2, 3, 16):
        assert lib.nvt_str_hash(off, width, chars, None, 2, out, None) == -1
        assert b"offset_bytes" in lib.nvt_last_error()
    # chars must be 4-byte aligned: the kernel reads whole aligned words
    assert lib.nvt_str_hash(off, 4, C.addressof(chars) + 1, None, 2, out, None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_str_hash(off, 4, chars, None, 0, out, None) == 0      # nothing to do


def test_str_take_keys_rejects_bad_arguments():
    lib = _lib()
    keys = (C.c_int64 * 2)(1, 2)
    idx = (C.c_int32 * 2)(0, 1)
    out = (C.c_int64 * 2)()
    assert lib.nvt_str_take_keys(keys, 2, None, 4, None, 2, out, None) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_str_take_keys(keys, 2, idx, 2, None, 2, out, None) == -1
    assert b"index_bytes" in lib.nvt_last_error()


def test_str_dedup_rejects_bad_arguments():
    lib = _lib()
    n = 1000
    need = C.c_uint64()
    assert lib.nvt_str_dedup_ws_bytes(n, None) == -1
    assert lib.nvt_str_dedup_ws_bytes(n, C.byref(need)) == 0
    # table of >= 4/3 n slots (8 B key + 4 B row) plus the n + 1 scan words
    assert need.value >= (n * 4 // 3) * 12 + (n + 1) * 4
    assert lib.nvt_str_dedup_ws_bytes(1 << 32, C.byref(need)) == -1
    assert lib.nvt_str_dedup_ws_bytes(n, C.byref(need)) == 0
    ws = (C.c_uint8 * (need.value + 512))()
    base = (C.addressof(ws) + 255) & ~255
    keys = (C.c_int64 * n)()
    off = (C.c_int32 * (n + 1))()
    chars = (C.c_uint64 * 1)()
    out = (C.c_int64 * n)()
    counts = (C.c_uint64 * 2)()
    args = lambda **kw: [kw.get(k, v) for k, v in [  # noqa: E731
        ("keys", keys), ("valid", None), ("n", n), ("index", None), ("index_bytes", 0), ("offsets", off),
        ("offset_bytes", 4), ("chars", chars), ("n_strings", n), ("ws", base), ("ws_bytes", need.value),
        ("out_keys", out), ("out_strs", out), ("out_counts", counts), ("stream", None)]]
    assert lib.nvt_str_dedup(*args(ws_bytes=need.value - 1)) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_str_dedup(*args(ws=None)) == -1
    assert lib.nvt_str_dedup(*args(ws=base + 8)) == -1                  # not 256-byte aligned
    assert lib.nvt_str_dedup(*args(offset_bytes=2)) == -1
    assert b"offset_bytes" in lib.nvt_last_error()
    assert lib.nvt_str_dedup(*args(index=off, index_bytes=1)) == -1
    assert b"index_bytes" in lib.nvt_last_error()
    assert lib.nvt_str_dedup(*args(keys=None)) == -1
    assert lib.nvt_str_dedup(*args(offsets=None)) == -1
    assert lib.nvt_str_dedup(*args(chars=None)) == -1
    assert lib.nvt_str_dedup(*args(out_counts=None)) == -1


def test_str_gather_rejects_bad_arguments():
    lib = _lib()
    m = 10
    need = C.c_uint64()
    assert lib.nvt_str_gather_ws_bytes(m, C.byref(need)) == 0 and need.value >= (m + 1) * 4
    ws = (C.c_uint8 * (need.value + 512))()
    base = (C.addressof(ws) + 255) & ~255
    strs = (C.c_int64 * m)()
    off = (C.c_int64 * (m + 1))()
    chars = (C.c_uint64 * 1)()
    out_off = (C.c_int64 * (m + 1))()
    out_chars = (C.c_uint8 * 64)()
    args = lambda **kw: [kw.get(k, v) for k, v in [  # noqa: E731
        ("strs", strs), ("m", m), ("offsets", off), ("offset_bytes", 8), ("chars", chars), ("n_strings", m),
        ("ws", base), ("ws_bytes", need.value), ("out_offsets", out_off), ("out_chars", out_chars),
        ("out_capacity", 64), ("stream", None)]]
    assert lib.nvt_str_gather(*args(ws_bytes=need.value - 1)) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_str_gather(*args(offset_bytes=5)) == -1
    assert b"offset_bytes" in lib.nvt_last_error()
    assert lib.nvt_str_gather(*args(strs=None)) == -1
    assert lib.nvt_str_gather(*args(out_offsets=None)) == -1
    assert lib.nvt_str_gather(*args(out_capacity=1 << 32)) == -1
    assert b"4 GiB" in lib.nvt_last_error()
