"""nvt_snappy_*: every refusal is NVT_EINVAL, names its argument in nvt_last_error and comes before
the first launch (host buffers stand in for device memory: nothing is read through them, and this
runs without a GPU)."""
import ctypes as C

import pytest


@pytest.fixture()
def args():
    from nvtabular_amd import _lib

    raw = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(raw) + 63) & ~63

    def make(ncols=2):
        cols = (_lib.SnappyCol * ncols)()
        total = 0
        for i, c in enumerate(cols):
            c.src, c.page_start, c.npages, c.nbytes = base + 4096 * i, base + 8192 + 64 * i, 2, 1000
            c.unit, c.elem = 8, 8
            c.frag_base, c.max_frags = total, 3
            c.dense, c.dense_cap, c.out = base + 16384 + 2048 * i, 1000, base + 24576 + 64 * i
            total += 3
        batch = _lib.SnappyBatch(base + 32768, base + 36864, base + 40960, base + 45056, total, 64, base + 61440, 64)
        return cols, batch

    return raw, make


def _entries(lib):
    return [lib.nvt_snappy_plan_many, lib.nvt_snappy_compress_many, lib.nvt_snappy_gather_many]


def _refused(lib, rc, *words):
    from nvtabular_amd import _lib

    assert rc == _lib.NVT_EINVAL, rc
    msg = lib.nvt_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_constants_match_the_header():
    from nvtabular_amd import _lib

    lib = _lib.load()
    n = C.c_uint64()
    assert lib.nvt_snappy_slot_bytes(C.byref(n)) == 0 and n.value == _lib.SNAPPY_SLOT_BYTES
    assert _lib.SNAPPY_SLOT_BYTES == _lib.SNAPPY_FRAG + _lib.SNAPPY_FRAG // 32 + 16 and n.value % 4 == 0
    assert lib.nvt_snappy_ws_bytes(10, C.byref(n)) == 0 and n.value >= 16 and n.value % 8 == 0
    _refused(lib, lib.nvt_snappy_slot_bytes(None), b"null")
    _refused(lib, lib.nvt_snappy_ws_bytes(10, None), b"null")


def test_null_pointers_and_zero_columns_are_refused(args):
    from nvtabular_amd import _lib

    lib = _lib.load()
    _, make = args
    for fn in _entries(lib):
        cols, batch = make()
        _refused(lib, fn(None, 2, C.byref(batch), None), b"null descriptors")
        _refused(lib, fn(cols, 2, None, None), b"null descriptors")
        _refused(lib, fn(cols, 0, C.byref(batch), None), b"ncols")
        _refused(lib, fn(cols, -1, C.byref(batch), None), b"ncols")
        for field in ("frag_table", "frag_size", "frag_pos", "slots", "ws"):
            cols, batch = make()
            setattr(batch, field, None)
            _refused(lib, fn(cols, 2, C.byref(batch), None), b"null pointer")
        for field in ("src", "page_start", "out", "dense"):
            cols, batch = make()
            setattr(cols[1], field, None)
            _refused(lib, fn(cols, 2, C.byref(batch), None), b"null pointer")


def test_element_size_and_shapes_are_refused(args):
    from nvtabular_amd import _lib

    lib = _lib.load()
    _, make = args
    for fn in _entries(lib):
        for elem in (0, 1, 2, 3, 5, 16):
            cols, batch = make()
            cols[0].elem = elem
            _refused(lib, fn(cols, 2, C.byref(batch), None), b"element size")
        cols, batch = make()
        cols[0].unit = 0
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"unit")
        cols, batch = make()
        cols[0].npages = 0
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"npages")
        cols, batch = make()
        cols[1].max_frags = 2     # (below ceil(1000 / FRAG) + 2 pages)
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"max_frags")
        cols, batch = make()
        cols[1].frag_base = 4     # (a hole behind column 0)
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"follow")
        cols, batch = make()
        batch.total_frags = 7     # (the ranges cover 6)
        batch.ws_bytes = 1 << 10
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"add up")
        cols, batch = make()
        batch.total_frags = 5
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"total_frags")
        cols, batch = make()
        batch.slot_cap = 66
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"slot_cap")
        cols, batch = make()
        batch.ws_bytes = 8
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"workspace")
        cols, batch = make()
        cols[0].dense += 2
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"dense", b"aligned")
        cols, batch = make()
        cols[0].out += 4
        _refused(lib, fn(cols, 2, C.byref(batch), None), b"out", b"aligned")
