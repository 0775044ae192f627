"""nvt_pq_dict_* without a GPU: the symbols are in the header, exported and bound; bad arguments are
rejected on the host side with NVT_EINVAL (-1) and a message before any launch."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nvt_pq_dict_ws_bytes", "nvt_pq_dict_build", "nvt_pq_dict_pack")
I32, I64 = 2, 3


def _lib():
    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def _need(n, max_entries=1 << 20, npages=1):
    need = C.c_uint64()
    assert _lib().nvt_pq_dict_ws_bytes(n, max_entries, npages, C.byref(need)) == 0
    return need.value


class Args:
    """Host buffers standing in for device memory: the calls below never get as far as a launch."""

    def __init__(self, n=64, max_entries=1 << 20, npages=1, dtype=I64):
        self.keep = dict(values=(C.c_int64 * 64)(), dict=(C.c_int64 * 64)(), state=(C.c_uint64 * 4)(),
                         pages=(C.c_int64 * 8)(), out=(C.c_uint8 * 1024)())
        ws_bytes = _need(n, max_entries, npages)
        self.keep["ws"] = (C.c_uint8 * (ws_bytes + 16))()
        a = {k: C.cast(v, C.c_void_p).value for k, v in self.keep.items()}
        a["ws"] = (a["ws"] + 15) & ~15
        a["out"] = (a["out"] + 15) & ~15
        self.a, self.n, self.max_entries, self.npages, self.dtype, self.ws_bytes = a, n, max_entries, npages, dtype, ws_bytes

    def build(self, **kw):
        a = dict(self.a, **kw)
        return [a["values"], kw.get("dtype", self.dtype), kw.get("n", self.n), kw.get("max_entries", self.max_entries),
                a["dict"], a["state"], a["ws"], kw.get("ws_bytes", self.ws_bytes), None]

    def pack(self, **kw):
        a = dict(self.a, **kw)
        return [a["values"], kw.get("dtype", self.dtype), kw.get("n", self.n), kw.get("max_entries", self.max_entries),
                a["pages"], kw.get("npages", self.npages), a["state"], a["out"], kw.get("out_cap", 1024 - 16),
                a["ws"], kw.get("ws_bytes", self.ws_bytes), None]


def test_symbols_are_declared_exported_and_bound():
    from nvtabular_amd import _lib as L

    lib = _lib()
    header = open(os.path.join(ROOT, "include", "nvt_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert len(L.SIGNATURES["nvt_pq_dict_build"]) == 9 and len(L.SIGNATURES["nvt_pq_dict_pack"]) == 12
    assert "#define NVT_PQ_DICT_MAX_ENTRIES (1u << 20)" in header and L.PQ_DICT_MAX_ENTRIES == 1 << 20
    assert "#define NVT_PQ_DICT_STATE_WORDS 4" in header and L.PQ_DICT_STATE_WORDS == 4


def test_ws_bytes():
    lib = _lib()
    need = C.c_uint64()
    assert lib.nvt_pq_dict_ws_bytes(1000, 1 << 20, 1, None) == -1
    assert b"null" in lib.nvt_last_error()
    for bad in (0, (1 << 20) + 1):
        assert lib.nvt_pq_dict_ws_bytes(1000, bad, 1, C.byref(need)) == -1
        assert b"max_entries" in lib.nvt_last_error()
    assert lib.nvt_pq_dict_ws_bytes(1 << 31, 1 << 20, 1, C.byref(need)) == -1
    assert lib.nvt_pq_dict_ws_bytes(0, 1 << 20, 0, C.byref(need)) == 0
    small = _need(1000)
    assert small >= 2048 * 12 + 1000 * 12                 # the table (keys + ranks), the compact list and its sort words
    assert _need(100_000) > small and _need(1000, npages=500) > small
    assert _need(1 << 24) == _need(1 << 25) <= 64 << 20   # bounded by max_entries, not by n
    assert _need(1 << 24, max_entries=16) < _need(1 << 24) // 4   # (the radix sort's scratch has a fixed part)


def test_build_rejects_bad_arguments():
    lib = _lib()
    for hole in ("values", "dict", "state", "ws"):
        assert lib.nvt_pq_dict_build(*Args().build(**{hole: None})) == -1, hole
        assert b"null" in lib.nvt_last_error()
    for dtype in (0, 1, 4, 5, 6, 7, -1):                  # floats, u8 and the narrow integers
        assert lib.nvt_pq_dict_build(*Args().build(dtype=dtype)) == -1
        assert b"dtype" in lib.nvt_last_error()
    for bad in (0, (1 << 20) + 1):
        assert lib.nvt_pq_dict_build(*Args().build(max_entries=bad)) == -1
        assert b"max_entries" in lib.nvt_last_error()
    a = Args()
    assert lib.nvt_pq_dict_build(*a.build(ws_bytes=a.ws_bytes - 1)) == -1
    assert b"workspace too small" in lib.nvt_last_error()
    assert lib.nvt_pq_dict_build(*a.build(ws=a.a["ws"] + 4)) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_pq_dict_build(*a.build(n=1 << 31)) == -1


def test_pack_rejects_bad_arguments():
    lib = _lib()
    for hole in ("values", "pages", "state", "out", "ws"):
        assert lib.nvt_pq_dict_pack(*Args().pack(**{hole: None})) == -1, hole
        assert b"null" in lib.nvt_last_error()
    for dtype in (0, 1, 4, 5, 6, 7, -1):
        assert lib.nvt_pq_dict_pack(*Args().pack(dtype=dtype)) == -1
        assert b"dtype" in lib.nvt_last_error()
    for bad in (0, (1 << 20) + 1):
        assert lib.nvt_pq_dict_pack(*Args().pack(max_entries=bad)) == -1
        assert b"max_entries" in lib.nvt_last_error()
    a = Args(npages=3)
    assert lib.nvt_pq_dict_pack(*a.pack(ws_bytes=a.ws_bytes - 1)) == -1
    assert b"workspace too small" in lib.nvt_last_error()
    assert lib.nvt_pq_dict_pack(*a.pack(out=a.a["out"] + 8)) == -1
    assert b"aligned" in lib.nvt_last_error()
    # a workspace sized for the build alone does not hold the page tables
    assert lib.nvt_pq_dict_pack(*a.pack(ws_bytes=_need(a.n, npages=0))) == -1
    assert b"workspace too small" in lib.nvt_last_error()


def test_nothing_to_pack_returns_ok():
    lib = _lib()
    a = Args()
    assert lib.nvt_pq_dict_pack(*a.pack(n=0)) == 0        # pages without values have no bytes
    assert lib.nvt_pq_dict_pack(*a.pack(npages=0)) == 0
