"""The C-ABI shared library loads and exports every symbol include/nvt_hip.h declares
(no compute calls: this runs without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "nvt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nvt_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _lib.load()
    declared = _declared()
    assert len(declared) >= 40
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nvt_hip.h but not exported"
    # the ctypes table covers the header exactly (no stale or missing bindings)
    assert sorted(_lib.SIGNATURES) == declared
    assert lib.nvt_version() >= 100


def test_argument_validation_needs_no_gpu():
    """Bad arguments are rejected on the host side with NVT_EINVAL + a message."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    nbytes = C.c_uint64()
    assert lib.nvt_count_table_bytes(3, 64, C.byref(nbytes)) == -1
    assert b"key_bytes" in lib.nvt_last_error()
    assert lib.nvt_count_table_bytes(4, 1 << 20, C.byref(nbytes)) == 0 and nbytes.value == 8 << 20
    assert lib.nvt_encode_table_bytes(8, 1 << 10, C.byref(nbytes)) == 0 and nbytes.value == 16 << 10
    assert lib.nvt_dense_count_ws_bytes(4, 1000, 9, 0, C.byref(nbytes)) == -1
    # round 6: key directory / one-pass images reject bad arguments before any launch
    assert lib.nvt_keydir_build(None, 10, 10, None, None) == -1 and b"null" in lib.nvt_last_error()
    buf = (C.c_uint32 * 64)()
    keys = (C.c_int32 * 4)(1, 2, 3, 4)
    assert lib.nvt_keydir_build(keys, 0, 10, buf, None) == -1          # no keys
    assert lib.nvt_keydir_build(keys, 4, 0, buf, None) == -1           # no buckets
    part = _lib.ImagePart(kind=7)
    arr = (_lib.ImagePart * 1)(part)
    assert lib.nvt_image_build(arr, 1, 16, buf, 64, None) == -1 and b"kind" in lib.nvt_last_error()
    assert lib.nvt_image_build(arr, 5, 16, buf, 64, None) == -1        # more than 4 parts
    assert lib.nvt_image_build(arr, 0, 16, buf, 200, None) == -1       # stride > 192
    assert lib.nvt_image_build(arr, 0, 0, buf, 64, None) == 0          # nothing to do


def test_encode_entry_points_refuse_bad_arguments_before_any_launch():
    """nvt_encode_* / nvt_encode_build_* / nvt_encode_many: every refusal is NVT_EINVAL, names its
    argument in nvt_last_error and comes before the first launch (host buffers stand in for device
    memory: nothing is read through them)."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    raw = (C.c_uint8 * 4096)()
    base = (C.addressof(raw) + 63) & ~63           # 64-byte aligned inside the buffer
    keys, out, table, sent, vocab = base, base + 1024, base + 2048, base + 3072, base + 3200

    def refused(rc, *words):
        assert rc == _lib.NVT_EINVAL, rc
        msg = lib.nvt_last_error()
        for w in words:
            assert w in msg, (w, msg)

    for enc in (lib.nvt_encode_i32, lib.nvt_encode_i64):
        # (keys, valid, n, table, capacity, sentinel, null, oov, nb, out, out_bytes, vocab, n_vocab, first, stream)
        refused(enc(keys + 4, None, 8, table, 64, sent, 1, 2, 0, out, 8, None, 0, 3, None), b"keys/out", b"aligned")
        refused(enc(keys, None, 8, table, 64, sent, 1, 2, 0, out + 8, 8, None, 0, 3, None), b"keys/out", b"aligned")
        refused(enc(keys, None, 8, table, 96, sent, 1, 2, 0, out, 8, None, 0, 3, None), b"capacity")
        refused(enc(keys, None, 8, table, 32, sent, 1, 2, 0, out, 8, None, 0, 3, None), b"capacity")
        refused(enc(keys, None, 8, table, 64, sent, 1, 2, 0, out, 2, None, 0, 3, None), b"out_bytes")
        refused(enc(keys, None, 8, None, 64, sent, 1, 2, 0, out, 8, None, 0, 3, None), b"null table")
        refused(enc(None, None, 8, table, 64, sent, 1, 2, 0, out, 8, None, 0, 3, None), b"null keys/out")
        assert enc(None, None, 0, table, 64, sent, 1, 2, 0, None, 8, None, 0, 3, None) == 0   # no rows: nothing to do
    for build in (lib.nvt_encode_build_i32, lib.nvt_encode_build_i64):
        # (vocab, n, first_label, table, capacity, sentinel, unique, stream)
        refused(build(vocab, 10, 3, table, 96, sent, 0, None), b"capacity", b"2^k")
        refused(build(vocab, 10, 3, table, 32, sent, 0, None), b"capacity")
        refused(build(vocab, 64, 3, table, 64, sent, 0, None), b"capacity", b"exceed")     # capacity == n_vocab
        refused(build(vocab, 100, 3, table, 64, sent, 1, None), b"capacity", b"exceed")    # capacity < n_vocab
        refused(build(vocab, 10, 3, None, 64, sent, 0, None), b"null table")
        refused(build(vocab, 10, 3, table, 64, None, 0, None), b"null table")
    # int32 slots hold int32 labels: first_label + n_vocab must stay below INT32_MAX
    refused(lib.nvt_encode_build_i32(vocab, 10, 2**31 - 11, table, 64, sent, 0, None), b"labels overflow int32")
    refused(lib.nvt_encode_build_i32(vocab, 10, 2**40, table, 64, sent, 1, None), b"labels overflow int32")
    refused(lib.nvt_encode_build_i64(vocab, 10, -1, table, 64, sent, 0, None), b"first_label")
    # descriptors: key width and label width
    d = (_lib.EncodeCol * 1)()
    d[0].keys, d[0].out, d[0].table, d[0].sentinel_label = keys, out, table, sent
    d[0].n, d[0].capacity, d[0].null_label, d[0].oov_label, d[0].first_label = 8, 64, 1, 2, 3
    d[0].key_bytes, d[0].out_bytes = 3, 8
    refused(lib.nvt_encode_many(d, 1, None), b"key_bytes", b"column 0")
    d[0].key_bytes, d[0].out_bytes = 4, 2
    refused(lib.nvt_encode_many(d, 1, None), b"out_bytes")
    d[0].key_bytes, d[0].out_bytes = 8, 8
    d[0].keys = keys + 8
    refused(lib.nvt_encode_many(d, 1, None), b"keys/out", b"aligned")
    refused(lib.nvt_encode_many(None, 1, None), b"null descriptors")
    assert lib.nvt_encode_many(None, 0, None) == 0


def test_count_entry_points_refuse_bad_arguments_before_any_launch():
    """nvt_dense_count_i32 / _i64 / nvt_dense_count_many / nvt_dense_count_ws_bytes: every refusal is
    NVT_EINVAL, names its argument in nvt_last_error and comes before the first launch (host buffers
    stand in for device memory: nothing is read through them)."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    raw = (C.c_uint8 * 8192)()
    base = (C.addressof(raw) + 63) & ~63
    keys, outk, outc, state, ws, aux, wts = (base + 512 * i for i in range(7))
    RANGE, SORT, HOT, PIECES = 9, 10, 16, 0x10000

    def refused(rc, *words):
        assert rc == _lib.NVT_EINVAL, (rc, lib.nvt_last_error())
        msg = lib.nvt_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def many(**kw):
        d = (_lib.CountCol * 1)()
        c = dict(keys=keys, valid=None, weights=None, n=8, key_bytes=4, path=0, ws=ws, out_keys=outk,
                 out_counts=outc, out_capacity=9, state=state, hot_image=None, range_table=None)
        c.update(kw)
        for name, v in c.items():
            setattr(d[0], name, v)
        return lib.nvt_dense_count_many(d, 1, None)

    # (keys, valid, weights, n, path, ws, out_keys, out_counts, out_capacity, state, stream)
    for fn in (lib.nvt_dense_count_i32, lib.nvt_dense_count_i64):
        for path in (0, 6, 7, 1, 2, 3):
            refused(fn(keys + 8, None, None, 8, path, ws, outk, outc, 9, state, None), b"keys", b"aligned")
        refused(fn(keys, None, None, 8, 0, ws, outk, outc, 9, None, None), b"null state/workspace")
        refused(fn(keys, None, None, 8, 0, None, outk, outc, 9, state, None), b"null state/workspace")
        refused(fn(None, None, None, 8, 1, ws, outk, outc, 9, state, None), b"null keys/out")
        for path in (4, 5, 8, 11, -1, 255):
            refused(fn(keys, None, None, 8, path, ws, outk, outc, 9, state, None), b"path must be")
        for path in (0 | HOT, 6 | HOT, 7 | HOT):               # the filter on a path that does not take it
            refused(fn(keys, None, None, 8, path, ws, outk, outc, 9, state, None), b"hot filter")
        refused(fn(keys, None, wts, 8, 1 | HOT, ws, outk, outc, 9, state, None), b"hot filter", b"without weights")
    # paths 9 and 10 without the column's aux block (the single-column entry points have none)
    refused(lib.nvt_dense_count_i32(keys, None, None, 8, RANGE | (8 << 8), ws, outk, outc, 9, state, None), b"aux block")
    refused(lib.nvt_dense_count_i32(keys, None, None, 8, SORT, ws, outk, outc, 9, state, None), b"histogram block")
    refused(lib.nvt_dense_count_i64(keys, None, None, 8, 2 | HOT, ws, outk, outc, 9, state, None), b"hot filter", b"int32")
    refused(lib.nvt_dense_count_i64(keys, None, None, 8, RANGE | (8 << 8), ws, outk, outc, 9, state, None),
            b"range path", b"int32")
    refused(lib.nvt_dense_count_i64(keys, None, None, 8, SORT, ws, outk, outc, 9, state, None), b"sort path", b"int32")
    # the descriptors of nvt_dense_count_many
    refused(many(key_bytes=3), b"key_bytes", b"column 0")
    refused(many(key_bytes=8, path=RANGE | (8 << 8), hot_image=aux), b"range path", b"int32")
    refused(many(key_bytes=8, path=SORT, hot_image=aux), b"sort path", b"int32")
    refused(many(weights=wts, path=RANGE | (8 << 8), hot_image=aux), b"range path", b"without weights")
    refused(many(weights=wts, path=SORT, hot_image=aux), b"sort path", b"without weights")
    refused(many(path=RANGE | (8 << 8)), b"aux block")
    refused(many(path=RANGE | (8 << 8) | PIECES), b"aux block")
    refused(many(path=SORT), b"histogram block")
    for bits in (0, 5, 11, 255):
        refused(many(path=RANGE | (bits << 8), hot_image=aux), b"64 .. 1024 buckets")
    for path in (RANGE | (8 << 8), SORT, 1 | HOT, 0):
        refused(many(path=path, hot_image=aux, keys=keys + 4), b"keys", b"aligned")
        refused(many(path=path, hot_image=aux, state=None), b"null state/workspace")
        refused(many(path=path, hot_image=aux, ws=None), b"null state/workspace")
    refused(many(path=7 | HOT), b"hot filter")
    refused(many(path=12), b"path must be")
    refused(lib.nvt_dense_count_many(None, 1, None), b"null descriptors")
    assert lib.nvt_dense_count_many(None, 0, None) == 0
    # more distinct workspaces than internal streams (kSideStreams = 3)
    d = (_lib.CountCol * 4)()
    for i in range(4):
        d[i].keys, d[i].n, d[i].key_bytes, d[i].path, d[i].ws = keys, 8, 4, 0, ws + 16 * i
        d[i].out_keys, d[i].out_counts, d[i].out_capacity, d[i].state = outk, outc, 9, None
    refused(lib.nvt_dense_count_many(d, 4, None), b"at most 3 distinct workspaces")
    # the workspace size follows the same rules
    nbytes = C.c_uint64()
    refused(lib.nvt_dense_count_ws_bytes(3, 1000, 0, 0, C.byref(nbytes)), b"key_bytes must be 4 or 8")
    refused(lib.nvt_dense_count_ws_bytes(4, 1000, 8, 0, C.byref(nbytes)), b"path must be")
    refused(lib.nvt_dense_count_ws_bytes(4, 1000, 0 | HOT, 0, C.byref(nbytes)), b"hot filter")
    refused(lib.nvt_dense_count_ws_bytes(8, 1000, 1 | HOT, 0, C.byref(nbytes)), b"hot filter")
    refused(lib.nvt_dense_count_ws_bytes(4, 1000, 1 | HOT, 1, C.byref(nbytes)), b"hot filter")
    refused(lib.nvt_dense_count_ws_bytes(8, 1000, RANGE | (8 << 8), 0, C.byref(nbytes)), b"range path")
    refused(lib.nvt_dense_count_ws_bytes(4, 1000, RANGE | (8 << 8), 1, C.byref(nbytes)), b"range path")
    refused(lib.nvt_dense_count_ws_bytes(4, 1000, RANGE | (5 << 8), 0, C.byref(nbytes)), b"64 .. 1024 buckets")
    refused(lib.nvt_dense_count_ws_bytes(4, 1000, RANGE | (11 << 8), 0, C.byref(nbytes)), b"64 .. 1024 buckets")
    refused(lib.nvt_dense_count_ws_bytes(8, 1000, SORT, 0, C.byref(nbytes)), b"sort path")
    refused(lib.nvt_range_table_bytes(11, C.byref(nbytes)), b"64 .. 1024 buckets")
    for path in (0, 6, 7, 1, 2, 3, 1 | HOT, RANGE | (6 << 8), RANGE | (10 << 8) | PIECES, SORT):
        assert lib.nvt_dense_count_ws_bytes(4, 1000, path, 0, C.byref(nbytes)) == 0 and nbytes.value > 0


_WS_N = (0, 1, 8191, 8192, 8193, 65536, 1 << 20, 2**32 - 1)
# (key_bytes, path, weighted) -> nvt_dense_count_ws_bytes for every n of _WS_N, as returned by the
# library before the counting driver was split into units (profiles/dense_count_split_notes.md).
# path: 0x10 = NVT_PATH_HOT, 0x609 / 0xa09 = range path with 64 / 1024 buckets, 0x10000 =
# NVT_PATH_PIECES, 0xa = sort path
_WS_BYTES = {
    (4, 0x0, 0): (38011968, 38011968, 38011968, 38011968, 38011968, 38011968, 38011968, 38011968),
    (4, 0x0, 1): (19137600, 19137600, 19137600, 19137600, 19137600, 19137600, 19137600, 19137600),
    (8, 0x0, 0): (25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056),
    (8, 0x0, 1): (25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056),
    (4, 0x6, 0): (38011968, 38011968, 38011968, 38011968, 38011968, 38011968, 38011968, 38011968),
    (4, 0x6, 1): (19137600, 19137600, 19137600, 19137600, 19137600, 19137600, 19137600, 19137600),
    (8, 0x6, 0): (25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056),
    (8, 0x6, 1): (25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056, 25429056),
    (4, 0x7, 0): (76023872, 76023872, 76023872, 76023872, 76023872, 76023872, 76023872, 76023872),
    (4, 0x7, 1): (38275136, 38275136, 38275136, 38275136, 38275136, 38275136, 38275136, 38275136),
    (8, 0x7, 0): (50858048, 50858048, 50858048, 50858048, 50858048, 50858048, 50858048, 50858048),
    (8, 0x7, 1): (50858048, 50858048, 50858048, 50858048, 50858048, 50858048, 50858048, 50858048),
    (4, 0x1, 0): (34704640, 34705728, 34869504, 34869504, 34870592, 36760928, 67605760, 89491541200),
    (4, 0x1, 1): (34557184, 34558304, 34853120, 34853120, 34854240, 37293408, 78337280, 156701068496),
    (8, 0x1, 0): (34606336, 34607424, 34869504, 34869504, 34870592, 37203296, 76158208, 140024515792),
    (8, 0x1, 1): (34606336, 34607456, 35000576, 35000576, 35001696, 38251872, 92935424, 208743992528),
    (4, 0x2, 0): (34483456, 34484544, 34648320, 34648320, 34649408, 35876144, 56766592, 91306134736),
    (4, 0x2, 1): (34557184, 34558304, 34853120, 34853120, 34854240, 37072176, 74797184, 164857449680),
    (8, 0x2, 0): (34508032, 34509120, 34771200, 34771200, 34772288, 36711728, 69767296, 144456355024),
    (8, 0x2, 1): (34606336, 34607456, 35000576, 35000576, 35001696, 37956912, 88215680, 219618282704),
    (4, 0x3, 0): (34557184, 34558272, 34722048, 34722048, 34723136, 36023600, 58019968, 96137972944),
    (4, 0x3, 1): (34557184, 34558304, 34853120, 34853120, 34854240, 37072176, 74797184, 164857449680),
    (8, 0x3, 0): (34606336, 34607424, 34869504, 34869504, 34870592, 36908336, 71438464, 150898805968),
    (8, 0x3, 1): (34606336, 34607456, 35000576, 35000576, 35001696, 37956912, 88215680, 219618282704),
    (4, 0x11, 0): (43126016, 43128128, 43291904, 43291904, 43294016, 45190496, 76158208, 90036833488),
    (4, 0x12, 0): (42904832, 42906944, 43070720, 43070720, 43072832, 44305712, 65319040, 91851427024),
    (4, 0x13, 0): (42978560, 42980672, 43144448, 43144448, 43146560, 44453168, 66572416, 96683265232),
    (4, 0x609, 0): (12681856, 12681856, 12681856, 12681856, 12681856, 13730432, 21070464, 34372420224),
    (4, 0xa09, 0): (76587136, 76587136, 76587136, 76587136, 76587136, 76587136, 93364352, 34436325504),
    (4, 0x10609, 0): (12681856, 12681856, 12681856, 12681856, 12681856, 13730432, 21070464, 34372420224),
    (4, 0x10a09, 0): (76587136, 76587136, 76587136, 76587136, 76587136, 76587136, 93364352, 34436325504),
    (4, 0xa, 0): (1053504, 1058368, 1155904, 1155904, 1160768, 1872704, 14161728, 53692339008),
}


@pytest.mark.parametrize("key_bytes, path, weighted", sorted(_WS_BYTES))
def test_count_workspace_sizes_are_unchanged(key_bytes, path, weighted):
    """The workspace of every counting path, byte for byte what the unsplit driver asked for."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    nbytes = C.c_uint64()
    for n, want in zip(_WS_N, _WS_BYTES[key_bytes, path, weighted]):
        assert lib.nvt_dense_count_ws_bytes(key_bytes, n, path, weighted, C.byref(nbytes)) == 0
        assert nbytes.value == want, (n, nbytes.value, want)


_GB_WS_N = (1, 4095, 4096, 4097, 32768, 1 << 20, (1 << 26) - 1)
# read from the library of the commit before the split of nvt_groupby.hip into four units
_GB_WS_BYTES = {
    "nvt_gb_update_ws_bytes": (8406064, 8504080, 8504096, 8512560, 9249568, 35660576, 1753228048),
    "nvt_order_rows_ws_bytes": (8406064, 8504080, 8504096, 8512560, 9249568, 35660576, 1753228048),
    "nvt_sgb_sort_ws_bytes": (8406272, 8504320, 8504320, 8512768, 9249792, 35660800, 1753228288),
    "nvt_sgb_regroup_ws_bytes": (512, 512, 512, 512, 512, 2560, 131584),
    "nvt_count_merge_sorted_ws_bytes": (8407040, 8553728, 8553728, 8562688, 9643264, 48246016, 2558665984),
}
# (nkeys, nvals, flags) -> bytes at capacity 64 and 1 << 20; flags 3 = NVT_GB_SUMSQ | NVT_GB_MINMAX
_GB_TABLE_BYTES = {
    (1, 0, 0): (2560, 33554944),
    (1, 1, 0): (3072, 41943552),
    (3, 8, 3): (19968, 318767616),
    (2, 0, 3): (3072, 41943552),
}


def test_groupby_workspace_sizes_are_unchanged():
    """The workspaces and the table block of the groupby family, byte for byte what the unsplit
    nvt_groupby.hip asked for; the shapes and the short block a table refuses."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    assert (_lib.NVT_GB_SUMSQ | _lib.NVT_GB_MINMAX) == 3
    nbytes = C.c_uint64()
    for name, wants in sorted(_GB_WS_BYTES.items()):
        for n, want in zip(_GB_WS_N, wants):
            assert getattr(lib, name)(n, C.byref(nbytes)) == 0, (name, n, lib.nvt_last_error())
            assert nbytes.value == want, (name, n, nbytes.value, want)
    for (nkeys, nvals, flags), wants in sorted(_GB_TABLE_BYTES.items()):
        for capacity, want in zip((64, 1 << 20), wants):
            assert lib.nvt_gb_table_bytes(nkeys, nvals, flags, capacity, C.byref(nbytes)) == 0
            assert nbytes.value == want, (nkeys, nvals, flags, capacity, nbytes.value, want)
    for nkeys, nvals in ((0, 0), (4, 0), (1, 9)):
        assert lib.nvt_gb_table_bytes(nkeys, nvals, 0, 64, C.byref(nbytes)) == _lib.NVT_EINVAL, (nkeys, nvals)
    # a block one byte short (host memory: the refusal comes before anything touches it)
    want = _GB_TABLE_BYTES[1, 1, 0][0]
    raw = (C.c_uint8 * want)()
    handle = C.c_void_p()
    assert lib.nvt_gb_create_in(1, 1, 0, 64, C.addressof(raw), want - 1, C.byref(handle)) == _lib.NVT_EINVAL
    assert b"too small" in lib.nvt_last_error() and not handle.value


def test_count_workspace_refuses_the_paths_the_launch_refuses():
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    nbytes = C.c_uint64()
    for path in (4, 5, 4 | 16, 5 | 16):
        for key_bytes in (4, 8):
            assert lib.nvt_dense_count_ws_bytes(key_bytes, 1000, path, 0, C.byref(nbytes)) == _lib.NVT_EINVAL
            assert b"path must be" in lib.nvt_last_error()


@pytest.mark.parametrize("bad", [dict(key_bytes=3), dict(path=12)])
def test_count_many_checks_every_column_before_the_first_launch(bad):
    """A valid column in front of a bad one: NVT_EINVAL naming column 1.  The buffers are host memory
    and there is no device, so a call that had started on column 0 would return a HIP error."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    raw = (C.c_uint8 * 8192)()
    base = (C.addressof(raw) + 63) & ~63
    keys, outk, outc, state, ws = (base + 512 * i for i in range(5))
    d = (_lib.CountCol * 2)()
    for i in range(2):
        d[i].keys, d[i].n, d[i].key_bytes, d[i].path, d[i].ws = keys, 8, 4, 0, ws
        d[i].out_keys, d[i].out_counts, d[i].out_capacity, d[i].state = outk, outc, 9, state + 128 * i
    for name, v in bad.items():
        setattr(d[1], name, v)
    assert lib.nvt_dense_count_many(d, 2, None) == _lib.NVT_EINVAL, lib.nvt_last_error()
    msg = lib.nvt_last_error()
    assert b"column 1" in msg and (b"key_bytes" if "key_bytes" in bad else b"path must be") in msg, msg


@pytest.mark.parametrize("n, n_big", [(1, 0), (1, 1), (4096, 0), (4097, 2), (4097, 4097), (1 << 20, 16385),
                                      ((1 << 30) - 1, 0)])
def test_vocab_order_workspace_layout(n, n_big):
    """nvt_vocab_order_tmp_bytes is the layout of the ordering workspace (order_ws, nvt_vocab_order.hip)
    written out: status words of the class scatter | sort scratch of class 255 | label_of[n] | status
    words of the flat build, every block padded to 16 bytes, 64 bytes behind the last."""
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()

    def pad16(x):
        return (x + 15) & ~15

    got, sort_bytes = C.c_uint64(), C.c_uint64(0)
    assert lib.nvt_vocab_order_tmp_bytes(n, n_big, C.byref(got)) == 0
    if n_big > 1:
        assert lib.nvt_vocab_sort_tmp_bytes(4, n_big, C.byref(sort_bytes)) == 0 and sort_bytes.value > 0
    ntiles = -(-n // 4096)
    want = pad16(ntiles * 1024 + 64) + pad16(sort_bytes.value) + pad16(4 * n) + pad16(8 * ntiles + 64) + 64
    assert got.value == want, (n, n_big, got.value, want)


def test_ops_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pandas as pd

    import nvtabular_amd as nvt
    from nvtabular_amd import _lib, ops

    wf = nvt.Workflow(["a"] >> ops.Categorify())
    with pytest.raises(_lib.NvtHipError, match="no CPU fallback"):
        wf.fit(nvt.Dataset(pd.DataFrame({"a": [1, 2, 3]})))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "nvtabular_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle", src, flags=re.M), f
