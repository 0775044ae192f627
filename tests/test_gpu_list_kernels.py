"""Kernel-level matrix for the session kernels of nvtabular_amd/csrc/nvt_list.hip (ops.ListSlice,
ops.ValueCount, ops.DifferenceLag).  Every entry point is called through ``_lib.load()`` on buffers
this file owns and every output is compared bit for bit with list_reference.py (pinned on the CPU by
test_list_reference.py): leaves as raw bytes, offsets, bitmaps with the bits past the end, NaN
positions.  Every output lies between two 64-byte guards of 0xA5 that must be intact afterwards.

Kernel or branch -> the case that reaches it (kTile = 2048 rows / output leaves, kListStage = 2050
staged offsets, kBlock = 256 lanes x 8 rows, NVT_LIST_MAX_COLS = 32 descriptors a launch).

  nvt_list_slice_offsets
    slice_len_kernel, 8 rows a lane         the last lane's rows end at n: n = 1, 7, 8, 9          test_slice_offsets[1 .. 9]
    one tile, full tile, second tile        n = 2047, 2048, 2049                                  test_slice_offsets[2047 .. 2049]
    scan_totals_kernel, second round        600 000 rows = 293 tiles > 256                        test_slice_offsets[600000]
    slice_row clamps                        start, end in {0, +-1, +-L, +-(L + 1), INT64_MAX,     test_slice_offsets (81 pairs; 6 at 600 000)
                                            INT64_MIN}, rows of 0, 1, L - 1, L, L + 1 leaves
    slice_add_kernel, out[n]                the last row sliced again: every case
    offsets[0] != 0                         first = 13                                            test_slice_offsets[*-13]
    64-bit lengths and totals               rows of 2^33 and 2^40 leaves (fabricated offsets)     test_slice_offsets_of_huge_rows
  nvt_list_slice_many, ragged (slice_move_kernel<false>)
    staged, 2049 / 2050 offsets in LDS      sliced lengths [1] + [0] * E + [1] * 2047, E = 0, 1   test_ragged[stage0 / stage1]
    global search between the bounds        E = 2 (2050 rows under tile 0), 2100 empty rows       test_ragged[stage2 / edge_run]
                                            in front of a tile's last leaf
    last tile short, q >= p1 lanes          totals 63, 64, 65, 2047, 2048, 2049                   test_ragged[total*]
    one row over three tiles                [5, 5000, 0, 7]                                       test_ragged[three_tiles]
    a row starting at leaf 2048             [2048, 10], [1000, 1048, 0, 0, 33]                    test_ragged[at2048 / at2048b]
    runs of empty rows                      leading, trailing, around a tile edge                 test_ragged[empty_runs / edge_run]
    width 1 / 4 / 8, src_valid or not       six columns in every call                             test_ragged
    two launches                            33 columns                                            test_thirty_three_columns
    dst_valid in whole words                bitmap compared over ceil(total / 64) * 8 bytes, the guards behind it
    total == 0                              every row sliced to nothing: a no-op                  test_nothing_left
  nvt_list_slice_many, padded (slice_move_kernel<true>, 32-bit division)
    pad_width 1, 7 (no divisor of 64),      pad_bits of every width, padded leaves valid,         test_padded
    a width above every row                 dst_valid with and without src_valid
    total == 0                              n = 0                                                 test_nothing_left
  nvt_list_len_minmax (len_minmax_kernel)
    blocks that see no row                  columns of 1, 255, 257 and 70 000 rows in one launch  test_len_minmax
    two launches, two calls into one acc    33 columns; a second call                             test_len_minmax
    64-bit lengths                          a fabricated row of 2^40 leaves                       test_len_minmax
  nvt_difference_lag_many (lag_kernel)
    j outside [0, n)                        shifts {0, +-1, +-(n - 1), +-n, INT64_MAX, INT64_MIN} test_lag[n = 1, 63, 64, 65, 257]
    shift groups across launches            45 descriptors in shuffled shift order (40 in         test_lag, test_lag_forty_descriptors
                                            test_lag_forty_descriptors), each its own `out`
    key_same, every dtype                   0 .. 4 keys, NaN keys, null keys                      test_lag
    lag_diff, every dtype                   int64 beyond 2^53, float64 differences that round,    test_lag
                                            uint8, int32, float32; validity null at i or j
  argument checks                           every refusal of the header, nothing launched         test_argument_checks

Left out: the 64-bit division of the padded move (total > 2^32 - 1 output leaves) needs more than
4 GiB for one column of bytes; multi-rank runs; timing.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import list_reference as R
from kernel_buffers import Guarded, Lib, dev

pytestmark = pytest.mark.gpu

INT64_MAX, INT64_MIN = R.INT64_MAX, R.INT64_MIN
CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3,
        np.dtype(np.uint8): 4}                                       # include/nvt_hip.h NVT_F32 ..


@pytest.fixture(scope="module")
def L():
    lib = Lib()
    assert [lib.m.NVT_F32, lib.m.NVT_F64, lib.m.NVT_I32, lib.m.NVT_I64, lib.m.NVT_U8] == list(CODE.values())
    assert (lib.m.LIST_MAX_COLS, lib.m.LAG_MAX_KEYS) == (32, 4)
    yield lib
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def offsets_of(lens, first=0):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
    return off + first


# ---------------------------------------------------------------------------------------------
# nvt_list_slice_offsets
# ---------------------------------------------------------------------------------------------
def slice_offsets(L, off, start, end):
    n = len(off) - 1
    need = C.c_uint64()
    L.m.check(L.lib.nvt_list_slice_ws_bytes(n, C.byref(need)), "nvt_list_slice_ws_bytes")
    assert need.value == ((n + 2047) // 2048 + 1) * 8
    d_off, ws, out = dev(off), Guarded(need.value), Guarded((n + 1) * 8)
    L.call("nvt_list_slice_offsets", d_off.data_ptr(), n, start, end, out.ptr, ws.ptr, need.value)
    got = out.read(np.int64, "out_offsets").copy()
    ws.read(what="workspace")
    return got


BOUND = 5        # the L of the slice bounds below; the frames hold rows of 0, 1, L - 1, L, L + 1 leaves
BOUNDS = [0, 1, -1, BOUND, -BOUND, BOUND + 1, -(BOUND + 1), INT64_MAX, INT64_MIN]


@pytest.mark.parametrize("first", [0, 13])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 600_000])
def test_slice_offsets(L, n, first):
    rng = np.random.default_rng(seed_of("so", n, first))
    lens = rng.choice([0, 1, BOUND - 1, BOUND, BOUND + 1, 2 * BOUND + 1], n)
    if n == 1:
        lens[:] = BOUND
    off = offsets_of(lens, first)
    pairs = [(a, b) for a in BOUNDS for b in BOUNDS]
    if n > 10_000:   # the scan's second round does not depend on the slice
        pairs = [(0, INT64_MAX), (1, -1), (-BOUND, INT64_MAX), (INT64_MIN, BOUND), (-1, INT64_MAX), (BOUND, 1)]
    for start, end in pairs:
        got = slice_offsets(L, off, start, end)
        np.testing.assert_array_equal(got, R.slice_offsets(off, start, end), err_msg=f"[{start}:{end}]")


@pytest.mark.parametrize("start,end", [(-10, INT64_MAX), (3, 5), (1, -1), (0, INT64_MAX), (INT64_MIN, -(1 << 33))])
def test_slice_offsets_of_huge_rows(L, start, end):
    """Only the offsets are read, so rows of 2^33 and 2^40 leaves cost nothing: neither a length nor
    a tile total nor the running sum (2^49 over 2500 rows, two tiles) may be narrowed to 32 bits."""
    for lens in ([1 << 33, 1 << 40], [1 << 33, 0, 1 << 40, 3, 1] * 500):
        off = offsets_of(lens, 7)
        exp = R.slice_offsets(off, start, end)
        np.testing.assert_array_equal(slice_offsets(L, off, start, end), exp)
    if (start, end) == (1, -1):
        assert int(exp[-1]) == 500 * ((1 << 33) + (1 << 40) - 4 + 1)


# ---------------------------------------------------------------------------------------------
# nvt_list_slice_many
# ---------------------------------------------------------------------------------------------
KINDS = [(np.uint8, True), (np.int32, False), (np.float64, True), (np.int64, False), (np.float32, True),
         (np.uint8, False), (np.int32, True), (np.float64, False)]
PAD_VALUES = {np.uint8: 0xEE, np.int32: -123456, np.float64: -2.5, np.int64: -(1 << 40) - 3, np.float32: 1.5}


def pad_bits(value, dt):
    return int.from_bytes(np.array([value]).astype(dt).tobytes().ljust(8, b"\0"), "little")


def columns(nl, kinds, rng):
    """[(leaves, leaf validity or None)]: random bytes in every leaf (NaN payloads included)."""
    out = []
    for dt, has_valid in kinds:
        vals = rng.integers(0, 256, nl * np.dtype(dt).itemsize, dtype=np.uint8).view(dt)
        out.append((vals, (rng.random(nl) < 0.7) if has_valid else None))
    return out


def slice_many(L, cols, off, start, end, pad_width=None, valid_out=False):
    """Offsets from nvt_list_slice_offsets (ragged), one nvt_list_slice_many call for all columns;
    every output compared with the reference.  valid_out: a padded column without src_valid asks
    for dst_valid all the same."""
    n = len(off) - 1
    d_off = dev(off)
    new_off = None
    if pad_width is None:
        exp_off = R.slice_offsets(off, start, end)
        total = int(exp_off[-1])
        new_off = Guarded((n + 1) * 8, init=slice_offsets(L, off, start, end))
        np.testing.assert_array_equal(new_off.read(np.int64), exp_off)
    else:
        total = n * pad_width
    descs = (L.m.ListCol * len(cols))()
    keep, outs = [], []
    for d, (vals, valid) in zip(descs, cols):
        w = vals.dtype.itemsize
        src = dev(vals) if len(vals) else torch.zeros(1, dtype=torch.uint8, device="cuda")
        sv = None if valid is None else dev(R.pack_bits(valid))
        dst = Guarded(total * w)
        dv = Guarded((total + 63) // 64 * 8) if (valid is not None or valid_out) else None
        keep.append((src, sv))
        outs.append((dst, dv))
        d.src, d.dst, d.width = src.data_ptr(), dst.ptr, w
        d.src_valid = None if sv is None else sv.data_ptr()
        d.dst_valid = None if dv is None else dv.ptr
        d.pad_bits = pad_bits(PAD_VALUES[vals.dtype.type], vals.dtype) if pad_width is not None else 0
    L.call("nvt_list_slice_many", descs, len(cols), d_off.data_ptr(), n, start, end,
           None if new_off is None else new_off.ptr, total, pad_width or 0)
    for ci, ((vals, valid), (dst, dv)) in enumerate(zip(cols, outs)):
        what = f"column {ci} {vals.dtype} [{start}:{end}] pad {pad_width}"
        ev, eok, eoff = R.slice_rows(vals, valid, off, start, end, pad_width, PAD_VALUES[vals.dtype.type])
        assert int(eoff[-1]) == total and len(ev) == total
        np.testing.assert_array_equal(dst.read(what=what), ev.view(np.uint8), err_msg=what)
        if dv is not None:
            np.testing.assert_array_equal(dv.read(what=what + " bitmap"), R.pack_bits(eok), err_msg=what)
    return total


def frame_for(sliced, first, rng):
    """A frame whose rows, sliced [1:], have the given lengths: a row of s + 1 leaves for s > 0, an
    empty row or a row of one leaf for s = 0."""
    sliced = np.asarray(sliced, dtype=np.int64)
    lens = np.where(sliced > 0, sliced + 1, rng.integers(0, 2, len(sliced)))
    return offsets_of(lens, first)


def partition_of(total, rng):
    """Row lengths 0 .. 5 that sum to ``total``."""
    out = []
    while sum(out) < total:
        out.append(int(min(rng.integers(0, 6), total - sum(out))))
    return out + [0]


RAGGED = {
    "stage0": [1] + [1] * 2047 + [3, 0, 2],
    "stage1": [1] + [0] * 1 + [1] * 2047 + [3, 0, 2],
    "stage2": [1] + [0] * 2 + [1] * 2047 + [3, 0, 2],
    "three_tiles": [5, 5000, 0, 7],
    "at2048": [2048, 10],
    "at2048b": [1000, 1048, 0, 0, 33],
    "empty_runs": [0] * 70 + [2048] + [0] * 3000 + [5] + [0] * 40,
    "edge_run": [0, 0, 2047] + [0] * 2100 + [2] + [0] * 2100 + [2047, 0, 1] + [0] * 5,
}
TOTALS = [63, 64, 65, 2047, 2048, 2049]


@pytest.mark.parametrize("first", [0, 13])
@pytest.mark.parametrize("case", list(RAGGED) + [f"total{t}" for t in TOTALS])
def test_ragged(L, case, first):
    rng = np.random.default_rng(seed_of("ragged", case, first))
    sliced = RAGGED[case] if case in RAGGED else partition_of(int(case[5:]), rng)
    off = frame_for(sliced, first, rng)
    cols = columns(int(off[-1] - off[0]), KINDS[:6], rng)
    total = slice_many(L, cols, off, 1, INT64_MAX)
    assert total == sum(sliced)
    if case in ("three_tiles", "total65", "total2049"):               # the same frame, other slices
        for start, end in [(-3, INT64_MAX), (1, -1), (0, 2), (INT64_MIN, INT64_MAX)]:
            slice_many(L, cols, off, start, end)


def test_thirty_three_columns(L):
    rng = np.random.default_rng(33)
    off = frame_for(partition_of(2100, rng), 5, rng)
    kinds = [KINDS[i % len(KINDS)] for i in range(33)]
    slice_many(L, columns(int(off[-1] - off[0]), kinds, rng), off, 1, INT64_MAX)
    slice_many(L, columns(int(off[-1] - off[0]), kinds, rng), off, -4, INT64_MAX, pad_width=4, valid_out=True)


@pytest.mark.parametrize("first", [0, 13])
@pytest.mark.parametrize("n", [1, 9, 300])
def test_padded(L, n, first):
    rng = np.random.default_rng(seed_of("pad", n, first))
    lens = rng.integers(0, 7, n)
    off = offsets_of(lens, first)
    nl = int(lens.sum())
    for valid_out in (False, True):
        cols = columns(nl, KINDS, rng)
        slice_many(L, cols, off, -1, INT64_MAX, pad_width=1, valid_out=valid_out)      # rows of 0 or 1 leaves
        slice_many(L, cols, off, 0, 1, pad_width=1, valid_out=valid_out)
        slice_many(L, cols, off, 0, INT64_MAX, pad_width=9, valid_out=valid_out)       # above every row
        slice_many(L, cols, off, 1, 8, pad_width=7, valid_out=valid_out)               # 7 divides no tile
        slice_many(L, cols, off, -3, -1, pad_width=3, valid_out=valid_out)
        slice_many(L, cols, off, 2, INT64_MAX, pad_width=64, valid_out=valid_out)


def test_nothing_left(L):
    """total == 0 is a no-op: ragged when every row is sliced to nothing, padded when n == 0."""
    rng = np.random.default_rng(0)
    off = offsets_of([3, 0, 1, 2], 4)
    cols = columns(6, KINDS[:6], rng)
    assert slice_many(L, cols, off, 3, INT64_MAX) == 0
    assert slice_many(L, cols, off, 0, 0) == 0
    assert slice_many(L, cols, offsets_of([], 4), 0, 2, pad_width=3, valid_out=True) == 0


# ---------------------------------------------------------------------------------------------
# nvt_list_len_minmax
# ---------------------------------------------------------------------------------------------
def len_minmax(L, offs, accs):
    descs = (L.m.ListLenCol * len(offs))()
    keep = [dev(o) for o in offs]
    for d, o, a in zip(descs, keep, accs):
        d.offsets, d.n, d.acc = o.data_ptr(), o.numel() - 1, a.ptr
    L.call("nvt_list_len_minmax", descs, len(offs))
    return [tuple(int(v) for v in a.read(np.int64, "acc")) for a in accs]


def new_acc():
    return Guarded(16, init=np.array([INT64_MAX, INT64_MIN], dtype=np.int64))


def test_len_minmax(L):
    rng = np.random.default_rng(4)
    rows = [1, 255, 257, 70_000]
    # the extremes of the long column lie in rows that only its later blocks read
    offs = [offsets_of(rng.integers(3, 9, r), first=r) for r in rows]
    lens = rng.integers(3, 9, 70_000)
    lens[[40_000, 69_999]] = (0, 77)
    offs[3] = offsets_of(lens, 5)
    accs = [new_acc() for _ in rows]
    assert len_minmax(L, offs, accs) == [R.len_minmax(o) for o in offs]
    # a second call folds into the same accumulators; a row of 2^40 leaves
    more = [offsets_of([2, 1 << 40, 4], 9), offsets_of([11], 0), offsets_of(rng.integers(0, 3, 300)), offs[0]]
    exp = [(min(a[0], b[0]), max(a[1], b[1])) for a, b in zip(map(R.len_minmax, offs), map(R.len_minmax, more))]
    assert len_minmax(L, more, accs) == exp
    assert exp[0][1] == 1 << 40
    # 33 columns: two launches; column sizes that put the short ones in front of and behind long ones
    sizes = [1, 3000, 2, 255, 257, 5000] * 5 + [1, 2049, 64]
    offs = [offsets_of(rng.integers(i % 4, 12 + i, s), first=i) for i, s in enumerate(sizes)]
    accs = [new_acc() for _ in sizes]
    assert len_minmax(L, offs, accs) == [R.len_minmax(o) for o in offs]


# ---------------------------------------------------------------------------------------------
# nvt_difference_lag_many
# ---------------------------------------------------------------------------------------------
X_DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint8]


def lag_values(dt, n, rng):
    if dt == np.uint8:
        return rng.integers(0, 256, n).astype(dt)
    if dt == np.int32:
        return rng.integers(-(2 ** 31), 2 ** 31, n).astype(dt)
    if dt == np.int64:
        return (rng.integers(-(2 ** 62), 2 ** 62, n) | 1).astype(dt)        # beyond 2^53, odd
    return (rng.standard_normal(n) * 1e3 + 1e9).astype(dt)                 # differences that round in float32


def lag_key(dt, n, rng, with_valid):
    k = rng.integers(0, 2, n).astype(dt)
    if np.dtype(dt).kind == "f":
        k[rng.random(n) < 0.1] = np.nan
    return k, (rng.random(n) < 0.85) if with_valid else None


def lag_many(L, keys, cols, n):
    """keys: [(values, validity or None)], cols: [(values, validity or None, shift)] in the order
    they are handed over.  Returns one float32[n] per entry of cols, read from its own `out`."""
    kd = (L.m.LagKey * max(len(keys), 1))()
    keep = []
    for d, (k, kv) in zip(kd, keys):
        t, v = dev(k), None if kv is None else dev(R.pack_bits(kv))
        keep.append((t, v))
        d.x, d.valid, d.dtype = t.data_ptr(), None if v is None else v.data_ptr(), CODE[k.dtype]
    cd = (L.m.LagCol * len(cols))()
    outs = []
    for d, (x, xv, shift) in zip(cd, cols):
        t, v, out = dev(x), None if xv is None else dev(R.pack_bits(xv)), Guarded(n * 4)
        keep.append((t, v))
        outs.append(out)
        d.x, d.valid, d.out = t.data_ptr(), None if v is None else v.data_ptr(), out.ptr
        d.shift, d.dtype = shift, CODE[x.dtype]
    L.call("nvt_difference_lag_many", kd, len(keys), cd, len(cols), n)
    return [o.read(np.float32, f"out {i}").copy() for i, o in enumerate(outs)]


def same_floats(got, exp, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=what)              # NaN positions
    np.testing.assert_array_equal(got[~np.isnan(got)].view(np.uint32), exp[~np.isnan(exp)].view(np.uint32),
                                  err_msg=what)


def check_lag(L, keys, cols, n):
    for i, (got, (x, xv, shift)) in enumerate(zip(lag_many(L, keys, cols, n), cols)):
        same_floats(got, R.lag(keys, x, xv, shift), f"descriptor {i}: {x.dtype} shift {shift} n {n}")


@pytest.mark.parametrize("nkeys", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_lag(L, n, nkeys):
    rng = np.random.default_rng(seed_of("lag", n, nkeys))
    shifts = [0, 1, -1, n - 1, -(n - 1), n, -n, INT64_MAX, INT64_MIN]
    # every key dtype in turn over the (n, nkeys) grid; every other key carries a bitmap
    rot = [1, 63, 64, 65, 257].index(n)
    keys = [lag_key(X_DTYPES[(rot + q) % 5], n, rng, with_valid=(q + rot) % 2 == 0) for q in range(nkeys)]
    cols = [(lag_values(dt, n, rng), (rng.random(n) < 0.8) if (si + di) % 2 else None, s)
            for di, dt in enumerate(X_DTYPES) for si, s in enumerate(shifts)]
    order = rng.permutation(len(cols))                                     # 45: two launches
    check_lag(L, keys, [cols[i] for i in order], n)


def test_lag_forty_descriptors(L):
    """Five shifts, eight descriptors each, handed over shuffled: the entry sorts them by shift, so
    every group of eight ends up side by side and the fourth straddles the two launches; each
    result must still land in the `out` of the descriptor it came with."""
    n = 300
    rng = np.random.default_rng(40)
    keys = [lag_key(np.int32, n, rng, True), lag_key(np.float64, n, rng, False)]
    cols = [(lag_values(X_DTYPES[i % 5], n, rng), (rng.random(n) < 0.8) if i % 3 else None, s)
            for s in (-2, 0, 1, 3, 299) for i in range(8)]
    assert len(cols) == 40
    check_lag(L, keys, [cols[i] for i in rng.permutation(40)], n)


# ---------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------
def test_argument_checks(L):
    """Every refusal comes before any launch: NVT_EINVAL, a message, and untouched outputs."""
    off = dev(offsets_of([2, 3]))
    out, ws = Guarded(24), Guarded(16)
    base = [off.data_ptr(), 2, 0, 1, out.ptr, ws.ptr, 16]

    def offsets_call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[{"off": 0, "n": 1, "out": 4, "ws": 5, "ws_bytes": 6}[k]] = v
        return L.refused("nvt_list_slice_offsets", *a)

    assert "null pointer" in offsets_call(off=None)
    assert "null pointer" in offsets_call(out=None)
    assert "positive" in offsets_call(n=0)
    assert "null workspace" in offsets_call(ws=None)
    assert "aligned" in offsets_call(ws=ws.ptr + 4)
    assert "smaller" in offsets_call(ws_bytes=8)
    assert (out.read() == 0xA5).all() and (ws.read() == 0xA5).all()

    src, dst, dv = dev(np.arange(5, dtype=np.int64)), Guarded(40), Guarded(8)
    sv = dev(R.pack_bits(np.ones(5, bool)))
    noff = dev(np.array([0, 2, 5], dtype=np.int64))

    def many(ncols=1, width=8, src_valid=None, dst_valid=None, out_offsets=noff.data_ptr(), total=5, pad_width=0,
             descs="own", s=src.data_ptr(), d=dst.ptr):
        c = (L.m.ListCol * 1)()
        c[0].src, c[0].dst, c[0].width, c[0].src_valid, c[0].dst_valid = s, d, width, src_valid, dst_valid
        return L.refused("nvt_list_slice_many", c if descs == "own" else None, ncols, off.data_ptr(), 2, 0, INT64_MAX,
                         out_offsets, total, pad_width)

    assert "null descriptors" in many(descs=None)
    assert "positive" in many(ncols=0)
    assert "not both" in many(pad_width=3, total=6)
    assert "is needed" in many(out_offsets=None)
    assert "n * pad_width" in many(out_offsets=None, pad_width=3, total=5)
    assert "n * pad_width" in many(out_offsets=None, pad_width=3, total=7)
    assert "width must be" in many(width=2)
    assert "needs dst_valid" in many(src_valid=sv.data_ptr())
    assert "8-byte aligned" in many(src_valid=sv.data_ptr(), dst_valid=dv.ptr + 4)
    assert "null pointer" in many(s=None)
    assert "null pointer" in many(d=None)
    assert "null pointer" in many(d=None, out_offsets=None, pad_width=3, total=6)
    assert (dst.read() == 0xA5).all() and (dv.read() == 0xA5).all()

    acc = new_acc()
    lc = (L.m.ListLenCol * 1)()
    lc[0].offsets, lc[0].n, lc[0].acc = off.data_ptr(), 2, acc.ptr
    assert "null descriptors" in L.refused("nvt_list_len_minmax", None, 1)
    assert "positive" in L.refused("nvt_list_len_minmax", lc, 0)
    lc[0].acc = None
    assert "null pointer" in L.refused("nvt_list_len_minmax", lc, 1)
    lc[0].offsets, lc[0].acc = None, acc.ptr
    assert "null pointer" in L.refused("nvt_list_len_minmax", lc, 1)
    assert acc.read(np.int64).tolist() == [INT64_MAX, INT64_MIN]

    x, res = dev(np.arange(4, dtype=np.int32)), Guarded(16)
    kd, cd = (L.m.LagKey * 5)(), (L.m.LagCol * 1025)()
    for d in kd:
        d.x, d.dtype = x.data_ptr(), 2
    for d in cd:
        d.x, d.out, d.dtype, d.shift = x.data_ptr(), res.ptr, 2, 1

    def lag(nkeys=1, ncols=1, keys=kd, cols=cd):
        return L.refused("nvt_difference_lag_many", keys, nkeys, cols, ncols, 4)

    assert "at most 4" in lag(nkeys=5)
    assert "at most 4" in lag(nkeys=-1)
    assert "null partition descriptors" in lag(keys=None)
    assert "null descriptors" in lag(cols=None)
    assert "positive" in lag(ncols=0)
    assert "at most 1024" in lag(ncols=1025)
    kd[0].dtype = 5
    assert "unsupported partition dtype" in lag()
    kd[0].dtype, kd[0].x = 2, None
    assert "null partition column" in lag()
    kd[0].x, cd[0].dtype = x.data_ptr(), -1
    assert "unsupported dtype" in lag()
    cd[0].dtype, cd[0].out = 2, None
    assert "null pointer" in lag()
    cd[0].out, cd[0].x = res.ptr, None
    assert "null pointer" in lag()
    assert (res.read() == 0xA5).all()
