"""Kernel-level matrix for the device steps around the multi-GPU vocabulary exchange
(nvtabular_amd/csrc/nvt_exchange.hip).  Every entry point is called through ``_lib.load()`` on
buffers this file owns and compared bit for bit with exchange_reference.py (pinned on the CPU by
test_exchange_reference.py).  Every output lies between two 64-byte guards of 0xA5 that must be
intact afterwards; what a call does not write inside an output still holds 0xA5.

Kernel or branch -> the case that reaches it (a wave = 64 adjacent entries of the virtual
concatenation of all columns; kXMaxCols = 64, kXMaxCells = 4096 = ranks x columns).

  nvt_exchange_ranges (x_ranges_kernel)
    wave inside one column                  entries 64 .. 127 (column 3) and most of column 6     test_cells[adjacent-*]
    wave straddling columns, an empty       columns of 0, 1, 63, 64, 65, 1, 4097 entries: the     test_cells[adjacent-*]
    column between them                     waves at 0 and at 192 hold two and three columns
    last wave partly past the end           4291 entries in all                                   test_cells[adjacent-*]
    ssum == 0: reported as empty            a column of zero counts; a column without entries     test_ranges_of_nothing
    INT32_MIN / INT32_MAX                   both keys in one column                               test_cells[edges-*]
  nvt_exchange_hist / _scatter (x_group_kernel<false / true>)
    wave inside one cell                    key-ordered column of 4097 entries, G = 3             test_cells[adjacent-3]
    wave straddling cells or columns        the same column at its owner boundaries; the short    test_cells[adjacent-*], [*-shuffled lists]
                                            columns; every shuffled list
    G = 1; width = 1 (all but the first     G = 1; column 6 of `adjacent`                         test_cells[*-1], test_cells[adjacent-*]
    keys clamp to G - 1); lo < 0            negative key ranges and a lo below the least key
    64 columns, 4096 cells                  64 columns x G = 64                                   test_cells[sixty_four-64]
    cursors advanced to the cell ends       cursors = starts + histogram afterwards               test_cells
  nvt_exchange_pack_ordered                 the key-ordered lists, compared as the words lie      test_cells
  nvt_exchange_unpack / _unpack2            round trips of scatter -> unpack and pack_ordered     test_cells
                                            -> unpack2, counts of 2^31 - 1 among them;
    empty segment, odd destinations         segments of 0, 7, 0, 493, 500 words to 3, 1001, 101   test_unpack_segments
  counts of 2^31 and above                  leave the word (header): pinned                       test_counts_beyond_the_word
  argument checks                           65 columns, 4097 cells, G = 0, null pointers          test_argument_checks

Left out: nvt_exchange_ranges_sorted (two loads per column, read in test_gpu_sorted_groupby.py);
multi-rank runs; timing.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import exchange_reference as R
from kernel_buffers import Guarded, Lib, dev

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
BIG = 2 ** 31 - 1
POISON64 = np.frombuffer(b"\xA5" * 8, dtype=np.int64)[0]
POISON32 = np.frombuffer(b"\xA5" * 4, dtype=np.int32)[0]


@pytest.fixture(scope="module")
def L():
    yield Lib()
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


class Batch:
    """The descriptor array of some (keys int32, counts int64) columns on the device."""

    def __init__(self, L, cols):
        self.L, self.cols, self.ncol = L, cols, len(cols)
        self.total = sum(len(k) for k, _ in cols)
        self.held = [(dev(k), dev(c)) if len(k) else (None, None) for k, c in cols]
        self.desc = (L.m.XCol * max(self.ncol, 1))()
        for d, (k, c), (tk, tc) in zip(self.desc, cols, self.held):
            assert k.dtype == np.int32 and c.dtype == np.int64
            d.keys, d.counts, d.n = (None, None, 0) if tk is None else (tk.data_ptr(), tc.data_ptr(), len(k))

    def owner_args(self, lo, width):
        return (C.c_int64 * self.ncol)(*[int(v) for v in lo]), (C.c_uint64 * self.ncol)(*[int(v) for v in width])

    def ranges(self):
        out = Guarded(self.ncol * 24)
        self.L.call("nvt_exchange_ranges", self.desc, self.ncol, out.ptr)
        return out.read(np.int64, "ranges").reshape(self.ncol, 3)

    def hist(self, lo, width, G):
        out = Guarded(G * self.ncol * 8)
        a, b = self.owner_args(lo, width)
        self.L.call("nvt_exchange_hist", self.desc, self.ncol, a, b, G, out.ptr)
        return out.read(np.int64, "send_mat").reshape(G, self.ncol)

    def scatter(self, lo, width, G, starts):
        cur, rows = Guarded(G * self.ncol * 8, init=starts.astype(np.uint64)), Guarded(self.total * 8)
        a, b = self.owner_args(lo, width)
        self.L.call("nvt_exchange_scatter", self.desc, self.ncol, a, b, G, cur.ptr, rows.ptr)
        return rows.read(np.int64, "rows_out").copy(), cur.read(np.int64, "cursors").reshape(G, self.ncol)

    def pack_ordered(self, lo, width, G, starts, first_row):
        rows = Guarded(self.total * 8)
        a, b = self.owner_args(lo, width)
        d_first, d_start = dev(first_row.astype(np.uint64)), dev(starts.astype(np.uint64))
        self.L.call("nvt_exchange_pack_ordered", self.desc, self.ncol, a, b, G, d_first.data_ptr(), d_start.data_ptr(),
                    rows.ptr)
        return rows.read(np.int64, "rows_out").copy()


def unpack(L, words, seg_off, dst_off, out_n, extra=None):
    """nvt_exchange_unpack (extra: _unpack2) into poisoned outputs of out_n entries."""
    d_words, d_seg, d_dst = dev(words), dev(np.asarray(seg_off, np.uint64)), dev(np.asarray(dst_off, np.uint64))
    keys, cnts = Guarded(out_n * 4), Guarded(out_n * 8)
    if extra is None:
        L.call("nvt_exchange_unpack", d_words.data_ptr(), len(words), d_seg.data_ptr(), d_dst.data_ptr(),
               len(seg_off) - 1, keys.ptr, cnts.ptr)
        return keys.read(np.int32, "keys_out").copy(), cnts.read(np.int64, "counts_out").copy()
    d_extra, xo = dev(extra), Guarded(out_n * 4)
    L.call("nvt_exchange_unpack2", d_words.data_ptr(), d_extra.data_ptr(), len(words), d_seg.data_ptr(),
           d_dst.data_ptr(), len(seg_off) - 1, keys.ptr, cnts.ptr, xo.ptr)
    return (keys.read(np.int32, "keys_out").copy(), cnts.read(np.int64, "counts_out").copy(),
            xo.read(np.int32, "extra_out").copy())


def ref_unpack(words, seg_off, dst_off, out_n, extra=None):
    keys, cnts, xo = np.full(out_n, POISON32), np.full(out_n, POISON64), np.full(out_n, POISON32)
    R.unpack(words, seg_off, dst_off, keys, cnts, extra, xo)
    return (keys, cnts) if extra is None else (keys, cnts, xo)


def column(size, lo, hi, rng):
    """A key-ordered list (keys may repeat) whose counts include the largest the word holds."""
    k = np.sort(rng.integers(lo, hi + 1, size)).astype(np.int32)
    c = rng.integers(1, 1000, size).astype(np.int64)
    c[rng.random(size) < 0.2] = BIG
    return k, c


def layout(name, rng):
    """(columns, lo, span): span = the key range the owner widths are cut from."""
    if name == "adjacent":
        sizes = [0, 1, 63, 64, 65, 1, 4097]
        spans = [(0, 0), (7, 7), (-300, -200), (-5000, 4000), (0, 40), (I32.max, I32.max), (-100_000, 100_000)]
    elif name == "sixty_four":
        sizes = [int(v) for v in rng.integers(0, 150, 64)]
        sizes[5], sizes[63] = 0, 1
        spans = [(int(a), int(a) + int(b)) for a, b in zip(rng.integers(-10_000, 10_000, 64), rng.integers(0, 5000, 64))]
    else:   # edges
        sizes = [2, 3000, 2]
        spans = [(I32.min, I32.max)] * 3
    cols = [column(s, a, b, rng) for s, (a, b) in zip(sizes, spans)]
    if name == "edges":
        for j in (0, 2):
            cols[j][0][:] = (I32.min, I32.max)
        cols[0][1][:] = BIG
    lo = [max(a - (j % 3) * 10, I32.min) for j, (a, _) in enumerate(spans)]       # lo at or below the least key
    return cols, lo, [b - l + 1 for l, (_, b) in zip(lo, spans)]


@pytest.mark.parametrize("G", [1, 3, 64])
@pytest.mark.parametrize("name", ["adjacent", "sixty_four", "edges"])
def test_cells(L, name, G):
    rng = np.random.default_rng(seed_of("cells", name, G))
    cols, lo, span = layout(name, rng)
    ncol = len(cols)
    width = [max(1, -(-s // G)) for s in span]
    if name == "adjacent":
        width[6] = 1                       # every key but the least few belongs to the last rank
    shuffled = []
    for k, c in cols:
        p = rng.permutation(len(k))
        shuffled.append((k[p], c[p]))
    mat = R.hist(cols, lo, width, G)
    assert (mat > 0).sum() > min(G, 2) - 1 and mat.sum() == sum(len(k) for k, _ in cols)
    starts = np.zeros(G * ncol, dtype=np.int64)
    starts[1:] = np.cumsum(mat.ravel())[:-1]                          # (owner, column) groups side by side
    starts = starts.reshape(G, ncol)
    first_row = np.cumsum(mat, axis=0) - mat
    col_at = np.concatenate([[0], np.cumsum([len(k) for k, _ in cols])])
    seg_off = np.concatenate([[0], np.cumsum(mat.ravel())])
    dst_off = (col_at[:-1][None, :] + first_row).ravel()              # column-major: every column one list
    total = int(col_at[-1])

    for what, lists in (("key-ordered lists", cols), ("shuffled lists", shuffled)):
        b = Batch(L, lists)
        np.testing.assert_array_equal(b.ranges(), R.ranges(lists), err_msg=what)
        np.testing.assert_array_equal(b.hist(lo, width, G), mat, err_msg=what)
        rows, cursors = b.scatter(lo, width, G, starts)
        np.testing.assert_array_equal(cursors, starts + mat, err_msg=what)       # advanced to the cell ends
        owners = [R.owner(k, lo[j], width[j], G) for j, (k, _) in enumerate(lists)]
        for g in range(G):
            for j, (k, c) in enumerate(lists):
                sel = owners[j] == g
                got = rows[starts[g, j]: starts[g, j] + mat[g, j]]
                np.testing.assert_array_equal(np.sort(got), np.sort(R.pack_words(k[sel], c[sel])),
                                              err_msg=f"{what}: cell ({g}, {j})")
        # back through unpack: every column gets its rows, in some order inside a cell
        keys, cnts = unpack(L, rows, seg_off, dst_off, total)
        for j, (k, c) in enumerate(lists):
            got = sorted(zip(keys[col_at[j]: col_at[j + 1]].tolist(), cnts[col_at[j]: col_at[j + 1]].tolist()))
            assert got == sorted(zip(k.tolist(), c.tolist())), f"{what}: column {j}"

    b = Batch(L, cols)
    rows = b.pack_ordered(lo, width, G, starts, first_row)
    np.testing.assert_array_equal(rows, R.pack_ordered(cols, lo, width, G, first_row, starts, total, POISON64))
    extra = rng.integers(I32.min, I32.max, total, dtype=np.int64).astype(np.int32)
    keys, cnts, xo = unpack(L, rows, seg_off, dst_off, total, extra)
    np.testing.assert_array_equal(keys, np.concatenate([k for k, _ in cols]))    # exactly the lists again
    np.testing.assert_array_equal(cnts, np.concatenate([c for _, c in cols]))
    ek, ec, ex = ref_unpack(rows, seg_off, dst_off, total, extra)
    np.testing.assert_array_equal(xo, ex)
    assert (cnts == BIG).any()


def test_ranges_of_nothing(L):
    """A column whose counts sum to 0 is reported like a column without entries; and a call in
    which no column has an entry launches only the initialisation."""
    rng = np.random.default_rng(1)
    zero = (np.array([5, -9, 12], np.int32), np.zeros(3, np.int64))
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int64))
    cols = [column(100, -50, 50, rng), zero, empty, column(1, 3, 3, rng), (zero[0], np.array([0, 1, 0], np.int64))]
    got = Batch(L, cols).ranges()
    np.testing.assert_array_equal(got, R.ranges(cols))
    assert got[1].tolist() == got[2].tolist() == list(R.EMPTY) and got[4].tolist() == [9, 12, 1]
    np.testing.assert_array_equal(Batch(L, [empty, empty]).ranges(), [R.EMPTY] * 2)


def test_unpack_segments(L):
    rng = np.random.default_rng(2)
    n, out_n = 1000, 1601
    words = R.pack_words(rng.integers(I32.min, I32.max + 1, n), rng.integers(0, 2 ** 31, n))
    extra = rng.integers(I32.min, I32.max + 1, n).astype(np.int32)
    seg_off, dst_off = [0, 0, 7, 7, 500, 1000], [3, 3, 701, 1001, 101]
    for got, exp in zip(unpack(L, words, seg_off, dst_off, out_n), ref_unpack(words, seg_off, dst_off, out_n)):
        np.testing.assert_array_equal(got, exp)                       # and 0xA5 wherever no segment went
    for got, exp in zip(unpack(L, words, seg_off, dst_off, out_n, extra),
                        ref_unpack(words, seg_off, dst_off, out_n, extra)):
        np.testing.assert_array_equal(got, exp)
    k, c = unpack(L, words[:1], [0, 0, 1], [9, 1], 3)                 # one word behind an empty segment
    assert k.tolist() == [POISON32, int(R.unpack_words(words[:1])[0][0]), POISON32]
    k, c = unpack(L, words[:0], [0, 0], [0], 2)                       # n = 0: nothing is written
    assert k.tolist() == [POISON32] * 2 and c.tolist() == [POISON64] * 2


def test_counts_beyond_the_word(L):
    """include/nvt_hip.h: a count of 2^31 or more does not fit the word -- its low 32 bits travel
    and come back sign-extended (dist.py keeps G * max rows below 2^31).  The sum of
    nvt_exchange_ranges is 64 bits wide and exact."""
    keys = np.array([1, 2, 3, 4], np.int32)
    cnts = np.array([2 ** 31, 2 ** 32 + 5, 2 ** 32 - 1, BIG], np.int64)
    b = Batch(L, [(keys, cnts)])
    assert b.ranges().tolist() == [[-1, 4, int(cnts.sum())]]
    starts = np.zeros((1, 1), np.int64)
    for rows in (b.scatter([1], [4], 1, starts)[0], b.pack_ordered([1], [4], 1, starts, starts)):
        k, c = unpack(L, np.sort(rows), [0, 4], [0], 4)
        got = sorted(zip(k.tolist(), c.tolist()))
        assert got == [(1, -2 ** 31), (2, 5), (3, -1), (4, BIG)]
        assert got == sorted(zip(*[a.tolist() for a in R.unpack_words(R.pack_words(keys, cnts))]))


def test_argument_checks(L):
    """Refused before any launch: NVT_EINVAL, a message, untouched outputs."""
    rng = np.random.default_rng(3)
    one = column(10, 0, 9, rng)
    out = Guarded(8 * 4200)
    b65 = Batch(L, [one] * 65)
    assert "1..64 columns" in L.refused("nvt_exchange_ranges", b65.desc, 65, out.ptr, by="fill_batch")
    assert "1..64 columns" in L.refused("nvt_exchange_ranges", b65.desc, 0, out.ptr, by="fill_batch")
    assert "null out" in L.refused("nvt_exchange_ranges", b65.desc, 1, None)
    b = Batch(L, [one] * 17)
    a, w = b.owner_args([0] * 17, [1] * 17)
    cur, rows = Guarded(8 * 4200, init=np.zeros(4200, np.uint64)), Guarded(8 * 170)
    first = dev(np.zeros(4200, np.uint64))
    for G in (241, 0, -1):                 # 17 x 241 = 4097 cells
        assert "<= 4096" in L.refused("nvt_exchange_hist", b.desc, 17, a, w, G, out.ptr)
        assert "<= 4096" in L.refused("nvt_exchange_scatter", b.desc, 17, a, w, G, cur.ptr, rows.ptr)
        assert "<= 4096" in L.refused("nvt_exchange_pack_ordered", b.desc, 17, a, w, G, first.data_ptr(),
                                      first.data_ptr(), rows.ptr)
    a65, w65 = b65.owner_args([0] * 65, [1] * 65)
    assert "1..64 columns" in L.refused("nvt_exchange_hist", b65.desc, 65, a65, w65, 1, out.ptr, by="fill_batch")
    assert "1..64 columns" in L.refused("nvt_exchange_scatter", b65.desc, 65, a65, w65, 1, cur.ptr, rows.ptr,
                                        by="fill_batch")
    assert "null pointer" in L.refused("nvt_exchange_hist", b.desc, 17, None, w, 2, out.ptr)
    assert "null pointer" in L.refused("nvt_exchange_hist", b.desc, 17, a, None, 2, out.ptr)
    assert "null pointer" in L.refused("nvt_exchange_hist", b.desc, 17, a, w, 2, None)
    assert "null pointer" in L.refused("nvt_exchange_scatter", b.desc, 17, a, w, 2, None, rows.ptr)
    assert "null pointer" in L.refused("nvt_exchange_scatter", b.desc, 17, a, w, 2, cur.ptr, None)
    bad = Batch(L, [one])
    bad.desc[0].counts = None
    assert "null column" in L.refused("nvt_exchange_ranges", bad.desc, 1, out.ptr, by="fill_batch")
    words = dev(np.zeros(4, np.int64))
    assert "null pointer" in L.refused("nvt_exchange_unpack", words.data_ptr(), 4, first.data_ptr(), first.data_ptr(),
                                       0, out.ptr, out.ptr)
    assert "null pointer" in L.refused("nvt_exchange_unpack2", words.data_ptr(), None, 4, first.data_ptr(),
                                       first.data_ptr(), 1, out.ptr, out.ptr, out.ptr)
    assert (out.read() == 0xA5).all() and (rows.read() == 0xA5).all() and (cur.read() == 0).all()
    # 64 columns x 64 ranks = 4096 cells are accepted (test_cells[sixty_four-64] compares them)
    assert Batch(L, [one] * 64).hist([0] * 64, [1] * 64, 64).sum() == 640
