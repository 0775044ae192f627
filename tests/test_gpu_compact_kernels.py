"""Kernel-level matrix for the parts of nvtabular_amd/csrc/nvt_compact.hip that the operator tests
reach only by chance: the Dropna keep mask over more than one batch of descriptors, and the list
half (leaf keep mask and new offsets).  Every entry point is called through ``_lib.load()`` on
buffers this file owns and compared bit for bit with compact_reference.py (pinned on the CPU by
test_compact_reference.py): mask words with the bits past n, tile counts, bases, leaves as raw
bytes, bitmaps with the bits past m, offsets.  Plans lie between 256-byte guards of 0xA5 (a plan
must be 256-byte aligned), every other output between 64-byte guards; all must be intact afterwards.

Kernel or branch -> the case that reaches it (kTile = 2048 rows = 32 mask words, 64 descriptors a
launch).

  nvt_compact_keep_dropna (keep_dropna_kernel, produce_tiles)
    one launch                              1 and 64 descriptors                                  test_dropna[1 / 64-*]
    accumulate: AND into the mask           65 descriptors (two launches), 130 (three); every     test_dropna[65 / 130-*]
                                            column nulls rows no other column nulls
    the last word short, a second tile      n = 1, 63, 64, 65, 2047, 2048, 2049                   test_dropna[*-n]
    bitmap null, NaN (float32 / float64),   columns of every dtype, x = NULL for integers         test_dropna
    integers without a bitmap
  nvt_compact_plan                          words, counts, base and m against the reference       test_dropna, test_list
  nvt_compact_list_keep (keep_expand_kernel)
    a row covering whole words and tiles    rows of 63, 64, 65, 2047, 2048, 2049, 5000 leaves     test_list[mixed-*]
    many rows starting inside one word      runs of 200 rows of one leaf                          test_list[mixed-*]
    the search lands on a run of empty rows rows of 0 leaves in front of a word's first leaf      test_list[mixed / trailing-*]
    last word full / last tile full         leaf totals 256 and 4096                              test_list[mult64 / mult2048-*]
    bit_range: a run of 62, 63, 64 bits     rows of 63 leaves from bit 0 and bit 1 of a word, a   test_list[word_edges-*-even / odd]
                                            row that is one word, every other row dropped
    offsets[0] != 0                         first = 9                                             test_list[*-9-*]
    n_leaves == 0                           every row empty: a no-op, leaf_plan NULL downstream   test_list[all_empty-*]
  nvt_compact_list_offsets (compact_offsets_kernel, plan_rank)
    rank at a tile start / at n_leaves      rows starting at leaf 2048 and 4096, trailing empty   test_list[mult2048 / trailing-*]
                                            rows kept (their start = n_leaves)
    kept rows without leaves                keep forced on every empty row                        test_list[*-empties]
    all rows dropped / all rows kept        m = 0, m = n                                          test_list[*-none / *-all]
  nvt_compact_many (compact_kernel)         the leaf plan (n = n_leaves) and the row plan (n rows) test_list
                                            in one call: leaves of width 8 with a bitmap, leaves
                                            of width 1, a row-level int32 column with a bitmap

Left out: flat columns (test_gpu_compact.py compares compact_frame with boolean indexing at every
tile size); multi-rank runs; timing.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import compact_reference as R
from kernel_buffers import Guarded, Lib, dev

pytestmark = pytest.mark.gpu

CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3,
        np.dtype(np.uint8): 4}                                       # include/nvt_hip.h NVT_F32 ..
DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint8]


@pytest.fixture(scope="module")
def L():
    lib = Lib()
    assert [lib.m.NVT_F32, lib.m.NVT_F64, lib.m.NVT_I32, lib.m.NVT_I64, lib.m.NVT_U8] == list(CODE.values())
    assert lib.m.COMPACT_MAX_COLS == 64
    yield lib
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


class Plan:
    """A plan's workspace between guards, and its parts as the file header of nvt_compact.hip lays
    them out."""

    def __init__(self, L, n):
        need = C.c_uint64()
        L.m.check(L.lib.nvt_compact_ws_bytes(n, C.byref(need)), "nvt_compact_ws_bytes")
        self.L, self.n, self.bytes = L, n, need.value
        self.at_words, self.at_base, self.end_base = R.plan_layout(n)
        assert self.bytes >= self.end_base
        self.ws = Guarded(self.bytes, guard=256)

    @property
    def ptr(self):
        return self.ws.ptr

    def parts(self):
        raw = self.ws.read(what="plan")
        return (raw[self.at_words: self.at_base].view(np.uint64).copy(),
                raw[self.at_base: self.end_base].view(np.uint32).copy())

    def check_produced(self, keep, what):
        """After a keep producer: the mask words, the kept rows per tile, base[ntiles] = 0."""
        words, counts, _ = R.plan(keep)
        got_w, got_b = self.parts()
        np.testing.assert_array_equal(got_w, words, err_msg=what + ": mask words")
        np.testing.assert_array_equal(got_b[:-1], counts, err_msg=what + ": tile counts")
        assert got_b[-1] == 0, what

    def scan(self, keep, what):
        """nvt_compact_plan: the words stay, base becomes the exclusive scan, *out_m = m."""
        out_m = Guarded(8)
        self.L.call("nvt_compact_plan", self.n, self.ptr, self.bytes, out_m.ptr)
        words, _, base = R.plan(keep)
        got_w, got_b = self.parts()
        np.testing.assert_array_equal(got_w, words, err_msg=what + ": mask words")
        np.testing.assert_array_equal(got_b, base, err_msg=what + ": bases")
        m = int(out_m.read(np.uint64, "out_m")[0])
        assert m == int(np.count_nonzero(keep)), what
        return m


# ---------------------------------------------------------------------------------------------
# nvt_compact_keep_dropna
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("ncols", [1, 64, 65, 130])
def test_dropna(L, ncols, n):
    rng = np.random.default_rng(seed_of("dropna", ncols, n))
    period = ncols + 3                     # column c nulls the rows with row % period == c, and no other
    rows = np.arange(n)
    cols, descs, keep_alive = [], (L.m.DropnaCol * ncols)(), []
    for c in range(ncols):
        dt = DTYPES[c % 5]
        mine = rows % period == c
        x = rng.integers(1, 100, n).astype(dt)
        valid = None
        if np.dtype(dt).kind == "f" and c % 2 == 0:
            x[mine] = np.nan                                         # null by value
        elif c % 7 != 3:
            valid = ~mine                                            # null by bitmap
            if np.dtype(dt).kind == "f":
                x[rng.random(n) < 0.01] = np.nan                     # and a few NaN on top
        cols.append((x, valid))
        is_float = np.dtype(dt).kind == "f"
        t = dev(x) if is_float or c % 2 else None                    # integers: x is not read
        v = None if valid is None else dev(R.pack_bits(valid))
        keep_alive.append((t, v))
        descs[c].x = None if t is None else t.data_ptr()
        descs[c].valid = None if v is None else v.data_ptr()
        descs[c].dtype = CODE[np.dtype(dt)]
    keep = R.dropna_keep(cols, n)
    if n >= period:
        for lo in range(0, ncols, 64):     # every batch removes rows that the other batches keep
            alone = R.dropna_keep(cols[lo: lo + 64], n)
            others = R.dropna_keep(cols[:lo] + cols[lo + 64:], n)
            assert (others & ~alone).any()
    plan = Plan(L, n)
    L.call("nvt_compact_keep_dropna", descs, ncols, n, plan.ptr, plan.bytes)
    plan.check_produced(keep, f"{ncols} columns, {n} rows")
    plan.scan(keep, f"{ncols} columns, {n} rows")


# ---------------------------------------------------------------------------------------------
# the list half
# ---------------------------------------------------------------------------------------------
ONES = [1] * 200
FRAMES = {
    "mixed": ONES + [63, 0, 64] + ONES + [65, 0, 0, 2047] + ONES + [2048, 1, 2049, 0, 5000] + ONES + [0, 0, 3],
    "mult64": [64, 0, 64, 1] + [1] * 62 + [0, 65],                           # 256 leaves
    # runs of 63 bits from bit 0 and from bit 1 of a word, one row that is exactly a word, 62 bits
    "word_edges": [63, 1, 1, 63, 64, 1, 62, 1, 64, 0, 1, 63],
    "mult2048": [2048, 1000, 0, 1048],                                       # 4096 leaves
    "trailing": ONES + [0] * 3 + [2047, 2, 0, 70] + [0] * 50,
    "all_empty": [0] * 100,
}


def keep_of(kind, lens, rng):
    n = len(lens)
    if kind == "none":
        return np.zeros(n, dtype=bool)
    if kind == "all":
        return np.ones(n, dtype=bool)
    if kind in ("even", "odd"):
        return np.arange(n) % 2 == (kind == "odd")                           # no kept row beside a kept row
    keep = rng.random(n) < 0.5
    if kind == "empties":
        keep[np.asarray(lens) == 0] = True                                   # kept rows that have no leaves
    return keep


@pytest.mark.parametrize("kind", ["random", "empties", "even", "odd", "none", "all"])
@pytest.mark.parametrize("first", [0, 9])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_list(L, frame, first, kind):
    rng = np.random.default_rng(seed_of("list", frame, first, kind))
    lens = FRAMES[frame]
    n, nl = len(lens), int(sum(lens))
    off = first + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keep = keep_of(kind, lens, rng)
    d_off, d_mask = dev(off), dev(keep.astype(np.uint8))

    rows = Plan(L, n)
    L.call("nvt_compact_keep_mask", d_mask.data_ptr(), n, rows.ptr, rows.bytes)
    rows.check_produced(keep, "row plan")
    m = rows.scan(keep, "row plan")

    leaf_keep = R.list_keep(off, keep)
    leaves = Plan(L, nl) if nl else None
    leaf_m = 0
    if nl:
        L.call("nvt_compact_list_keep", d_off.data_ptr(), n, rows.ptr, nl, leaves.ptr, leaves.bytes)
        leaves.check_produced(leaf_keep, "leaf plan")
        leaf_m = leaves.scan(leaf_keep, "leaf plan")
    else:   # n_leaves == 0 is a no-op, whatever else is passed
        L.call("nvt_compact_list_keep", d_off.data_ptr(), n, rows.ptr, 0, None, 0)

    # the leaves with their plan (n = nl) and a row-level column with its own (n rows) in one call
    jobs = []
    if nl:
        jobs.append((rng.integers(0, 256, nl * 8, dtype=np.uint8).view(np.int64), rng.random(nl) < 0.6, leaves, leaf_keep))
        jobs.append((rng.integers(0, 256, nl, dtype=np.uint8), None, leaves, leaf_keep))
    jobs.append((rng.integers(0, 256, n * 4, dtype=np.uint8).view(np.int32), rng.random(n) < 0.6, rows, keep))
    descs = (L.m.CompactCol * len(jobs))()
    held, outs = [], []
    for d, (vals, valid, plan, k) in zip(descs, jobs):
        mm = int(np.count_nonzero(k))
        src, sv = dev(vals), None if valid is None else dev(R.pack_bits(valid))
        dst = Guarded(mm * vals.dtype.itemsize)
        dv = None if valid is None else Guarded((mm + 63) // 64 * 8)
        held.append((src, sv))
        outs.append((dst, dv))
        d.src, d.dst, d.plan, d.n, d.width = src.data_ptr(), dst.ptr, plan.ptr, len(vals), vals.dtype.itemsize
        d.src_valid = None if sv is None else sv.data_ptr()
        d.dst_valid = None if dv is None else dv.ptr
    L.call("nvt_compact_many", descs, len(jobs))
    for i, ((vals, valid, plan, k), (dst, dv)) in enumerate(zip(jobs, outs)):
        what = f"descriptor {i} ({vals.dtype}, {len(vals)} values)"
        np.testing.assert_array_equal(dst.read(what=what), R.compact(vals, k).view(np.uint8), err_msg=what)
        if dv is not None:
            np.testing.assert_array_equal(dv.read(what=what + " bitmap"), R.pack_bits(R.compact(valid, k)), err_msg=what)

    new_off = Guarded((m + 1) * 8)
    L.call("nvt_compact_list_offsets", d_off.data_ptr(), n, rows.ptr, None if leaves is None else leaves.ptr, nl,
           new_off.ptr)
    exp = R.list_offsets(off, keep)
    np.testing.assert_array_equal(new_off.read(np.int64, "new offsets"), exp)
    assert int(exp[-1]) == leaf_m
    rows.ws.read(what="row plan")          # the consumers only read the plans
    if leaves is not None:
        leaves.ws.read(what="leaf plan")
