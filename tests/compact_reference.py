"""Plain numpy statements of what the row-compaction kernels of nvt_compact.hip compute (ops.Filter /
ops.Dropna), as include/nvt_hip.h and the file header of nvt_compact.hip word them.  Nothing here
imports the package: test_compact_reference.py pins these functions to boolean indexing and Python
list slicing on the CPU, test_gpu_compact_kernels.py compares the kernels with them bit for bit.

A PLAN covers n rows in tiles of 2048: ``words`` uint64[ntiles * 32], bit i of word i / 64 = row i
is kept (bits past n are 0); ``counts`` uint32[ntiles], the kept rows of every tile (what a keep
producer leaves in ``base``); ``base`` uint32[ntiles + 1], their exclusive scan after
nvt_compact_plan, base[ntiles] = m."""
import numpy as np

TILE = 2048
TILE_WORDS = TILE // 64


def ntiles(n):
    return (n + TILE - 1) // TILE


def plan(keep):
    """keep bool[n] -> (words uint64[ntiles * 32], counts uint32[ntiles], base uint32[ntiles + 1])."""
    keep = np.asarray(keep, dtype=bool)
    nt = ntiles(len(keep))
    bits = np.zeros(nt * TILE, dtype=bool)
    bits[: len(keep)] = keep
    words = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)
    counts = bits.reshape(nt, TILE).sum(axis=1).astype(np.uint32)
    base = np.zeros(nt + 1, dtype=np.uint32)
    np.cumsum(counts, out=base[1:])
    return words, counts, base


def plan_layout(n):
    """Byte positions inside a plan's workspace: (words at, base at, end of base)."""
    nt = ntiles(n)
    return 0, nt * (TILE // 8), nt * (TILE // 8) + (nt + 1) * 4


def dropna_keep(cols, n):
    """cols: [(values, validity bool[] or None)].  Row i is kept only if, in every column, its
    validity is set and, for a float column, its value is not NaN."""
    keep = np.ones(n, dtype=bool)
    for x, valid in cols:
        if valid is not None:
            keep &= np.asarray(valid, dtype=bool)
        if x is not None and np.asarray(x).dtype.kind == "f":
            keep &= ~np.isnan(x)
    return keep


def list_keep(off, keep):
    """Leaf keep bool[n_leaves] of a list column: a leaf is kept iff its row is.  offsets[0] may be
    non-zero; leaf 0 is the leaf it names."""
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.asarray(keep, dtype=bool), np.diff(off))


def list_offsets(off, keep):
    """The m + 1 new offsets (from 0) of the kept rows."""
    lens = np.diff(np.asarray(off, dtype=np.int64))[np.asarray(keep, dtype=bool)]
    out = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=out[1:])
    return out


def compact(vals, keep):
    return np.asarray(vals)[np.asarray(keep, dtype=bool)]


def pack_bits(ok):
    """bool[m] -> uint8[ceil(m / 64) * 8], LSB first, the bits past m zero."""
    ok = np.asarray(ok, dtype=bool)
    out = np.zeros((len(ok) + 63) // 64 * 8, dtype=np.uint8)
    packed = np.packbits(ok, bitorder="little")
    out[: len(packed)] = packed
    return out
