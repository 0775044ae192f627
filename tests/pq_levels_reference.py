"""Numpy restatement of the level arithmetic of the parquet list reader ("List columns in
the parquet reader"): the reference of tests/test_parquet_list_in_host.py and
tests/test_gpu_parquet_list_in.py.

A slot is a row start when its repetition level is 0, a leaf when its definition level is at least
``leaf_level`` (1 + the outer group being optional) and a non-null leaf when it equals ``max_def``.
``offsets[r]`` = leaf slots in front of the r-th row start, ``offsets[rows]`` = leaves; a null or an
empty list is one slot that is no leaf.  The staged streams hold 1 (rep) and W (def) bits per slot,
LSB first."""
import numpy as np


def levels_to_offsets(rep, dfn, leaf_level, max_def):
    """(offsets int64[rows + 1], valid bool[leaves]) of unpacked level arrays."""
    rep, dfn = np.asarray(rep, dtype=np.int64), np.asarray(dfn, dtype=np.int64)
    starts = rep == 0
    leaf = dfn >= leaf_level
    c = np.cumsum(leaf) - leaf
    offsets = np.append(c[starts], leaf.sum()).astype(np.int64)
    valid = (dfn == max_def)[leaf]
    return offsets, valid


def pack_levels(levels, width, nbytes=None):
    """Levels at ``width`` bits per slot, LSB first, padded with zero bytes to ``nbytes`` (default:
    whole 64-bit words)."""
    levels = np.asarray(levels, dtype=np.uint8)
    bits = ((levels[:, None] >> np.arange(width, dtype=np.uint8)) & 1).reshape(-1)
    out = np.packbits(bits, bitorder="little")
    if nbytes is None:
        nbytes = -(-len(levels) * width // 64) * 8
    return np.concatenate([out, np.zeros(nbytes - len(out), dtype=np.uint8)])


def unpack_levels(buf, width, n):
    """The first n levels of a packed stream (any bytes-like / uint8 array)."""
    bits = np.unpackbits(np.asarray(buf, dtype=np.uint8), bitorder="little")[: n * width]
    return (bits.reshape(n, width) << np.arange(width, dtype=np.uint8)).sum(axis=1).astype(np.int64)


def levels_of_rows(lengths, leaf_null=None, list_null=None, outer_optional=True, elem_optional=True):
    """(rep, dfn, leaf_level, max_def) of rows of ``lengths`` leaves; ``leaf_null``: bool per leaf,
    ``list_null``: bool per row (needs an optional outer group; its length must be 0)."""
    O, E = int(outer_optional), int(elem_optional)
    rep, dfn, k = [], [], 0
    for r, L in enumerate(lengths):
        if L == 0:
            rep.append(0)
            dfn.append(O - 1 if (list_null is not None and list_null[r]) else O)
            continue
        for i in range(L):
            rep.append(0 if i == 0 else 1)
            dfn.append(O + 1 + E - int(leaf_null is not None and bool(leaf_null[k])))
            k += 1
    return np.asarray(rep, dtype=np.int64), np.asarray(dfn, dtype=np.int64), O + 1, O + 1 + E
