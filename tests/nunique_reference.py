"""numpy reference of nvt_seg_nunique (include/nvt_hip.h): distinct non-null values per group over
rows ordered by group.  Shares no code with the device side: np.unique per group on the column's
own dtype, after dropping invalid and NaN entries.  test_nunique_reference.py pins it to pandas'
groupby(...).nunique()."""
import numpy as np


def pack_bits(ok):
    """bool[n] -> Arrow validity bitmap (LSB first), padded to a multiple of 8 bytes."""
    bits = np.packbits(np.asarray(ok, bool), bitorder="little")
    return np.concatenate([bits, np.zeros((-bits.size) % 8, np.uint8)])


def words_of(group, rows=None):
    """The words of rows that are ALREADY ordered by group: group << 32 | row."""
    group = np.asarray(group, np.uint64)
    rows = np.arange(group.size, dtype=np.uint64) if rows is None else np.asarray(rows, np.uint64)
    return (group << np.uint64(32)) | rows


def seg_nunique(words, ngroups, vals, val_valid):
    """int64[V, G].  words: uint64 (group << 32 | row), groups ascending, words of a group >=
    ngroups ignored.  vals[c]: host column indexed by row; val_valid[c]: bool[rows] or None."""
    words = np.asarray(words, np.uint64)
    group = (words >> np.uint64(32)).astype(np.int64)
    row = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (np.diff(group[group < ngroups]) >= 0).all(), "words are not ordered by group"
    out = np.zeros((len(vals), ngroups), np.int64)
    live = group < ngroups
    group, row = group[live], row[live]
    cuts = np.flatnonzero(np.diff(group)) + 1
    starts = np.concatenate([[0], cuts]) if group.size else np.zeros(0, np.int64)
    ends = np.concatenate([cuts, [group.size]]) if group.size else np.zeros(0, np.int64)
    for c, (v, ok) in enumerate(zip(vals, val_valid)):
        v = np.asarray(v)
        x = v[row]
        keep = np.ones(row.size, bool) if ok is None else np.asarray(ok, bool)[row]
        if v.dtype.kind == "f":
            keep &= ~np.isnan(x)
        for a, b in zip(starts, ends):
            out[c, group[a]] = np.unique(x[a:b][keep[a:b]]).size
    return out
