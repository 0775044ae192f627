"""Numpy restatement of how a list column becomes parquet level streams ("List columns
in the PLAIN parquet writer"): the reference of tests/test_parquet_list_host.py and
tests/test_gpu_parquet_list.py.

A row of L leaves occupies max(L, 1) slots.  Empty row: one slot (rep 0, def 1).  Leaf i of a row:
rep 0 if it is the row's first leaf, else 1; def 3 if the leaf is valid, else 2.  With S the
exclusive prefix sum of the slots per row, page p starts at the first row r with
S[r] >= p * page_slots; a page that gets no row is dropped.  Both streams of a page are one
bit-packed run: LSB first at bit width 1 (rep) and 2 (def), ceil(slots / 8) groups, pad bits 0."""
import numpy as np


def slot_starts(offsets, r0, r1):
    """S[0 .. n] of the rows [r0, r1)."""
    lens = np.diff(np.asarray(offsets, dtype=np.int64)[r0:r1 + 1])
    S = np.zeros(r1 - r0 + 1, dtype=np.int64)
    np.cumsum(np.maximum(lens, 1), out=S[1:])
    return S


def page_rows(S, page_slots):
    """[(first row, one past the last row)] of the pages, rows counted from r0."""
    n, total = len(S) - 1, int(S[-1])
    pnom = -(-total // page_slots)
    starts = [int(np.searchsorted(S[:n], p * page_slots, side="left")) for p in range(pnom)] + [n]
    return [(a, b) for a, b in zip(starts[:-1], starts[1:]) if b > a]


def _pack(levels, width):
    levels = np.asarray(levels, dtype=np.uint8)
    bits = ((levels[:, None] >> np.arange(width, dtype=np.uint8)) & 1).reshape(-1)
    out = np.packbits(bits, bitorder="little")
    groups = -(-len(levels) // 8)
    return np.concatenate([out, np.zeros(groups * width - len(out), dtype=np.uint8)]).tobytes()


def list_pages(offsets, leaf_valid, r0, r1, page_slots):
    """The pages of rows [r0, r1): a list of dicts {row0, rows, slot0, slots, leaves, nonnull, rep,
    dfn} (rep / dfn: the packed level bytes).  ``leaf_valid``: None, or bool per leaf of the column
    (leaf_valid[0] is the leaf that offsets[0] names)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    S = slot_starts(offsets, r0, r1)
    pages = []
    for a, b in page_rows(S, page_slots):
        off = offsets[r0 + a: r0 + b + 1]
        rep, dfn = [], []
        for r in range(b - a):
            L = int(off[r + 1] - off[r])
            if L < 1:
                rep.append(0)
                dfn.append(1)
                continue
            for i in range(L):
                leaf = int(off[r]) + i - int(offsets[0])
                rep.append(0 if i == 0 else 1)
                dfn.append(3 if (leaf_valid is None or leaf_valid[leaf]) else 2)
        assert len(rep) == int(S[b] - S[a])
        pages.append(dict(row0=a, rows=b - a, slot0=int(S[a]), slots=len(rep), leaves=int(off[-1] - off[0]),
                          nonnull=int(sum(d == 3 for d in dfn)), rep=_pack(rep, 1), dfn=_pack(dfn, 2)))
    return pages
