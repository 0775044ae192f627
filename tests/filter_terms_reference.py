"""Plain numpy statement of what ``Dataset(filters=...)`` keeps and of what nvt_compact_keep_terms
writes (include/nvt_hip.h), pinned to ``pyarrow.parquet.read_table(filters=...)`` on the CPU by
test_filter_terms_reference.py.  Nothing here imports the package.

A filter is a DNF: a list of conjunctions, each a list of ``(column, op, value)`` with ``op`` one of
``== != < <= > >= in "not in"``.  A column is ``(values, valid)``: a numpy array (ints, floats, bool,
datetime64, or objects holding str) and a bool array (False: null) or None.  A row is kept iff in
some conjunction every term holds; a null fails every term but ``not in``, which it passes; NaN fails
every comparison but ``!=`` and is in no set; -0.0 == 0.0.  Integers, bools and datetime counts are
compared in int64, floats in float64 (a float32 value is widened, the constant is not narrowed)."""
import numpy as np

TILE = 2048
TILE_WORDS = TILE // 64
OPS = ("==", "!=", "<", "<=", ">", ">=", "in", "not in")


def _domain(values, constant_of):
    """(the column's values, a function that maps a constant) in the domain they are compared in."""
    values = np.asarray(values)
    k = values.dtype.kind
    if k == "M":
        unit = np.datetime_data(values.dtype)[0]
        return values.view(np.int64), lambda c: int(np.datetime64(c, unit).astype(np.int64))
    if k in "iub":
        return values.astype(np.int64), lambda c: int(c)
    if k == "f":
        return values.astype(np.float64), lambda c: float(c)
    return values, lambda c: c     # objects: str, compared by equality


def term_mask(values, valid, op, constant):
    x, conv = _domain(values, constant)
    n = len(x)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    if op in ("in", "not in"):
        members = [conv(c) for c in constant]
        hit = np.zeros(n, dtype=bool)
        with np.errstate(invalid="ignore"):
            for m in members:
                hit |= np.asarray(x == m, dtype=bool)
        return np.where(ok, hit if op == "in" else ~hit, op == "not in")
    c = conv(constant)
    with np.errstate(invalid="ignore"):
        if op == "==":
            r = x == c
        elif op == "!=":
            r = x != c
        elif op == "<":
            r = x < c
        elif op == "<=":
            r = x <= c
        elif op == ">":
            r = x > c
        elif op == ">=":
            r = x >= c
        else:
            raise ValueError(op)
    return np.asarray(r, dtype=bool) & ok


def keep_mask(dnf, cols, n):
    """dnf: [[(column, op, constant)]]; cols: {column: (values, valid or None)} -> bool[n]."""
    keep = np.zeros(n, dtype=bool)
    for conj in dnf:
        acc = np.ones(n, dtype=bool)
        for name, op, constant in conj:
            values, valid = cols[name]
            acc &= term_mask(values, valid, op, constant)
        keep |= acc
    return keep


def plan(keep):
    """keep bool[n] -> (mask words uint64[ntiles * 32] with the bits past n zero, kept rows per tile
    uint32[ntiles]): tiles of 2048 rows, bit i of word i / 64 = row i."""
    keep = np.asarray(keep, dtype=bool)
    nt = (len(keep) + TILE - 1) // TILE
    bits = np.zeros(nt * TILE, dtype=bool)
    bits[: len(keep)] = keep
    words = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)
    counts = bits.reshape(nt, TILE).sum(axis=1).astype(np.uint32)
    return words, counts
