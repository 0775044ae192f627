"""numpy restatement of nvt_pq_expand_runs (include/nvt_hip.h, "parquet in: string columns").

A run table is a uint32 array of shape (nruns + 1, 4): records {start, kind | width << 8, a, b} in
value order and the closing record {total, END, 0, 0}.  ``expand`` returns the entry id of every
value and the number of bad ones, by the rules the kernel states:

* repeat:   id = a
* sequence: id = a + k                       (k = position of the value in its run)
* packed:   id = a + (the width-bit number at bit k * width of the bytes from packed[4 * b] on,
            LSB first); the value is read as two aligned 32-bit words, and one whose second word
            would lie outside ``packed`` is bad
* anything else (another kind, width 0 or above 32), and an id outside [0, entries): -1, counted.
"""
import numpy as np

REPEAT, PACKED, SEQUENCE, END = 0, 1, 2, 3


def expand(runs, packed, entries):
    runs = np.asarray(runs, dtype=np.uint32).reshape(-1, 4)
    packed = np.asarray(packed, dtype=np.uint8)
    words = packed[: len(packed) // 4 * 4].view("<u4").astype(np.uint64)
    total = int(runs[-1, 0])
    ids = np.full(total, -1, dtype=np.int64)
    for r in range(len(runs) - 1):
        start, word1, a, b = (int(x) for x in runs[r])
        n = int(runs[r + 1, 0]) - start
        kind, width = word1 & 0xFF, (word1 >> 8) & 0xFF
        k = np.arange(n, dtype=np.uint64)
        if kind == REPEAT:
            ids[start:start + n] = a
        elif kind == SEQUENCE:
            ids[start:start + n] = a + k.astype(np.int64)
        elif kind == PACKED and 1 <= width <= 32:
            bit = k * np.uint64(width)
            w = np.uint64(b) + (bit >> np.uint64(5))
            ok = w + np.uint64(1) < np.uint64(len(words))
            wi = np.where(ok, w, 0).astype(np.int64)
            both = words[wi] | (words[np.minimum(wi + 1, len(words) - 1)] << np.uint64(32))
            v = (both >> (bit & np.uint64(31))) & np.uint64((1 << width) - 1)
            ids[start:start + n] = np.where(ok, a + v.astype(np.int64), -1)
    bad = (ids < 0) | (ids >= entries)
    ids[bad] = -1
    return ids.astype(np.int32), int(bad.sum())


def pack_values(values, width):
    """``values`` at ``width`` bits each, LSB first, padded to whole groups of 8 values (what a
    parquet bit-packed run holds) -> uint8 array."""
    values = np.asarray(values, dtype=np.uint64)
    n = -(-len(values) // 8) * 8
    v = np.zeros(n, dtype=np.uint64)
    v[: len(values)] = values
    bits = ((v[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little")


class TableBuilder:
    """Builds a run table and its packed bytes run by run (each packed run on a 4-byte boundary,
    8 zero bytes behind the last, as the host decoder stages them)."""

    def __init__(self):
        self.records, self.packed, self.at = [], bytearray(), 0

    def repeat(self, entry, n):
        self.records.append((self.at, REPEAT, entry, 0))
        self.at += n

    def sequence(self, first, n):
        self.records.append((self.at, SEQUENCE, first, 0))
        self.at += n

    def packed_run(self, values, width, base=0, clip=None):
        """``clip``: the run keeps only its first ``clip`` values (the bytes hold all of them)."""
        self.packed += bytes(-len(self.packed) % 4)
        self.records.append((self.at, PACKED | (width << 8), base, len(self.packed) // 4))
        self.packed += pack_values(values, width).tobytes()
        self.at += len(values) if clip is None else clip

    def done(self):
        runs = np.array(self.records + [(self.at, END, 0, 0)], dtype=np.uint32).reshape(-1, 4)
        return runs, np.frombuffer(bytes(self.packed) + bytes(8), dtype=np.uint8).copy()


def random_table(rng, nvalues, entries, widths=(1, 2, 3, 7, 8, 9, 16, 17, 24, 31, 32), max_run=300):
    """A random mix of the three kinds over ``nvalues`` values; packed values are drawn below
    min(2^width, entries) so that every id is good.  -> (runs, packed)"""
    tb = TableBuilder()
    while tb.at < nvalues:
        n = int(min(nvalues - tb.at, rng.integers(1, max_run + 1)))
        kind = int(rng.integers(0, 3))
        if kind == REPEAT:
            tb.repeat(int(rng.integers(0, entries)), n)
        elif kind == SEQUENCE and n <= entries:
            tb.sequence(int(rng.integers(0, entries - n + 1)), n)
        else:
            width = int(rng.choice(widths))
            base = int(rng.integers(0, max(1, entries // 2)))
            hi = min(1 << width, entries - base)
            tb.packed_run(rng.integers(0, hi, n, dtype=np.uint64), width, base)
    return tb.done()
