"""Plain numpy statements of the device steps around the multi-GPU vocabulary exchange
(nvt_exchange.hip), as include/nvt_hip.h words them.  Nothing here imports the package:
test_exchange_reference.py pins owner and histogram to dist._range_owner and np.bincount on the CPU,
test_gpu_exchange_kernels.py compares the kernels with these functions bit for bit.

A column is (keys int32[], counts int64[]); a word is (count << 32 | key), the key in the low 32
bits as its two's complement pattern.  A count of 2^31 or more does not fit: its top bits fall off
the word and bit 31 comes back as the sign (``unpack_words`` states that too)."""
import numpy as np

INT64_MAX = (1 << 63) - 1
EMPTY = (-INT64_MAX, -INT64_MAX, 0)


def ranges(cols):
    """int64[ncol, 3] = (-min key, max key, sum of counts); a column without entries, or whose
    counts sum to 0: (-INT64_MAX, -INT64_MAX, 0)."""
    out = np.zeros((len(cols), 3), dtype=np.int64)
    for j, (k, c) in enumerate(cols):
        tot = sum(int(v) for v in c)
        out[j] = (-int(np.min(k)), int(np.max(k)), tot) if len(k) and tot > 0 else EMPTY
    return out


def owner(keys, lo, width, G):
    """min((key - lo) // width, G - 1) per key (key >= lo)."""
    return np.array([min((int(k) - int(lo)) // int(width), G - 1) for k in keys], dtype=np.int64)


def hist(cols, lo, width, G):
    """int64[G, ncol]: rows of column j owned by rank g."""
    mat = np.zeros((G, len(cols)), dtype=np.int64)
    for j, (k, _) in enumerate(cols):
        np.add.at(mat[:, j], owner(k, lo[j], width[j], G), 1)
    return mat


def pack_words(keys, counts):
    """int64[]: (count << 32 | key), modulo 2^64."""
    w = [((int(c) << 32) | (int(k) & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF for k, c in zip(keys, counts)]
    return np.array(w, dtype=np.uint64).view(np.int64)


def unpack_words(words):
    """(keys int32[], counts int64[]): the low half as a signed key, the high half as a signed
    count (an arithmetic shift)."""
    w = np.asarray(words, dtype=np.int64)
    return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32), w >> 32


def pack_ordered(cols, lo, width, G, first_row, start, total, fill):
    """The send buffer of KEY-SORTED columns: row r of column j, owned by g, lies at
    start[g, j] + (r - first_row[g, j]); positions nothing goes to keep ``fill``."""
    out = np.full(total, fill, dtype=np.int64)
    for j, (k, c) in enumerate(cols):
        own = owner(k, lo[j], width[j], G)
        words = pack_words(k, c)
        for r in range(len(k)):
            g = own[r]
            out[int(start[g, j]) + r - int(first_row[g, j])] = words[r]
    return out


def unpack(words, seg_off, dst_off, keys_out, counts_out, extra=None, extra_out=None):
    """Segment s = words[seg_off[s]: seg_off[s + 1]] goes to dst_off[s] ... of the outputs, which
    are written in place (what they held elsewhere stays)."""
    k, c = unpack_words(words)
    for s in range(len(seg_off) - 1):
        a, b, d = int(seg_off[s]), int(seg_off[s + 1]), int(dst_off[s])
        keys_out[d: d + b - a] = k[a:b]
        counts_out[d: d + b - a] = c[a:b]
        if extra is not None:
            extra_out[d: d + b - a] = extra[a:b]
