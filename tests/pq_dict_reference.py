"""numpy reference of the dictionary pages the PLAIN parquet writer makes ("Dictionary
pages in the PLAIN parquet writer"): what ``nvt_pq_dict_build`` / ``nvt_pq_dict_pack`` must produce
bit for bit, written from the layout and from numpy alone (``np.unique`` / ``np.searchsorted``),
never from the code under test.  tests/test_pq_dict_reference.py pins it to pyarrow."""
import numpy as np


def index_width(d: int) -> int:
    """W = max(1, bit_length(d - 1))."""
    return max(1, (int(d) - 1).bit_length())


def page_offsets(nv, W):
    """(byte offset of every page in the packed buffer, total bytes): page p starts at
    16 * sum_{q<p} ceil(W * ceil(nv_q / 8) / 16)."""
    at, pos = [], 0
    for x in nv:
        at.append(pos)
        pos += 16 * (-(-(W * (-(-int(x) // 8))) // 16))
    return at, pos


def pack_page(idx: np.ndarray, W: int) -> bytes:
    """ceil(len / 8) groups of 8 indices at W bits each, LSB first, pad bits 0."""
    groups = -(-len(idx) // 8)
    bits = np.zeros(groups * 8 * W, dtype=np.uint8)
    idx = np.asarray(idx, dtype=np.uint64)
    for b in range(W):
        bits[b: len(idx) * W: W] = (idx >> np.uint64(b)) & np.uint64(1)
    return np.packbits(bits, bitorder="little").tobytes()


def encode(values: np.ndarray, page_start):
    """values: the non-null values of a chunk; page_start[npages + 1]: value positions.
    -> (dictionary, W, nv per page, packed bytes with the pad bytes 0)."""
    values = np.asarray(values)
    dictionary = np.unique(values)                     # ascending signed order
    idx = np.searchsorted(dictionary, values)
    W = index_width(len(dictionary))
    nv = [int(b - a) for a, b in zip(page_start[:-1], page_start[1:])]
    at, total = page_offsets(nv, W)
    packed = bytearray(total)
    for p, (a, b) in enumerate(zip(page_start[:-1], page_start[1:])):
        raw = pack_page(idx[a:b], W)
        assert len(raw) == W * (-(-nv[p] // 8))
        packed[at[p]: at[p] + len(raw)] = raw
    return dictionary, W, nv, bytes(packed)


def flat_page_start(valid, n, page_rows):
    """Value positions of the pages of a flat column of n rows cut every page_rows rows
    (valid: bool per row or None)."""
    valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    ends = list(range(0, n, page_rows))[1:] + [n]
    cs = np.concatenate([[0], np.cumsum(valid)])
    return [0] + [int(cs[e]) for e in ends]
