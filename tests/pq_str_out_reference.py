"""numpy restatement of the string half of the PLAIN parquet writer: the entry table of a
{surrogate -> str} dict, nvt_pq_str_entry_ids, nvt_pq_byte_array_plan and nvt_pq_byte_array_fill
(include/nvt_hip.h, "parquet out: string columns").  Plain Python, no GPU; test_pq_str_out_reference.py
checks it against pyarrow, the GPU tests check the kernels against it byte for byte."""
import struct

import numpy as np


def entry_table(strings):
    """{surrogate -> str} -> (keys int64[E] ascending, offsets int64[E + 1], chars uint8 padded with
    zeros to a 4-byte boundary (at least 4 bytes), the longest entry in bytes)."""
    keys = sorted(strings)
    raw = [strings[k].encode("utf-8") for k in keys]
    offsets = np.zeros(len(keys) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(b) for b in raw])
    blob = b"".join(raw)
    chars = np.zeros(max(4, (len(blob) + 3) & ~3), dtype=np.uint8)
    chars[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return np.array(keys, dtype=np.int64), offsets, chars, max([len(b) for b in raw], default=0)


def entry_ids(keys, surrogates):
    """-> (int32 position of every surrogate in the ascending keys -- 0 for one that is no key --, the
    number of those)."""
    keys, surrogates = np.asarray(keys, dtype=np.int64), np.asarray(surrogates, dtype=np.int64)
    at = np.searchsorted(keys, surrogates, side="left")
    found = (at < keys.size) & (keys[np.minimum(at, max(keys.size - 1, 0))] == surrogates) if keys.size else \
        np.zeros(surrogates.size, dtype=bool)
    return np.where(found, at, 0).astype(np.int32), int((~found).sum())


def plan(ids, offsets, page_start):
    """-> (pos int64[m + 1]: exclusive scan of 4 + len(entry ids[j]), pos[m] the total;
    page_at[p] = pos[page_start[p]])."""
    ids, offsets = np.asarray(ids, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    sizes = 4 + (offsets[ids + 1] - offsets[ids])
    pos = np.zeros(ids.size + 1, dtype=np.int64)
    pos[1:] = np.cumsum(sizes)
    return pos, pos[np.asarray(page_start, dtype=np.int64)]


def fill(ids, offsets, chars, pos, out, out_bytes=None):
    """Writes every value's u32 length (little endian) and bytes at out[pos[j]:]; a value that would
    end past ``out_bytes`` (default: all of ``out``) is not written.  -> out."""
    out_bytes = out.size if out_bytes is None else out_bytes
    for j, e in enumerate(np.asarray(ids).tolist()):
        a, b = int(pos[j]), int(pos[j + 1])
        if b > out_bytes:
            continue
        out[a: a + 4] = np.frombuffer(struct.pack("<I", b - a - 4), dtype=np.uint8)
        out[a + 4: b] = chars[int(offsets[e]): int(offsets[e + 1])]
    return out


def page_start_of(valid, rows, page_rows):
    """Positions in the non-null values at which the pages of ``page_rows`` rows start
    (``valid``: bool per row or None)."""
    valid = np.ones(rows, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    cuts = list(range(0, rows, page_rows)) + [rows] if rows else [0, 0]
    before = np.concatenate([[0], np.cumsum(valid)])
    return before[cuts].astype(np.int64)


def byte_array_pages(values, page_rows):
    """A column chunk given as a list of str / None -> (body uint8, page_at, nv per page, the validity
    bitmap as uint8 LSB first or None): what ``parquet_plain.ByteArrayPages`` takes, made the way the
    device makes it -- surrogates 0 .. E-1 over the distinct strings, entry ids, plan, fill."""
    valid = np.array([v is not None for v in values], dtype=bool)
    distinct = sorted({v for v in values if v is not None})
    strings = dict(enumerate(distinct))
    key_of = {v: k for k, v in strings.items()}
    keys, offsets, chars, _ = entry_table(strings)
    ids, bad = entry_ids(keys, [key_of[v] for v in values if v is not None])
    assert bad == 0
    ps = page_start_of(valid, len(values), page_rows)
    pos, page_at = plan(ids, offsets, ps)
    body = fill(ids, offsets, chars, pos, np.zeros(int(pos[-1]), dtype=np.uint8))
    bitmap = None if valid.all() else np.packbits(valid, bitorder="little")
    return body, page_at, np.diff(ps), bitmap
