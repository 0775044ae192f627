"""String columns of the PLAIN parquet writer: the host driver of ``nvt_pq_str_entry_ids`` and
``nvt_pq_byte_array_*`` (include/nvt_hip.h, "parquet out: string columns"), behind
``Dataset.to_parquet`` (``parquet_write.write_plain``).

A string column is int64 surrogates on the device and a {surrogate -> str} dict on the host.  The
dict becomes an ``EntryTable`` once -- keys ascending and the entries in key order as Arrow string
buffers, built with numpy and pyarrow, no Python loop over the entries -- and ``StringTables`` keeps
the tables of one ``to_parquet`` call, keyed by the dict object.  ``entry_ids`` / ``plan`` / ``fill``
enqueue the three entries; nothing is read back here.  Part of the host driver of the C ABI, with the
facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on torch's current stream, errors
through ``_lib.check``, workspace from torch's allocator ("String columns in the PLAIN
parquet writer")."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_parquet_list import _buffer
from .parquet_plain import MAX_ENTRY_BYTES, string_page_rows


class EntryTable:
    """The entries of one {surrogate -> str} dict: ``keys`` int64[E] ascending, ``offsets``
    int64[E + 1], ``chars`` the UTF-8 bytes in key order padded with zeros to a 4-byte boundary (numpy
    arrays), ``longest`` the longest entry in bytes.  ``on(device)`` gives the same three as tensors
    there, copied once."""

    def __init__(self, keys, offsets, chars, longest):
        self.keys, self.offsets, self.chars, self.longest = keys, offsets, chars, int(longest)
        self.entries = int(keys.size)
        self.page_rows = string_page_rows(self.longest)
        self._dev = {}

    def on(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(torch.from_numpy(a).to(device) for a in (self.keys, self.offsets, self.chars))
        return t


def entry_table(strings) -> Optional[EntryTable]:
    """The EntryTable of a {surrogate -> str} dict; None when the PLAIN writer does not take the dict:
    a value that is not a ``str`` (bytes, the mixed objects of the host fall-back of strings.py) or an
    entry longer than 2^30 - 4 bytes."""
    import pyarrow as pa

    n = len(strings)
    keys = np.fromiter(strings.keys(), dtype=np.int64, count=n)
    if n == 0:
        return EntryTable(keys, np.zeros(1, dtype=np.int64), np.zeros(4, dtype=np.uint8), 0)
    vals = list(strings.values())
    # (pyarrow would take bytes for a string: the check is on the distinct TYPES, a handful)
    if not all(issubclass(t, str) for t in set(map(type, vals))):
        return None
    try:
        arr = pa.array(vals, pa.large_string())
    except (pa.ArrowInvalid, pa.ArrowTypeError, UnicodeError):   # (a lone surrogate: no UTF-8)
        return None
    if arr.null_count:
        return None
    order = np.argsort(keys, kind="stable")
    arr = arr.take(pa.array(order))
    bufs = arr.buffers()
    offsets = np.frombuffer(bufs[1], dtype=np.int64)[arr.offset: arr.offset + n + 1]
    longest = int(np.diff(offsets).max())
    if longest > MAX_ENTRY_BYTES:
        return None
    nchars = int(offsets[-1] - offsets[0])
    chars = np.zeros(max(4, (nchars + 3) & ~3), dtype=np.uint8)
    if nchars:
        chars[:nchars] = np.frombuffer(bufs[2], dtype=np.uint8)[int(offsets[0]): int(offsets[-1])]
    return EntryTable(np.ascontiguousarray(keys[order]), np.ascontiguousarray(offsets - offsets[0]), chars, longest)


class StringTables:
    """The entry tables of one ``to_parquet`` call, keyed by the dict object; a reference to every dict
    is held so that its ``id`` cannot be reused.  All row groups of a partition share a table."""

    def __init__(self):
        self._tables = {}

    def get(self, strings) -> Optional[EntryTable]:
        hit = self._tables.get(id(strings))
        if hit is None:
            hit = self._tables[id(strings)] = (strings, entry_table(strings))
        return hit[1]


def entry_ids(keys: torch.Tensor, surrogates: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
    """int32 position in ``keys`` (int64, ascending, on the device) of every one of the NON-NULL
    ``surrogates``; one that is no key gives 0 and adds 1 to ``bad`` (int64[1] on the device)."""
    assert keys.dtype == torch.int64 and surrogates.dtype == torch.int64 and bad.dtype == torch.int64
    assert keys.is_contiguous() and surrogates.is_contiguous() and surrogates.dim() == 1
    _lib.require_gpu()
    m = int(surrogates.numel())
    out = torch.empty(m, dtype=torch.int32, device=surrogates.device)
    with K.LAUNCH_LOCK:
        K.stat_add("pq_str_entry_ids")
        check(_lib.load().nvt_pq_str_entry_ids(K.ptr(keys), int(keys.numel()), K.ptr(surrogates), m, K.ptr(out),
                                               K.ptr(bad), K.stream_ptr()), "nvt_pq_str_entry_ids")
    return out


def plan(ids: torch.Tensor, offsets: torch.Tensor, page_start: Optional[torch.Tensor] = None, guard: int = 0):
    """-> (pos int64[m + 1], page_at int64[pages + 1] or None), both on the device: the 64-bit exclusive
    scan of 4 + len(entry ids[j]) and its values at ``page_start`` (int64[pages + 1] on the device).
    m = 0: zeros.  ``guard`` (tests): bytes left untouched around both outputs, whose raw buffers are
    returned as a third item."""
    assert ids.dtype == torch.int32 and ids.is_contiguous() and offsets.dtype == torch.int64 and offsets.is_contiguous()
    assert page_start is None or (page_start.dtype == torch.int64 and page_start.is_contiguous())
    _lib.require_gpu()
    lib = _lib.load()
    dev = ids.device
    m, pages = int(ids.numel()), (int(page_start.numel()) - 1 if page_start is not None else 0)
    pos_raw, pos8 = _buffer(8 * (m + 1), guard, dev)
    at_raw, at8 = _buffer(8 * (pages + 1), guard, dev)
    pos, page_at = pos8.view(torch.int64), at8.view(torch.int64)
    if m == 0:
        pos.zero_()
        page_at.zero_()
    else:
        with K.LAUNCH_LOCK:
            need = C.c_uint64()
            check(lib.nvt_pq_byte_array_ws_bytes(m, C.byref(need)), "nvt_pq_byte_array_ws_bytes")
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            K.stat_add("pq_byte_array_plan")
            check(lib.nvt_pq_byte_array_plan(K.ptr(ids), m, K.ptr(offsets), int(offsets.numel()) - 1, K.ptr(page_start),
                                             pages, K.ptr(pos), K.ptr(page_at), K.ptr(ws), ws.numel(), K.stream_ptr()),
                  "nvt_pq_byte_array_plan")
    page_at = page_at if page_start is not None else None
    return (pos, page_at, (pos_raw, at_raw)) if guard else (pos, page_at)


def fill(ids: torch.Tensor, offsets: torch.Tensor, chars: torch.Tensor, pos: torch.Tensor, out_bytes: int,
         guard: int = 0, room: Optional[int] = None):
    """-> uint8[out_bytes] on the device: every value's u32 length and bytes at ``pos[j]`` (parquet's
    PLAIN BYTE_ARRAY).  ``guard`` / ``room`` (tests): guard bytes around a buffer of ``room`` >=
    out_bytes bytes; the raw buffer is returned as a second item."""
    assert ids.dtype == torch.int32 and ids.is_contiguous() and pos.dtype == torch.int64 and pos.is_contiguous()
    assert chars.dtype == torch.uint8 and chars.is_contiguous() and offsets.is_contiguous()
    _lib.require_gpu()
    m = int(ids.numel())
    assert pos.numel() == m + 1
    raw, out = _buffer(max(int(out_bytes), int(room or 0)), guard, ids.device)
    with K.LAUNCH_LOCK:
        K.stat_add("pq_byte_array_fill")
        check(_lib.load().nvt_pq_byte_array_fill(K.ptr(ids), m, K.ptr(offsets), K.ptr(chars), int(offsets.numel()) - 1,
                                                 K.ptr(pos), K.ptr(out), int(out_bytes), K.stream_ptr()),
              "nvt_pq_byte_array_fill")
    return (out[:int(out_bytes)], raw) if guard else out[:int(out_bytes)]
