"""Parquet level streams of list columns on the device: the host driver of ``nvt_pqlist_*``
(include/nvt_hip.h), behind ``Dataset.to_parquet`` (``parquet_write.write_plain``).

For one row range of a partition, the list columns whose ``offsets`` are the same tensor (what
``ops.Groupby`` hands over and ``ops.ListSlice`` keeps) are planned ONCE: one slot prefix sum, one
page table, one repetition stream.  A definition stream is written per leaf bitmap; the columns
without one share a single stream.  ``pack_levels`` only enqueues; ``DeviceLevels.read_back`` is
the group's one host synchronisation and brings the page table, the stream sizes and the non-null
counts of every stream back together -- the writer lays the pages out from them while the level
bytes and the values are still being copied.  Part of the host driver of the C ABI, with the
facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on torch's current stream, errors
through ``_lib.check``, workspace from torch's allocator.

``unpack_levels`` is the opposite direction, behind the parquet reader: level streams staged by the
host decoder -> offsets and leaf bitmap ("List columns in the parquet reader")."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

HDR, PG = _lib.PQLIST_HEADER_WORDS, _lib.PQLIST_PAGE_WORDS


def _buffer(nbytes, guard, dev):
    """(raw, view) of an output buffer of nbytes on ``dev``; ``guard`` bytes of 0xA5 in front of and
    behind the view (tests check that they stay)."""
    assert guard % 16 == 0
    raw = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev) if guard else \
        torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return raw, raw[guard: guard + nbytes]


class LevelTable:
    """What one read-back brings to the host: per page ``slots`` / ``rows`` / ``leaves`` and the
    byte offsets ``rep_at`` / ``def_at`` of its levels in the packed buffers, ``rep_bytes`` /
    ``def_bytes`` (the parts of the buffers that are in use), ``nonnull[s][p]`` per definition
    stream, and ``leaf_lo`` / ``leaf_hi``: the leaves of the rows are ``data[leaf_lo:leaf_hi]``."""

    def __init__(self, words: np.ndarray, nstreams: int, max_pages: int):
        w = words.view(np.uint64)
        if int(w[7]) != 0:
            raise _lib.NvtHipError(f"nvt_pqlist_plan: {int(w[0])} pages / {int(w[2])} + {int(w[3])} level bytes do "
                                   f"not fit the buffers sized from the column (offsets outside the leaves?)")
        self.npages = int(w[0])
        self.total_slots, self.rep_bytes, self.def_bytes = int(w[1]), int(w[2]), int(w[3])
        self.leaf_lo, self.leaf_hi = int(w[5]), int(w[6])
        pages = w[HDR: HDR + self.npages * PG].reshape(self.npages, PG).astype(np.int64)
        self.row0, self.rows, self.slot0, self.slots = pages[:, 0], pages[:, 1], pages[:, 2], pages[:, 3]
        self.rep_at, self.def_at, self.leaves = pages[:, 4], pages[:, 5], pages[:, 7]
        base = HDR + max_pages * PG
        self.nonnull = [w[base + s * max_pages: base + s * max_pages + self.npages].astype(np.int64)
                        for s in range(nstreams)]


class DeviceLevels:
    """The enqueued plan and pack of one (row range, offsets tensor): ``rep`` and ``defs[s]`` are
    the packed level buffers on the device, ``stream_of[j]`` the definition stream of the j-th
    column handed to ``pack_levels``."""

    def __init__(self, meta, rep, defs, stream_of, max_pages, raw, keep):
        self.meta, self.rep, self.defs, self.stream_of, self.max_pages = meta, rep, defs, stream_of, max_pages
        self.raw = raw       # (meta, rep, [defs]) with their guard bytes
        self._keep = keep    # what the enqueued kernels read

    def read_back(self) -> LevelTable:
        K.stat_add("pqlist_readback")
        return LevelTable(K.read_back(self.meta), len(self.defs), self.max_pages)


def pack_levels(offsets: torch.Tensor, r0: int, r1: int, bitmaps: Sequence[Optional[torch.Tensor]],
                n_leaves: int, page_slots: int, guard: int = 0) -> DeviceLevels:
    """Enqueue plan and pack of rows [r0, r1) of the list columns that share ``offsets`` (int64,
    n + 1 entries, on the device).  ``bitmaps[j]``: the leaf bitmap of column j or None; leaf
    ``offsets[0]`` is bit 0.  ``n_leaves``: the leaves the columns hold (an upper bound on what the
    row range names: it sizes the buffers).  ``guard``: bytes left untouched in front of and behind
    every output buffer (tests)."""
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and 0 <= r0 < r1 < offsets.numel()
    _lib.require_gpu()
    lib = _lib.load()
    dev = offsets.device
    n = r1 - r0
    max_slots = int(n_leaves) + n
    max_pages = -(-max_slots // int(page_slots)) + 1
    rep_cap = (max_slots + 7) // 8 + 8 * max_pages          # (a page's region is padded to 8 / 16 bytes)
    def_cap = 2 * ((max_slots + 7) // 8) + 16 * max_pages
    streams: List[Optional[torch.Tensor]] = []              # distinct definition streams
    keys: Dict = {}
    stream_of = []
    for bm in bitmaps:
        key = None if bm is None else (bm.data_ptr(), bm.numel())
        if key not in keys:
            keys[key] = len(streams)
            streams.append(bm)
        stream_of.append(keys[key])

    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        need = C.c_uint64()
        check(lib.nvt_pqlist_ws_bytes(n, C.byref(need)), "nvt_pqlist_ws_bytes")
        ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
        slot_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
        words = HDR + max_pages * PG + len(streams) * max_pages
        meta_raw, meta8 = _buffer(words * 8, guard, dev)
        meta = meta8.view(torch.int64)
        rep_raw, rep = _buffer(rep_cap, guard, dev)
        defs_raw, defs = zip(*[_buffer(def_cap, guard, dev) for _ in streams])
        off_ptr = offsets.data_ptr() + 8 * r0
        K.stat_add("pqlist_plan")
        check(lib.nvt_pqlist_plan(off_ptr, offsets.data_ptr(), n, int(page_slots), max_pages, rep_cap, def_cap, slot_start.data_ptr(),
                                  meta.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream), "nvt_pqlist_plan")
        descs = (_lib.PqListCol * len(streams))()
        for s, (d, bm) in enumerate(zip(descs, streams)):
            d.leaf_valid = K.ptr(bm)
            d.bit0 = 0
            d.nbits = 0 if bm is None else min(int(bm.numel()) * 8, int(n_leaves))
            d.def_out = defs[s].data_ptr()
            d.nonnull = meta.data_ptr() + 8 * (HDR + max_pages * PG + s * max_pages)
        K.stat_add("pqlist_pack_many", -(-len(streams) // _lib.PQLIST_MAX_COLS))
        check(lib.nvt_pqlist_pack_many(descs, len(streams), off_ptr, offsets.data_ptr(), n, slot_start.data_ptr(),
                                       meta.data_ptr(), max_pages, max_slots, rep.data_ptr(), stream),
              "nvt_pqlist_pack_many")
    return DeviceLevels(meta, rep, list(defs), stream_of, max_pages, (meta_raw, rep_raw, list(defs_raw)),
                        (ws, slot_start, offsets, streams))


def unpack_levels(rep: torch.Tensor, dfn: torch.Tensor, width: int, n_slots: int, leaf_level: int, max_def: int,
                  rows: int, leaves: int, want_valid: bool, guard: int = 0):
    """The way back (the parquet reader, ``parquet_plain.StagedPartition.to_device``): enqueue
    ``nvt_pqlist_unpack`` on the staged level streams of one list column (uint8 on the device, 8-byte
    aligned: 1 and ``width`` bits per slot) -> (offsets int64[rows + 1], leaf validity bitmap of
    ceil(leaves / 64) words or None when ``want_valid`` is False).  ``rows`` and ``leaves`` are the
    host decoder's counts, so nothing is read back.  ``guard``: bytes left untouched in front of and
    behind both outputs (tests); the raw buffers are returned as a third element then."""
    _lib.require_gpu()
    lib = _lib.load()
    dev = rep.device
    assert rep.dtype == torch.uint8 and dfn.dtype == torch.uint8
    assert rep.numel() >= ((n_slots + 63) // 64) * 8 and dfn.numel() >= ((n_slots * width + 63) // 64) * 8

    with K.LAUNCH_LOCK:
        need = C.c_uint64()
        check(lib.nvt_pqlist_unpack_ws_bytes(n_slots, C.byref(need)), "nvt_pqlist_unpack_ws_bytes")
        ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
        off_raw, off8 = _buffer((rows + 1) * 8, guard, dev)
        offsets = off8.view(torch.int64)
        valid_raw = valid = None
        if want_valid:
            valid_raw, valid = _buffer(((leaves + 63) // 64) * 8, guard, dev)
        K.stat_add("pqlist_unpack")
        check(lib.nvt_pqlist_unpack(K.ptr(rep), K.ptr(dfn), width, n_slots, leaf_level, max_def, rows, leaves,
                                    offsets.data_ptr(), K.ptr(valid), ws.data_ptr(), ws.numel() * 8, K.stream_ptr()),
              "nvt_pqlist_unpack")
    return (offsets, valid, (off_raw, valid_raw)) if guard else (offsets, valid)
