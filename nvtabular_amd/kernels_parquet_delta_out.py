"""DELTA_BINARY_PACKED pages on the device: the host driver of ``nvt_pq_delta_out_*`` (include/nvt_hip.h),
behind ``Dataset.to_parquet(column_encoding=...)`` (``parquet_write.write_plain``).

``encode`` enqueues the sizing launch, the scan and the pack for the non-null values of ONE flat column
chunk and returns a ``DeviceDelta``: the packed regions of every page and the page table {state, at,
len}, all still on the device.  Nothing is read back here: the chunk rule runs on the device (the pack
returns at once for a chunk that stays PLAIN), and the write driver brings the page tables of ALL
offered columns of a row group back in the one read-back it makes anyway
(``kernels_parquet_dict.read_back_states(..., extra=...)``); ``take_words`` then restates the rule on
the host with ``parquet_plain.delta_pays`` from the same numbers.  Part of the host driver of the C
ABI, with the facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on torch's current stream,
errors through ``_lib.check``, workspace from torch's allocator ("DELTA_BINARY_PACKED in the
PLAIN parquet writer")."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_parquet_list import _buffer
from .parquet_plain import delta_pays

STATE_WORDS = _lib.PQ_DELTA_OUT_STATE_WORDS


def out_capacity(n: int, itemsize: int, npages: int) -> int:
    """Bytes of the packed buffer: a chunk that pays takes fewer than the values do, plus the slack
    that starts every page's region at a 16-byte boundary -- not the worst case of the encoding."""
    return int(n) * int(itemsize) + 16 * int(npages)


class DeviceDelta:
    """The enqueued encode of one column chunk: ``packed`` (uint8, ``out_capacity`` bytes) and
    ``table`` (int64[4 + 2 * pages]: {total, pays, error, used}, at[pages], len[pages]) on the device.
    After ``take_words``: ``pays`` (the chunk rule's verdict), ``used`` (the bytes of ``packed`` in use)
    and the numpy arrays ``at`` / ``lengths`` / ``nv`` per page."""

    def __init__(self, packed, table, page_start, n, itemsize, raw, keep):
        self.packed, self.table, self.page_start, self.n, self.itemsize = packed, table, page_start, n, itemsize
        self.raw = raw       # (packed, table) with their guard bytes
        self._keep = keep    # what the enqueued kernels read
        self.pays = self.used = self.at = self.lengths = self.nv = self.starts = None

    def device_words(self):
        """What rides along in the row group's read-back."""
        return [self.table, self.page_start]

    def take_words(self, arrays):
        """The front of ``arrays`` (what the read-back made of ``device_words``) becomes the host's
        page table; the host's verdict must be the device's."""
        table, starts = arrays[:2]
        del arrays[:2]
        npages = int(starts.size) - 1
        total, pays, error, used = (int(x) for x in table[:STATE_WORDS])
        self.at = np.array(table[STATE_WORDS: STATE_WORDS + npages], dtype=np.int64)
        self.lengths = np.array(table[STATE_WORDS + npages: STATE_WORDS + 2 * npages], dtype=np.int64)
        self.starts, self.nv = np.array(starts, dtype=np.int64), np.diff(starts)
        if error:
            raise RuntimeError("nvt_pq_delta_out_size: the page table is negative, descending or passes the values")
        self.pays, self.used = delta_pays(self.lengths, self.nv, self.itemsize), used
        if self.pays != bool(pays) or total != int(self.lengths.sum()):
            raise RuntimeError(f"nvt_pq_delta_out: the device's chunk rule says {pays} for {total} bytes, the host's "
                               f"{self.pays} for {int(self.lengths.sum())}")
        self._keep = None   # (the kernels are done: the workspace goes back to the allocator)
        return self


def encode(values: torch.Tensor, page_start: torch.Tensor, guard: int = 0) -> DeviceDelta:
    """Enqueue ``nvt_pq_delta_out_size`` and ``nvt_pq_delta_out_pack`` for ``values`` (int32 / int64, on
    the device, contiguous: the NON-NULL values of a flat chunk in order) cut into pages at
    ``page_start`` (int64[npages + 1] on the device, in value positions).  ``guard``: bytes left
    untouched in front of and behind every output buffer (tests)."""
    assert values.dtype in (torch.int32, torch.int64) and values.is_contiguous() and values.dim() == 1
    assert page_start.dtype == torch.int64 and page_start.is_contiguous() and page_start.numel() >= 2
    _lib.require_gpu()
    lib = _lib.load()
    dev = values.device
    n, npages, size = int(values.numel()), int(page_start.numel()) - 1, values.element_size()
    out_cap = out_capacity(n, size, npages)
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        need = C.c_uint64()
        check(lib.nvt_pq_delta_out_ws_bytes(n, npages, C.byref(need)), "nvt_pq_delta_out_ws_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        packed_raw, packed = _buffer(out_cap, guard, dev)
        table_raw, table8 = _buffer((STATE_WORDS + 2 * npages) * 8, guard, dev)
        table = table8.view(torch.int64)
        code = K.dtype_code(values.dtype)
        K.stat_add("pqdelta_size")   # (the sizing launch and the scan behind it)
        check(lib.nvt_pq_delta_out_size(K.ptr(values), code, n, page_start.data_ptr(), npages, table.data_ptr(),
                                        ws.data_ptr(), ws.numel(), stream), "nvt_pq_delta_out_size")
        K.stat_add("pqdelta_pack")
        check(lib.nvt_pq_delta_out_pack(K.ptr(values), code, n, page_start.data_ptr(), npages, table.data_ptr(),
                                        packed.data_ptr(), out_cap, ws.data_ptr(), ws.numel(), stream),
              "nvt_pq_delta_out_pack")
    return DeviceDelta(packed, table, page_start, n, size, (packed_raw, table_raw), (ws, values))
