"""Snappy pages on the device: the host driver of ``nvt_snappy_*`` (include/nvt_hip.h), behind
``Dataset.to_parquet(device_compression="snappy")`` (``parquet_write.write_plain``).

``compress`` enqueues plan, compress and gather for the values regions of ALL column chunks of a row
group -- three batched calls over one descriptor array -- and returns a ``DeviceSnappy``: per region
the dense element streams of its pages and an ``out`` record {compressed bytes of every page, total,
error, fragments}, still on the device.  ``read_back`` brings the records of all regions to the host
in one read-back.  Part of the host driver of the C ABI, with the facade's conventions: launches
under ``kernels.LAUNCH_LOCK`` on torch's current stream, errors through ``_lib.check``, workspace
from torch's allocator ("Snappy pages in the PLAIN parquet writer")."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_parquet_list import _buffer

FRAG, SLOT_BYTES, OUT_WORDS, FRAG_WORDS = _lib.SNAPPY_FRAG, _lib.SNAPPY_SLOT_BYTES, _lib.SNAPPY_OUT_WORDS, \
    _lib.SNAPPY_FRAG_WORDS


class Region(NamedTuple):
    """The values region of one column chunk: ``src`` (a contiguous device tensor; its bytes are the
    region, at any byte alignment when it is a uint8 view), ``page_start`` (int64[npages + 1] on the
    device, in units of ``unit`` bytes), ``elem`` (4 or 8: how far back the parse also looks) and
    ``dense_cap`` (bytes of the dense buffer; None: the region's size -- a region that does not
    shrink is not moved, and its total says so)."""
    src: torch.Tensor
    page_start: torch.Tensor
    unit: int
    elem: int
    dense_cap: Optional[int] = None


def max_frags(nbytes: int, npages: int) -> int:
    """The bound the host sizes the fragment table from: ceil(nbytes / FRAG) + npages."""
    return -(-int(nbytes) // FRAG) + int(npages)


class DeviceSnappy:
    """The enqueued compression of the regions of one call: ``dense[i]`` (uint8) and ``out[i]``
    (int64[npages + OUT_WORDS]) of region i; ``frag_table`` / ``frag_size`` / ``frag_pos`` / ``slots``
    are the batch's arrays (tests read them), ``frag_base[i]`` region i's first record."""

    def __init__(self, regions, dense, out, frag_table, frag_size, frag_pos, slots, slot_cap, frag_base, raw, keep):
        self.regions, self.dense, self.out = regions, dense, out
        self.frag_table, self.frag_size, self.frag_pos, self.slots = frag_table, frag_size, frag_pos, slots
        self.slot_cap, self.frag_base = slot_cap, frag_base
        self.raw = raw       # the buffers with their guard bytes
        self._keep = keep    # what the enqueued kernels read


class PageSizes(NamedTuple):
    """What the read-back brings for one region: the compressed bytes of every page (their element
    streams follow each other in ``dense``), their total, the error word and the fragments."""
    sizes: np.ndarray
    total: int
    error: int
    frags: int


def compress(regions: Sequence[Region], slot_cap: int = SLOT_BYTES, guard: int = 0) -> DeviceSnappy:
    """Enqueue ``nvt_snappy_plan_many``, ``nvt_snappy_compress_many`` and ``nvt_snappy_gather_many``
    for ``regions`` (at least one).  ``slot_cap``: bytes of a fragment's slot (tests pass a short
    one).  ``guard``: bytes left untouched in front of and behind every output buffer (tests)."""
    assert len(regions) >= 1
    _lib.require_gpu()
    lib = _lib.load()
    dev = regions[0].src.device
    descs = (_lib.SnappyCol * len(regions))()
    dense, dense_raw, out, out_raw, bases = [], [], [], [], []
    total = 0
    for r, d in zip(regions, descs):
        assert r.src.is_cuda and r.src.is_contiguous() and r.src.device == dev
        assert r.page_start.dtype == torch.int64 and r.page_start.is_contiguous() and r.page_start.numel() >= 2
        nbytes, npages = int(r.src.numel()) * r.src.element_size(), int(r.page_start.numel()) - 1
        cap = nbytes if r.dense_cap is None else int(r.dense_cap)
        raw, view = _buffer((cap + 15) & ~15, guard, dev)
        dense_raw.append(raw)
        dense.append(view)
        raw, view = _buffer((npages + OUT_WORDS) * 8, guard, dev)
        out_raw.append(raw)
        out.append(view.view(torch.int64))
        d.src, d.page_start, d.npages, d.nbytes = K.ptr(r.src) if nbytes else None, r.page_start.data_ptr(), npages, nbytes
        d.unit, d.elem = int(r.unit), int(r.elem)
        d.frag_base, d.max_frags = total, max_frags(nbytes, npages)
        d.dense, d.dense_cap, d.out = dense[-1].data_ptr(), cap, out[-1].data_ptr()
        bases.append(total)
        total += d.max_frags
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        need = C.c_uint64()
        check(lib.nvt_snappy_ws_bytes(total, C.byref(need)), "nvt_snappy_ws_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        table_raw, table = _buffer(total * FRAG_WORDS * 8, guard, dev)
        size_raw, size = _buffer((total + 1) * 8, guard, dev)
        pos_raw, pos = _buffer((total + 1) * 8, guard, dev)
        slots_raw, slots = _buffer(total * int(slot_cap), guard, dev)
        batch = _lib.SnappyBatch(table.data_ptr(), size.data_ptr(), pos.data_ptr(), slots.data_ptr(), total,
                                 int(slot_cap), ws.data_ptr(), ws.numel())
        launches = -(-len(regions) // _lib.SNAPPY_MAX_COLS)
        K.stat_add("snappy_plan", launches)
        check(lib.nvt_snappy_plan_many(descs, len(regions), C.byref(batch), stream), "nvt_snappy_plan_many")
        K.stat_add("snappy_compress", launches)
        check(lib.nvt_snappy_compress_many(descs, len(regions), C.byref(batch), stream), "nvt_snappy_compress_many")
        K.stat_add("snappy_gather", launches)
        check(lib.nvt_snappy_gather_many(descs, len(regions), C.byref(batch), stream), "nvt_snappy_gather_many")
    return DeviceSnappy(list(regions), dense, out, table.view(torch.int64).view(total, FRAG_WORDS),
                        size.view(torch.int64), pos.view(torch.int64), slots, int(slot_cap), bases,
                        (dense_raw, out_raw, table_raw, size_raw, pos_raw, slots_raw), (ws, list(regions)))


def read_back(ds: DeviceSnappy, release: bool = True, extra: Sequence[torch.Tensor] = None):
    """The ``out`` records of all regions of ``ds`` in ONE read-back.  ``release``: the slots and the
    fragment arrays go back to the allocator (the kernels are done); ``dense`` stays.  ``extra``:
    further int64 tensors on the device that ride along (page starts only the device has); the
    result is then (the list, [their numpy arrays])."""
    K.stat_add("snappy_readback")
    w = K.read_back(torch.cat(list(ds.out) + [t.reshape(-1) for t in (extra or ())])).view(np.int64)
    got, at = [], 0
    for o in ds.out:
        npages = o.numel() - OUT_WORDS
        tail = w[at + npages: at + npages + OUT_WORDS]
        got.append(PageSizes(np.array(w[at: at + npages], dtype=np.int64), int(tail[_lib.SNAPPY_OUT_TOTAL]),
                             int(tail[_lib.SNAPPY_OUT_ERROR]), int(tail[_lib.SNAPPY_OUT_FRAGS])))
        at += o.numel()
    ds._keep = None
    if release:
        ds.slots = ds.frag_table = ds.frag_size = ds.frag_pos = ds.raw = None
    if extra is None:
        return got
    more = []
    for t in extra:
        more.append(np.array(w[at: at + t.numel()], dtype=np.int64))
        at += t.numel()
    return got, more
