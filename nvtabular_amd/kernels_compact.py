"""Row compaction on the device: the host driver of ``nvt_compact_*`` (include/nvt_hip.h), behind
``ops.Filter``, ``ops.Dropna`` and ``Dataset(filters=...)``.

A keep mask (from a bool tensor, from the null test of Dropna, or from the terms of a Dataset filter) and its plan -- the exclusive
scan of the kept rows per 2048-row tile -- drive ONE ``nvt_compact_many`` launch that moves the
kept rows of every column: values, validity bitmaps (bit-exact, bits past m zero), string
surrogates, and the leaves of list columns, whose leaf keep mask is the row mask expanded over
their leaf ranges.  A pending FillMissing constant is carried over, not materialised; the
{surrogate -> str} dictionary of a string column is carried over unchanged.  Part of the host
driver of the C ABI, with the facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on
torch's current stream, errors through ``_lib.check``, workspace from torch's allocator."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional

import torch

from . import _lib
from . import kernels as K
from ._lib import check

_WIDTHS = {torch.bool: 1, torch.uint8: 1, torch.int8: 1, torch.int32: 4, torch.float32: 4, torch.int64: 8, torch.float64: 8}


def _plan_ws(n: int, device) -> torch.Tensor:
    """Workspace of a plan over n rows (mask words, tile counts, scan scratch), 256-byte aligned."""
    need = C.c_uint64()
    check(_lib.load().nvt_compact_ws_bytes(n, C.byref(need)), "nvt_compact_ws_bytes")
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device=device)
    off = (-ws.data_ptr()) % 256
    return ws[off: off + need.value]


def _bitmap_bytes(m: int) -> int:
    return (m + 63) // 64 * 8   # padded to 8 bytes, as pack_bitmap / pack_bitmap_device pad


def compact_frame(frame, keep: torch.Tensor):
    """The rows of ``frame`` where ``keep`` (bool / uint8 device tensor of length n) is set, in
    order, renumbered from 0.  Reads the kept row count back once to size the outputs: that is
    the one host synchronisation of the call."""
    from .device import DeviceFrame

    n = len(frame)
    if not isinstance(keep, torch.Tensor) or keep.dim() != 1 or keep.dtype not in (torch.bool, torch.uint8):
        raise TypeError("keep must be a 1-D bool / uint8 tensor")
    if keep.numel() != n:
        raise ValueError(f"keep mask of length {keep.numel()} for a frame of {n} rows")
    if n == 0:
        return frame.copy()
    _lib.require_gpu()
    keep = keep.contiguous()
    if not keep.is_cuda:
        keep = keep.to(_device_of(frame))
    with K.LAUNCH_LOCK:
        ws = _plan_ws(n, keep.device)
        K.stat_add("compact_keep")
        check(_lib.load().nvt_compact_keep_mask(keep.data_ptr(), n, ws.data_ptr(), ws.numel(), K.stream_ptr()),
              "nvt_compact_keep_mask")
        return _compact(frame, ws, n)


def dropna_frame(frame, subset: Optional[Iterable[str]] = None):
    """``df.dropna(subset=subset)`` with the index renumbered: a row is dropped when one of the
    tested columns is null there (validity bit 0, or NaN in a float column).  A column with a
    pending FillMissing constant has no nulls, and a list row is never NA (device list columns
    have no row validity; pandas does not treat a list that holds nulls as NA)."""
    names = list(subset) if subset else frame.columns
    n = len(frame)
    tested = []
    for name in names:
        col = frame[name]
        if col.is_list or col.fill is not None:
            continue
        if col.valid is None and col.dtype not in (torch.float32, torch.float64):
            continue
        tested.append(col)
    if n == 0 or not tested:
        return frame.copy()   # no row can be NA
    _lib.require_gpu()
    descs = (_lib.DropnaCol * len(tested))()
    keep_alive = []
    for d, col in zip(descs, tested):
        data = col.data.contiguous()
        keep_alive.append(data)
        d.x = data.data_ptr()
        d.valid = K.ptr(col.valid)
        d.dtype = K.dtype_code(data.dtype)
    with K.LAUNCH_LOCK:
        ws = _plan_ws(n, tested[0].data.device)
        K.stat_add("compact_keep")
        check(_lib.load().nvt_compact_keep_dropna(descs, len(tested), n, ws.data_ptr(), ws.numel(),
                                                  K.stream_ptr()), "nvt_compact_keep_dropna")
        return _compact(frame, ws, n)


_FILTER_CODE = {torch.float32: _lib.NVT_F32, torch.float64: _lib.NVT_F64, torch.int32: _lib.NVT_I32,
                torch.int64: _lib.NVT_I64, torch.uint8: _lib.NVT_U8, torch.bool: _lib.NVT_U8,
                torch.int8: _lib.NVT_I8, torch.int16: _lib.NVT_I16}


def filter_frame(frame, flt):
    """The rows of ``frame`` that pass ``flt`` (a ``filters.Filter``, or the ``filters.Lowered`` of
    one), in order, renumbered from 0.  ONE ``nvt_compact_keep_terms`` launch reads the columns the
    filter names at their own width (bool / int8 / int16 included: no temporary per term) and writes
    the plan's mask; the compaction follows as in ``compact_frame``, with its one read-back.  A
    column with a pending FillMissing constant is materialised first, in the result too."""
    from .filters import Lowered

    n = len(frame)
    names = flt.columns
    missing = [c for c in names if c not in frame]
    if missing:
        raise ValueError(f"filters: the frame has no columns {missing}")
    cols, copied = [], False
    for name in names:
        col = frame[name]
        if col.is_list:
            raise TypeError(f"filters: column {name!r} is a list column")
        if col.fill is not None:
            if not copied:   # (the caller's frame keeps its pending constant)
                frame, copied = frame.copy(), True
            col = frame[name] = col.materialize()
        if col.data.dtype not in _FILTER_CODE:
            raise TypeError(f"filters: unsupported column dtype {col.data.dtype} of {name!r}")
        cols.append(col)
    low = flt if isinstance(flt, Lowered) else \
        flt.lower({name: col.data.dtype in (torch.float32, torch.float64) for name, col in zip(names, cols)})
    if n == 0:
        return frame.copy()
    _lib.require_gpu()
    dev = cols[0].data.device
    descs = (_lib.FilterCol * len(cols))()
    keep_alive = []
    for d, col in zip(descs, cols):
        data = col.data.contiguous()
        keep_alive.append(data)
        d.x = data.data_ptr()
        d.valid = K.ptr(col.valid)
        d.dtype = _FILTER_CODE[data.dtype]
    terms = (_lib.FilterTerm * len(low.terms))()
    for d, (j, op, conj, set_len, set_off, value) in zip(terms, low.terms):
        d.col, d.op, d.conj, d.set_len, d.set_off = j, op, conj, set_len, set_off
        if low.floats[j]:
            d.value.f = value
        else:
            d.value.i = value
    with K.LAUNCH_LOCK:
        sets = low._device_sets.get(dev)
        if sets is None and low.sets.size:
            sets = low._device_sets[dev] = torch.from_numpy(low.sets.view("int64").copy()).to(dev)
        ws = _plan_ws(n, dev)
        K.stat_add("compact_keep")
        check(_lib.load().nvt_compact_keep_terms(descs, len(cols), terms, len(low.terms), K.ptr(sets),
                                                 int(low.sets.size), n, ws.data_ptr(), ws.numel(), K.stream_ptr()),
              "nvt_compact_keep_terms")
        return _compact(frame, ws, n)


def _device_of(frame):
    for _, col in frame.items():
        return col.data.device
    from .device import default_device

    return default_device()


def _compact(frame, ws: torch.Tensor, n: int):
    from .device import DeviceColumn, DeviceFrame

    lib = _lib.load()
    stream = K.stream_ptr()
    cols = list(frame.items())
    lists = [(name, col) for name, col in cols if col.is_list]
    dev = ws.device
    counts = torch.empty(1 + len(lists), dtype=torch.int64, device=dev)
    check(lib.nvt_compact_plan(n, ws.data_ptr(), ws.numel(), counts.data_ptr(), stream), "nvt_compact_plan")
    leaf_ws = {}
    for i, (name, col) in enumerate(lists):
        offsets = col.offsets.contiguous()
        nl = int(col.data.numel())
        if nl == 0:
            counts[1 + i].zero_()
            continue
        lws = _plan_ws(nl, dev)
        check(lib.nvt_compact_list_keep(offsets.data_ptr(), n, ws.data_ptr(), nl, lws.data_ptr(), lws.numel(),
                                        stream), "nvt_compact_list_keep")
        check(lib.nvt_compact_plan(nl, lws.data_ptr(), lws.numel(), counts[1 + i:].data_ptr(), stream),
              "nvt_compact_plan")
        leaf_ws[name] = (lws, offsets, nl)
    sizes = counts.cpu().tolist()   # the call's one host synchronisation: m (and the kept leaves)
    m = sizes[0]
    leaf_m = {name: sizes[1 + i] for i, (name, _) in enumerate(lists)}

    out = DeviceFrame()
    jobs: List = []
    for name, col in cols:
        if col.is_list:
            if name in leaf_ws:
                lws, src_n = leaf_ws[name][0], leaf_ws[name][2]
            else:
                lws, src_n = None, 0
            mm = leaf_m[name]
        else:
            lws, src_n, mm = ws, n, m
        data = col.data.contiguous()
        if data.dtype not in _WIDTHS:
            raise TypeError(f"unsupported column dtype {data.dtype}")
        dst = torch.empty(mm, dtype=data.dtype, device=dev)
        dst_valid = None
        if col.valid is not None:
            dst_valid = torch.empty(_bitmap_bytes(mm), dtype=torch.uint8, device=dev)
        if mm > 0:
            jobs.append((data, dst, col.valid, dst_valid, lws, src_n))
        out[name] = DeviceColumn(dst, dst_valid, None, col.fill, col.strings, logical=col.logical)
    if jobs:
        descs = (_lib.CompactCol * len(jobs))()
        for d, (data, dst, valid, dst_valid, lws, src_n) in zip(descs, jobs):
            d.src = data.data_ptr()
            d.dst = dst.data_ptr()
            d.src_valid = K.ptr(valid)
            d.dst_valid = K.ptr(dst_valid)
            d.plan = lws.data_ptr()
            d.n = src_n
            d.width = _WIDTHS[data.dtype]
        K.stat_add("compact_many")
        check(lib.nvt_compact_many(descs, len(jobs), stream), "nvt_compact_many")
    for name, col in lists:
        new_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
        if name in leaf_ws:
            lws, offsets, nl = leaf_ws[name]
            leaf_ptr = lws.data_ptr()
        else:
            offsets, nl, leaf_ptr = col.offsets.contiguous(), 0, None
        check(lib.nvt_compact_list_offsets(offsets.data_ptr(), n, ws.data_ptr(), leaf_ptr, nl, new_off.data_ptr(),
                                           stream), "nvt_compact_list_offsets")
        out[name].offsets = new_off
    return out
