"""Batch gather of a dataloader chunk: the host driver of ``nvt_batch_take_many`` and
``nvt_take_list_*`` (include/nvt_hip.h), behind ``loader.torch.TorchAsyncItr``.

``take_frame`` writes the rows ``index`` of every planned scalar column of a frame into the
destination the plan names -- a contiguous column or one column of a row-major matrix, cast to the
destination's dtype -- in ONE ``nvt_batch_take_many`` call; the columns of one matrix are kept
inside one launch so that the kernel can stage their rows in LDS.  ``take_lists`` gathers the list
columns that share an offsets tensor: new offsets, ONE read-back (the leaf total and any offsets
the caller asks for), then the leaves of all of them in one launch.  ``take_frames`` and
``take_lists_multi`` do the same over the concatenation of several frames -- a chunk of partitions
shuffled as a whole -- on ``nvt_batch_take_multi`` / ``nvt_take_list_*_multi``: the per-source
pointers travel in a table in device memory, filled by one small copy.  Part of the host driver of the
C ABI, with the facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on torch's current
stream, errors through ``_lib.check``, workspace from torch's allocator."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from . import kernels as K
from ._lib import check

DTYPE_CODE = {torch.float32: _lib.NVT_F32, torch.float64: _lib.NVT_F64, torch.int32: _lib.NVT_I32,
              torch.int64: _lib.NVT_I64, torch.uint8: _lib.NVT_U8, torch.bool: _lib.NVT_U8,
              torch.int8: _lib.NVT_I8, torch.int16: _lib.NVT_I16}
_FLOATS = (torch.float32, torch.float64)


def dtype_code(dt: torch.dtype) -> int:
    try:
        return DTYPE_CODE[dt]
    except KeyError:
        raise TypeError(f"unsupported column dtype {dt}") from None


def cast_allowed(src: torch.dtype, dst: torch.dtype) -> bool:
    """What the kernel converts: same type, int64 from an integer, float32 / float64 from anything."""
    return dtype_code(src) == dtype_code(dst) or dst in _FLOATS or (dst == torch.int64 and src not in _FLOATS)


def bitmap_bytes(m: int) -> int:
    return (m + 63) // 64 * 8


@dataclass
class Take:
    """One column of a ``take_frame`` plan: rows ``row`` .. ``row + m`` of ``dst`` (1-D, or column
    ``column`` of a 2-D row-major tensor) receive the gathered values in ``dst``'s dtype;
    ``dst_valid`` (uint8, ``bitmap_bytes(m)``) receives the gathered bitmap when given."""
    name: str
    dst: torch.Tensor
    column: Optional[int] = None
    row: int = 0
    dst_valid: Optional[torch.Tensor] = None


def _source(frame, name):
    col = frame[name]
    if col.strings is not None:
        raise TypeError(f"column '{name}' holds strings: Categorify it before it reaches the dataloader")
    if col.fill is not None:
        col = col.materialize()
    return col


def take_frame(frame, index: Optional[torch.Tensor], plan: Sequence[Take], m: Optional[int] = None):
    """Gather the rows ``index`` (int64 on the device; None = the first ``m`` rows in order) of every
    column of ``plan`` in one ``nvt_batch_take_many`` call."""
    if index is not None:
        assert index.dtype == torch.int64 and index.is_contiguous()
        m = int(index.numel())
    n_src = len(frame)
    m = n_src if m is None else m
    keep, descs = [], (_lib.TakeCol * max(len(plan), 1))()
    # the columns of one matrix side by side, and never across the 64 descriptors of a launch: the
    # entry launches once per 64 descriptors of a call, so a matrix that would straddle starts a call
    order = sorted(range(len(plan)), key=lambda i: (plan[i].dst.dim() < 2, plan[i].dst.data_ptr(),
                                                    plan[i].column or 0))
    cuts = [0]
    for pos, i in enumerate(order):
        t = plan[i]
        col = _source(frame, t.name)
        if col.is_list:
            raise TypeError(f"column '{t.name}' is a list column (take_lists gathers those)")
        if not cast_allowed(col.data.dtype, t.dst.dtype):
            raise TypeError(f"column '{t.name}': no conversion from {col.data.dtype} to {t.dst.dtype}")
        data = col.data.contiguous()
        keep.append(data)
        dst = t.dst if t.column is None else t.dst[:, t.column]
        if t.dst.dim() == 2 and not t.column and t.dst.shape[1] <= _lib.TAKE_MAX_COLS and \
                (pos - cuts[-1]) % _lib.TAKE_MAX_COLS + t.dst.shape[1] > _lib.TAKE_MAX_COLS:
            cuts.append(pos)
        d = descs[pos]
        d.src = data.data_ptr()
        d.src_valid = K.ptr(col.valid)
        d.dst = dst.data_ptr() + t.row * dst.stride(0) * dst.element_size()
        d.dst_valid = K.ptr(t.dst_valid)
        d.dst_stride = max(dst.stride(0), 1)
        d.src_dtype = dtype_code(data.dtype)
        d.dst_dtype = dtype_code(t.dst.dtype)
    if not plan or m == 0:
        return
    _lib.require_gpu()
    lib = _lib.load()
    cuts.append(len(order))
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        for start, stop in zip(cuts[:-1], cuts[1:]):
            K.stat_add("loader_take_many")
            sub = C.cast(C.byref(descs, start * C.sizeof(_lib.TakeCol)), C.POINTER(_lib.TakeCol))
            check(lib.nvt_batch_take_many(K.ptr(index), m, n_src, sub, stop - start, stream),
                  "nvt_batch_take_many")


def src_begin(lengths: Sequence[int]) -> List[int]:
    """First chunk row of every source and the chunk's row count behind them: ``nsrc + 1`` entries,
    an empty source repeats its neighbour's."""
    out = [0]
    for n in lengths:
        if n < 0:
            raise ValueError("a source cannot have a negative length")
        out.append(out[-1] + int(n))
    return out


def _upload(words: List[int], dev) -> torch.Tensor:
    """The chunk's source table on the device: ONE small stream-ordered copy."""
    return torch.tensor(words, dtype=torch.int64).to(dev, non_blocking=True)


def _check_sources(frames):
    if not frames:
        raise ValueError("a chunk needs at least one source")
    if len(frames) > _lib.TAKE_MAX_SOURCES:
        raise ValueError(f"{len(frames)} sources in one chunk: the gather kernels take at most "
                         f"{_lib.TAKE_MAX_SOURCES} (NVT_TAKE_MAX_SOURCES)")


def take_frames(frames, index: Optional[torch.Tensor], plan: Sequence[Take], m: Optional[int] = None):
    """``take_frame`` over the concatenation of ``frames``: ``index`` numbers the rows of all of them,
    one behind the other (None = the first ``m`` in order).  The frames may differ per column in
    dtype and in whether there is a bitmap.  One source is ``take_frame`` itself; several go through
    ``nvt_batch_take_multi`` with the source table -- ``src_begin``, then per column of the plan
    ``nsrc`` records {src, src_valid, src_dtype} -- built here and copied to the device once."""
    _check_sources(frames)
    if len(frames) == 1:
        return take_frame(frames[0], index, plan, m)
    if index is not None:
        assert index.dtype == torch.int64 and index.is_contiguous()
        m = int(index.numel())
    begin = src_begin([len(f) for f in frames])
    nsrc, total = len(frames), begin[-1]
    m = total if m is None else m
    if not plan or m == 0:
        return
    dev = plan[0].dst.device
    order = sorted(range(len(plan)), key=lambda i: (plan[i].dst.dim() < 2, plan[i].dst.data_ptr(),
                                                    plan[i].column or 0))
    keep, words, cuts = [], list(begin), [0]
    descs = (_lib.TakeCol * len(plan))()
    rec = _lib.TAKE_SRC_WORDS
    for pos, i in enumerate(order):
        t = plan[i]
        for f in frames:
            col = _source(f, t.name)
            if col.is_list:
                raise TypeError(f"column '{t.name}' is a list column (take_lists_multi gathers those)")
            if not cast_allowed(col.data.dtype, t.dst.dtype):
                raise TypeError(f"column '{t.name}': no conversion from {col.data.dtype} to {t.dst.dtype}")
            data = col.data.contiguous()
            keep.append(data)
            words += [data.data_ptr(), K.ptr(col.valid) or 0, dtype_code(data.dtype)]
        dst = t.dst if t.column is None else t.dst[:, t.column]
        if t.dst.dim() == 2 and not t.column and t.dst.shape[1] <= _lib.TAKE_MAX_COLS and \
                (pos - cuts[-1]) % _lib.TAKE_MAX_COLS + t.dst.shape[1] > _lib.TAKE_MAX_COLS:
            cuts.append(pos)
        d = descs[pos]
        d.dst = dst.data_ptr() + t.row * dst.stride(0) * dst.element_size()
        d.dst_valid = K.ptr(t.dst_valid)
        d.dst_stride = max(dst.stride(0), 1)
        d.dst_dtype = dtype_code(t.dst.dtype)
    _lib.require_gpu()
    lib = _lib.load()
    cuts.append(len(order))
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        table = _upload(words, dev)
        K.stat_add("loader_source_table")
        for pos, d in enumerate(descs):
            d.src = table.data_ptr() + (nsrc + 1 + pos * nsrc * rec) * 8     # its column's row of the table
        for start, stop in zip(cuts[:-1], cuts[1:]):
            K.stat_add("loader_take_multi")
            sub = C.cast(C.byref(descs, start * C.sizeof(_lib.TakeCol)), C.POINTER(_lib.TakeCol))
            check(lib.nvt_batch_take_multi(K.ptr(index), m, table.data_ptr(), nsrc, total, sub, stop - start,
                                           stream), "nvt_batch_take_multi")


def take_lists_multi(frames, names: Sequence[str], index: Optional[torch.Tensor], m: Optional[int] = None,
                     want_offsets: Optional[torch.Tensor] = None, dtypes: Optional[Dict] = None):
    """``take_lists`` over the concatenation of ``frames``, with the same return shapes: one
    read-back per group of columns that share their offsets in every frame, and no piecewise
    concatenation.  The leaves take the first frame's dtype unless ``dtypes`` names another; a leaf
    bitmap comes out when any frame has one."""
    _check_sources(frames)
    if len(frames) == 1:
        return take_lists(frames[0], names, index, m, want_offsets, dtypes)
    if index is not None:
        m = int(index.numel())
    begin = src_begin([len(f) for f in frames])
    nsrc, n_total = len(frames), begin[-1]
    m = n_total if m is None else m
    rec = _lib.TAKE_SRC_WORDS
    groups: Dict = {}
    for name in names:
        cols = [_source(f, name) for f in frames]
        if not all(c.is_list for c in cols):
            raise TypeError(f"column '{name}' is not a list column")
        key = tuple((c.offsets.data_ptr(), c.offsets.numel()) for c in cols)
        groups.setdefault(key, []).append((name, cols))
    out, bounds = {}, {}
    for group in groups.values():
        offsets = [c.offsets.contiguous() for c in group[0][1]]
        dev = offsets[0].device
        new_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        total, host, table = 0, None, None
        jobs: List = []
        words = list(begin) + [o.data_ptr() for o in offsets]
        for name, cols in group:
            datas = [c.data.contiguous() for c in cols]
            dt = (dtypes or {}).get(name, datas[0].dtype)
            for data, c in zip(datas, cols):
                if not cast_allowed(data.dtype, dt):
                    raise TypeError(f"column '{name}': no conversion from {data.dtype} to {dt}")
                words += [data.data_ptr(), K.ptr(c.valid) or 0, dtype_code(data.dtype)]
            jobs.append((name, datas, dt, any(c.valid is not None for c in cols)))
        if m > 0:
            _lib.require_gpu()
            lib = _lib.load()
            with K.LAUNCH_LOCK:
                stream = K.stream_ptr()
                table = _upload(words, dev)
                K.stat_add("loader_source_table")
                need = C.c_uint64()
                check(lib.nvt_take_list_ws_bytes(m, C.byref(need)), "nvt_take_list_ws_bytes")
                ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
                check(lib.nvt_take_list_offsets_multi(table.data_ptr() + (nsrc + 1) * 8, table.data_ptr(), nsrc,
                                                      n_total, K.ptr(index), m, new_off.data_ptr(), ws.data_ptr(),
                                                      ws.numel() * 8, stream), "nvt_take_list_offsets_multi")
                K.stat_add("loader_list_readback")
                if want_offsets is not None:
                    host = K.read_back(torch.cat([new_off[want_offsets], new_off[m:]]))
                    total = int(host[-1])
                    host = host[:-1]
                else:
                    total = int(K.read_back(new_off[m:])[0])   # the chunk's one host synchronisation
        elif want_offsets is not None:
            host = [0] * int(want_offsets.numel())
        descs = (_lib.TakeCol * len(jobs))()
        for k, (d, (name, datas, dt, any_valid)) in enumerate(zip(descs, jobs)):
            dst = torch.empty(total, dtype=dt, device=dev)
            dst_valid = torch.empty(bitmap_bytes(total), dtype=torch.uint8, device=dev) if any_valid else None
            out[name] = (dst, new_off, dst_valid)
            bounds[name] = host
            if table is not None:
                d.src = table.data_ptr() + (nsrc + 1 + nsrc + k * nsrc * rec) * 8
            d.dst = dst.data_ptr()
            d.dst_valid = K.ptr(dst_valid)
            d.dst_stride = 1
            d.dst_dtype = dtype_code(dt)
        if total > 0:
            with K.LAUNCH_LOCK:
                K.stat_add("loader_take_list_multi")
                check(_lib.load().nvt_take_list_multi(descs, len(jobs), table.data_ptr() + (nsrc + 1) * 8,
                                                      table.data_ptr(), nsrc, K.ptr(index), new_off.data_ptr(), m,
                                                      total, K.stream_ptr()), "nvt_take_list_multi")
    return out, bounds


def take_lists(frame, names: Sequence[str], index: Optional[torch.Tensor], m: Optional[int] = None,
               want_offsets: Optional[torch.Tensor] = None, dtypes: Optional[Dict] = None):
    """Rows ``index`` of the named list columns.  Returns ``{name: (values, offsets, valid)}`` with
    int64 offsets from 0 (shared by the columns that shared one), and ``bounds``: the host values of
    ``offsets[want_offsets]`` (int64 row numbers on the device) for the first group, read back in the
    same one transfer as the leaf total."""
    if index is not None:
        m = int(index.numel())
    n_src = len(frame)
    m = n_src if m is None else m
    groups: Dict = {}
    for name in names:
        col = _source(frame, name)
        if not col.is_list:
            raise TypeError(f"column '{name}' is not a list column")
        groups.setdefault((col.offsets.data_ptr(), col.offsets.numel()), []).append((name, col))
    out, bounds = {}, {}
    for group in groups.values():
        offsets = group[0][1].offsets.contiguous()
        dev = offsets.device
        new_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        total, host = 0, None
        if m > 0:
            _lib.require_gpu()
            lib = _lib.load()
            with K.LAUNCH_LOCK:
                stream = K.stream_ptr()
                need = C.c_uint64()
                check(lib.nvt_take_list_ws_bytes(m, C.byref(need)), "nvt_take_list_ws_bytes")
                ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
                check(lib.nvt_take_list_offsets(offsets.data_ptr(), n_src, K.ptr(index), m, new_off.data_ptr(),
                                                ws.data_ptr(), ws.numel() * 8, stream), "nvt_take_list_offsets")
                K.stat_add("loader_list_readback")
                if want_offsets is not None:
                    host = K.read_back(torch.cat([new_off[want_offsets], new_off[m:]]))
                    total = int(host[-1])
                    host = host[:-1]
                else:
                    total = int(K.read_back(new_off[m:])[0])   # the chunk's one host synchronisation
        elif want_offsets is not None:
            host = [0] * int(want_offsets.numel())
        jobs: List = []
        for name, col in group:
            data = col.data.contiguous()
            dt = (dtypes or {}).get(name, data.dtype)
            if not cast_allowed(data.dtype, dt):
                raise TypeError(f"column '{name}': no conversion from {data.dtype} to {dt}")
            dst = torch.empty(total, dtype=dt, device=dev)
            dst_valid = None
            if col.valid is not None:
                dst_valid = torch.empty(bitmap_bytes(total), dtype=torch.uint8, device=dev)
            jobs.append((data, col.valid, dst, dst_valid))
            out[name] = (dst, new_off, dst_valid)
            bounds[name] = host
        if total > 0:
            descs = (_lib.TakeCol * len(jobs))()
            for d, (data, valid, dst, dst_valid) in zip(descs, jobs):
                d.src = data.data_ptr()
                d.src_valid = K.ptr(valid)
                d.dst = dst.data_ptr()
                d.dst_valid = K.ptr(dst_valid)
                d.dst_stride = 1
                d.src_dtype = dtype_code(data.dtype)
                d.dst_dtype = dtype_code(dst.dtype)
            with K.LAUNCH_LOCK:
                K.stat_add("loader_take_list_many")
                check(_lib.load().nvt_take_list_many(descs, len(jobs), offsets.data_ptr(), K.ptr(index),
                                                     new_off.data_ptr(), m, total, K.stream_ptr()),
                      "nvt_take_list_many")
    return out, bounds
