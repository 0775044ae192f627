"""Flat int8 / int16 / bool columns in the parquet path: the host driver of ``nvt_pq_widen_i32_many``,
``nvt_pq_bool_pack`` (out) and ``nvt_expand_narrow`` (in) (include/nvt_hip.h; DESIGN.md, "Narrow and
bool columns in the parquet path").

Out: ``widen_many`` sign-extends the non-null values of every int8 / int16 column of a row group to
int32 in one launch -- behind it the chunk is an int32 chunk for the dictionary, snappy and
statistics code --, ``bool_pack`` turns the non-null values of a bool chunk into the bytes of its
BOOLEAN pages.  In: ``expand_narrow`` gives every row of a staged chunk (int32 values, or one byte
per bool) its slot and narrows on the way.  Nothing here reads back.  The facade's conventions:
launches on torch's current stream, errors through ``_lib.check``, buffers from torch's allocator;
the writers take ``kernels.LAUNCH_LOCK``, ``expand_narrow`` -- called by the parquet prefetcher's
thread like ``kernels.expand_valid`` -- brings a workspace of its own and does not."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_parquet_list import _buffer

NARROW = {torch.int8: _lib.NVT_I8, torch.int16: _lib.NVT_I16}
_SIZES = {torch.int8: (4, 1), torch.int16: (4, 2), torch.bool: (1, 1)}   # staged bytes -> column bytes


def widen_many(srcs: Sequence[torch.Tensor], guard: int = 0) -> List[torch.Tensor]:
    """int32 copies of the int8 / int16 tensors ``srcs`` (1-D, contiguous, on the device; slices of
    columns: aligned to their element size only), ONE call for all of them.  ``guard``: bytes left
    untouched in front of and behind every output (tests)."""
    if not srcs:
        return []
    _lib.require_gpu()
    lib = _lib.load()
    descs = (_lib.PqWidenCol * len(srcs))()
    outs = []
    for d, t in zip(descs, srcs):
        assert t.dtype in NARROW and t.dim() == 1 and t.is_contiguous() and t.is_cuda
        raw, view = _buffer(4 * t.numel(), guard, t.device)
        out = view.view(torch.int32)
        out.raw = raw
        d.src, d.dst, d.n, d.src_dtype = t.data_ptr(), out.data_ptr(), t.numel(), NARROW[t.dtype]
        outs.append(out)
    with K.LAUNCH_LOCK:
        K.stat_add("pq_widen")
        check(lib.nvt_pq_widen_i32_many(descs, len(srcs), K.stream_ptr()), "nvt_pq_widen_i32_many")
    return outs


def bool_byte_at(page_start: torch.Tensor) -> torch.Tensor:
    """int64[npages + 1]: the byte at which every page's bits start -- page p takes
    ceil(values of p / 8) bytes, the pages lie one behind the other."""
    nbytes = (page_start[1:] - page_start[:-1] + 7) // 8
    return torch.cat([nbytes.new_zeros(1), torch.cumsum(nbytes, 0)])


def bool_pack(vals: torch.Tensor, page_start: torch.Tensor, guard: int = 0) -> torch.Tensor:
    """The bytes of the BOOLEAN pages of one chunk: ``vals`` (torch.bool, on the device, contiguous:
    the NON-NULL values in order) cut into pages at ``page_start`` (int64[npages + 1] on the device)
    -> uint8 on the device, page p's ceil(values / 8) bytes behind those of page p - 1.  The buffer
    is sized by the bound ceil(n / 8) + npages (the page sizes are the device's); bytes behind the
    last page are not written."""
    assert vals.dtype == torch.bool and vals.dim() == 1 and vals.is_contiguous() and vals.is_cuda
    assert page_start.dtype == torch.int64 and page_start.is_contiguous() and page_start.numel() >= 1
    _lib.require_gpu()
    lib = _lib.load()
    n, npages = int(vals.numel()), int(page_start.numel()) - 1
    raw, out = _buffer((n + 7) // 8 + npages, guard, vals.device)
    out.raw = raw
    if n == 0 or npages == 0:
        return out
    byte_at = bool_byte_at(page_start).contiguous()
    with K.LAUNCH_LOCK:
        K.stat_add("pq_bool_pack")
        check(lib.nvt_pq_bool_pack(vals.data_ptr(), page_start.data_ptr(), byte_at.data_ptr(), npages,
                                   out.data_ptr(), K.stream_ptr()), "nvt_pq_bool_pack")
    out.keep = (vals, page_start, byte_at)   # what the enqueued kernel reads
    return out


def expand_narrow(packed: torch.Tensor, dtype: torch.dtype, bitmap: Optional[torch.Tensor], n: int,
                  guard: int = 0) -> torch.Tensor:
    """The staged non-null values ``packed`` (int32 for an int8 / int16 column, uint8 for a bool
    column; in order) -> ``dtype`` [n] with one slot per row: out[i] = bit i of ``bitmap`` ? the next
    value, narrowed : 0 (nvt_expand_narrow).  ``bitmap`` None: the narrowing copy of n values."""
    src_size, dst_size = _SIZES[dtype]
    assert packed.element_size() == src_size and packed.is_contiguous() and packed.is_cuda
    lib = _lib.load()
    raw, view = _buffer(n * dst_size, guard, packed.device)
    out = view.view(dtype)
    out.raw = raw
    if n == 0:
        return out
    if bitmap is not None and packed.numel() == 0:   # (no values at all)
        view.zero_()
        return out
    ws = None
    if bitmap is not None:
        need = C.c_uint64()
        check(lib.nvt_expand_valid_ws_bytes(n, C.byref(need)), "nvt_expand_valid_ws_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=packed.device)
    check(lib.nvt_expand_narrow(packed.data_ptr(), src_size, dst_size, K.ptr(bitmap), n, out.data_ptr(), K.ptr(ws),
                                K.stream_ptr()), "nvt_expand_narrow")
    return out
