"""Session features on the device: the host driver of ``nvt_list_*`` and
``nvt_difference_lag_many`` (include/nvt_hip.h), behind ``ops.ListSlice``, ``ops.ValueCount`` and
``ops.DifferenceLag``.

ListSlice: the columns of a frame whose ``offsets`` are the same tensor (what ``ops.Groupby`` hands
over) are planned ONCE and share ONE output offsets tensor.  Ragged output: sliced row lengths ->
exclusive scan -> new offsets, the leaf total read back once per distinct offsets tensor (the call's
one host synchronisation); padded output: row i starts at ``i * max_elements`` and nothing is read
back.  The leaves of all columns of a plan move in one ``nvt_list_slice_many`` launch whose work is
spread over the output leaves.  A pending FillMissing constant and the {surrogate -> str} dictionary
of a string column are carried over, as ``kernels_compact.compact_frame`` carries them.  Part of the
host driver of the C ABI, with the facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on
torch's current stream, errors through ``_lib.check``, workspace from torch's allocator."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

_WIDTHS = {torch.bool: 1, torch.uint8: 1, torch.int32: 4, torch.float32: 4, torch.int64: 8, torch.float64: 8}
_NP = {torch.bool: np.bool_, torch.uint8: np.uint8, torch.int32: np.int32, torch.float32: np.float32,
       torch.int64: np.int64, torch.float64: np.float64}
INT64_MAX = (1 << 63) - 1


def _bitmap_bytes(m: int) -> int:
    return (m + 63) // 64 * 8   # padded to 8 bytes, as pack_bitmap / pack_bitmap_device pad


def pad_bits(pad_value, dtype: torch.dtype) -> int:
    """The bits of ``pad_value`` cast to the leaf dtype, as the low bytes of a uint64."""
    np_dt = _NP[dtype]
    v = np.array([pad_value]).astype(np_dt)
    return int.from_bytes(v.tobytes().ljust(8, b"\0"), "little")


def slice_lists(frame, names: Sequence[str], start: int, end: int, pad_width: Optional[int] = None,
                pad_value=0.0):
    """``{name: DeviceColumn}``: row i of every named list column becomes ``row[start:end]``; with
    ``pad_width`` every row is then extended to that many leaves with ``pad_value`` (valid leaves).
    ``end`` = INT64_MAX is "to the end of the row"."""
    from .device import DeviceColumn

    plans: Dict = {}
    for name in names:
        col = frame[name]
        if not col.is_list:
            raise TypeError(f"ListSlice: column '{name}' is not a list column")
        if col.data.dtype not in _WIDTHS:
            raise TypeError(f"unsupported column dtype {col.data.dtype}")
        if pad_width is not None and col.strings is not None:
            raise NotImplementedError(f"ListSlice(pad=True) on the string leaves of '{name}'")
        plans.setdefault((col.offsets.data_ptr(), col.offsets.numel()), []).append((name, col))
    out = {}
    for group in plans.values():
        offsets = group[0][1].offsets.contiguous()
        n = int(offsets.numel()) - 1
        dev = offsets.device
        if n == 0:
            new_off = torch.zeros(1, dtype=torch.int64, device=dev)
            for name, col in group:
                valid = None if col.valid is None else torch.empty(0, dtype=torch.uint8, device=dev)
                out[name] = DeviceColumn(torch.empty(0, dtype=col.data.dtype, device=dev), valid, new_off,
                                         col.fill, col.strings)
            continue
        _lib.require_gpu()
        lib = _lib.load()
        with K.LAUNCH_LOCK:
            stream = K.stream_ptr()
            if pad_width is None:
                need = C.c_uint64()
                check(lib.nvt_list_slice_ws_bytes(n, C.byref(need)), "nvt_list_slice_ws_bytes")
                ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
                new_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
                K.stat_add("list_plan")
                check(lib.nvt_list_slice_offsets(offsets.data_ptr(), n, start, end, new_off.data_ptr(),
                                                 ws.data_ptr(), ws.numel() * 8, stream), "nvt_list_slice_offsets")
                K.stat_add("list_readback")
                total = int(K.read_back(new_off[n:])[0])   # the plan's one host synchronisation
            else:
                new_off = torch.arange(0, (n + 1) * pad_width, pad_width, dtype=torch.int64, device=dev) \
                    if pad_width > 0 else torch.zeros(n + 1, dtype=torch.int64, device=dev)
                total = n * pad_width
            jobs: List = []
            for name, col in group:
                data = col.data.contiguous()
                dst = torch.empty(total, dtype=data.dtype, device=dev)
                dst_valid = None
                if col.valid is not None:
                    dst_valid = torch.empty(_bitmap_bytes(total), dtype=torch.uint8, device=dev)
                jobs.append((data, dst, col.valid, dst_valid))
                out[name] = DeviceColumn(dst, dst_valid, new_off, col.fill, col.strings)
            if total > 0:
                descs = (_lib.ListCol * len(jobs))()
                for d, (data, dst, valid, dst_valid) in zip(descs, jobs):
                    d.src = data.data_ptr()
                    d.dst = dst.data_ptr()
                    d.src_valid = K.ptr(valid)
                    d.dst_valid = K.ptr(dst_valid)
                    d.pad_bits = pad_bits(pad_value, data.dtype) if pad_width is not None else 0
                    d.width = _WIDTHS[data.dtype]
                K.stat_add("list_slice_many")
                check(lib.nvt_list_slice_many(descs, len(jobs), offsets.data_ptr(), n, start, end,
                                              None if pad_width is not None else new_off.data_ptr(), total,
                                              pad_width or 0, stream), "nvt_list_slice_many")
    return out


_LEN_ACC0 = {}


def new_len_acc(k: int, device) -> torch.Tensor:
    """int64 [k, 2] accumulator of ``list_len_minmax``: {min, max} start at INT64_MAX / INT64_MIN."""
    row = _LEN_ACC0.get(device)
    if row is None:
        row = _LEN_ACC0[device] = torch.tensor([[INT64_MAX, -INT64_MAX - 1]], dtype=torch.int64).to(device)
    return row.repeat(k, 1)


def list_len_minmax(items):
    """items: [(offsets int64[n + 1], acc int64[2] on the device)].  Folds min / max of the row
    lengths into every acc in ONE launch; an offsets tensor of zero rows adds nothing."""
    items = [(o.contiguous(), a) for o, a in items if o.numel() > 1]
    if not items:
        return
    _lib.require_gpu()
    descs = (_lib.ListLenCol * len(items))()
    for d, (off, acc) in zip(descs, items):
        assert acc.dtype == torch.int64 and acc.numel() == 2 and acc.is_contiguous()
        d.offsets = off.data_ptr()
        d.n = off.numel() - 1
        d.acc = acc.data_ptr()
    with K.LAUNCH_LOCK:
        K.stat_add("list_len_minmax")
        check(_lib.load().nvt_list_len_minmax(descs, len(items), K.stream_ptr()), "nvt_list_len_minmax")


def difference_lag(keys, cols, n: int):
    """keys: [(data, valid)] partition columns (at most 4); cols: [(data, valid, shift)].  Returns
    one float32 tensor per entry of ``cols``: x[i] - x[i - shift] inside a partition, NaN elsewhere.
    Every output comes from ONE launch."""
    if len(keys) > _lib.LAG_MAX_KEYS:
        raise NotImplementedError(f"DifferenceLag over more than {_lib.LAG_MAX_KEYS} partition columns")
    dev = cols[0][0].device
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in cols]
    if n == 0 or not cols:
        return outs
    _lib.require_gpu()
    kd = (_lib.LagKey * max(len(keys), 1))()
    keep = []
    for d, (data, valid) in zip(kd, keys):
        data = data.contiguous()
        keep.append(data)
        d.x = data.data_ptr()
        d.valid = K.ptr(valid)
        d.dtype = K.dtype_code(data.dtype)
    cd = (_lib.LagCol * len(cols))()
    for d, (data, valid, shift), out in zip(cd, cols, outs):
        data = data.contiguous()
        keep.append(data)
        d.x = data.data_ptr()
        d.valid = K.ptr(valid)
        d.out = out.data_ptr()
        d.shift = int(shift)
        d.dtype = K.dtype_code(data.dtype)
    with K.LAUNCH_LOCK:
        K.stat_add("difference_lag_many")
        check(_lib.load().nvt_difference_lag_many(kd, len(keys), cd, len(cols), n, K.stream_ptr()),
              "nvt_difference_lag_many")
    return outs
