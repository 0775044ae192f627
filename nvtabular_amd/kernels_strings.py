"""String categoricals from Arrow string buffers: the device side of ``strings.py``.

A string column becomes its int64 surrogate keys (``strings.string_key64``: pandas' keyed
SipHash + mixing step) and the {surrogate -> string} dictionary without hashing on the host:
the offsets / chars / validity buffers go to HBM as they are, ``nvt_str_hash`` hashes one string
per lane, ``nvt_str_dedup`` finds the first row of every distinct key and checks every other row's
bytes against it, and ``nvt_str_gather`` packs the distinct strings so that one copy brings them
back.  Part of the host driver of the C ABI (include/nvt_hip.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

COLLISION_MSG = "64-bit surrogate collision between distinct strings"
_MAX_CHARS = (1 << 32) - 2   # nvt_str_gather's output is addressed with 32-bit prefix sums


@dataclass
class StringBuffers:
    """An Arrow string array's buffers on the device (offsets as Arrow has them: int32 or int64,
    first entry possibly non-zero; chars from the byte that entry names)."""
    n: int
    offsets: torch.Tensor
    offset_bytes: int
    chars: torch.Tensor
    nchars: int
    valid: Optional[torch.Tensor]


def is_string_type(t) -> bool:
    import pyarrow as pa

    return pa.types.is_string(t) or pa.types.is_large_string(t)


def _stage_bytes(view: np.ndarray, device) -> torch.Tensor:
    """uint8 host bytes -> device, padded to a multiple of 8 bytes (at least 8): the kernels read
    whole aligned words.  One host copy into pinned memory, then an asynchronous copy."""
    size = max(8, (len(view) + 7) & ~7)
    if device.type != "cuda":
        raise _lib.NvtHipError("string columns need a GPU device")
    pin = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    if len(view):
        np.copyto(pin.numpy()[: len(view)], view)
    return pin.to(device, non_blocking=True)


def _valid_bitmap(arr, device) -> Optional[torch.Tensor]:
    """Arrow validity -> device bitmap of the array's own rows (None when nothing is null); a
    bitmap that does not start on a byte boundary is re-packed."""
    from .device import pack_bitmap, to_device_async

    if arr.null_count == 0:
        return None
    n = len(arr)
    buf = arr.buffers()[0]
    if buf is not None and arr.offset % 8 == 0:
        bits = np.frombuffer(buf, dtype=np.uint8, count=(n + 7) // 8, offset=arr.offset // 8)
        pad = (-len(bits)) % 8
        if pad:
            bits = np.concatenate([bits, np.zeros(pad, dtype=np.uint8)])
    else:
        bits = pack_bitmap(np.asarray(arr.is_valid()))
    return to_device_async(bits, device)


def _offsets(arr):
    """(the array's n + 1 offsets as Arrow stores them, offset width in bytes)."""
    import pyarrow as pa

    assert is_string_type(arr.type)
    w = 8 if pa.types.is_large_string(arr.type) else 4
    dt = np.int64 if w == 8 else np.int32
    n = len(arr)
    if n == 0:
        return np.zeros(1, dtype=dt), w
    return np.frombuffer(arr.buffers()[1], dtype=dt, count=n + 1, offset=arr.offset * w), w


def fits(arr) -> bool:
    """Whether the device path takes this string array (its chars stay below 4 GiB)."""
    off, _ = _offsets(arr)
    return int(off[-1]) - int(off[0]) <= _MAX_CHARS


def upload(arr, device) -> StringBuffers:
    """pa.StringArray / pa.LargeStringArray -> StringBuffers (only the array's own chars travel)."""
    from .device import to_device_async

    off, w = _offsets(arr)
    c0, c1 = int(off[0]), int(off[-1])
    data = arr.buffers()[2]
    chars = (np.frombuffer(data, dtype=np.uint8, count=c1 - c0, offset=c0)
             if data is not None and c1 > c0 else np.zeros(0, dtype=np.uint8))
    return StringBuffers(len(arr), to_device_async(off, device), w, _stage_bytes(chars, device), c1 - c0,
                         _valid_bitmap(arr, device))


def hash_buffers(b: StringBuffers) -> torch.Tensor:
    """int64 surrogate of every row (0 for a null row): nvt_str_hash."""
    out = torch.empty(b.n, dtype=torch.int64, device=b.chars.device)
    K.stat_add("str_hash")
    check(_lib.load().nvt_str_hash(b.offsets.data_ptr(), b.offset_bytes, b.chars.data_ptr(), K.ptr(b.valid),
                                   b.n, out.data_ptr(), K.stream_ptr()), "nvt_str_hash")
    return out


def take_keys(dict_keys: torch.Tensor, indices: torch.Tensor, valid: Optional[torch.Tensor]) -> torch.Tensor:
    """Keys of a dictionary-encoded column: dict_keys[indices[i]] (0 for a null row)."""
    assert indices.dtype in (torch.int32, torch.int64)
    n = indices.numel()
    out = torch.empty(n, dtype=torch.int64, device=indices.device)
    check(_lib.load().nvt_str_take_keys(dict_keys.data_ptr(), dict_keys.numel(), indices.data_ptr(),
                                        indices.element_size(), K.ptr(valid), n, out.data_ptr(),
                                        K.stream_ptr()), "nvt_str_take_keys")
    return out


def dedup(keys: torch.Tensor, valid: Optional[torch.Tensor], strings: StringBuffers,
          index: Optional[torch.Tensor] = None):
    """(distinct, collisions, rep_keys, rep_strs): the first row of every distinct key among the
    valid rows, in row order -- its key and its string (``index[row]`` with an index, else the
    row) -- and the number of valid rows whose bytes differ from their key's first row.  One
    read-back of the two counts."""
    lib = _lib.load()
    n, dev = keys.numel(), keys.device
    need = C.c_uint64()
    check(lib.nvt_str_dedup_ws_bytes(n, C.byref(need)), "nvt_str_dedup_ws_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    rep_keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    rep_strs = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    K.stat_add("str_dedup")
    check(lib.nvt_str_dedup(keys.data_ptr(), K.ptr(valid), n, K.ptr(index),
                            index.element_size() if index is not None else 0, strings.offsets.data_ptr(),
                            strings.offset_bytes, strings.chars.data_ptr(), strings.n, ws.data_ptr(),
                            need.value, rep_keys.data_ptr(), rep_strs.data_ptr(), counts.data_ptr(),
                            K.stream_ptr()), "nvt_str_dedup")
    # (a plain copy, not K.read_back: DeviceFrame.from_arrow builds columns from several threads
    # on one stream, and the read-back mailbox of a stream holds one value at a time)
    m, bad = (int(x) for x in counts.cpu().numpy())
    return m, bad, rep_keys[:m], rep_strs[:m]


def gather(strs: torch.Tensor, strings: StringBuffers):
    """Strings ``strs`` -> pa.LargeStringArray on the host, packed on the device first so that
    only they cross the link (two read-backs: the offsets, then the chars)."""
    import pyarrow as pa

    lib = _lib.load()
    m, dev = strs.numel(), strings.chars.device
    need = C.c_uint64()
    check(lib.nvt_str_gather_ws_bytes(m, C.byref(need)), "nvt_str_gather_ws_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
    out_chars = torch.empty(max(strings.nchars, 1), dtype=torch.uint8, device=dev)
    check(lib.nvt_str_gather(strs.data_ptr(), m, strings.offsets.data_ptr(), strings.offset_bytes,
                             strings.chars.data_ptr(), strings.n, ws.data_ptr(), need.value,
                             out_off.data_ptr(), out_chars.data_ptr(), strings.nchars, K.stream_ptr()),
          "nvt_str_gather")
    off = out_off.cpu().numpy()
    total = int(off[-1])
    if total > strings.nchars:
        raise _lib.NvtHipError("nvt_str_gather: the gathered strings overflow the chars buffer")
    chars = out_chars[:total].cpu().numpy()
    return pa.LargeStringArray.from_buffers(m, pa.py_buffer(off), pa.py_buffer(chars))


def lookup_dict(keys: torch.Tensor, valid: Optional[torch.Tensor], strings: StringBuffers,
                index: Optional[torch.Tensor] = None) -> dict:
    """{surrogate -> str} of a column, in first-appearance order (the host path's dict); raises
    the host path's ValueError when two distinct strings share a surrogate."""
    m, bad, rep_keys, rep_strs = dedup(keys, valid, strings, index)
    if bad:
        raise ValueError(COLLISION_MSG)
    if m == 0:
        return {}
    values = gather(rep_strs, strings).to_pylist()
    return dict(zip(rep_keys.cpu().numpy().tolist(), values))


def column_from_string_array(arr, device):
    """pa.StringArray / pa.LargeStringArray -> DeviceColumn (keys, validity, dict) on the device."""
    from .device import DeviceColumn

    b = upload(arr, device)
    keys = hash_buffers(b)
    strings = lookup_dict(keys, b.valid, b)
    return DeviceColumn(keys, b.valid, None, None, strings)


def column_from_dictionary_array(arr, device):
    """pa.DictionaryArray with string values -> DeviceColumn: the dictionary is hashed and every
    row takes its entry's key (a null index is a null row)."""
    from .device import DeviceColumn, to_device_async

    d = upload(arr.dictionary, device)
    dict_keys = hash_buffers(d)
    idx = arr.indices
    ids = idx.to_numpy(zero_copy_only=False) if idx.null_count == 0 else \
        np.frombuffer(idx.buffers()[1], dtype=idx.type.to_pandas_dtype(), count=len(idx),
                      offset=idx.offset * idx.type.bit_width // 8)
    ids = ids.astype(np.int64 if ids.dtype.itemsize == 8 or ids.dtype.kind == "u" else np.int32,
                     copy=False)
    indices = to_device_async(ids, device)
    valid = _valid_bitmap(idx, device)
    keys = take_keys(dict_keys, indices, valid)
    strings = lookup_dict(keys, valid, d, index=indices)
    return DeviceColumn(keys, valid, None, None, strings)


def hash_array(arr, device) -> torch.Tensor:
    """Surrogates of a string array's rows (0 for a null row) on the device."""
    return hash_buffers(upload(arr, device))
