"""Parquet dictionary pages on the device: the host driver of ``nvt_pq_dict_*`` (include/nvt_hip.h),
behind ``Dataset.to_parquet(use_dictionary=...)`` (``parquet_write.write_plain``).

``encode`` enqueues build and pack for the non-null values of ONE column chunk and returns a
``DeviceDict``: the ascending dictionary, the bit-packed indices of every page and a 4-word state
record {d, overflow, ...}, all still on the device.  Nothing is read back here: the pack derives
the index width from the state record on the device, and the write driver brings the state records
of ALL offered columns of a row group back in one read-back (``read_back_states``);
``parquet_plain.dict_page_offsets`` restates on the host where the pack put every page.  Part of the host driver of the C ABI, with the
facade's conventions: launches under ``kernels.LAUNCH_LOCK`` on torch's current stream, errors
through ``_lib.check``, workspace from torch's allocator ("Dictionary pages in the PLAIN
parquet writer")."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_parquet_list import _buffer
from .parquet_plain import DICT_MAX_ENTRIES, dict_index_width

assert DICT_MAX_ENTRIES == _lib.PQ_DICT_MAX_ENTRIES   # (include/nvt_hip.h NVT_PQ_DICT_MAX_ENTRIES)
STATE_WORDS = _lib.PQ_DICT_STATE_WORDS


def table_slots(n: int, max_entries: int = DICT_MAX_ENTRIES) -> int:
    """Slots of the value -> rank table nvt_pq_dict_build makes for n values."""
    return max(16, 2 * (1 << (max(1, min(int(n), int(max_entries))) - 1).bit_length()))


def home_slot(values: np.ndarray, nslots: int) -> np.ndarray:
    """The table slot the values hash to (include/nvt_hip.h; tests build colliding values with it)."""
    v = np.asarray(values)
    key = (v.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)) if v.dtype == np.int64 else \
        (v.astype(np.int32).view(np.uint32) ^ np.uint32(1 << 31)).astype(np.uint64)
    with np.errstate(over="ignore"):
        return (key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - (int(nslots).bit_length() - 1))


class DeviceDict:
    """The enqueued build and pack of one column chunk: ``dictionary`` (room for min(n,
    max_entries) values, the first d are the dictionary), ``packed`` (uint8, sized for the widest
    index the chunk can need) and ``state`` (int64[4]: d, overflow) on the device."""

    def __init__(self, dictionary, packed, state, n, raw, keep):
        self.dictionary, self.packed, self.state, self.n = dictionary, packed, state, n
        self.page_start = keep[-1]
        self.raw = raw       # (dictionary, packed, state) with their guard bytes
        self._keep = keep    # what the enqueued kernels read


def encode(values: torch.Tensor, page_start: torch.Tensor, max_entries: int = DICT_MAX_ENTRIES,
           guard: int = 0) -> DeviceDict:
    """Enqueue ``nvt_pq_dict_build`` and ``nvt_pq_dict_pack`` for ``values`` (int32 / int64, on the
    device, contiguous: the NON-NULL values of a chunk in order) cut into pages at ``page_start``
    (int64[npages + 1] on the device, in value positions).  ``guard``: bytes left untouched in
    front of and behind every output buffer (tests)."""
    assert values.dtype in (torch.int32, torch.int64) and values.is_contiguous() and values.dim() == 1
    assert page_start.dtype == torch.int64 and page_start.is_contiguous() and page_start.numel() >= 1
    _lib.require_gpu()
    lib = _lib.load()
    dev = values.device
    n, npages = int(values.numel()), int(page_start.numel()) - 1
    cap = max(1, min(n, int(max_entries)))
    wmax = dict_index_width(cap)
    out_cap = 16 * (-(-(wmax * ((n + 7) // 8 + npages)) // 16) + npages)
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        need = C.c_uint64()
        check(lib.nvt_pq_dict_ws_bytes(n, int(max_entries), npages, C.byref(need)), "nvt_pq_dict_ws_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        dict_raw, dict8 = _buffer(cap * values.element_size(), guard, dev)
        packed_raw, packed = _buffer(out_cap, guard, dev)
        state_raw, state8 = _buffer(STATE_WORDS * 8, guard, dev)
        state = state8.view(torch.int64)
        code = K.dtype_code(values.dtype)
        K.stat_add("pqdict_build")
        check(lib.nvt_pq_dict_build(K.ptr(values), code, n, int(max_entries), dict8.data_ptr(), state.data_ptr(),
                                    ws.data_ptr(), ws.numel(), stream), "nvt_pq_dict_build")
        K.stat_add("pqdict_pack")
        check(lib.nvt_pq_dict_pack(K.ptr(values), code, n, int(max_entries), page_start.data_ptr(), npages,
                                   state.data_ptr(), packed.data_ptr(), out_cap, ws.data_ptr(), ws.numel(), stream),
              "nvt_pq_dict_pack")
    return DeviceDict(dict8.view(values.dtype), packed, state, n, (dict_raw, packed_raw, state_raw),
                      (ws, values, page_start))


def read_back_states(dicts: Sequence[DeviceDict], extra: Sequence[torch.Tensor] = None):
    """[(d, overflow, page_start as a numpy array)] of the enqueued chunks: ONE read-back for all of
    them (the page starts come along: a flat column's are popcounts only the device has).
    ``extra``: further int64 tensors on the device that ride along in the same read-back (the page
    tables of string columns); the result is then (the list above, [their numpy arrays])."""
    if not dicts and not extra:
        return [] if extra is None else ([], [])
    K.stat_add("pqdict_readback")
    w = K.read_back(torch.cat([t for dd in dicts for t in (dd.state, dd.page_start)] +
                              [t.reshape(-1) for t in (extra or ())])).view(np.int64)
    out, at = [], 0
    for dd in dicts:
        ps = w[at + STATE_WORDS: at + STATE_WORDS + dd.page_start.numel()]
        out.append((int(w[at]), int(w[at + 1]), np.array(ps, dtype=np.int64)))
        at += STATE_WORDS + dd.page_start.numel()
        dd._keep = None   # (the kernels are done: the workspace goes back to the allocator)
    if extra is None:
        return out
    more = []
    for t in extra:
        more.append(np.array(w[at: at + t.numel()], dtype=np.int64))
        at += t.numel()
    return out, more
