"""Hash join against an external table on the device: the host driver of ``nvt_join_*``
(include/nvt_hip.h), behind ``ops.JoinExternal``.

``ExternalIndex`` is built once per operator (and per key-mode tuple): the external key words and
their tags come from ``nvt_join_hash``, a stable sort groups the rows by key (external order within a
key), the payload columns are permuted into that order and the distinct keys go into an
open-addressing table with ``nvt_join_insert``.  Host reads in the build (the distinct-key count,
the largest row count per key, the choice of the empty tag) happen once.

``join_frame`` then takes one of three paths per partition:

* left join, unique keys: ONE ``nvt_join_probe_gather`` launch per 16 payload columns, no read-back;
  the left columns are the same tensors;
* inner join, unique keys: ``nvt_join_probe`` (matched row, keep mask), ``kernels_compact`` over the
  left columns plus the row column (one read-back, m), ``nvt_join_gather`` for the payload;
* duplicate keys: ``nvt_join_probe`` (per-row output counts and their 64-bit total: one read-back),
  ``nvt_join_offsets``, ``nvt_join_expand`` (one lane per output row) and ``nvt_join_gather`` for
  the left scalar columns and the payload; left list columns go through ``DeviceFrame.take_rows``.

Same conventions as kernels_compact: launches under ``kernels.LAUNCH_LOCK`` on torch's current
stream, errors through ``_lib.check``, workspace from torch's allocator, one ``K.stat_add`` counter
per launch."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence

import torch

from . import _lib
from . import kernels as K
from ._lib import check

_WIDTHS = {torch.bool: 1, torch.uint8: 1, torch.int32: 4, torch.float32: 4, torch.int64: 8, torch.float64: 8}
_FLOATS = (torch.float32, torch.float64)
_EMPTY_CANDIDATES = [-(1 << 63) + i for i in range(64)]   # tags stored as int64 (bit patterns)


def key_class(col) -> str:
    """"s" (string surrogates), "f" (float) or "i" (integer / bool) for a key column."""
    if col.is_list:
        raise TypeError("list columns cannot be join keys")
    if col.strings is not None:
        return "s"
    return "f" if col.dtype in _FLOATS else "i"


def key_modes(left_classes: Sequence[str], ext_classes: Sequence[str], on, on_ext) -> tuple:
    modes = []
    for lc, ec, a, b in zip(left_classes, ext_classes, on, on_ext):
        if (lc == "s") != (ec == "s"):
            raise ValueError(f"You are trying to merge on a string column and a numeric column "
                             f"({a!r} and {b!r}); pandas' merge refuses this too")
        modes.append(_lib.JOIN_FLOAT if "f" in (lc, ec) else _lib.JOIN_INT)
    return tuple(modes)


def key_descs(cols, modes):
    """nvt_join_key descriptors of the key columns (pending fills applied), and the tensors to keep
    alive while the launches are enqueued."""
    descs = (_lib.JoinKey * len(cols))()
    alive = []
    for d, col, mode in zip(descs, cols, modes):
        col = col.materialize()
        data = col.data.contiguous()
        if data.dtype == torch.bool:
            data = data.view(torch.uint8)
        if data.dtype in _FLOATS and mode != _lib.JOIN_FLOAT:
            raise TypeError("a float key column needs float mode")
        alive += [data, col.valid]
        d.x = data.data_ptr() if data.numel() else None
        d.valid = K.ptr(col.valid)
        d.dtype = K.dtype_code(data.dtype)
        d.mode = mode
    return descs, alive


def _bitmap_bytes(m: int) -> int:
    return (m + 63) // 64 * 8


def _permute_bits(valid: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    from .device import pack_bitmap_device

    bits = (valid[order >> 3] >> (order & 7).to(torch.uint8)) & 1
    return pack_bitmap_device(bits.to(torch.bool))


class ExternalIndex:
    """The external table grouped by key, and its hash table (device-resident)."""

    def __init__(self, ext, on_ext: List[str], payload: List[str], modes: tuple):
        from .device import DeviceColumn

        _lib.require_gpu()
        lib = _lib.load()
        stream = K.stream_ptr()
        n = len(ext)
        nk = len(on_ext)
        dev = next(iter(ext.items()))[1].data.device if ext.columns else torch.device("cuda")
        self.nkeys, self.n_ext, self.modes = nk, n, modes
        keys, alive = key_descs([ext[c] for c in on_ext], modes)
        tag = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        nulls = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        words = torch.empty((nk, max(n, 1)), dtype=torch.int64, device=dev) if nk > 1 else None
        K.stat_add("join_hash")
        check(lib.nvt_join_hash(keys, nk, n, tag.data_ptr(), K.ptr(words), nulls.data_ptr(), stream),
              "nvt_join_hash")
        tag, nulls = tag[:n], nulls[:n]
        # group the rows by key, external order within a key (stable sorts); one component: the null
        # rows (tag 0) go last, as one group kept outside the table
        order = torch.sort(tag, stable=True)[1]
        if nk == 1:
            order = order[torch.sort(nulls[order], stable=True)[1]]
        st, sn = tag[order], nulls[order]
        new = torch.ones(n, dtype=torch.bool, device=dev)
        if n > 1:
            new[1:] = (st[1:] != st[:-1]) | (sn[1:] != sn[:-1])
        starts = torch.nonzero(new).flatten()
        counts = torch.diff(torch.cat([starts, torch.tensor([n], device=dev)]))
        gtag, gnull = st[starts], sn[starts]
        self.words = self.nulls = None
        if nk > 1:
            sw = words[:, :n][:, order].contiguous()
            gid = torch.cumsum(new.to(torch.int64), 0) - 1
            same = (sw == sw[:, starts[gid]]).all(0) & (sn == sn[starts[gid]])
            if n and (not bool(same.all()) or torch.unique(gtag).numel() != gtag.numel()):
                raise ValueError("JoinExternal: two different external keys share a 64-bit fingerprint")
            self.words, self.nulls = sw, sn.contiguous()
        self.null_first = self.null_count = 0
        if nk == 1 and starts.numel() and bool(gnull[-1] != 0):
            self.null_first, self.null_count = int(starts[-1]), int(counts[-1])
            gtag, starts, counts = gtag[:-1], starts[:-1], counts[:-1]
        ng = int(starts.numel())
        self.n_groups = ng + (1 if self.null_count else 0)
        self.max_count = max(int(counts.max()) if ng else 0, self.null_count)
        self.unique = self.max_count <= 1
        if n >= (1 << 32):
            raise ValueError("JoinExternal: the external table must have fewer than 2^32 rows")
        empty = next(c for c in _EMPTY_CANDIDATES if ng == 0 or not bool((gtag == c).any()))
        self.empty = empty & ((1 << 64) - 1)
        cap, nbytes = C.c_uint64(), C.c_uint64()
        check(lib.nvt_join_table_bytes(ng, C.byref(cap), C.byref(nbytes)), "nvt_join_table_bytes")
        self.capacity = cap.value
        slots = torch.zeros((self.capacity, 2), dtype=torch.int64, device=dev)
        slots[:, 0] = empty
        self.slots = slots
        if ng:
            first32 = starts.to(torch.int32).contiguous()
            count32 = counts.to(torch.int32).contiguous()
            gtag = gtag.contiguous()
            K.stat_add("join_insert")
            check(lib.nvt_join_insert(slots.data_ptr(), self.capacity, self.empty, gtag.data_ptr(),
                                      first32.data_ptr(), count32.data_ptr(), ng, stream), "nvt_join_insert")
        # the payload in grouped order; an empty table keeps one dummy row so that no pointer is null
        self.payload: Dict[str, "DeviceColumn"] = {}
        for name in payload:
            col = ext[name].materialize()
            if col.is_list:
                raise TypeError(f"JoinExternal: list column {name!r} in the external table is not supported")
            if n == 0:
                data = torch.zeros(1, dtype=col.dtype, device=dev)
                valid = torch.zeros(8, dtype=torch.uint8, device=dev)
            else:
                data = col.data[order].contiguous()
                valid = _permute_bits(col.valid, order) if col.valid is not None else None
            self.payload[name] = col.like(data, valid)
        self._alive = alive
        s = _lib.JoinIndex()
        s.slots = slots.data_ptr()
        s.capacity = self.capacity
        s.empty = self.empty
        s.words = K.ptr(self.words)
        s.nulls = K.ptr(self.nulls)
        s.n_ext = n
        s.null_first = self.null_first
        s.null_count = self.null_count
        s.nkeys = nk
        self.struct = s


def _cols_desc(jobs):
    descs = (_lib.JoinCol * len(jobs))()
    for d, (src, src_valid, dst, dst_valid) in zip(descs, jobs):
        d.src = src.data_ptr()
        d.src_valid = K.ptr(src_valid)
        d.dst = dst.data_ptr()
        d.dst_valid = K.ptr(dst_valid)
        d.width = _WIDTHS[src.dtype]
    return descs


def _alloc(src, m, with_valid, dev):
    dst = torch.empty(m, dtype=src.dtype, device=dev)
    return dst, (torch.empty(_bitmap_bytes(m), dtype=torch.uint8, device=dev) if with_valid else None)


def _gather(idx: torch.Tensor, m: int, cols, force_valid: bool, dev):
    """[(name, DeviceColumn)] -> {name: DeviceColumn} with rows idx (int64, -1 = null row)."""
    from .device import DeviceColumn

    out = {}
    items = list(cols)
    for i0 in range(0, len(items), _lib.JOIN_MAX_COLS):
        jobs = []
        for name, col in items[i0: i0 + _lib.JOIN_MAX_COLS]:
            src = col.data.contiguous()
            dst, dst_valid = _alloc(src, m, force_valid or col.valid is not None, dev)
            jobs.append((src, col.valid, dst, dst_valid))
            out[name] = DeviceColumn(dst, dst_valid, None, col.fill, col.strings, logical=col.logical)
        if m:
            K.stat_add("join_gather")
            check(_lib.load().nvt_join_gather(idx.data_ptr(), m, _cols_desc(jobs), len(jobs), K.stream_ptr()),
                  "nvt_join_gather")
    return out


def join_frame(left, on: List[str], ix: ExternalIndex, how: str, ext_names: List[str]):
    """``left.merge(ext, left_on=on, right_on=on_ext, how=how)`` in left-row order, renumbered from 0;
    ``ext_names`` are the payload columns appended after the left columns."""
    from .device import DeviceColumn, DeviceFrame

    lib = _lib.load()
    n = len(left)
    dev = None
    for _, col in left.items():
        dev = col.data.device
        break
    payload = [(name, ix.payload[name]) for name in ext_names]
    if n == 0:
        out = left.copy()
        for name, col in payload:
            out[name] = col.like(col.data[:0])
        return out
    stream = K.stream_ptr()
    keys, alive = key_descs([left[c] for c in on], ix.modes)
    inner = how == "inner"

    if ix.unique and not inner:
        out = left.copy()   # the left columns are the same tensors
        for i0 in range(0, len(payload), _lib.JOIN_MAX_COLS):
            jobs = []
            for name, col in payload[i0: i0 + _lib.JOIN_MAX_COLS]:
                dst, dst_valid = _alloc(col.data, n, True, dev)
                jobs.append((col.data, col.valid, dst, dst_valid))
                out[name] = col.like(dst, dst_valid)
            K.stat_add("join_probe_gather")
            check(lib.nvt_join_probe_gather(C.byref(ix.struct), keys, ix.nkeys, n, _cols_desc(jobs), len(jobs),
                                            None, stream), "nvt_join_probe_gather")
        return out

    first = torch.empty(n, dtype=torch.int64, device=dev)
    if ix.unique:   # inner join, unique keys: a row compaction of the left columns plus the matched row
        from .kernels_compact import compact_frame

        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        K.stat_add("join_probe")
        check(lib.nvt_join_probe(C.byref(ix.struct), keys, ix.nkeys, n, 1, first.data_ptr(), None,
                                 keep.data_ptr(), None, stream), "nvt_join_probe")
        tmp = "__join_row__"
        while tmp in left:
            tmp += "_"
        both = left.copy()
        both[tmp] = DeviceColumn(first)
        kept = compact_frame(both, keep)
        idx = kept[tmp].data
        out = kept.drop([tmp])
        for name, col in _gather(idx, int(idx.numel()), payload, False, dev).items():
            out[name] = col
        return out

    # duplicate keys: per-row output counts, their offsets, one lane per output row
    counts = torch.empty(n + 1, dtype=torch.int32, device=dev)   # uint32 counts; counts[n] = 0 for the scan
    counts[n:].zero_()
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    K.stat_add("join_probe")
    check(lib.nvt_join_probe(C.byref(ix.struct), keys, ix.nkeys, n, int(inner), first.data_ptr(),
                             counts.data_ptr(), None, total.data_ptr(), stream), "nvt_join_probe")
    m = int(total.item())   # the one host synchronisation of this path
    if m >= (1 << 32):
        raise ValueError(f"JoinExternal: {m} output rows; the duplicate-key path supports fewer than 2^32")
    need = C.c_uint64()
    check(lib.nvt_join_scan_ws_bytes(n, C.byref(need)), "nvt_join_scan_ws_bytes")
    ws = torch.empty(max(1, need.value // 8), dtype=torch.int64, device=dev)
    K.stat_add("join_offsets")
    check(lib.nvt_join_offsets(counts.data_ptr(), n, ws.data_ptr(), need.value, stream), "nvt_join_offsets")
    left_row = torch.empty(m, dtype=torch.int64, device=dev)
    ext_row = torch.empty(m, dtype=torch.int64, device=dev)
    if m:
        K.stat_add("join_expand")
        check(lib.nvt_join_expand(counts.data_ptr(), first.data_ptr(), n, m, left_row.data_ptr(),
                                  ext_row.data_ptr(), stream), "nvt_join_expand")
    scalar = [(name, col) for name, col in left.items() if not col.is_list]
    lists = [name for name, col in left.items() if col.is_list]
    moved = _gather(left_row, m, scalar, False, dev)
    if lists:
        moved.update(left[lists].take_rows(left_row).items())
    out = DeviceFrame({name: moved[name] for name in left.columns})
    for name, col in _gather(ext_row, m, payload, not inner, dev).items():
        out[name] = col
    return out
