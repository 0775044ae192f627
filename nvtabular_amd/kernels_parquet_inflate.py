"""Snappy bodies of PLAIN parquet pages: the host driver of ``nvt_snappy_inflate_pages``
(include/nvt_hip.h; csrc/nvt_snappy_inflate.hip; DESIGN.md, "Snappy pages in the parquet reader").

The host decoder stages such bodies compressed (``parquet_plain.StagedInflate``) and leaves a hole for
their values in the column's packed values.  ``values_to_device`` brings what is NOT a hole to the
device, ``fill_holes`` the stages of every such column of a partition into ONE device buffer, builds ONE
page table for all of them (numpy) and inflates all pages with one launch.  Nothing here reads back:
``fill_holes`` returns the device status words, and the caller hands them to ``raise_failed`` once per
partition.  Like ``kernels.expand_valid`` this runs on the parquet prefetcher's thread and stream:
buffers come from torch's allocator on the current stream, no shared workspace is used and
``LAUNCH_LOCK`` is not taken."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

_MAX_GAPS = 64   # more runs of host-decoded values than this between the holes: the buffer travels whole


def launch(src: torch.Tensor, dst_ptr: int, table: np.ndarray) -> torch.Tensor:
    """One nvt_snappy_inflate_pages call on the current stream.  ``src``: uint8 on the device; ``dst_ptr``:
    the device address that the records' ``dst_at`` count from; ``table``: int64 [npages, 5]
    (nvt_inflate_page).  -> the status words (int32 on the device, one per page)."""
    lib = _lib.load()
    npages = int(table.shape[0])
    assert src.is_cuda and src.dtype == torch.uint8 and table.dtype == np.int64 and table.shape[1] == _lib.INFLATE_PAGE_WORDS
    host = torch.from_numpy(np.ascontiguousarray(table).reshape(-1))
    pages = host.pin_memory().to(src.device, non_blocking=True)
    status = torch.empty(npages, dtype=torch.int32, device=src.device)
    K.stat_add("pq_inflate")
    check(lib.nvt_snappy_inflate_pages(src.data_ptr(), dst_ptr, pages.data_ptr(), npages, status.data_ptr(),
                                       K.stream_ptr()), "nvt_snappy_inflate_pages")
    return status


def page_table(streams: Sequence[bytes], flags: Sequence[int], sizes: Sequence[int], dst_at: int = 0,
               gap: int = 0) -> Tuple[np.ndarray, bytes]:
    """(int64 [npages, 5] nvt_inflate_page records, the source bytes) of raw snappy ``streams``: bodies
    on 16-byte boundaries, as the reader stages them; page i gives ``sizes[i]`` bytes, the first at
    ``dst_at``, ``gap`` bytes between two pages' outputs."""
    table = np.zeros((len(streams), _lib.INFLATE_PAGE_WORDS), dtype=np.int64)
    src_at, parts = 0, []
    for i, (s, f, size) in enumerate(zip(streams, flags, sizes)):
        table[i] = (src_at, len(s), dst_at, size, f)
        parts.append(bytes(s) + b"\0" * (-len(s) % 16))
        src_at += len(parts[-1])
        dst_at += size + gap
    return table, b"".join(parts)


def inflate_pages(streams: Sequence[bytes], flags: Optional[Sequence[int]] = None,
                  sizes: Optional[Sequence[int]] = None) -> List[bytes]:
    """The raw entry, for tests and tools: every raw snappy stream of ``streams`` inflated in ONE launch.
    ``flags``: per stream 0 or NVT_INFLATE_V1_LEVELS; ``sizes``: the bytes each page gives (default: what
    its varint says; a page with the levels flag gives 4 + L fewer, so pass them).  -> the pages'
    values; NvtHipError names the first page that stopped and its code."""
    _lib.require_gpu()
    n = len(streams)
    if n == 0:
        return []
    flags = [0] * n if flags is None else list(flags)
    if sizes is None:
        if any(flags):
            raise ValueError("inflate_pages: pass `sizes` for pages with NVT_INFLATE_V1_LEVELS")
        sizes = [_declared_size(bytes(s)) for s in streams]
    table, body = page_table(streams, flags, sizes)
    src = torch.frombuffer(bytearray(body or b"\0"), dtype=torch.uint8).to("cuda")
    dst = torch.zeros(max(int(sum(sizes)), 1), dtype=torch.uint8, device="cuda")
    raise_failed((launch(src, dst.data_ptr(), table), [("inflate_pages", 0)]))
    whole = dst.cpu().numpy()
    return [whole[int(a): int(a) + int(b)].tobytes() for a, b in zip(table[:, 2], table[:, 3])]


def _declared_size(s: bytes) -> int:
    total = shift = 0
    for b in s[:10]:
        total |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    return total


def values_to_device(sc, device) -> torch.Tensor:
    """The packed values of staged column ``sc`` on ``device``: the values the host decoded are copied,
    the holes of its staged pages are not -- they never held anything."""
    vals = sc.values[: sc.nvalid]
    rec = sc.inflate.records()
    lo, hi = rec[:, 2] // vals.element_size(), (rec[:, 2] + rec[:, 3]) // vals.element_size()
    gaps = [(a, b) for a, b in zip([0] + hi.tolist(), lo.tolist() + [sc.nvalid]) if b > a]
    if len(gaps) > _MAX_GAPS:
        return vals.to(device, non_blocking=True)
    out = torch.empty(sc.nvalid, dtype=vals.dtype, device=device)
    for a, b in gaps:
        out[a:b].copy_(vals[a:b], non_blocking=True)
    return out


def fill_holes(items: Sequence[Tuple[object, torch.Tensor]]):
    """``items``: (StagedInflate, the column's packed values on the device: 4- or 8-byte elements,
    contiguous) per staged column of a partition.  Copies every stage into one device buffer and
    inflates all their pages into the holes (nvt_snappy_inflate_pages), on the current stream.
    -> (status words on the device, per column (where, first page)) for ``raise_failed``; None: nothing
    was launched."""
    items = [(st, v) for st, v in items if st is not None and st.npages and v.numel()]
    if not items:
        return None
    _lib.require_gpu()
    dev = items[0][1].device
    starts = np.cumsum([0] + [(st.nbytes + 15) & ~15 for st, _ in items])
    src = torch.empty(int(starts[-1]), dtype=torch.uint8, device=dev)
    base = min(v.data_ptr() for _, v in items)   # dst_at counts from the lowest column
    tables, owners, first = [], [], 0
    for (st, vals), at in zip(items, starts[:-1].tolist()):
        assert vals.is_cuda and vals.is_contiguous() and vals.element_size() in (4, 8)
        rec = st.records().copy()
        if int((rec[:, 2] + rec[:, 3]).max()) > vals.numel() * vals.element_size():
            raise _lib.NvtHipError(f"{st.where}: a staged page lies outside the column's {vals.numel()} values")
        src[at: at + st.nbytes].copy_(st.bytes[: st.nbytes], non_blocking=True)
        rec[:, 0] += at
        rec[:, 2] += vals.data_ptr() - base
        tables.append(rec)
        owners.append((st.where, first))
        first += rec.shape[0]
    return launch(src, base, np.concatenate(tables)), owners


def raise_failed(handle) -> None:
    """Reads the status words of a ``fill_holes`` once (this waits for the stream) and raises
    NvtHipError naming file, column, page and code of the first page that stopped."""
    status, owners = handle
    words = status.cpu().numpy()
    bad = np.flatnonzero(words)
    if bad.size == 0:
        return
    i = int(bad[0])
    where, first = [o for o in owners if o[1] <= i][-1]
    code = int(words[i])
    raise _lib.NvtHipError(f"{where}: snappy page {i - first} of the staged pages: "
                           f"{_lib.INFLATE_ERRORS.get(code, code)} (status {code}; {bad.size} pages failed)")
