"""DELTA_BINARY_PACKED pages of flat INT32 / INT64 parquet columns: the host driver of
``nvt_pq_delta_decode`` (include/nvt_hip.h; csrc/nvt_parquet_delta.hip; DESIGN.md,
"DELTA_BINARY_PACKED in the parquet reader").

The host decoder stages such pages as they are (``parquet_plain.StagedDelta``) and leaves a hole for
their values in the column's packed values.  ``values_to_device`` brings what is NOT a hole to the
device, ``fill_holes`` the stages of every delta column of a partition, builds ONE page table and ONE
tile table for all of them (numpy, from the page records) and fills all holes with one call -- three
launches per partition whatever the number of columns and pages.  Nothing here reads back.  Like
``kernels.expand_valid`` this runs on the parquet prefetcher's thread and stream: buffers come from
torch's allocator on the current stream, no shared workspace is used and ``LAUNCH_LOCK`` is not taken."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

TILE = _lib.PQ_DELTA_TILE
_MAX_GAPS = 64   # more runs of decoded values than this between the holes: the buffer travels whole


def page_records(stage):
    """(first_value, pos, count, vpm, first_mb) of the stage's pages, uint64 arrays."""
    W = _lib.PQ_DELTA_RECORD_WORDS
    pg = stage.pages[: W * stage.npages].numpy().view(np.uint64).reshape(-1, W)
    return pg[:, 0], pg[:, 1], pg[:, 2] & np.uint64(0xFFFFFFFF), pg[:, 2] >> np.uint64(32), pg[:, 3]


def values_to_device(sc, device) -> torch.Tensor:
    """The packed values of staged column ``sc`` on ``device``: the values the host decoded (PLAIN and
    dictionary pages) are copied, the holes of its delta pages are not -- they never held anything."""
    vals = sc.values[: sc.nvalid]
    if sc.delta is None:
        return vals.to(device, non_blocking=True)
    _, pos, count, _, _ = page_records(sc.delta)
    order = np.argsort(pos, kind="stable")
    lo, hi = pos[order].astype(np.int64), (pos[order] + count[order]).astype(np.int64)
    starts, ends = np.concatenate([[0], hi]), np.concatenate([lo, [sc.nvalid]])   # what lies between the holes
    keep = ends > starts
    if int(keep.sum()) > _MAX_GAPS:
        return vals.to(device, non_blocking=True)
    out = torch.empty(sc.nvalid, dtype=vals.dtype, device=device)
    for a, b in zip(starts[keep].tolist(), ends[keep].tolist()):
        out[a:b].copy_(vals[a:b], non_blocking=True)
    return out


def fill_holes(items: Sequence[Tuple[object, torch.Tensor]]) -> None:
    """``items``: (StagedDelta, the column's packed values on the device: int32 / int64, contiguous)
    per delta column of a partition.  Copies every stage to the device and writes the values of all
    their pages into the holes (nvt_pq_delta_decode), on the current stream."""
    items = [(st, v) for st, v in items if st is not None and st.npages]
    if not items:
        return
    _lib.require_gpu()
    lib = _lib.load()
    recs, tile_pages, keep = [], [], []
    page_at = tile_at = 0
    for st, vals in items:
        assert vals.is_cuda and vals.is_contiguous() and vals.dtype in (torch.int32, torch.int64)
        first, pos, count, vpm, first_mb = page_records(st)
        if int((pos + count).max()) > vals.numel() or int(count.min()) < 1 or int(vpm.min()) < 32 or \
                int(vpm.max()) > TILE:
            raise _lib.NvtHipError("fill_holes: a page record does not fit its column's packed values")
        per = (np.uint64(TILE) // vpm) * vpm                      # deltas per tile
        ntiles = (count - np.uint64(1) + per - np.uint64(1)) // per
        nmb = (count - np.uint64(1) + vpm - np.uint64(1)) // vpm
        if int((first_mb + nmb).max()) > st.nmbs:
            raise _lib.NvtHipError("fill_holes: a page record names miniblocks its stage does not hold")
        raw = st.bytes[: ((st.nbytes + 15) & ~15) + 16].to(vals.device, non_blocking=True)
        mbs = st.mbs[: 2 * max(1, st.nmbs)].to(vals.device, non_blocking=True)
        assert raw.data_ptr() % 16 == 0 and mbs.data_ptr() % 16 == 0 and vals.data_ptr() % vals.element_size() == 0
        keep += [raw, mbs, vals]
        width = vals.element_size()
        rec = np.empty((st.npages, _lib.PQ_DELTA_PAGE_WORDS), dtype=np.uint64)
        rec[:, 0] = raw.data_ptr()
        rec[:, 1] = np.uint64(mbs.data_ptr()) + first_mb * np.uint64(16)
        rec[:, 2] = np.uint64(vals.data_ptr()) + pos * np.uint64(width)
        rec[:, 3] = first
        rec[:, 4] = count | (vpm << np.uint64(32))
        first_tile = np.uint64(tile_at) + np.cumsum(ntiles) - ntiles
        rec[:, 5] = np.uint64(width) | (first_tile << np.uint64(32))
        recs.append(rec)
        tile_pages.append(np.repeat(np.arange(page_at, page_at + st.npages, dtype=np.uint32), ntiles.astype(np.int64)))
        page_at += st.npages
        tile_at += int(ntiles.sum())
    if tile_at >= (1 << 31):
        raise _lib.NvtHipError("fill_holes: 2^31 tiles or more in one partition")
    dev = items[0][1].device
    pin = torch.cuda.is_available()
    # (a stage filled before this call is no longer touched by the host: the tables are the only new bytes)
    pages_h = torch.from_numpy(np.concatenate(recs).view(np.int64).reshape(-1))
    tiles_h = torch.from_numpy(np.concatenate(tile_pages).view(np.int32)) if tile_at else None
    pages_d = (pages_h.pin_memory() if pin else pages_h).to(dev, non_blocking=True)
    tiles_d = (tiles_h.pin_memory() if pin else tiles_h).to(dev, non_blocking=True) if tile_at else None
    sums = torch.empty(max(1, tile_at), dtype=torch.int64, device=dev)
    check(lib.nvt_pq_delta_decode(pages_d.data_ptr(), page_at, K.ptr(tiles_d), tile_at, sums.data_ptr(),
                                  K.stream_ptr()), "nvt_pq_delta_decode")
