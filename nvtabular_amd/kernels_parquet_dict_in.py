"""Dictionary-encoded pages of flat 4- / 8-byte parquet number columns: the host driver of
``nvt_pq_dict_fill_many`` (include/nvt_hip.h; csrc/nvt_parquet_dict_in.hip; DESIGN.md, "Dictionary
pages of number columns in the parquet reader").

The host decoder stages such pages as they are (``parquet_plain.StagedDict``) and leaves a hole for
their values in the column's packed values.  ``values_to_device`` brings what is NOT a hole to the
device (the values of PLAIN pages: KEEP records), ``fill_holes`` the stages of every such column of a
partition, builds ONE descriptor table and ONE group table for all of them (numpy) and fills all
holes with one launch.  Nothing here reads back: ``fill_holes`` returns the device word that counts
indices outside their dictionaries, and the caller reads it once per partition.  Like
``kernels.expand_valid`` this runs on the parquet prefetcher's thread and stream: buffers come from
torch's allocator on the current stream, no shared workspace is used and ``LAUNCH_LOCK`` is not taken."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

TILE, TILES_PER_WG = _lib.PQ_DICT_TILE, _lib.PQ_DICT_TILES_PER_WG
_MAX_GAPS = 64   # more runs of host-decoded values than this between the holes: the buffer travels whole


def run_records(stage) -> np.ndarray:
    """The stage's run table, closing record included: uint32 [nruns + 1, 4]."""
    return stage.runs[: 4 * (stage.nruns + 1)].numpy().view(np.uint32).reshape(-1, 4)


def values_to_device(sc, device) -> torch.Tensor:
    """The packed values of staged column ``sc`` on ``device``: the values the host decoded (KEEP
    records) are copied, the holes of its dictionary pages are not -- they never held anything."""
    vals = sc.values[: sc.nvalid]
    recs = run_records(sc.dict_stage)
    if int(recs[0, 0]) != 0 or int(recs[-1, 0]) != sc.nvalid:
        raise _lib.NvtHipError(f"{sc.dict_stage.where}: the run table does not cover the column's {sc.nvalid} values")
    keep = (recs[:-1, 1] & 0xFF) == _lib.PQ_RUN_KEEP
    if int(keep.sum()) > _MAX_GAPS:
        return vals.to(device, non_blocking=True)
    out = torch.empty(sc.nvalid, dtype=vals.dtype, device=device)
    for a, b in zip(recs[:-1, 0][keep].tolist(), recs[1:, 0][keep].tolist()):
        out[a:b].copy_(vals[a:b], non_blocking=True)
    return out


def fill_many(cols: Sequence[Tuple[torch.Tensor, int, torch.Tensor, torch.Tensor, int, torch.Tensor]],
              bad: torch.Tensor) -> None:
    """One nvt_pq_dict_fill_many call.  ``cols``: per column (runs: int32 words on the device, closing
    record included; nruns; packed: uint8 on the device, a multiple of 16 bytes; dict: uint8 on the
    device, heads included; ndict: its elements; values: the packed values on the device, 4- or 8-byte
    elements).  ``bad``: an int32 device word that receives += the indices outside their dictionaries."""
    lib = _lib.load()
    desc = np.zeros((len(cols), _lib.PQ_DICT_COL_WORDS), dtype=np.uint64)
    groups = []
    for i, (runs, nruns, packed, dct, ndict, vals) in enumerate(cols):
        width = vals.element_size()
        assert vals.is_cuda and vals.is_contiguous() and width in (4, 8)
        assert runs.numel() >= 4 * (nruns + 1) and packed.numel() % 16 == 0 and dct.numel() >= ndict * width
        assert all(t.data_ptr() % 16 == 0 for t in (runs, packed, dct, vals))
        if vals.numel() >= (1 << 32) - TILE or ndict >= (1 << 31) or packed.numel() >= (1 << 34):
            raise _lib.NvtHipError("fill_many: a column beyond 2^32 values, 2^31 dictionary entries or 16 GiB of indices")
        desc[i] = (runs.data_ptr(), nruns, packed.data_ptr(), packed.numel(), dct.data_ptr(), ndict, width,
                   vals.data_ptr(), vals.numel())
        ntiles = (vals.numel() + TILE - 1) // TILE
        first = np.arange(0, ntiles, TILES_PER_WG, dtype=np.uint32)
        groups.append(np.stack([np.full(first.size, i, dtype=np.uint32), first], axis=1))
    groups = np.concatenate(groups).reshape(-1) if groups else np.zeros(0, dtype=np.uint32)
    ngroups = groups.size // 2
    if ngroups == 0:
        return
    dev = cols[0][5].device
    pin = torch.cuda.is_available()
    desc_h = torch.from_numpy(desc.view(np.int64).reshape(-1))
    groups_h = torch.from_numpy(groups.view(np.int32))
    desc_d = (desc_h.pin_memory() if pin else desc_h).to(dev, non_blocking=True)
    groups_d = (groups_h.pin_memory() if pin else groups_h).to(dev, non_blocking=True)
    K.stat_add("pq_dict_fill")
    check(lib.nvt_pq_dict_fill_many(desc_d.data_ptr(), len(cols), groups_d.data_ptr(), ngroups, bad.data_ptr(),
                                    K.stream_ptr()), "nvt_pq_dict_fill_many")


def fill_holes(items: Sequence[Tuple[object, torch.Tensor]]) -> Optional[torch.Tensor]:
    """``items``: (StagedDict, the column's packed values on the device: 4- or 8-byte elements,
    contiguous) per staged column of a partition.  Copies every stage to the device and writes the
    values of all their dictionary pages into the holes (nvt_pq_dict_fill_many), on the current
    stream.  -> the int32 device word that counts the indices outside their dictionaries (None: nothing
    was launched)."""
    items = [(st, v) for st, v in items if st is not None and st.nruns and v.numel()]
    if not items:
        return None
    _lib.require_gpu()
    cols = []
    for st, vals in items:
        dev, width = vals.device, vals.element_size()
        runs = st.runs[: 4 * (st.nruns + 1)].to(dev, non_blocking=True)
        packed = st.packed[: ((st.npacked + 8 + 15) & ~15)].to(dev, non_blocking=True)
        dct = st.dict[: max(16, (st.ndict_bytes + 15) & ~15)].to(dev, non_blocking=True)
        cols.append((runs, st.nruns, packed, dct, st.ndict_bytes // width, vals))
    bad = torch.zeros(1, dtype=torch.int32, device=items[0][1].device)
    fill_many(cols, bad)
    return bad
