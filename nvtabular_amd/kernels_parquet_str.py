"""String columns of the parquet reader: the device side of ``parquet_plain.StagedStrings``.

The host decoder stages a column's dictionary entries (an Arrow string table), the run table of its
index streams and the bytes of the bit-packed runs (include/nvt_hip.h, "parquet in: string columns").
Here they are copied to HBM on the current stream and turned into the column ``DeviceColumn.from_arrow``
builds from pyarrow's read of the same rows: ``nvt_pq_expand_runs`` gives an entry id per non-null value,
``kernels.expand_valid`` spreads the ids over the rows, the entries are hashed once (``nvt_str_hash``),
every row takes its entry's key (``nvt_str_take_keys``) and the {surrogate -> string} dict is built
through the ids (``nvt_str_dedup`` / ``nvt_str_gather``).  Part of the host driver of the C ABI."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import kernels as K
from . import kernels_strings as KS
from ._lib import check


def expand_runs(runs: torch.Tensor, nruns: int, closing, packed: torch.Tensor, entries: int, nvalues: int,
                bad: torch.Tensor) -> torch.Tensor:
    """int32 entry id of every non-null value (nvt_pq_expand_runs): ``runs`` the run table on the device
    (int32 words, 4 per record, the closing record behind the ``nruns`` runs), ``closing`` that record on
    the host (4 words), ``packed`` the packed bytes on the device with 8 readable bytes behind the last
    run.  An id outside [0, entries) comes out as -1 and is added to the device word ``bad``."""
    out = torch.empty(nvalues, dtype=torch.int32, device=runs.device)
    closing = np.ascontiguousarray(closing, dtype=np.uint32)
    K.stat_add("pq_expand_runs")
    check(_lib.load().nvt_pq_expand_runs(runs.data_ptr(), nruns, closing.ctypes.data, packed.data_ptr(),
                                         packed.numel(), entries, nvalues, out.data_ptr(), bad.data_ptr(),
                                         K.stream_ptr()), "nvt_pq_expand_runs")
    return out


def column_from_staged(sc, device):
    """StagedColumn of a string column -> DeviceColumn (keys, validity, dict)."""
    from .device import DeviceColumn

    st = sc.strs
    entries, nruns, nvalues = st.entries, st.nruns, st.nvalues
    offsets = st.offsets[: entries + 1].to(device, non_blocking=True)
    chars = st.chars[: max(8, (st.nchars + 7) & ~7)].to(device, non_blocking=True)
    runs = st.runs[: 4 * (nruns + 1)].to(device, non_blocking=True)
    packed = st.packed[: ((st.npacked + 7) & ~7) + 8].to(device, non_blocking=True)
    bitmap = None
    if sc.valid is not None:
        bitmap = sc.valid[: ((sc.rows + 63) // 64) * 8].to(device, non_blocking=True)
    if nvalues == 0:   # no rows, or nulls only: nothing to expand, hash or look up
        return DeviceColumn(torch.zeros(sc.rows, dtype=torch.int64, device=device), bitmap, None, None, {})
    bad = torch.zeros(1, dtype=torch.int32, device=device)
    closing = st.runs[4 * nruns: 4 * nruns + 4].numpy().view(np.uint32)
    ids = expand_runs(runs, nruns, closing, packed, entries, nvalues, bad)
    if bitmap is not None:
        ids = K.expand_valid(ids, bitmap, sc.rows)
    table = KS.StringBuffers(entries, offsets, 8, chars, st.nchars, None)
    keys = KS.take_keys(KS.hash_buffers(table), ids, bitmap)
    # (KS.lookup_dict with the reader's own check between its two halves: the count of bad ids is read
    # right behind the counts dedup copies back, before any string is gathered through an id)
    m, collisions, rep_keys, rep_strs = KS.dedup(keys, bitmap, table, ids)
    nbad = int(bad.cpu().numpy()[0])
    if nbad:
        raise ValueError(f"{st.where}: {nbad} dictionary indices outside the {entries} entries of their pages")
    if collisions:
        raise ValueError(KS.COLLISION_MSG)
    strings = {}
    if m:
        strings = dict(zip(rep_keys.cpu().numpy().tolist(), KS.gather(rep_strs, table).to_pylist()))
    return DeviceColumn(keys, bitmap, None, None, strings)
