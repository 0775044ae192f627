"""Exact column medians on the device: the host driver of ``nvt_select_*`` (include/nvt_hip.h),
behind ``ops.FillMedian``.

``select_median_many`` takes, per column, the chunks (partitions) the column arrived in and runs
the MSD radix select over all of them without concatenating anything: per digit pass one
``nvt_select_hist_many`` launch per chunk index (every column's chunk in ONE launch), then one
``nvt_select_step``; behind pass 1 one ``nvt_select_finish`` for the columns whose rank bins fit
the candidate buffer.  The launch sequence does not depend on the data, so nothing is read back
until the end: one read-back of ``{m, key_lo, key_hi, path}`` per call.  32-bit columns are done
after 3 passes, 64-bit columns after 6; the launches of the later passes return at once for a
column that is done.

Across ranks the histograms (they carry ``m`` on pass 0) are summed with ``dist.all_reduce_sum``
between the last chunk of a pass and its step, and the candidate path is off (each rank would hold
only its own candidates): every rank steps to the same prefix and ends with the median of the
union.

Part of the host driver of the C ABI, with the facade's conventions: launches under
``kernels.LAUNCH_LOCK`` on torch's current stream, errors through ``_lib.check``, state from
torch's allocator."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

PATH_NONE, PATH_CAND, PATH_FULL = 0, _lib.SELECT_PATH_CAND, _lib.SELECT_PATH_FULL
_NP = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}
_BITS = {torch.int32: 32, torch.float32: 32, torch.int64: 64, torch.float64: 64}


def key_of(value, dtype) -> int:
    """The order-preserving unsigned key of ``value`` as a ``dtype`` (numpy) element: what the
    kernels compare.  Floats flip every bit of a negative value and the sign bit of the others
    (so -0.0 < +0.0 as keys), integers flip the sign bit."""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    u = int(np.array([value], dtype=dt).view(np.uint32 if bits == 32 else np.uint64)[0])
    top = 1 << (bits - 1)
    if dt.kind == "f" and u & top:
        return u ^ ((1 << bits) - 1)
    return u ^ top


def value_of(key: int, dtype):
    """The ``dtype`` element whose key is ``key`` (numpy scalar)."""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    top = 1 << (bits - 1)
    if dt.kind == "f" and not key & top:
        u = key ^ ((1 << bits) - 1)
    else:
        u = key ^ top
    return np.array([u], dtype=np.uint32 if bits == 32 else np.uint64).view(dt)[0]


def median_of(lo, hi) -> float:
    """The median of a column whose two middle values are ``lo <= hi`` (numpy scalars of the
    column's dtype): numpy's linear interpolation at t = 0.5, ``hi - (hi - lo) * 0.5`` -- the
    difference in the column's own type, the rest in float64, which is bit for bit what
    ``pandas.Series.quantile(0.5)`` returns for every dtype (``lo + (hi - lo) * 0.5`` is not)."""
    if lo == hi:
        return float(lo)
    with np.errstate(over="ignore"):
        diff = hi - lo
    return float(np.float64(hi) - np.float64(diff) * 0.5)


class SelectResult(tuple):
    """``(m, lo, hi, median)`` of one column: the participating rows, the two middle values (numpy
    scalars of the column's dtype; None when m == 0) and the median (NaN when m == 0).  Debug
    fields: ``path`` (PATH_CAND: resolved inside the candidate buffer behind pass 1; PATH_FULL:
    all the full passes; PATH_NONE: no rows) and the keys ``key_lo`` / ``key_hi``."""

    def __new__(cls, m, lo, hi, median, path=PATH_NONE, key_lo=None, key_hi=None):
        self = super().__new__(cls, (m, lo, hi, median))
        self.m, self.lo, self.hi, self.median = m, lo, hi, median
        self.path, self.key_lo, self.key_hi = path, key_lo, key_hi
        return self


def _fill_fits(dtype: torch.dtype, fill) -> bool:
    """An integer column takes its fill constant as an element of its own type."""
    if dtype.is_floating_point or fill is None:
        return True
    f = float(fill)
    info = torch.iinfo(dtype)
    return f == f and abs(f) <= 2.0 ** 53 and f == int(f) and info.min <= int(f) <= info.max


def _prepare(chunks):
    """[(data, valid, fill)] of one column -> the same with contiguous, 16-byte aligned data of one
    dtype the kernels take (bool / uint8 widened; an integer column whose pending fill is not an
    integer of its type becomes float64, as the filled column itself would)."""
    # (a NaN fill constant leaves the null rows null, and null rows do not take part)
    out = [(K.numeric(d), v, None if f is not None and float(f) != float(f) else f) for d, v, f in chunks]
    dts = {d.dtype for d, _, _ in out}
    if len(dts) > 1:
        raise TypeError(f"select_median_many: the chunks of a column have different dtypes {sorted(map(str, dts))}")
    if dts and not all(_fill_fits(d.dtype, f) for d, _, f in out):
        out = [(K.fill_normalize(d, v, f, False, 0.0, 1.0, torch.float64)[0], None, None) if d.numel()
               else (torch.empty(0, dtype=torch.float64, device=d.device), None, None) for d, v, f in out]
    for d, _, _ in out:
        if d.dtype not in _BITS:
            raise TypeError(f"unsupported column dtype {d.dtype}")
    return [(K.aligned(d), v, f) for d, v, f in out]


def select_median_many(chunks_per_column: Sequence[Sequence], allow_candidates: bool = True) -> List[SelectResult]:
    """chunks_per_column[c] = [(data, valid or None, fill or None)]: the chunks of column c, in
    any number and of any lengths (an empty list: a column without rows).  -> one SelectResult
    ``(m, lo, hi, median)`` per column.  With more than one rank: collective, every rank calls it
    with the same number of columns, and the results are those of the union of the ranks' rows."""
    from . import dist

    ncols = len(chunks_per_column)
    if ncols == 0:
        return []
    world = dist.world_size()
    cols = [_prepare(ch) for ch in chunks_per_column]
    dtypes: List[Optional[torch.dtype]] = [ch[0][0].dtype if ch else None for ch in cols]
    if world > 1:
        # a rank without partitions does not know its columns' dtypes: one MAX reduce of the codes
        dev = torch.device("cuda", torch.cuda.current_device())
        order = [torch.int32, torch.float32, torch.int64, torch.float64]
        code = torch.tensor([float(order.index(dt) + 1) if dt is not None else 0.0 for dt in dtypes],
                            dtype=torch.float64, device=dev)
        code = dist.all_reduce_max(code).cpu().tolist()
        for c, v in enumerate(code):
            agreed = order[int(v) - 1] if v >= 1 else None
            if dtypes[c] is not None and dtypes[c] != agreed:
                raise TypeError(f"select_median_many: column {c} is {dtypes[c]} here and {agreed} on another rank")
            dtypes[c] = agreed
    live = [c for c in range(ncols) if dtypes[c] is not None]
    results: List[Optional[SelectResult]] = [None] * ncols
    for c in range(ncols):
        if dtypes[c] is None:
            results[c] = SelectResult(0, None, None, float("nan"))
    if not live:
        return results
    _lib.require_gpu()
    lib = _lib.load()
    dev = next((ch[0][0].device for ch in cols if ch), torch.device("cuda", torch.cuda.current_device()))
    nlive = len(live)
    W = _lib.SELECT_STATE_WORDS
    nchunks = max(len(cols[c]) for c in live)
    npass = max(_BITS[dtypes[c]] for c in live) // 11 + 1     # 3 or 6
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        # (the candidate buffers are written before they are read: only the head needs zeroing)
        state = torch.empty(nlive, W, dtype=torch.int64, device=dev)
        head = torch.zeros(nlive, _lib.SELECT_ST_CAND, dtype=torch.int64)
        for i, c in enumerate(live):
            head[i, _lib.SELECT_ST_BITS] = _BITS[dtypes[c]]
            head[i, _lib.SELECT_ST_ALLOW_CAND] = 1 if (allow_candidates and world == 1) else 0
        state[:, :_lib.SELECT_ST_CAND] = head.to(dev)
        # descriptors of chunk index j of every column (a column with fewer chunks: n = 0)
        descs = []
        for j in range(nchunks):
            d = (_lib.SelectCol * nlive)()
            for i, c in enumerate(live):
                d[i].dtype = K.dtype_code(dtypes[c])
                if j < len(cols[c]):
                    data, valid, fill = cols[c][j]
                    d[i].x = data.data_ptr() if data.numel() else None
                    d[i].valid = K.ptr(valid)
                    d[i].n = data.numel()
                    d[i].has_fill = 0 if fill is None else 1
                    d[i].fill_val = 0.0 if fill is None else float(fill)
            descs.append(d)
        for p in range(npass):
            for d in descs:
                K.stat_add("select_hist_many")
                check(lib.nvt_select_hist_many(d, nlive, p, state.data_ptr(), stream), "nvt_select_hist_many")
            if world > 1:
                # A collective under LAUNCH_LOCK (6 per fit at the most, 32 KiB per column; staged
                # through the host under gloo): other threads' launches wait for it.  The lock is
                # kept because the state, the descriptors and the pass order belong to this one
                # launch sequence, as for the moments' all-reduce in Normalize.fit_end.
                hist = state[:, _lib.SELECT_ST_HIST:_lib.SELECT_ST_CAND].contiguous()
                state[:, _lib.SELECT_ST_HIST:_lib.SELECT_ST_CAND] = dist.all_reduce_sum(hist)
            check(lib.nvt_select_step(state.data_ptr(), nlive, p, stream), "nvt_select_step")
            if p == 1:
                check(lib.nvt_select_finish(state.data_ptr(), nlive, stream), "nvt_select_finish")
        K.stat_add("select_readback")
        host = K.read_back(state[:, :_lib.SELECT_ST_HIST].contiguous())   # the call's one read-back
    for i, c in enumerate(live):
        row = [int(v) & 0xFFFFFFFFFFFFFFFF for v in host[i].tolist()]
        m = row[_lib.SELECT_ST_M]
        if not row[_lib.SELECT_ST_DONE]:
            raise _lib.NvtHipError(f"select_median_many: column {c} was not resolved")
        if m == 0:
            results[c] = SelectResult(0, None, None, float("nan"))
            continue
        np_dt = _NP[dtypes[c]]
        klo, khi = row[_lib.SELECT_ST_KEY_LO], row[_lib.SELECT_ST_KEY_HI]
        lo, hi = value_of(klo, np_dt), value_of(khi, np_dt)
        results[c] = SelectResult(m, lo, hi, median_of(lo, hi), row[_lib.SELECT_ST_PATH], klo, khi)
    return results
