"""Shared by ReduceDtypeSize and DataStats: the streaming fit around ``K.col_profile_many`` (one
launch per partition for every profiled column, accumulators folded on the device), the cross-rank
reduction, and the small pieces of host arithmetic that finish the statistics."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import kernels as K

INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
_INT_DTYPES = (np.int8, np.int16, np.int32, np.int64)
_PROFILED = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool)


def reduced_dtype(dtype, lo, hi, float_dtype=np.float32) -> np.dtype:
    """The dtype ReduceDtypeSize gives a column of ``dtype`` whose valid values span [lo, hi]: the
    first of int8 / int16 / int32 / int64 that holds both ends (signed integers), ``float_dtype``
    (floats); unchanged for anything else and for a column without a valid value (lo / hi None or
    NaN)."""
    dtype = np.dtype(dtype)
    if lo is None or hi is None or lo != lo or hi != hi:
        return dtype
    if dtype.kind == "f":   # (never wider than the input, like the integers below)
        return np.dtype(float_dtype) if np.dtype(float_dtype).itemsize < dtype.itemsize else dtype
    if dtype.kind != "i":
        return dtype
    for cand in _INT_DTYPES:
        info = np.iinfo(cand)
        if lo >= info.min and hi <= info.max:
            return np.dtype(cand) if np.dtype(cand).itemsize < dtype.itemsize else dtype
    return dtype


def per_nan(valid: int, rows: int) -> float:
    """Percentage of missing rows, evaluated as the reference does (data_stats.py:90) in float64."""
    if rows == 0:
        return float("nan")
    return float(100 * (1 - np.float64(valid) / np.float64(rows)))


def length_stats(pairs):
    """(min, max, mean, std) of string lengths from [(length, count)] -- each distinct string's
    length weighted by its rows; NaN for an empty list.  std as moments.py:89-116 (ddof = 1)."""
    from .normalize import finalize_moments

    pairs = [(int(l), int(c)) for l, c in pairs if c > 0]
    if not pairs:
        nan = float("nan")
        return nan, nan, nan, nan
    n = sum(c for _, c in pairs)
    total = math.fsum(float(l) * c for l, c in pairs)
    sq = math.fsum(float(l) * l * c for l, c in pairs)
    mean, _, std = finalize_moments(n, total, sq)
    return min(l for l, _ in pairs), max(l for l, _ in pairs), mean, std


def f64_order_key(bits: torch.Tensor) -> torch.Tensor:
    """int64 bit patterns of float64 values <-> int64 keys in the order of the values (-0.0 below
    +0.0): the magnitude bits of a negative value flipped.  Its own inverse."""
    return bits ^ ((bits >> 63) & INT64_MAX)


def extrema_to_keys(ext: torch.Tensor, is_float: torch.Tensor):
    """[k, 2] int64 {min, max} words of a profile accumulator -> (lo, hi) int64 keys that an
    integer MIN / MAX reduction folds exactly: integer rows as they are, float rows (``is_float``,
    bool [k]) as order keys with NaN (nothing seen) -> the empty markers INT64_MAX / INT64_MIN."""
    fl = is_float.unsqueeze(1)
    empty = fl & torch.isnan(ext.view(torch.float64))
    keys = torch.where(fl, f64_order_key(ext), ext)
    marks = torch.tensor([INT64_MAX, INT64_MIN], dtype=torch.int64, device=ext.device).expand_as(keys)
    keys = torch.where(empty, marks, keys)
    return keys[:, 0].contiguous(), keys[:, 1].contiguous()


def keys_to_extrema(lo: torch.Tensor, hi: torch.Tensor, is_float: torch.Tensor) -> torch.Tensor:
    """Inverse of ``extrema_to_keys``: [k, 2] int64 words (float rows: float64 bits, NaN = empty)."""
    keys = torch.stack([lo, hi], dim=1)
    marks = torch.tensor([INT64_MAX, INT64_MIN], dtype=torch.int64, device=keys.device).expand_as(keys)
    nan = torch.full_like(keys, 0).view(torch.float64).fill_(float("nan")).view(torch.int64)
    fl = is_float.unsqueeze(1)
    as_float = torch.where(keys == marks, nan, f64_order_key(keys))
    return torch.where(fl, as_float, keys)


def merge_ranks(acc: torch.Tensor, is_float) -> torch.Tensor:
    """A profile accumulator ([k, PROFILE_WORDS] int64) reduced over the ranks: counts and sums
    added, extrema by MIN / MAX -- all of them as int64 keys, so integer extrema stay exact."""
    from .. import dist

    if dist.world_size() == 1 or acc.numel() == 0:
        return acc
    fl = torch.tensor(list(is_float), dtype=torch.bool, device=acc.device)
    counts = dist.all_reduce_sum(acc[:, 0:2].contiguous())
    sums = dist.all_reduce_sum(acc[:, 4:6].contiguous().view(torch.float64))
    lo, hi = extrema_to_keys(acc[:, 2:4].contiguous(), fl)
    ext = keys_to_extrema(dist.all_reduce_min(lo), dist.all_reduce_max(hi), fl)
    return torch.cat([counts, ext, sums.view(torch.int64)], dim=1)


class ProfileFit:
    """Streaming state: one accumulator row per profiled column.  A column's dtype is taken from
    the first partition that holds it; string and datetime columns and dtypes outside
    ``dtypes_taken`` are left out (``dtypes[name]`` stays None)."""

    def __init__(self, names, leaves_of_lists=False, dtypes_taken=_PROFILED, device=None):
        self.names = list(names)
        self.leaves = leaves_of_lists
        self.taken = tuple(dtypes_taken)
        self.dtypes = {n: None for n in self.names}   # torch dtype of the data as profiled
        self.acc = None
        self.rows = {}
        self.device = device

    def _begin(self, frame):
        for n in self.names:
            col = frame[n]
            self.device = col.data.device
            if col.strings is None and col.logical is None and col.data.dtype in self.taken:
                self.dtypes[n] = col.data.dtype
        self._allocate()

    def _allocate(self):
        live = [n for n in self.names if self.dtypes[n] is not None]
        self.rows = {n: i for i, n in enumerate(live)}
        device = self.device or torch.device("cuda", torch.cuda.current_device())
        self.acc = K.new_profile_acc([self.profiled_dtype(n) for n in live], device)

    def partition(self, frame):
        if self.acc is None:
            self._begin(frame)
        items = []
        for n, i in self.rows.items():
            col = frame[n]
            if col.is_list and not self.leaves:
                raise NotImplementedError(f"column {n!r}: list columns are not profiled")
            if col.fill is not None:
                col = col.materialize()
            if col.data.dtype != self.dtypes[n]:
                raise TypeError(f"column {n!r}: dtype changed from {self.dtypes[n]} to {col.data.dtype} "
                                "between partitions")
            items.append((col.data, col.valid, self.acc[i]))
        K.col_profile_many(items)   # every column of the partition: ONE launch

    def profiled_dtype(self, name):
        """dtype of the accumulator row of ``name`` (bool / uint8 are profiled as int64)."""
        dt = self.dtypes[name]
        return torch.int64 if dt in (torch.bool, torch.uint8) else dt

    def reduced(self):
        """(names, accumulator dtypes, [k, PROFILE_WORDS] accumulator) after the cross-rank
        reduction.  COLLECTIVE: a rank that received no partition has seen no column, so the
        profiled dtypes are agreed first and that rank joins the reductions with an empty
        accumulator -- every rank makes the same all-reduces."""
        from .. import dist

        if dist.world_size() > 1:
            mine = None if self.acc is None else {n: str(dt).replace("torch.", "") for n, dt in self.dtypes.items()
                                                  if dt is not None}
            agreed = dist.merge_host_dicts(mine) or {}
            if self.acc is None:
                for n in self.names:
                    self.dtypes[n] = getattr(torch, agreed[n]) if n in agreed else None
                self._allocate()
        if self.acc is None or not self.rows:
            return [], [], None
        live = list(self.rows)
        dts = [self.profiled_dtype(n) for n in live]
        return live, dts, merge_ranks(self.acc, [K.profile_is_float(d) for d in dts])

    def end(self):
        """{name: dict(rows, valid, min, max, sum, sumsq)} after the cross-rank reduction: the ONE
        read-back of the fit."""
        live, dts, acc = self.reduced()
        if acc is None:
            return {}
        host = K.read_back(acc.contiguous().view(-1)).reshape(-1, K.PROFILE_WORDS)
        return dict(zip(live, K.profile_rows(host, dts)))
