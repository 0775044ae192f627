"""Filter (reference: nvtabular/ops/filter.py): drops the rows a predicate rejects.

``f`` receives a ``FilterFrameView`` of the frame: ``df["x"]`` and ``df.x`` are ``DeviceSeries``
(series.py), built lazily on first use, so list / string columns the predicate never touches are
only carried through; ``df[bool_series]`` stands for "these rows".  What ``f`` returns decides the
result, as in the reference:

* a bool ``DeviceSeries``, ``df[mask]``, or a bool device tensor of length n: the keep mask,
  compacted on the device (kernels_compact.py);
* anything else: ``ValueError``, at transform time.

A predicate that needs something only pandas offers (``df.s.str.startswith("a")``) raises
``HostFallback`` and is re-run on ``frame.to_pandas()``, as LambdaOp does: a bool Series it returns
is the keep mask (compacted on the device); a DataFrame is taken as-is, with the index renumbered.
``last_path`` records which route the last ``transform`` took ("device" / "host").
"""
from __future__ import annotations

import pandas as pd
import torch

from ..device import DeviceFrame, as_device_frame
from ..selector import ColumnSelector
from ..series import DeviceSeries, HostFallback
from .base import Operator


class _Rows:
    """``df[mask]`` inside a predicate: the rows where ``mask`` is True."""

    def __init__(self, mask: torch.Tensor):
        self.mask = mask


class FilterFrameView:
    """The ``df`` a Filter predicate receives on the device."""

    def __init__(self, frame: DeviceFrame):
        self._frame = frame
        self._series = {}

    def _column(self, name):
        s = self._series.get(name)
        if s is None:
            s = self._series[name] = DeviceSeries.from_column(self._frame[name], name)
        return s

    def __getitem__(self, key):
        if isinstance(key, str):
            if key not in self._frame:
                raise KeyError(key)
            return self._column(key)
        if isinstance(key, DeviceSeries):
            key = key.values
        if isinstance(key, torch.Tensor) and key.dtype == torch.bool and key.dim() == 1:
            return _Rows(key)
        raise HostFallback(f"frame indexing by {type(key).__name__}")

    def __getattr__(self, item):
        if item.startswith("_"):
            raise AttributeError(item)
        if item in self._frame:
            return self._column(item)
        raise HostFallback(f"DataFrame.{item}")

    def __contains__(self, name):
        return name in self._frame

    def __len__(self):
        return len(self._frame)

    @property
    def columns(self):
        return self._frame.columns


def _device_mask(res, n: int):
    """The keep mask a predicate's result stands for, or None when it is not a mask."""
    if isinstance(res, _Rows):
        mask = res.mask
    elif isinstance(res, DeviceSeries) and res.values.dtype == torch.bool:
        mask = res.values
    elif isinstance(res, torch.Tensor) and res.dtype == torch.bool and res.dim() == 1 and res.is_cuda:
        mask = res
    else:
        return None
    if mask.numel() != n:
        raise ValueError(f"Filter: mask of length {mask.numel()} for {n} rows")
    return mask


class Filter(Operator):
    accepts_datetime = True

    def __init__(self, f):
        super().__init__()
        if f is None:
            raise ValueError("f cannot be None. Filter op applies f to dataframe")
        self.f = f
        self.last_path = None

    def transform(self, col_selector: ColumnSelector, df):
        from ..kernels_compact import compact_frame

        frame, was_pandas = as_device_frame(df)
        n = len(frame)
        try:
            res = self.f(FilterFrameView(frame))
            mask = _device_mask(res, n)
            if mask is None:
                raise ValueError(f"Invalid output from filter op: {type(res)}")
            out = compact_frame(frame, mask)
            self.last_path = "device"
        except HostFallback:
            # the predicate is re-run from scratch on pandas (LambdaOp.transform does the same)
            host = frame.to_pandas()
            res = self.f(host)
            if isinstance(res, pd.DataFrame):
                out = DeviceFrame.from_pandas(res.reset_index(drop=True))
            elif isinstance(res, pd.Series) and res.dtype == bool:
                if len(res) != n:
                    raise ValueError(f"Filter: mask of length {len(res)} for {n} rows")
                mask = torch.from_numpy(res.to_numpy(dtype=bool).copy())
                out = compact_frame(frame, mask)
            else:
                raise ValueError(f"Invalid output from filter op: {type(res)}")
            self.last_path = "host"
        return out.to_pandas() if was_pandas else out
