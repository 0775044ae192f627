"""DifferenceLag (reference: nvtabular/ops/difference_lag.py): the difference between a row and the
row ``shift`` places before it (after it for a negative shift) inside one partition -- the time
since a user's previous interaction.  The frame must already be grouped by ``partition_cols`` and
sorted inside the groups; ``Dataset.shuffle_by_keys(keys=partition_cols)`` brings all rows of a key
into one partition, in their original order.

For row i and j = i - shift the value is ``x[i] - x[j]`` when 0 <= j < n, every partition column is
non-null and equal at i and j and x is non-null at both; NaN otherwise.  The output is float32
without a validity bitmap.  To be bit-equal with pandas, int32 / int64 values are converted to
float64 before the subtraction and the difference is then rounded to float32; float64 subtracts in
float64 and rounds; float32 subtracts in float32.  A pending fill counts as the value.  Every
(column, shift) output of one ``transform`` comes from ONE launch (``nvt_difference_lag_many``).
"""
from __future__ import annotations

import numbers

import numpy
import torch

from ..device import DeviceColumn, DeviceFrame, as_device_frame
from ..schema import Tags
from ..selector import ColumnSelector
from .base import Operator

_TARGETS = (torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8)
MAX_PARTITION_COLS = 4


class DifferenceLag(Operator):
    def __init__(self, partition_cols, shift=1):
        super().__init__()
        if isinstance(partition_cols, str):
            partition_cols = [partition_cols]
        self.partition_cols = list(partition_cols)
        self.shifts = [int(shift)] if isinstance(shift, numbers.Integral) else [int(s) for s in shift]

    def transform(self, col_selector: ColumnSelector, df):
        from ..kernels_list import difference_lag

        frame, was_pandas = as_device_frame(df)
        n = len(frame)
        if len(self.partition_cols) > MAX_PARTITION_COLS:
            raise NotImplementedError(
                f"DifferenceLag over more than {MAX_PARTITION_COLS} partition columns")
        keys = []
        for name in self.partition_cols:
            col = frame[name]
            if col.is_list:
                raise TypeError(f"DifferenceLag: partition column '{name}' is a list column")
            col = col.materialize()
            keys.append((col.data, col.valid))   # (string columns compare by surrogate)
        cols, names = [], []
        for name in col_selector.names:
            col = frame[name]
            if col.is_list or col.strings is not None or col.data.dtype not in _TARGETS:
                kind = "list" if col.is_list else "string" if col.strings is not None else str(col.data.dtype)
                raise TypeError(f"DifferenceLag: cannot take differences of the {kind} column '{name}'")
            col = col.materialize()
            for shift in self.shifts:
                cols.append((col.data, col.valid, shift))
                names.append(self._column_name(name, shift))
        out = DeviceFrame()
        if cols:
            for name, t in zip(names, difference_lag(keys, cols, n)):
                out[name] = DeviceColumn(t)
        return out.to_pandas() if was_pandas else out

    @property
    def dependencies(self):
        return self.partition_cols

    def column_mapping(self, col_selector):
        column_mapping = {}
        for col in col_selector.names:
            for shift in self.shifts:
                column_mapping[self._column_name(col, shift)] = [col]
        return column_mapping

    def _compute_dtype(self, col_schema, input_schema):
        return col_schema.with_dtype(self.output_dtype, is_list=False, is_ragged=False)

    @property
    def output_tags(self):
        return [Tags.CONTINUOUS]

    @property
    def output_dtype(self):
        return numpy.float32

    def _column_name(self, col, shift):
        return f"{col}_difference_lag_{shift}"
