"""ReduceDtypeSize (reference: nvtabular/ops/reduce_dtype_size.py): integer columns become the
narrowest of int8 / int16 / int32 / int64 that holds their fitted range, float columns become
``float_dtype``.

fit  = per partition ONE ``nvt_col_profile_many`` launch for all selected columns (exact int64
       min / max folded on the device), one read-back in ``fit_end``.
transform = ONE ``nvt_cast_many`` launch; the validity bitmap and list offsets are shared with the
       input.  A value outside the fitted range wraps as ``numpy.ndarray.astype`` wraps it.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K
from ..device import DeviceColumn, as_device_frame, numpy_dtype, torch_dtype
from ..selector import ColumnSelector
from ._profile import ProfileFit, reduced_dtype
from .base import StatOperator


class ReduceDtypeSize(StatOperator):
    accepts_datetime = True

    def __init__(self, float_dtype=np.float32):
        super().__init__()
        self.float_dtype = float_dtype
        self.ranges = {}
        self.dtypes = {}

    def fit_begin(self, col_selector: ColumnSelector):
        # (bool / uint8 and anything else reduced_dtype leaves alone is not read at all)
        return ProfileFit(col_selector.names, leaves_of_lists=True,
                          dtypes_taken=(torch.int32, torch.int64, torch.float32, torch.float64))

    def fit_partition(self, state, col_selector, df):
        frame, _ = as_device_frame(df)
        state.partition(frame)

    def fit_end(self, state, col_selector):
        # (the input dtype is the one the data had during the fit, not the schema's)
        return {name: (numpy_dtype(state.dtypes[name]), st["min"], st["max"])
                for name, st in state.end().items()}

    def fit_finalize(self, stats):
        for name, (dtype, lo, hi) in stats.items():
            self.ranges[name] = (lo, hi)
            self.dtypes[name] = reduced_dtype(dtype, lo, hi, self.float_dtype)

    def clear(self):
        self.ranges = {}
        self.dtypes = {}

    def transform(self, col_selector: ColumnSelector, df):
        frame, was_pandas = as_device_frame(df)
        names, items = [], []
        for name in col_selector.names:
            if name not in self.dtypes:
                continue
            col = frame[name]
            if col.fill is not None:
                col = col.materialize()
            names.append((name, col))
            items.append((col.data, torch_dtype(self.dtypes[name])))
        for (name, col), out in zip(names, K.cast_many(items)):   # every column: ONE launch
            frame[name] = DeviceColumn(out, col.valid, col.offsets, None, col.strings)
        return frame.to_pandas() if was_pandas else frame

    def compute_output_schema(self, input_schema, col_selector):
        out = super().compute_output_schema(input_schema, col_selector)
        if not self.dtypes:
            return out
        from ..schema import Schema

        return Schema([c.with_dtype(self.dtypes[c.name]) if c.name in self.dtypes else c for c in out])
