"""Dropna (reference: nvtabular/ops/dropna.py): ``df.dropna(subset=col_selector.names or None)``
with the rows renumbered from 0.

Rows of the whole frame the operator receives are dropped; only the selected columns are tested
(every column when the selector is empty).  A row is NA where a tested column is null (validity
bit 0, or NaN in a float column); a column with a pending FillMissing constant has no nulls, and
a list row is never NA.  The keep mask, its scan and the compaction of every column run on the
device (kernels_compact.py); dtypes do not change and validity buffers are compacted with the
values.
"""
from __future__ import annotations

from ..device import as_device_frame
from ..selector import ColumnSelector
from .base import Operator


class Dropna(Operator):
    accepts_datetime = True

    def transform(self, col_selector: ColumnSelector, df):
        from ..kernels_compact import dropna_frame

        frame, was_pandas = as_device_frame(df)
        names = col_selector.names if col_selector is not None else []
        out = dropna_frame(frame, [n for n in names if n in frame] or None)
        return out.to_pandas() if was_pandas else out
