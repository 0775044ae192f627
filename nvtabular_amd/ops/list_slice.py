"""ListSlice (reference: nvtabular/ops/list_slice.py): slices every row of a list column.

Row i of the output is exactly Python's ``row[start:end]``: negative indices count from the row's
end and everything is clamped to the row.  With ``pad=True`` each row is then extended to
``max_elements`` leaves with ``pad_value`` cast to the leaf dtype; padded leaves are valid.

Constructor, as in the reference: ``ListSlice(10)`` is ``[0:10]``, ``ListSlice(1, 11)`` skips the
first leaf, ``ListSlice(-10)`` keeps the last ten; ``max_elements`` is ``-start`` for
``start < 0 <= end`` (or no end) and ``end - start`` otherwise.  Two cases the reference leaves
ill-defined are decided here:

* a slice without a length bound -- ``ListSlice(0)`` with no end, or ``start >= 0 > end`` such as
  ``ListSlice(1, -1)`` -- has ``max_elements = None`` and ``value_count.max = None``; with
  ``pad=True`` the constructor raises ``ValueError`` (there is no row width to pad to);
* ``end <= start`` with the same sign: every row is empty, as Python slicing gives
  (``max_elements = 0``).

The leaves move on the device (kernels_list.py): columns that share one offsets tensor are planned
once and keep sharing one, validity bitmaps are carried bit-exactly, a pending fill and a string
column's dictionary are carried over.  ``pad=True`` on string leaves raises ``NotImplementedError``.
"""
from __future__ import annotations

from ..device import DeviceFrame, as_device_frame
from ..schema import Tags
from ..selector import ColumnSelector
from .base import Operator

_INT64_MAX = (1 << 63) - 1


class ListSlice(Operator):
    def __init__(self, start, end=None, pad=False, pad_value=0.0):
        super().__init__()
        self.start = int(start)
        self.end = None if end is None else int(end)
        self.pad = bool(pad)
        self.pad_value = pad_value

        if self.start > 0 and self.end is None:
            self.end = self.start
            self.start = 0
        open_end = self.end is None
        if open_end:
            self.end = _INT64_MAX

        if (self.start >= 0 and open_end) or (self.start >= 0 > self.end):
            self.max_elements = None   # no bound on the sliced length
        elif self.start < 0 and (open_end or self.end >= 0):
            self.max_elements = -self.start
        else:
            self.max_elements = max(self.end - self.start, 0)
        if self.pad and self.max_elements is None:
            raise ValueError(
                f"ListSlice(start={start}, end={end}, pad=True): the slice has no length bound to pad to")

    def transform(self, col_selector: ColumnSelector, df):
        from ..kernels_list import slice_lists

        frame, was_pandas = as_device_frame(df)
        cols = slice_lists(frame, col_selector.names, self.start, self.end,
                           self.max_elements if self.pad else None, self.pad_value)
        out = DeviceFrame({name: cols[name] for name in col_selector.names})
        return out.to_pandas() if was_pandas else out

    def _compute_dtype(self, col_schema, input_schema):
        col_schema = super()._compute_dtype(col_schema, input_schema)
        return col_schema.with_dtype(col_schema.dtype, is_list=True, is_ragged=not self.pad)

    @property
    def output_properties(self):
        return {"value_count": {"min": self.max_elements if self.pad else 0, "max": self.max_elements}}

    @property
    def output_tags(self):
        return [Tags.LIST]
