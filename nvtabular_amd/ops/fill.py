"""FillMissing / FillMedian (reference: nvtabular/ops/fill.py:25-80, 83-146).

On a DeviceFrame the fill is *deferred*: the column records the constant and
every downstream kernel (moments, normalize, encode) takes it as a parameter, so
FillMissing >> Normalize is one pass over the data instead of the reference's
two (fill.py:55 then normalize.py:80).  The fill is materialised (one
``nvt_fill_normalize`` pass, do_norm=0) only if the filled column itself is output.

FillMedian fits the exact median of every column (``kernels_select``: an MSD radix select on the
device, no sort) and then fills exactly as FillMissing does with that constant.
"""
from __future__ import annotations

import torch

from .. import kernels as K
from ..device import DeviceColumn, as_device_frame
from ..selector import ColumnSelector
from .base import Operator, StatOperator


def _fill_constant(frame, name, col, value, add_binary_cols):
    """``frame[name]`` = ``col`` with its null rows taking ``value``.  Without binary columns the
    fill is deferred (unless an earlier fill already decided the null rows); with them one
    ``nvt_fill_normalize`` pass writes the filled column and ``<name>_filled``, and an integer
    column whose constant is not integral becomes float64."""
    if add_binary_cols:
        data = K.numeric(col.data)  # bool / uint8 -> int64
        out_dt = data.dtype
        fv = float(value)
        if out_dt in (torch.int32, torch.int64) and fv != int(fv):
            out_dt = torch.float64
        out, filled = K.fill_normalize(data, col.valid, fv, False, 0.0, 1.0, out_dt,
                                       want_filled_mask=True)
        frame[f"{name}_filled"] = DeviceColumn(filled)
        frame[name] = DeviceColumn(out, None, col.offsets)
    else:
        pending = col.shallow_copy()
        if pending.fill is None:  # an earlier fill already decided null rows
            pending.fill = value
        frame[name] = pending


class _FilledColumns:
    """The ``<col>_filled`` bool columns of an operator with ``add_binary_cols`` (fill.py:67-78,
    135-146)."""

    def column_mapping(self, col_selector):
        mapping = super().column_mapping(col_selector)
        for name in col_selector.names:
            if self.add_binary_cols:
                mapping[f"{name}_filled"] = [name]
        return mapping

    def _compute_dtype(self, col_schema, input_schema):
        col_schema = super()._compute_dtype(col_schema, input_schema)
        if col_schema.name.endswith("_filled"):
            col_schema = col_schema.with_dtype(bool)
        return col_schema


class FillMissing(_FilledColumns, Operator):
    def __init__(self, fill_val=0, add_binary_cols=False):
        super().__init__()
        self.fill_val = fill_val
        self.add_binary_cols = add_binary_cols

    def transform(self, col_selector: ColumnSelector, df):
        frame, was_pandas = as_device_frame(df)
        for name in col_selector.names:
            _fill_constant(frame, name, frame[name], self.fill_val, self.add_binary_cols)
        return frame.to_pandas() if was_pandas else frame


class FillMedian(_FilledColumns, StatOperator):
    """Replace missing values with the column's median (fill.py:83-146).

    The fitted value is the exact median of the non-null, non-NaN rows, bit for bit
    ``df[col].dropna().quantile(0.5, interpolation="linear")`` -- what the reference's tests pin
    it to (its own fit is dask's approximate quantile).  Null rows upstream of which a FillMissing
    is pending take part with that constant.

    Memory: an exact median needs every value at the end of the fit, so ``fit_partition`` keeps
    references to each selected column's (data, validity, fill) tensors of every partition until
    ``fit_end``.  No copy is made, but the partitions' columns stay alive for the duration of the
    fit: the selected columns of the whole dataset (of this rank's shard) must fit in device
    memory, 8 bytes per row for a 64-bit column.  ``fit_end`` reads them 2 (candidate path) to 3
    / 6 times (32- / 64-bit columns) and drops the references.
    """

    def __init__(self, add_binary_cols=False):
        super().__init__()
        self.add_binary_cols = add_binary_cols
        self.medians = {}

    def fit_begin(self, col_selector: ColumnSelector):
        return {"names": list(col_selector.names), "chunks": [[] for _ in col_selector.names]}

    def fit_partition(self, state, col_selector, df):
        frame, _ = as_device_frame(df)
        for chunks, name in zip(state["chunks"], state["names"]):
            col = frame[name]
            chunks.append((col.data, col.valid, col.fill))

    def fit_end(self, state, col_selector):
        from .. import kernels_select as KS

        res = KS.select_median_many(state["chunks"])
        state["chunks"] = []
        return {name: r.median for name, r in zip(state["names"], res)}

    def fit_finalize(self, stats):
        # a {column: median} dict, or the reference's pandas Series indexed by column (fill.py:122-126)
        names = stats.keys() if isinstance(stats, dict) else list(stats.index)
        for col in names:
            self.medians[col] = float(stats[col])

    def transform(self, col_selector: ColumnSelector, df):
        if not self.medians:
            raise RuntimeError("need to call 'fit' before running transform")
        frame, was_pandas = as_device_frame(df)
        for name in col_selector.names:
            col = frame[name]
            med = self.medians[name]
            if self.add_binary_cols and col.fill is not None:
                # an earlier fill already decided the null rows (the reference's FillMissing has
                # filled them by now, fill.py:49-57): they keep its constant and are not "filled" here
                col = col.materialize()
            if med != med:  # no participating rows: nothing to fill with
                if self.add_binary_cols:
                    data = K.numeric(col.data)
                    _, filled = K.fill_normalize(data, col.valid, None, False, 0.0, 1.0, data.dtype,
                                                 want_filled_mask=True)
                    frame[f"{name}_filled"] = DeviceColumn(filled)
                    frame[name] = col
                continue
            _fill_constant(frame, name, col, med, self.add_binary_cols)
        return frame.to_pandas() if was_pandas else frame

    def clear(self):
        self.medians = {}
