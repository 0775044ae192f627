"""ColumnSimilarity (reference: nvtabular/ops/column_similarity.py): for every pair of id columns
``[["a", "b"]]`` the tf-idf, cosine or inner-product similarity of row ``a[i]`` of the left feature
matrix and row ``b[i]`` of the right one, as float64 ``a_b_sim``.

The feature matrices (torch sparse COO / CSR tensors, scipy.sparse matrices or ``(row, col, data,
shape)`` tuples; unsorted entries, duplicates and stored zeros allowed) are weighted entry by entry,
ordered and coalesced on the device on the first ``transform`` (kernels_similarity.py) and stay
resident.  ``right_features=None`` uses the prepared left matrix for both sides.  The id columns are
flat int32 / int64 columns; a null id or an id outside ``[0, shape[0])`` gives NaN and is never
dereferenced, a feature row without entries gives 0.0.  ``on_device`` is accepted for API
compatibility: there is no host path."""
from __future__ import annotations

import numpy
import torch

from ..device import DeviceColumn, DeviceFrame, as_device_frame
from ..schema import Tags
from ..selector import ColumnSelector
from .base import Operator


def _pairs(col_selector):
    groups = col_selector.grouped_names
    bad = [g for g in groups if isinstance(g, str) or len(g) != 2]
    if bad:
        raise ValueError(f"ColumnSimilarity takes groups of exactly two columns ([['a', 'b']]), not {bad}")
    return [tuple(g) for g in groups]


class ColumnSimilarity(Operator):
    def __init__(self, left_features, right_features=None, metric="tfidf", on_device=True):
        super().__init__()
        from .. import kernels_similarity as KS

        if metric not in KS.METRICS:
            raise ValueError(f"unknown distance metric {metric}")
        KS.check_features(left_features)   # TypeError / ValueError now, not on the first partition
        if right_features is not None:
            KS.check_features(right_features)
        self.metric = metric
        self.left_features = left_features
        self.right_features = right_features
        self.on_device = on_device
        self._prepared = None

    def _features(self, device):
        if self._prepared is None:   # (transform runs under LAUNCH_LOCK: two threads prepare once)
            from .. import kernels_similarity as KS

            left = KS.prepare(self.left_features, self.metric, device)
            right = left if self.right_features is None else KS.prepare(self.right_features, self.metric, device)
            self._prepared = (left, right)
        return self._prepared

    @staticmethod
    def _ids(frame, name) -> DeviceColumn:
        col = frame[name]
        if col.fill is not None:
            col = col.materialize()
        if col.is_list or col.strings is not None or col.logical is not None or \
                col.dtype not in (torch.int32, torch.int64):
            kind = "list" if col.is_list else "string" if col.strings is not None else str(col.logical or col.dtype)
            raise TypeError(f"ColumnSimilarity: column '{name}' is a {kind} column; the id columns are flat "
                            f"int32 / int64 columns such as Categorify's output")
        return col

    def transform(self, col_selector: ColumnSelector, df):
        from .. import kernels_similarity as KS

        frame, was_pandas = as_device_frame(df)
        out = DeviceFrame()
        for a, b in _pairs(col_selector):
            ca, cb = self._ids(frame, a), self._ids(frame, b)
            left, right = self._features(ca.data.device)
            out[f"{a}_{b}_sim"] = DeviceColumn(KS.row_similarity(ca.data, ca.valid, cb.data, cb.valid, left, right))
        return out.to_pandas() if was_pandas else out

    def compute_selector(self, input_schema, selector, parents_selector=None, dependencies_selector=None):
        sel = parents_selector or ColumnSelector()
        self._validate_matching_cols(input_schema, sel, "computing input selector")
        return sel

    def column_mapping(self, col_selector):
        return {f"{a}_{b}_sim": [a, b] for a, b in _pairs(col_selector)}

    def _compute_dtype(self, col_schema, input_schema):
        return col_schema.with_dtype(numpy.float64, is_list=False, is_ragged=False)

    def _compute_tags(self, col_schema, input_schema):
        return col_schema.with_tags([Tags.CONTINUOUS])

    def _compute_properties(self, col_schema, input_schema):
        return col_schema
