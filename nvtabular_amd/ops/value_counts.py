"""ValueCount (reference: nvtabular/ops/value_counts.py): min and max row length of list columns.

fit = per partition ONE reduction launch (``nvt_list_len_minmax``) that folds min / max of
``offsets[i + 1] - offsets[i]`` of every selected list column into a small device accumulator;
columns that share an offsets tensor are reduced once per partition, non-list columns are skipped,
a partition of zero rows adds nothing.  ``fit_end`` reads the partitions' {min, max} rows back once,
folds them per column on the host and merges the ranks.
transform = identity; the fitted counts go into the output schema's ``value_count`` property.
"""
from __future__ import annotations

import torch

from ..device import as_device_frame
from ..selector import ColumnSelector
from .base import StatOperator


class ValueCount(StatOperator):
    def __init__(self):
        super().__init__()
        self.stats = {}

    _FOLD_EVERY = 1024   # partitions whose {min, max} rows are held on the device between folds

    def fit_begin(self, col_selector: ColumnSelector):
        return {"names": list(col_selector.names), "parts": [], "host": {}, "device": None}

    def fit_partition(self, state, col_selector, df):
        from ..kernels_list import list_len_minmax, new_len_acc

        frame, _ = as_device_frame(df)
        names = state["names"]
        seen, items, part = {}, [], None
        for i, name in enumerate(names):
            col = frame[name]
            if not col.is_list or len(col) == 0:
                continue
            if part is None:
                # this partition's own {min, max} rows: a shared offsets tensor is reduced once, into
                # the row of its first column, and stands for the other columns of THIS partition only
                part = new_len_acc(len(names), col.offsets.device)
                state["device"] = col.offsets.device
            key = (col.offsets.data_ptr(), col.offsets.numel())
            if key in seen:
                seen[key][1].append(i)
                continue
            seen[key] = (i, [i])
            items.append((col.offsets, part[i]))
        if part is None:
            return
        list_len_minmax(items)
        state["parts"].append((part, list(seen.values())))
        if len(state["parts"]) >= self._FOLD_EVERY:
            self._fold(state)

    @staticmethod
    def _fold(state):
        """The partitions' rows -> the host {column index: [min, max]}: ONE read-back."""
        parts, state["parts"] = state["parts"], []
        if not parts:
            return
        host = torch.stack([p for p, _ in parts]).cpu().tolist()
        acc = state["host"]
        for rows, (_, groups) in zip(host, parts):
            for first, members in groups:
                lo, hi = rows[first]
                for i in members:
                    cur = acc.get(i)
                    acc[i] = [lo, hi] if cur is None else [min(cur[0], lo), max(cur[1], hi)]

    def fit_end(self, state, col_selector):
        from .. import dist
        from ..kernels_list import INT64_MAX

        names = state["names"]
        self._fold(state)   # the fit's one read-back (one more per _FOLD_EVERY partitions)
        acc = state["host"]
        if dist.world_size() > 1:
            # (float64 for the collectives of dist.py: row lengths are exact there, and the empty
            # interval INT64_MAX / INT64_MIN of a column this rank never saw stays empty)
            dev = state["device"] or torch.device("cuda", torch.cuda.current_device())
            rows = [acc.get(i, [INT64_MAX, -INT64_MAX - 1]) for i in range(len(names))]
            t = torch.tensor(rows, dtype=torch.float64, device=dev)
            mn = dist.all_reduce_min(t[:, 0].contiguous()).cpu().tolist()
            mx = dist.all_reduce_max(t[:, 1].contiguous()).cpu().tolist()
            acc = {i: [mn[i], mx[i]] for i in range(len(names)) if mn[i] <= mx[i]}
        return {names[i]: {"value_count": {"min": int(lo), "max": int(hi)}}
                for i, (lo, hi) in sorted(acc.items())}

    def fit_finalize(self, stats):
        self.stats = stats

    def transform(self, col_selector: ColumnSelector, df):
        return df

    def clear(self):
        self.stats = {}

    def _compute_properties(self, col_schema, input_schema):
        new_schema = super()._compute_properties(col_schema, input_schema)
        stat = self.stats.get(col_schema.name, {"value_count": {"min": 0, "max": None}})
        return col_schema.with_properties({**new_schema.properties, **stat})

    def _compute_shape(self, col_schema, input_schema):
        vc = self.stats.get(col_schema.name, {}).get("value_count", {"min": 0, "max": None})
        return col_schema.with_shape(is_list=True, is_ragged=vc["min"] != vc["max"])
