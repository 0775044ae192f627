"""DropLowCardinality (reference: nvtabular/ops/drop_low_cardinality.py): drops the categorical
columns whose known cardinality -- ``properties["domain"]["max"]``, which Categorify writes once it
is fitted -- is below ``min_cardinality``.

The selector depends on fitted properties, so ``selector_from_fit`` asks Workflow.fit to refresh
the graph's schemas and selectors behind every fit phase: a transform that follows the fit at once
already drops the columns."""
from __future__ import annotations

from ..schema import Tags
from ..selector import ColumnSelector
from .base import Operator


class DropLowCardinality(Operator):
    accepts_datetime = True

    selector_from_fit = True

    def __init__(self, min_cardinality=4):
        super().__init__()
        self.min_cardinality = min_cardinality

    def transform(self, col_selector: ColumnSelector, df):
        return df[list(col_selector.names)]

    def compute_selector(self, input_schema, selector, parents_selector=None,
                         dependencies_selector=None) -> ColumnSelector:
        self._validate_matching_cols(input_schema, selector or ColumnSelector(), "compute_selector")
        keep = [col.name for col in input_schema if Tags.CATEGORICAL not in col.tags]
        for col in input_schema:
            if Tags.CATEGORICAL in col.tags:
                domain = col.properties.get("domain") or {}
                if domain.get("max") is None or domain["max"] >= self.min_cardinality:
                    keep.append(col.name)
        return ColumnSelector(keep)
