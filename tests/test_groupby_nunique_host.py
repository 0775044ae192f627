"""Groupby(aggs="nunique") on the host side: the constructor takes it, the output schema names
`col + name_sep + "nunique"` as a scalar int32 column without the LIST tag, and what stays
refused stays refused.  No GPU."""
import numpy as np
import pytest


def _schema(cols):
    from nvtabular_amd.schema import ColumnSchema, Schema

    return Schema([ColumnSchema(c, dtype=dt) for c, dt in cols.items()])


def test_constructs_with_nunique():
    from nvtabular_amd import ops

    op = ops.Groupby(groupby_cols="k", aggs={"x": ["nunique", "count"]})
    assert op.conv_aggs == {"x": ["nunique", "count"]} and op.list_aggs == {}
    assert ops.Groupby(groupby_cols=["k"], aggs="nunique").conv_aggs == {"__all__": ["nunique"]}


def test_median_stays_refused():
    from nvtabular_amd import ops

    with pytest.raises(NotImplementedError):
        ops.Groupby(groupby_cols=["k"], aggs=["nunique", "median"])


@pytest.mark.parametrize("sep", ["_", "-"])
def test_output_schema(sep):
    from nvtabular_amd import ColumnSelector, ops
    from nvtabular_amd.schema import Tags

    op = ops.Groupby(groupby_cols="k", aggs={"x": ["nunique", "count"], "s": "nunique", "y": ["list", "nunique"]},
                     name_sep=sep)
    schema = _schema({"k": np.int64, "x": np.float64, "s": np.dtype("O"), "y": np.int64})
    out = op.compute_output_schema(schema, ColumnSelector(["k", "x", "s", "y"]))
    names = out.column_names
    assert names.index(f"x{sep}nunique") < names.index(f"x{sep}count")   # the order given
    for c in ("x", "s", "y"):
        col = out[f"{c}{sep}nunique"]
        assert col.dtype == np.int32, c
        assert not col.is_list and not col.is_ragged and Tags.LIST not in col.tags, c
    assert out[f"x{sep}count"].dtype == np.int32
    assert out[f"y{sep}list"].is_list


def test_datetime_columns_are_exempt_like_count():
    from nvtabular_amd import ColumnSelector, ops

    class Col:
        def __init__(self, logical):
            self.logical = logical

    frame = {"t": Col(np.dtype("datetime64[ns]")), "u": Col(np.dtype("datetime64[ns]")), "x": Col(None)}
    op = ops.Groupby(groupby_cols="k", aggs={"t": ["nunique", "count"], "u": ["nunique", "sum"], "x": "mean"})
    assert op.datetime_rejects(ColumnSelector(["k", "t", "u", "x"]), frame) == ["u"]
