"""ops.FillMedian through the operator and workflow layer, against pandas on the host:
``df[col].dropna().quantile(0.5, interpolation="linear")`` for the fitted medians (bit-equal) and
``df[col].fillna(median)`` for the output (reference: nvtabular/ops/fill.py:83-146,
tests/unit/workflow/test_workflow.py:537-546)."""
import math

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu


def _median_op(wf):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    return next(n.op for n in nvt.workflow.iter_nodes(wf.output_node) if isinstance(n.op, ops.FillMedian))


def _pd_median(s):
    return float(s.dropna().quantile(0.5, interpolation="linear"))


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(21)
    n = 5000
    df = pd.DataFrame({
        "f64": rng.normal(10.0, 3.0, n),
        "f32": rng.normal(-2.0, 50.0, n).astype(np.float32),
    })
    for c in ("f64", "f32"):
        df.loc[rng.random(n) < 0.1, c] = np.nan
    null = rng.random(n) < 0.1
    if (n - null.sum()) % 2:
        null[np.flatnonzero(~null)[0]] = True
    ints = np.zeros(n, dtype=np.int64)
    ints[~null] = rng.permutation(int((~null).sum()))     # distinct, even count: a fractional median
    df["i64"] = pd.array(ints, dtype="Int64")
    df.loc[null, "i64"] = pd.NA
    meds = {c: _pd_median(df[c]) for c in df.columns}
    assert meds["i64"] != int(meds["i64"])
    return df, meds


def test_reference_workflow_frame():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df = pd.DataFrame({"x": [0, 1, 2, None, 0, 1, 2], "y": [None, 3, 4, 5, 3, 4, 5]})
    wf = nvt.Workflow(["x", "y"] >> ops.FillMedian())
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    op = _median_op(wf)
    assert op.medians == {"x": 1.0, "y": 4.0}
    assert out["x"].tolist() == [0, 1, 2, 1, 0, 1, 2]
    assert out["y"].tolist() == [4, 3, 4, 5, 3, 4, 5]
    assert not out.isna().any().any()


@pytest.mark.parametrize("add_binary_cols", [False, True])
def test_mixed_frame_against_pandas(frame, add_binary_cols):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df, meds = frame
    cols = ["f64", "f32", "i64"]
    wf = nvt.Workflow(cols >> ops.FillMedian(add_binary_cols=add_binary_cols))
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    op = _median_op(wf)
    for c in cols:
        assert op.medians[c] == meds[c], (c, float.hex(op.medians[c]), float.hex(meds[c]))
    np.testing.assert_array_equal(out["f64"].to_numpy(), df["f64"].fillna(meds["f64"]).to_numpy())
    assert out["f32"].dtype == np.float32
    np.testing.assert_array_equal(out["f32"].to_numpy(), df["f32"].fillna(meds["f32"]).to_numpy())
    # the int64 column with a fractional median comes out float64
    assert out["i64"].dtype == np.float64
    np.testing.assert_array_equal(out["i64"].to_numpy(),
                                  df["i64"].astype("float64").fillna(meds["i64"]).to_numpy())
    for c in cols:
        if add_binary_cols:
            assert out[f"{c}_filled"].dtype == bool
            assert int(out[f"{c}_filled"].sum()) == int(df[c].isna().sum())
            np.testing.assert_array_equal(out[f"{c}_filled"].to_numpy(), df[c].isna().to_numpy())
        else:
            assert f"{c}_filled" not in out.columns
    assert wf.output_schema.column_names == (cols + [f"{c}_filled" for c in cols] if add_binary_cols else cols)


def test_integral_median_keeps_the_integer_type():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df = pd.DataFrame({"k": pd.array([5, None, 7, 7, None, 9, 1], dtype="Int64")})
    for flag in (False, True):
        wf = nvt.Workflow(["k"] >> ops.FillMedian(add_binary_cols=flag))
        out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
        assert _median_op(wf).medians == {"k": 7.0}
        assert out["k"].dtype == np.int64 and out["k"].tolist() == [5, 7, 7, 7, 7, 9, 1]


def test_fill_median_then_normalize(frame):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df, meds = frame
    cols = ["f64", "f32", "i64"]
    wf = nvt.Workflow(cols >> ops.FillMedian() >> ops.Normalize())
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    norm = next(n.op for n in nvt.workflow.iter_nodes(wf.output_node) if isinstance(n.op, ops.Normalize))
    for c in cols:
        # (pandas keeps a float32 column float32 through fillna and (x - mean) / std)
        filled = df[c].fillna(meds[c]) if c == "f32" else df[c].astype("float64").fillna(meds[c])
        mean, std = float(filled.astype("float64").mean()), float(filled.astype("float64").std())
        assert abs(norm.means[c] - mean) <= 1e-6 * max(1.0, abs(mean)), c
        assert abs(norm.stds[c] - std) <= 1e-6 * std, c
        # statistics within 1e-6 relative move an output by about 1e-6 of |x - mean| / std + 1e-6
        np.testing.assert_allclose(out[c].to_numpy().astype(np.float64),
                                   ((filled - mean) / std).to_numpy().astype(np.float64),
                                   rtol=1e-6, atol=1e-6, err_msg=c)


def test_three_partitions_give_the_medians_of_the_whole_frame(frame):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df, meds = frame
    cols = ["f64", "f32", "i64"]
    wf = nvt.Workflow(cols >> ops.FillMedian())
    ds = nvt.Dataset(df, npartitions=3)
    assert ds.npartitions == 3
    wf.fit(ds)
    assert _median_op(wf).medians == meds
    # partitions of unequal length, handed over as frames
    parts = [df.iloc[:700], df.iloc[700:701], df.iloc[701:]]
    wf.fit(nvt.Dataset([p.reset_index(drop=True) for p in parts]))
    assert _median_op(wf).medians == meds


def test_reference_style_fit_and_finalize(frame):
    from nvtabular_amd import ops
    from nvtabular_amd.selector import ColumnSelector

    df, meds = frame
    op = ops.FillMedian()
    op.fit_finalize(op.fit(ColumnSelector(["f64", "f32"]), [df.iloc[:2000], df.iloc[2000:]]).compute())
    assert op.medians == {"f64": meds["f64"], "f32": meds["f32"]}
    # what the reference's dask quantile hands over: a Series indexed by column
    op2 = ops.FillMedian()
    op2.fit_finalize(pd.Series({"f64": 1.5, "f32": np.float32(2.0)}))
    assert op2.medians == {"f64": 1.5, "f32": 2.0} and all(type(v) is float for v in op2.medians.values())


def test_pending_fill_missing_takes_part():
    """FillMissing >> FillMedian: the null rows count with the constant, and keep it."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df = pd.DataFrame({"x": [1.0, None, None, None, 9.0, 2.0]})
    wf = nvt.Workflow(["x"] >> ops.FillMissing(fill_val=100.0) >> ops.FillMedian())
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    assert _median_op(wf).medians == {"x": _pd_median(df["x"].fillna(100.0))} == {"x": 54.5}
    assert out["x"].tolist() == [1.0, 100.0, 100.0, 100.0, 9.0, 2.0]


def test_pending_fill_missing_with_binary_cols():
    """FillMissing >> FillMedian(add_binary_cols=True): the reference's FillMissing has filled the
    nulls before FillMedian sees the frame (fill.py:49-57), so they keep its constant and
    ``<col>_filled`` (``isna()`` of what FillMedian is given) is False everywhere."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df = pd.DataFrame({"x": [1.0, None, None, None, 9.0, 2.0],
                       "k": pd.array([4, None, 6, None, None, 8], dtype="Int64")})
    wf = nvt.Workflow(["x", "k"] >> ops.FillMissing(fill_val=100) >> ops.FillMedian(add_binary_cols=True))
    out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    exp = df.astype("float64").fillna(100.0)
    meds = {c: _pd_median(exp[c]) for c in exp.columns}
    assert _median_op(wf).medians == meds == {"x": 54.5, "k": 54.0}
    assert out["x"].tolist() == exp["x"].tolist() and out["k"].tolist() == exp["k"].tolist()
    assert out["x_filled"].tolist() == [False] * 6 and out["k_filled"].tolist() == [False] * 6
    assert out["x_filled"].dtype == bool


def test_errors_and_state():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.selector import ColumnSelector

    op = ops.FillMedian()
    with pytest.raises(RuntimeError, match="need to call 'fit' before running transform"):
        op.transform(ColumnSelector(["x"]), pd.DataFrame({"x": [1.0, None]}))
    df = pd.DataFrame({"x": [1.0, None, 3.0], "gone": [np.nan, np.nan, np.nan]})
    for flag in (False, True):
        wf = nvt.Workflow(["x", "gone"] >> ops.FillMedian(add_binary_cols=flag))
        out = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
        op = _median_op(wf)
        assert op.medians["x"] == 2.0 and math.isnan(op.medians["gone"])
        assert out["x"].tolist() == [1.0, 2.0, 3.0]
        assert out["gone"].isna().all()          # passed through unfilled
        if flag:
            assert out["gone_filled"].tolist() == [True, True, True]
    op.clear()
    assert op.medians == {}
    with pytest.raises(RuntimeError, match="need to call 'fit'"):
        op.transform(ColumnSelector(["x"]), df)


def test_save_load_round_trip(tmp_path, frame):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    df, meds = frame
    wf = nvt.Workflow((["f64", "i64"] >> ops.FillMedian(add_binary_cols=True)) + (["f32"] >> ops.FillMedian()
                                                                                 >> ops.Normalize()))
    a = wf.fit_transform(nvt.Dataset(df)).to_ddf().compute()
    wf.save(str(tmp_path / "saved"))
    graph = (tmp_path / "saved" / "graph.json").read_text()
    assert "nvtabular.ops.fill.FillMedian" in graph
    wf2 = nvt.Workflow.load(str(tmp_path / "saved"))
    loaded = [n.op for n in nvt.workflow.iter_nodes(wf2.output_node) if isinstance(n.op, ops.FillMedian)]
    assert sorted(sorted(op.medians) for op in loaded) == [["f32"], ["f64", "i64"]]
    for op in loaded:
        for c, v in op.medians.items():
            assert v == meds[c]
    b = wf2.transform(nvt.Dataset(df)).to_ddf().compute()     # no refit
    pd.testing.assert_frame_equal(a, b)


def test_import_nvtabular_resolves():
    import nvtabular
    import nvtabular.ops.fill
    import nvtabular_amd.ops

    assert nvtabular.ops.FillMedian is nvtabular_amd.ops.FillMedian
    assert nvtabular.ops.fill.FillMedian is nvtabular_amd.ops.FillMedian
