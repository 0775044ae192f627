"""ops.Groupby with the nunique aggregation against the reference project's Groupby on pandas
(oracle.groupby_op): the int32 ``*_nunique`` columns compared exactly, the aggregates that existed
before compared with the same call without nunique."""
import numpy as np
import pandas as pd
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


def _sorted(df, by):
    return df.sort_values(by, kind="stable", na_position="last", ignore_index=True)


def _same_column(got, exp, name):
    g, e = got[name], exp[name]
    if name.endswith("list"):
        assert [list(x) for x in g] == [list(x) for x in e], name
    elif g.dtype == object or e.dtype == object or g.dtype.kind == "M":
        assert g.tolist() == e.tolist(), name
    else:
        np.testing.assert_array_equal(g.to_numpy(), e.to_numpy(), err_msg=name)


def test_the_reference_projects_own_case():
    """tests/unit/ops/test_groupyby.py:197-230 of the reference: two string keys' worth of rows,
    every conventional aggregate of its list on an int8, a float64 and a float32 column, through
    Workflow.fit + transform -- here on 3 partitions shuffled by the key."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    n = 60
    df = pd.DataFrame({
        "name": ["Dave"] * 30 + ["Zelda"] * 30,
        "x": (np.arange(n) % 2).astype("int8"),
        "y": np.linspace(0.0, 10.0, n),
        "z": np.concatenate([np.linspace(-1.0, 1.0, 40), np.zeros(20)]).astype("float32"),
    })
    df = df.sample(frac=1.0, random_state=4).reset_index(drop=True)
    aggs = ["mean", "std", "var", "nunique", "sum"]
    sel = ["name", "x", "y", "z"]
    feats = sel >> ops.Groupby(groupby_cols=["name"], aggs=aggs, name_sep="-")
    ds = nvt.Dataset([df.iloc[i * 20:(i + 1) * 20].reset_index(drop=True) for i in range(3)])
    assert ds.npartitions == 3
    wf = nvt.Workflow(feats)
    wf.fit(ds)
    got = _sorted(wf.transform(ds.shuffle_by_keys(["name"])).to_ddf().compute(), ["name"])
    exp = _sorted(O.groupby_op(df, sel, ["name"], None, aggs, "-"), ["name"])
    assert sorted(got.columns) == sorted(exp.columns) and got["name"].tolist() == ["Dave", "Zelda"]
    for c in ("x", "y", "z"):
        assert got[f"{c}-nunique"].dtype == np.int32 == exp[f"{c}-nunique"].dtype
        np.testing.assert_array_equal(got[f"{c}-nunique"].to_numpy(), exp[f"{c}-nunique"].to_numpy(), err_msg=c)
        for a in ("mean", "std", "var", "sum"):
            assert got[f"{c}-{a}"].dtype == np.float32
            np.testing.assert_allclose(got[f"{c}-{a}"].to_numpy().astype("float64"),
                                       exp[f"{c}-{a}"].to_numpy().astype("float64"), rtol=1e-5, atol=1e-6,
                                       err_msg=f"{c}-{a}")
    assert got["x-nunique"].tolist() == [2, 2] and got["y-nunique"].tolist() == [30, 30]


def _mixed_frame(n):
    rng = np.random.default_rng(9)
    df = pd.DataFrame({
        "name": rng.choice(["Dave", "Zelda", "Ann", "Bo"], n),
        "id": pd.array(rng.integers(0, 40, n), dtype="Int64"),
        "ts": rng.permutation(n).astype("int64"),          # unique: the sort is unambiguous
        "x": rng.integers(0, 12, n).astype("int64"),
        "y": rng.integers(-3, 4, n) / 2.0,
        "s": rng.choice(["a", "bb", "ccc", "", "Dave"], n),
        "t": pd.to_datetime(rng.integers(0, 6, n) * 86_400_000_000_123, unit="ns"),
    })
    if n:
        df.loc[rng.random(n) < 0.2, "y"] = np.nan
        df.loc[rng.random(n) < 0.2, "s"] = None
        df.loc[rng.random(n) < 0.2, "t"] = pd.NaT
        df.loc[rng.random(n) < 0.05, "id"] = pd.NA         # null keys are dropped
        dead = (df["id"] == 7).fillna(False).to_numpy(dtype=bool)       # groups of nulls: 0
        df.loc[dead, "y"] = np.nan
        df.loc[dead, "s"] = None
        df.loc[dead, "t"] = pd.NaT
    return df


MIXED_AGGS = {"x": ["list", "nunique", "first", "last"], "y": ["mean", "nunique", "min", "count"],
              "s": ["nunique", "count"], "t": "nunique"}
SEL = ["name", "id", "ts", "x", "y", "s", "t"]
KEYS = ["name", "id"]


def _without_nunique(aggs):
    out = {}
    for c, v in aggs.items():
        rest = [a for a in (v if isinstance(v, list) else [v]) if a != "nunique"]
        if rest:
            out[c] = rest
    return out


def _run(df, aggs, ascending=False):
    from nvtabular_amd import ColumnSelector, ops

    op = ops.Groupby(groupby_cols=KEYS, sort_cols=["ts"], aggs=aggs, ascending=ascending)
    return op.transform(ColumnSelector(SEL), df)


@pytest.fixture(scope="module")
def mixed():
    df = _mixed_frame(4000)
    odf = df.copy()
    odf["id"] = odf["id"].astype("float64")
    return df, odf


def test_mixed_case_against_the_oracle(mixed):
    df, odf = mixed
    got = _run(df, MIXED_AGGS)                             # (a datetime column: no TypeError)
    exp = O.groupby_op(odf, SEL, KEYS, ["ts"], MIXED_AGGS, "_", False)
    assert sorted(got.columns) == sorted(exp.columns) and len(got) == len(exp)
    assert got["name"].tolist() == exp["name"].tolist()
    np.testing.assert_array_equal(got["id"].to_numpy().astype("int64"), exp["id"].to_numpy().astype("int64"))
    for c in ("x", "y", "s", "t"):
        name = f"{c}_nunique"
        assert got[name].dtype == np.int32 == exp[name].dtype, name
        assert not got[name].isna().any()
        np.testing.assert_array_equal(got[name].to_numpy(), exp[name].to_numpy(), err_msg=name)
    dead = (exp["id"] == 7).to_numpy()
    assert dead.any() and (got.loc[dead, ["y_nunique", "s_nunique", "t_nunique"]].to_numpy() == 0).all()
    assert got["x_nunique"].max() > 1 and got["s_nunique"].max() > 1 and got["t_nunique"].max() > 1
    # the order given: x_nunique between x_list's conventional neighbours, y_nunique after y_mean
    names = list(got.columns)
    assert names.index("y_mean") < names.index("y_nunique") < names.index("y_min") < names.index("y_count")
    assert [list(x) for x in got["x_list"]] == [list(x) for x in exp["x_list"]]
    for c in ("x_first", "x_last", "y_count", "s_count"):
        np.testing.assert_array_equal(got[c].to_numpy().astype("int64"), exp[c].to_numpy().astype("int64"), err_msg=c)


@pytest.mark.parametrize("n", [4000, 0])
def test_other_aggregates_do_not_change(n):
    df = _mixed_frame(n)
    rest = _without_nunique(MIXED_AGGS)
    assert "t" not in rest
    got, base = _run(df, MIXED_AGGS), _run(df, rest)
    assert len(got) == len(base) and (n == 0) == (len(got) == 0)
    assert [c for c in got.columns if not c.endswith("_nunique")] == list(base.columns)
    assert [c for c in got.columns if c.endswith("_nunique")] == ["x_nunique", "y_nunique", "s_nunique", "t_nunique"]
    for c in base.columns:
        assert got[c].dtype == base[c].dtype, c
        _same_column(got, base, c)
    assert all(got[c].dtype == np.int32 for c in got.columns if c.endswith("_nunique"))


def test_reference_case_aggregates_do_not_change():
    from nvtabular_amd import ColumnSelector, ops

    df = _mixed_frame(4000)[["name", "x", "y"]]
    run = lambda aggs: ops.Groupby(groupby_cols=["name"], aggs=aggs, name_sep="-").transform(  # noqa: E731
        ColumnSelector(["name", "x", "y"]), df)
    every = ["count", "sum", "mean", "min", "max", "std", "var"]
    got, base = run(every[:3] + ["nunique"] + every[3:]), run(every)
    assert [c for c in got.columns if not c.endswith("-nunique")] == list(base.columns)
    for c in base.columns:
        _same_column(got, base, c)


def test_nunique_as_the_only_aggregate(mixed):
    df, odf = mixed
    got = _run(df, "nunique", ascending=True)
    exp = O.groupby_op(odf, SEL, KEYS, ["ts"], "nunique", "_", True)
    assert list(got.columns) == KEYS + [f"{c}_nunique" for c in ("ts", "x", "y", "s", "t")]
    assert sorted(got.columns) == sorted(exp.columns) and len(got) == len(exp)
    for c in ("ts", "x", "y", "s", "t"):
        assert got[f"{c}_nunique"].dtype == np.int32
        np.testing.assert_array_equal(got[f"{c}_nunique"].to_numpy(), exp[f"{c}_nunique"].to_numpy(), err_msg=c)


def test_list_value_column_still_raises():
    from nvtabular_amd import ColumnSelector, ops

    df = pd.DataFrame({"k": [1, 1, 2], "l": [[1, 2], [3], [4, 4]]})
    op = ops.Groupby(groupby_cols=["k"], aggs={"l": "nunique"})
    with pytest.raises(NotImplementedError):
        op.transform(ColumnSelector(["k", "l"]), df)
