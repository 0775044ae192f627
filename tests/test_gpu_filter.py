"""Row compaction on the device (nvt_compact_*, kernels_compact.py) and the operators built on it,
ops.Filter and ops.Dropna: bit-exact against numpy / Python slicing, against
DeviceFrame.take_rows (the torch gather used by the parquet shuffle), and against pandas and the
CPU oracle through whole workflows."""
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 2048


def _dev():
    return torch.device("cuda", 0)


def _bitmap(valid_bool):
    from nvtabular_amd.device import pack_bitmap

    return torch.from_numpy(pack_bitmap(valid_bool)).to(_dev())


def _keep_pattern(kind, n, rng):
    if kind == "none":
        return np.zeros(n, dtype=bool)
    if kind == "all":
        return np.ones(n, dtype=bool)
    if kind == "half":
        return rng.random(n) < 0.5
    if kind == "runs":   # long runs of kept and dropped rows
        k = np.zeros(n, dtype=bool)
        pos, on = 0, True
        while pos < n:
            ln = int(rng.integers(1, 5000))
            k[pos: pos + ln] = on
            pos, on = pos + ln, not on
        return k
    if kind == "one":
        k = np.zeros(n, dtype=bool)
        if n:
            k[int(rng.integers(0, n))] = True
        return k
    if kind == "every64":
        k = np.zeros(n, dtype=bool)
        k[::64] = True
        return k
    raise ValueError(kind)


def _values(dt, n, rng):
    if dt == np.bool_:
        return rng.random(n) < 0.5
    if dt == np.uint8:
        return rng.integers(0, 256, n).astype(np.uint8)
    if dt in (np.int32, np.int64):
        return rng.integers(-(2 ** 31), 2 ** 31 - 1, n).astype(dt)
    v = rng.standard_normal(n).astype(dt)
    v[rng.random(n) < 0.05] = np.nan
    return v


DTYPES = [np.bool_, np.uint8, np.int32, np.int64, np.float32, np.float64]


def _check_column(got, vals, valid, keep, name):
    m = int(keep.sum())
    data = got.data.cpu().numpy()
    assert data.dtype == vals.dtype, name
    assert len(data) == m, name
    np.testing.assert_array_equal(data.view(np.uint8), vals[keep].view(np.uint8), err_msg=name)
    if valid is None:
        assert got.valid is None, name
        return
    assert got.valid is not None and got.valid.dtype == torch.uint8, name
    raw = got.valid.cpu().numpy()
    assert len(raw) == (m + 63) // 64 * 8, name
    np.testing.assert_array_equal(got.valid_mask_host(), valid[keep], err_msg=name)
    bits = np.unpackbits(raw, bitorder="little")
    assert not bits[m:].any(), f"{name}: bits past m are set"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 12_347, 3_000_001])
@pytest.mark.parametrize("kind", ["none", "all", "half", "runs", "one", "every64"])
def test_compact_every_dtype_against_numpy(n, kind):
    from nvtabular_amd.device import DeviceColumn, DeviceFrame
    from nvtabular_amd.kernels_compact import compact_frame

    rng = np.random.default_rng(n * 7 + len(kind))
    keep = _keep_pattern(kind, n, rng)
    frame, expect = DeviceFrame(), {}
    for dt in DTYPES:
        vals = _values(dt, n, rng)
        valid = rng.random(n) < 0.7
        name = np.dtype(dt).name
        frame[name] = DeviceColumn(torch.from_numpy(vals).to(_dev()))
        expect[name] = (vals, None)
        frame[name + "_v"] = DeviceColumn(torch.from_numpy(vals).to(_dev()), _bitmap(valid))
        expect[name + "_v"] = (vals, valid)
    # a column whose values do not start on a 16-byte boundary (the scalar-load path)
    base = _values(np.int32, n + 1, rng)
    valid = rng.random(n) < 0.5
    frame["unaligned"] = DeviceColumn(torch.from_numpy(base).to(_dev())[1:], _bitmap(valid))
    expect["unaligned"] = (base[1:], valid)
    out = compact_frame(frame, torch.from_numpy(keep).to(_dev()))
    assert out.columns == frame.columns
    assert len(out) == int(keep.sum())
    for name, (vals, valid) in expect.items():
        _check_column(out[name], vals, valid, keep, name)


def test_compact_many_columns_and_uint8_mask():
    """More columns than one launch takes (64), and a uint8 keep mask."""
    from nvtabular_amd.device import DeviceColumn, DeviceFrame
    from nvtabular_amd.kernels_compact import compact_frame

    rng = np.random.default_rng(5)
    n = 50_001
    keep = rng.random(n) < 0.3
    frame, expect = DeviceFrame(), {}
    for j in range(70):
        vals = _values(DTYPES[j % len(DTYPES)], n, rng)
        valid = rng.random(n) < 0.8 if j % 2 else None
        frame[f"c{j}"] = DeviceColumn(torch.from_numpy(vals).to(_dev()),
                                      _bitmap(valid) if valid is not None else None)
        expect[f"c{j}"] = (vals, valid)
    out = compact_frame(frame, torch.from_numpy(keep.astype(np.uint8)).to(_dev()))
    for name, (vals, valid) in expect.items():
        _check_column(out[name], vals, valid, keep, name)


def _list_column(n, rng, empty_frac=0.3, leaf_valid=True):
    from nvtabular_amd.device import DeviceColumn

    lens = rng.integers(0, 6, n)
    lens[rng.random(n) < empty_frac] = 0
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    leaves = rng.integers(0, 1000, int(off[-1])).astype(np.int64)
    lv = rng.random(len(leaves)) < 0.8 if leaf_valid else None
    col = DeviceColumn(torch.from_numpy(leaves).to(_dev()), _bitmap(lv) if lv is not None else None,
                       torch.from_numpy(off).to(_dev()))
    return col, off, leaves, lv


@pytest.mark.parametrize("n", [1, 100, TILE + 3, 70_001])
@pytest.mark.parametrize("kind", ["none", "all", "half", "runs", "one"])
def test_compact_list_columns(n, kind):
    from nvtabular_amd.device import DeviceColumn, DeviceFrame
    from nvtabular_amd.kernels_compact import compact_frame

    rng = np.random.default_rng(n + len(kind))
    keep = _keep_pattern(kind, n, rng)
    col, off, leaves, lv = _list_column(n, rng)
    empty = DeviceColumn(torch.empty(0, dtype=torch.float32, device=_dev()),
                         None, torch.zeros(n + 1, dtype=torch.int64, device=_dev()))
    frame = DeviceFrame({"l": col, "e": empty, "x": DeviceColumn(torch.arange(n, device=_dev()))})
    out = compact_frame(frame, torch.from_numpy(keep).to(_dev()))
    rows = np.nonzero(keep)[0]
    exp_leaves = [leaves[off[i]: off[i + 1]] for i in rows]
    exp_valid = [lv[off[i]: off[i + 1]] for i in rows]
    exp_off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in exp_leaves], out=exp_off[1:])
    got = out["l"]
    np.testing.assert_array_equal(got.offsets.cpu().numpy(), exp_off)
    flat = np.concatenate(exp_leaves) if exp_leaves else np.zeros(0, np.int64)
    np.testing.assert_array_equal(got.data.cpu().numpy(), flat)
    fv = np.concatenate(exp_valid) if exp_valid else np.zeros(0, bool)
    np.testing.assert_array_equal(got.valid_mask_host(), fv)
    bits = np.unpackbits(got.valid.cpu().numpy(), bitorder="little")
    assert not bits[len(fv):].any()
    np.testing.assert_array_equal(out["e"].offsets.cpu().numpy(), np.zeros(len(rows) + 1, np.int64))
    assert out["e"].data.numel() == 0 and out["e"].data.dtype == torch.float32
    np.testing.assert_array_equal(out["x"].data.cpu().numpy(), rows)
    # the torch gather of the parquet shuffle gives the same buffers, bit for bit
    ref = frame.take_rows(torch.from_numpy(rows).to(_dev()))
    assert torch.equal(ref["l"].offsets, got.offsets) and torch.equal(ref["l"].data, got.data)
    assert torch.equal(ref["l"].valid, got.valid)


def test_compact_strings_carry_their_dictionary():
    from nvtabular_amd.device import DeviceColumn, DeviceFrame
    from nvtabular_amd.kernels_compact import compact_frame

    rng = np.random.default_rng(3)
    n = 10_000
    words = np.array(["apple", "banana", "cherry", "", "durian", "eel"], dtype=object)
    s = pd.Series(words[rng.integers(0, len(words), n)], dtype=object)
    s[rng.random(n) < 0.2] = None
    col = DeviceColumn.from_pandas(s, _dev())
    assert col.strings is not None and col.valid is not None
    keep = rng.random(n) < 0.4
    out = compact_frame(DeviceFrame({"s": col}), torch.from_numpy(keep).to(_dev()))
    got = out["s"]
    assert got.strings is col.strings
    np.testing.assert_array_equal(got.data.cpu().numpy(), col.data.cpu().numpy()[keep])
    np.testing.assert_array_equal(got.valid_mask_host(), col.valid_mask_host()[keep])
    assert got.to_pandas("s").tolist() == s[keep].reset_index(drop=True).tolist()


def test_pending_fill_survives_dropna():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.selector import ColumnSelector

    rng = np.random.default_rng(11)
    n = 20_000
    df = pd.DataFrame({
        "a": np.where(rng.random(n) < 0.3, np.nan, rng.standard_normal(n)),
        "b": pd.array(np.where(rng.random(n) < 0.2, None, rng.integers(0, 100, n)), dtype="Int64"),
        "c": np.where(rng.random(n) < 0.25, np.nan, rng.standard_normal(n)).astype(np.float32),
    })
    exp = df.copy()
    exp[["a", "b"]] = exp[["a", "b"]].fillna(7)
    exp = exp.dropna().reset_index(drop=True)
    # on the device the fill stays pending through the compaction
    frame = DeviceFrame.from_pandas(df, _dev())
    filled = ops.FillMissing(fill_val=7).transform(ColumnSelector(["a", "b"]), frame)
    out = ops.Dropna().transform(ColumnSelector(["a", "b", "c"]), filled)
    assert out["a"].fill == 7 and out["b"].fill == 7 and len(out) == len(exp)
    got = out.to_pandas()
    for c in ("a", "b", "c"):
        np.testing.assert_array_equal(got[c].to_numpy(dtype=np.float64, na_value=np.nan),
                                      exp[c].to_numpy(dtype=np.float64, na_value=np.nan), err_msg=c)
    # and through a workflow
    wf = nvt.Workflow(((["a", "b"] >> ops.FillMissing(fill_val=7)) + ["c"]) >> ops.Dropna())
    got = wf.fit_transform(nvt.Dataset(df, npartitions=3)).to_ddf().compute().reset_index(drop=True)
    assert len(got) == len(exp)
    for c in ("a", "b", "c"):
        np.testing.assert_array_equal(got[c].to_numpy(dtype=np.float64, na_value=np.nan),
                                      exp[c].to_numpy(dtype=np.float64, na_value=np.nan), err_msg=c)


def _mixed_frame(n, seed):
    rng = np.random.default_rng(seed)
    words = np.array(["x", "yy", "zzz", "w"], dtype=object)
    s = pd.Series(words[rng.integers(0, 4, n)], dtype=object)
    s[rng.random(n) < 0.1] = None
    return pd.DataFrame({
        "f": np.where(rng.random(n) < 0.1, np.nan, rng.standard_normal(n)),
        "f32": np.where(rng.random(n) < 0.05, np.nan, rng.standard_normal(n)).astype(np.float32),
        "i": pd.array(np.where(rng.random(n) < 0.1, None, rng.integers(0, 1000, n)), dtype="Int64"),
        "k": rng.integers(0, 50, n).astype(np.int32),
        "b": rng.random(n) < 0.5,
        "s": s,
        "l": pd.Series([list(rng.integers(0, 9, int(rng.integers(0, 4)))) for _ in range(n)], dtype=object),
    })


def _assert_frames_equal(got, exp):
    assert list(got.columns) == list(exp.columns) and len(got) == len(exp)
    for c in exp.columns:
        if c == "l":
            for g, e in zip(got[c], exp[c]):
                assert list(g) == list(e)
        elif c == "s":
            assert got[c].tolist() == exp[c].tolist()
        else:
            np.testing.assert_array_equal(got[c].to_numpy(dtype=np.float64, na_value=np.nan),
                                          exp[c].to_numpy(dtype=np.float64, na_value=np.nan), err_msg=c)


def test_dropna_against_pandas():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.selector import ColumnSelector

    df = _mixed_frame(30_000, 1)
    cols = list(df.columns)
    # every column (the default), through a multi-partition Dataset
    wf = nvt.Workflow(cols >> ops.Dropna())
    got = wf.fit_transform(nvt.Dataset(df, npartitions=4)).to_ddf().compute().reset_index(drop=True)
    exp = df.dropna().reset_index(drop=True)
    assert len(exp) < len(df)
    _assert_frames_equal(got, exp)
    # a subset: the rows of the whole frame, tested on the subset only; dtypes and validity kept
    frame = DeviceFrame.from_pandas(df, _dev())
    out = ops.Dropna().transform(ColumnSelector(["f", "s"]), frame)
    exp = df.dropna(subset=["f", "s"]).reset_index(drop=True)
    for c in cols:
        assert out[c].data.dtype == frame[c].data.dtype
        assert (out[c].valid is None) == (frame[c].valid is None)
    _assert_frames_equal(out.to_pandas(), exp)
    # pandas in, pandas out
    got = ops.Dropna().transform(ColumnSelector(["i"]), df)
    assert isinstance(got, pd.DataFrame)
    _assert_frames_equal(got, df.dropna(subset=["i"]).reset_index(drop=True))


def test_filter_reference_cases():
    """tests/unit/ops/test_ops.py::test_filter of the reference, ported."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(2)
    n = 40_000
    df = pd.DataFrame({"x": rng.random(n), "y": rng.random(n), "id": rng.integers(0, 100, n)})
    ds = nvt.Dataset(df, npartitions=3)
    cont_names = ["x", "y"]
    op = ops.Filter(f=lambda df: df[df["y"] > 0.5])
    got = nvt.Workflow(cont_names >> op).fit(ds).transform(ds).to_ddf().compute().reset_index(drop=True)
    assert op.last_path == "device"
    exp = df[df["y"] > 0.5].reset_index(drop=True)
    for col in cont_names:
        np.testing.assert_array_equal(got[col].to_numpy(), exp[col].to_numpy())

    for col in cont_names:
        idx = rng.choice(n - 1, int(n * 0.2))
        df.loc[idx, col] = None
    ds = nvt.Dataset(df, npartitions=3)
    for f in (lambda df: df[df.x.isnull()], lambda df: df.x.isnull()):
        op = ops.Filter(f=f)
        got = nvt.Workflow(cont_names >> op).fit(ds).transform(ds).to_ddf().compute()
        assert op.last_path == "device"
        assert 0 < got.shape[0] < df.shape[0]
        assert got.shape[0] == int(df.x.isnull().sum()) and got["x"].isnull().all()
        np.testing.assert_array_equal(got["y"].to_numpy(), df[df.x.isnull()]["y"].to_numpy())

    wf = nvt.Workflow(cont_names >> ops.Filter(f=lambda df: "some invalid value"))
    with pytest.raises(ValueError):
        wf.transform(ds).to_ddf().compute()


def test_filter_host_path_and_bad_masks():
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.selector import ColumnSelector

    df = _mixed_frame(8_000, 4)
    frame = DeviceFrame.from_pandas(df, _dev())
    sel = ColumnSelector(list(df.columns))
    # a .str predicate takes the host path; its bool Series is compacted on the device
    op = ops.Filter(lambda d: d["s"].str.startswith("y", na=False))
    out = op.transform(sel, frame)
    assert op.last_path == "host" and isinstance(out, DeviceFrame)
    _assert_frames_equal(out.to_pandas(), df[df["s"].str.startswith("y", na=False)].reset_index(drop=True))
    # a DataFrame returned on the host is taken as it is
    op = ops.Filter(lambda d: d[d["s"].str.len() > 1])
    out = op.transform(ColumnSelector(["k", "s"]), frame[["k", "s"]])
    assert op.last_path == "host"
    exp = df[["k", "s"]]
    exp = exp[exp["s"].str.len() > 1].reset_index(drop=True)
    _assert_frames_equal(out.to_pandas(), exp)
    # device predicates over several columns, and a bool tensor result
    op = ops.Filter(lambda d: (d["k"] > 10) & (d.f > 0))
    out = op.transform(sel, frame)
    assert op.last_path == "device"
    _assert_frames_equal(out.to_pandas(), df[(df["k"] > 10) & (df.f > 0)].reset_index(drop=True))
    out = ops.Filter(lambda d: (d["k"] % 2 == 0).values).transform(sel, frame)
    _assert_frames_equal(out.to_pandas(), df[df["k"] % 2 == 0].reset_index(drop=True))
    # a mask of the wrong length, or something that is not a mask
    with pytest.raises(ValueError):
        ops.Filter(lambda d: torch.ones(3, dtype=torch.bool, device=_dev())).transform(sel, frame)
    with pytest.raises(ValueError):
        ops.Filter(lambda d: d["k"] + 1).transform(sel, frame)
    # pandas in, pandas out
    got = ops.Filter(lambda d: d["k"] < 5).transform(sel, df)
    assert isinstance(got, pd.DataFrame)
    _assert_frames_equal(got, df[df["k"] < 5].reset_index(drop=True))


def test_fit_sees_the_filtered_rows(tmp_path):
    import nvtabular_amd as nvt
    import oracle as O
    from nvtabular_amd import ops

    rng = np.random.default_rng(9)
    n = 60_000
    df = pd.DataFrame({
        "a": pd.array(np.where(rng.random(n) < 0.1, None, rng.zipf(1.3, n) % 500), dtype="Int64"),
        "b": rng.integers(0, 3000, n).astype(np.int64),
        "x": np.where(rng.random(n) < 0.2, np.nan, rng.lognormal(1, 1, n)),
        "y": np.where(rng.random(n) < 0.1, np.nan, rng.standard_normal(n)),
    })
    ds = nvt.Dataset(df, npartitions=4)
    cats = ["a", "b"] >> ops.Filter(lambda d: d["b"] % 3 != 0) >> ops.Categorify(out_path=str(tmp_path / "gpu"))
    got = nvt.Workflow(cats).fit_transform(ds).to_ddf().compute().reset_index(drop=True)
    filt = df[df["b"] % 3 != 0].reset_index(drop=True)
    paths = O.categorify_fit([filt], ["a", "b"], str(tmp_path / "cpu"), tie_break="stable")
    exp = O.categorify_transform(filt, ["a", "b"], paths)
    for c in ("a", "b"):
        np.testing.assert_array_equal(got[c].to_numpy(), exp[c].to_numpy(), err_msg=c)

    conts = ["x", "y"] >> ops.Dropna() >> ops.Normalize()
    got = nvt.Workflow(conts).fit_transform(ds).to_ddf().compute().reset_index(drop=True)
    filt = df[["x", "y"]].dropna().reset_index(drop=True)
    mom = O.custom_moments([filt], ["x", "y"])
    exp = O.normalize_transform(filt, ["x", "y"], mom["mean"].to_dict(), mom["std"].to_dict())
    assert len(got) == len(exp)
    for c in ("x", "y"):
        np.testing.assert_allclose(got[c].to_numpy(), exp[c].to_numpy(), rtol=1e-6, atol=1e-9, err_msg=c)


def test_session_pipeline(tmp_path):
    """Categorify >> Groupby(list, count) >> Filter(count >= 2) equals the same pipeline without the
    Filter, filtered afterwards with pandas (list column and all)."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(17)
    n = 30_000
    df = pd.DataFrame({"session_id": rng.integers(0, 8_000, n).astype(np.int64),
                       "item_id": (rng.zipf(1.2, n) % 5_000).astype(np.int64)})
    aggs = {"item_id": ["list", "count"]}

    def pipeline(tag, filt):
        node = (["session_id", "item_id"] >> ops.Categorify(out_path=str(tmp_path / tag))
                >> ops.Groupby(groupby_cols=["session_id"], aggs=aggs))
        if filt:
            node = node >> ops.Filter(lambda d: d["item_id_count"] >= 2)
        return nvt.Workflow(node).fit_transform(nvt.Dataset(df)).to_ddf().compute().reset_index(drop=True)

    got = pipeline("a", True)
    g = pipeline("b", False)
    exp = g[g["item_id_count"] >= 2].reset_index(drop=True)
    assert 0 < len(exp) < len(g)
    assert list(got.columns) == list(exp.columns) and len(got) == len(exp)
    for c in ("session_id", "item_id_count"):
        np.testing.assert_array_equal(got[c].to_numpy(), exp[c].to_numpy(), err_msg=c)
    for a, b in zip(got["item_id_list"], exp["item_id_list"]):
        assert list(a) == list(b)


def test_full_size_criteo_against_take_rows():
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    from nvtabular_amd.kernels_compact import compact_frame

    dev = _dev()
    frame = bench.synth_criteo(45_000_000, dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    keep = torch.rand(45_000_000, device=dev, generator=g) < 0.5
    a = compact_frame(frame, keep)
    b = compact_frame(frame, keep)
    ref = frame.take_rows(keep.nonzero().flatten())
    m = int(keep.sum())
    assert len(a) == m
    for name in frame.columns:
        ca, cb, cr = a[name], b[name], ref[name]
        assert torch.equal(ca.data.view(torch.uint8), cr.data.view(torch.uint8)), name
        assert torch.equal(ca.data.view(torch.uint8), cb.data.view(torch.uint8)), name
        assert (ca.valid is None) == (cr.valid is None), name
        if ca.valid is not None:
            assert torch.equal(ca.valid, cr.valid), name
            assert torch.equal(ca.valid, cb.valid), name
