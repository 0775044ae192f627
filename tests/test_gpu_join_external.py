"""ops.JoinExternal on the device against pandas' merge (left-row order, index from 0), the carried
left columns, the launch counts of the hot path, workflows with the CPU oracle, and two threads."""
import threading

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

pytestmark = pytest.mark.gpu


def _expected(left, ext_sel, on, on_ext, how):
    n = len(left)
    return (left.assign(__r=np.arange(n))
            .merge(ext_sel, left_on=on, right_on=on_ext, how=how)
            .sort_values("__r", kind="stable")
            .drop(columns="__r")
            .reset_index(drop=True))


def _cell(v):
    if isinstance(v, (list, np.ndarray)):
        return [None if x is None or (isinstance(x, float) and np.isnan(x)) else x for x in list(v)]
    return v


def _same(got, exp):
    assert list(got.columns) == list(exp.columns)
    assert len(got) == len(exp)
    for c in exp.columns:
        g, e = got[c], exp[c]
        gn, en = g.isna().to_numpy(), e.isna().to_numpy()
        np.testing.assert_array_equal(gn, en, err_msg=f"nulls of {c}")
        gv, ev = g[~gn].to_numpy(), e[~en].to_numpy()
        if ev.dtype == object or gv.dtype == object:
            assert [_cell(v) for v in gv] == [_cell(v) for v in ev], c
        else:
            np.testing.assert_array_equal(gv.astype(np.float64), ev.astype(np.float64), err_msg=c)


def _join(left, ext, on, how, on_ext=None, columns_ext=None, drop_duplicates_ext=None, frame=None):
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.selector import ColumnSelector

    op = ops.JoinExternal(ext, on=on, how=how, on_ext=on_ext, columns_ext=columns_ext,
                          drop_duplicates_ext=drop_duplicates_ext)
    frame = frame if frame is not None else DeviceFrame.from_pandas(left)
    out = op.transform(ColumnSelector(list(frame.columns)), frame)
    return op, out


def _check(left, ext, on, how, on_ext=None, columns_ext=None, drop_duplicates_ext=None):
    _, out = _join(left, ext, on, how, on_ext, columns_ext, drop_duplicates_ext)
    ext_pd = ext.to_pandas() if isinstance(ext, pa.Table) else ext
    sel = ext_pd[columns_ext] if columns_ext else ext_pd
    if drop_duplicates_ext:
        sel = sel.drop_duplicates(ignore_index=True)
    _same(out.to_pandas(), _expected(left, sel, on, on_ext or on, how))
    _tail_bits_zero(out)
    return out


def _tail_bits_zero(frame):
    for name, col in frame.items():
        if col.valid is None or col.is_list:
            continue
        m = int(col.data.numel())
        bits = np.unpackbits(col.valid.cpu().numpy(), bitorder="little")
        assert not bits[m:].any(), f"validity bits past the row count in {name}"


def _ext_table(keys, rng, with_strings=True):
    n = len(keys)
    cols = {
        "k": pa.array(keys),
        "i64": pa.array(rng.integers(-50, 50, n), pa.int64(), mask=rng.random(n) < 0.2),
        "f32": pa.array(rng.standard_normal(n).astype(np.float32), mask=rng.random(n) < 0.2),
        "f64": pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.2),
        "i32": pa.array(rng.integers(0, 9, n).astype(np.int32), mask=rng.random(n) < 0.2),
        "u8": pa.array(rng.integers(0, 9, n).astype(np.uint8)),
    }
    if with_strings:
        cols["s"] = pa.array([f"v{x}" if x % 5 else None for x in rng.integers(0, 40, n)])
    return pa.table(cols)


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_parity_sizes(how, dup, n):
    rng = np.random.default_rng(n + 7 * dup)
    keys = np.arange(0, 3000, 2, dtype=np.int64)
    if dup:
        keys = np.concatenate([keys, keys[::3], keys[::7]])
        rng.shuffle(keys)
    ext = _ext_table(keys, rng)
    left = pd.DataFrame({"k": rng.integers(0, 3000, n).astype(np.int32), "x": rng.random(n)})
    _check(left, ext, "k", how)


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("dup", [False, True])
def test_parity_three_million_rows(how, dup):
    rng = np.random.default_rng(3)
    n = 3_000_001
    keys = np.arange(200_000, dtype=np.int64) * 3
    if dup:
        keys = np.concatenate([keys, keys[::5]])
    ext = pd.DataFrame({"k": keys, "v": np.arange(len(keys), dtype=np.int64),
                        "w": rng.standard_normal(len(keys)).astype(np.float32)})
    left = pd.DataFrame({"k": rng.integers(0, 600_000, n).astype(np.int64)})
    _check(left, ext, "k", how)


@pytest.mark.parametrize("how", ["left", "inner"])
def test_key_kinds(how):
    rng = np.random.default_rng(11)
    # int32 <-> int64
    left = pd.DataFrame({"k": rng.integers(-5, 40, 500).astype(np.int32)})
    ext = pd.DataFrame({"k": np.arange(0, 30, dtype=np.int64), "v": np.arange(30) * 1.5})
    _check(left, ext, "k", how)
    # float64 with NaN (pandas' int-with-null) <-> int64, on != on_ext
    lk = rng.integers(0, 40, 500).astype(np.float64)
    lk[rng.random(500) < 0.2] = np.nan
    left = pd.DataFrame({"k": lk, "a": np.arange(500)})
    ext = pd.DataFrame({"kk": np.arange(0, 30, dtype=np.int64), "v": np.arange(30)})
    _check(left, ext, "k", how, on_ext="kk")
    # float <-> float: -0.0 equals 0.0, NaN matches NaN
    left = pd.DataFrame({"k": np.array([0.0, -0.0, 1.5, np.nan, 2.25, 7.0, -1.5] * 20)})
    ext = pd.DataFrame({"k": np.array([-0.0, 1.5, np.nan, 7.0, 3.0], np.float32).astype(np.float64),
                        "v": np.arange(5, dtype=np.int64)})
    _check(left, ext, "k", how)
    # string <-> string, nulls on both sides
    words = np.array(["apple", "pear", None, "fig", "kiwi", "plum"], dtype=object)
    left = pd.DataFrame({"k": words[rng.integers(0, 6, 700)]})
    ext = pd.DataFrame({"k": pd.Series(["pear", "fig", None, "lime", "apple"], dtype=object),
                        "v": np.arange(5, dtype=np.int64), "t": ["a", "b", "c", None, "e"]})
    _check(left, ext, "k", how)


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("nkeys", [2, 3])
@pytest.mark.parametrize("dup", [False, True])
def test_tuple_keys_with_nulls(how, nkeys, dup):
    rng = np.random.default_rng(nkeys * 10 + dup)

    def frame(n):
        a = rng.integers(0, 6, n).astype(np.float64)
        a[rng.random(n) < 0.15] = np.nan
        b = np.array(["x", "y", "z", None], dtype=object)[rng.integers(0, 4, n)]
        c = rng.integers(0, 3, n).astype(np.float64)
        c[rng.random(n) < 0.15] = np.nan
        return pd.DataFrame({"a": a, "b": b, "c": c})

    keys = ["a", "b", "c"][:nkeys]
    ext = frame(300)[keys].drop_duplicates(ignore_index=True)
    if dup:
        ext = pd.concat([ext, ext.iloc[::2]], ignore_index=True)
    ext["v"] = np.arange(len(ext), dtype=np.int64)
    left = frame(4000)[keys].assign(z=np.arange(4000))
    _check(left, ext, keys, how)


@pytest.mark.parametrize("how", ["left", "inner"])
def test_one_key_with_1e5_external_rows(how):
    from nvtabular_amd import kernels as K

    rng = np.random.default_rng(5)
    keys = np.concatenate([np.full(100_000, 7), np.arange(100, 2000)]).astype(np.int64)
    rng.shuffle(keys)
    ext = pd.DataFrame({"k": keys, "v": np.arange(len(keys), dtype=np.int64)})
    left = pd.DataFrame({"k": np.array([7, 1, 150, 7, 99999, 7, 3000, 120], dtype=np.int64),
                         "x": np.arange(8, dtype=np.float32)})
    before = dict(K.STATS)
    _check(left, ext, "k", how)
    assert K.STATS.get("join_expand", 0) == before.get("join_expand", 0) + 1


@pytest.mark.parametrize("how", ["left", "inner"])
def test_empty_tables(how):
    rng = np.random.default_rng(2)
    left = pd.DataFrame({"k": rng.integers(0, 10, 100).astype(np.int64), "x": rng.random(100)})
    ext = pd.DataFrame({"k": np.zeros(0, np.int64), "v": np.zeros(0, np.float64)})
    _, out = _join(left, ext, "k", how)
    got = out.to_pandas()
    assert list(got.columns) == ["k", "x", "v"]
    assert len(got) == (100 if how == "left" else 0)
    assert got["v"].isna().all()
    np.testing.assert_array_equal(got["x"].to_numpy(), left["x"].to_numpy()[: len(got)])
    empty = left.iloc[:0]
    ext = pd.DataFrame({"k": np.arange(5, dtype=np.int64), "v": np.arange(5.0)})
    _, out = _join(empty, ext, "k", how)
    assert list(out.to_pandas().columns) == ["k", "x", "v"] and len(out) == 0


@pytest.mark.parametrize("how", ["left", "inner"])
def test_columns_ext_and_drop_duplicates(how):
    rng = np.random.default_rng(8)
    base = pd.DataFrame({"k": np.arange(50, dtype=np.int64), "a": np.arange(50) % 7,
                         "b": rng.random(50), "s": [f"s{i % 9}" for i in range(50)]})
    ext = pd.concat([base, base.iloc[::3]], ignore_index=True)   # whole-row duplicates
    ext.loc[len(ext)] = [3, 100, 0.5, "other"]                    # a real duplicate key
    left = pd.DataFrame({"k": rng.integers(0, 60, 999).astype(np.int64)})
    _check(left, ext, "k", how, columns_ext=["k", "s", "a"])
    _check(left, ext, "k", how, columns_ext=["s", "k"], drop_duplicates_ext=True)
    _check(left, ext, "k", how, drop_duplicates_ext=True)


def _carried_frame(n, rng):
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    lists = pd.Series([list(rng.integers(0, 9, rng.integers(0, 4))) for _ in range(n)], dtype=object)
    strs = pd.Series(np.array(["p", "q", None, "r"], dtype=object)[rng.integers(0, 4, n)])
    iv = pd.array(np.where(rng.random(n) < 0.3, None, rng.integers(0, 99, n)), dtype="Int64")
    fv = np.where(rng.random(n) < 0.3, np.nan, rng.random(n))
    left = pd.DataFrame({"k": rng.integers(0, 40, n).astype(np.int64), "l": lists, "s": strs, "iv": iv, "fv": fv})
    frame = DeviceFrame.from_pandas(left)
    fcol = frame["fv"]
    nan = torch.isnan(fcol.data)
    from nvtabular_amd.device import pack_bitmap_device

    frame["fv"] = DeviceColumn(torch.where(nan, torch.zeros_like(fcol.data), fcol.data),
                               pack_bitmap_device(~nan), None, -1.0)   # a pending FillMissing(-1)
    exp_left = left.assign(fv=left["fv"].fillna(-1.0))
    return frame, exp_left


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("dup", [False, True])
def test_left_columns_carried(how, dup):
    rng = np.random.default_rng(21 + dup)
    frame, exp_left = _carried_frame(3001, rng)
    keys = np.arange(0, 30, dtype=np.int64)
    if dup:
        keys = np.concatenate([keys, keys[::4]])
    ext = pd.DataFrame({"k": keys, "v": np.arange(len(keys)) * 0.5})
    _, out = _join(None, ext, "k", how, frame=frame)
    assert out["fv"].fill == -1.0
    assert out["s"].strings == frame["s"].strings
    _same(out.to_pandas(), _expected(exp_left, ext, "k", "k", how))
    _tail_bits_zero(out)


def test_left_unique_is_one_probe_gather_launch():
    from nvtabular_amd import kernels as K
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd import ops
    from nvtabular_amd.selector import ColumnSelector

    rng = np.random.default_rng(4)
    n = 100_000
    ext = pd.DataFrame({"k": np.arange(5000, dtype=np.int64)})
    for j in range(16):
        ext[f"p{j}"] = rng.integers(0, 1000, 5000).astype(np.int64 if j % 2 else np.float32)
    left = pd.DataFrame({"k": rng.integers(0, 6000, n).astype(np.int64), "x": rng.random(n)})
    frame = DeviceFrame.from_pandas(left)
    op = ops.JoinExternal(ext, on="k")
    sel = ColumnSelector(["k", "x"])
    op.transform(sel, frame)   # builds the index
    before = dict(K.STATS)
    out = op.transform(sel, frame)
    diff = {k: v - before.get(k, 0) for k, v in K.STATS.items() if v != before.get(k, 0)}
    assert diff == {"join_probe_gather": 1}
    for c in ("k", "x"):
        assert out[c].data.data_ptr() == frame[c].data.data_ptr()
    assert op.builds == 1
    _same(out.to_pandas(), _expected(left, ext, "k", "k", "left"))


def test_workflow_with_categorify_and_normalize(tmp_path):
    import pyarrow.parquet as pq

    import nvtabular_amd as nvt
    import oracle as O
    from nvtabular_amd import ops

    rng = np.random.default_rng(13)
    n = 30_000
    items = pa.table({"item": pa.array(np.arange(2000, dtype=np.int64)),
                      "brand": pa.array([f"b{i % 37}" if i % 11 else None for i in range(2000)]),
                      "price": pa.array(rng.lognormal(1, 1, 2000), mask=rng.random(2000) < 0.1),
                      "stock": pa.array(rng.integers(0, 50, 2000), pa.int64(), mask=rng.random(2000) < 0.2)})
    df = pd.DataFrame({"user": rng.integers(0, 500, n).astype(np.int64),
                       "item": rng.integers(0, 2500, n).astype(np.int64),
                       "y": rng.random(n).astype(np.float32)})
    ds = nvt.Dataset(df, npartitions=3)
    joined = ["user", "item", "y"] >> ops.JoinExternal(items, on="item")
    cat = joined["brand"] >> ops.Categorify(out_path=str(tmp_path / "gpu"))
    norm = joined["price"] >> ops.Normalize()
    wf = nvt.Workflow(cat + norm + joined["stock"])
    out = wf.fit_transform(ds)
    got = out.to_ddf().compute().reset_index(drop=True)

    merged = _expected(df, items.to_pandas(), "item", "item", "left")
    paths = O.categorify_fit([merged], ["brand"], str(tmp_path / "cpu"), tie_break="stable")
    exp = O.categorify_transform(merged, ["brand"], paths)
    np.testing.assert_array_equal(got["brand"].to_numpy(), exp["brand"].to_numpy())
    mom = O.custom_moments([merged], ["price"])
    exp = O.normalize_transform(merged, ["price"], mom["mean"].to_dict(), mom["std"].to_dict())
    np.testing.assert_allclose(got["price"].to_numpy(), exp["price"].to_numpy(), rtol=1e-6, atol=1e-9,
                               equal_nan=True)
    _same(got[["stock"]], merged[["stock"]])
    assert wf.output_dtypes["stock"] == np.dtype("int64")

    out.to_parquet(str(tmp_path / "out"))
    files = sorted((tmp_path / "out").glob("*.parquet"))
    table = pa.concat_tables([pq.read_table(f) for f in files])
    assert table.schema.field("stock").type == pa.int64()
    assert table.column("stock").null_count == int(merged["stock"].isna().sum())


def test_two_threads_build_once():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(31)
    ext = pd.DataFrame({"k": np.arange(1000, dtype=np.int64), "v": rng.random(1000)})
    df = pd.DataFrame({"k": rng.integers(0, 1200, 50_000).astype(np.int64), "x": rng.random(50_000)})
    op = ops.JoinExternal(ext, on="k")
    wf = nvt.Workflow(["k", "x"] >> op)
    wf.fit_schema(nvt.Dataset(df).schema)
    assert op.builds == 0
    results, errors = [None, None], []

    def run(i):
        try:
            results[i] = wf.transform(nvt.Dataset(df, npartitions=2)).to_ddf().compute()
        except Exception as e:   # pragma: no cover (reported below)
            errors.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    exp = _expected(df, ext, "k", "k", "left")
    for r in results:
        _same(r.reset_index(drop=True), exp)
    assert op.builds == 1


def test_large_external_arrow_table_with_strings():
    """An external Arrow table above the threaded-staging size of DeviceFrame.from_arrow, with a
    string column: the build (under LAUNCH_LOCK) converts it in the calling thread."""
    rng = np.random.default_rng(41)
    d = 70_000
    ext = pa.table({"k": pa.array(np.arange(d, dtype=np.int64) * 2),
                    "s": pa.array([f"n{i % 997}" for i in range(d)]),
                    "v": pa.array(rng.standard_normal(d))})
    left = pd.DataFrame({"k": rng.integers(0, 2 * d + 100, 20_000).astype(np.int64)})
    for how in ("left", "inner"):
        _check(left, ext, "k", how)
        _check(left, ext, "k", how, drop_duplicates_ext=True)   # (the concatenated-table path)
