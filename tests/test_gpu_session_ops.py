"""The session operators on the device: ops.ListSlice, ops.ValueCount and ops.DifferenceLag
(nvt_list.hip, kernels_list.py).  Expected values are computed here with plain Python slicing,
numpy and pandas; everything compares bit-equal (values, offsets, validity bitmaps, NaN
positions): the operators move data and make one IEEE subtraction, there is no tolerance."""
import zlib

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INT64_MAX = (1 << 63) - 1
SLICES = [(10,), (1, 11), (-10,), (-10, -2), (-5, 0), (0,), (1, -1)]
UNBOUNDED = [(0,), (1, -1)]
DTYPES = [np.uint8, np.bool_, np.int32, np.float32, np.int64, np.float64]


def _dev():
    return torch.device("cuda", 0)


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


def _list_column(vals, lens, valid=None, strings=None):
    from nvtabular_amd.device import DeviceColumn, pack_bitmap

    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    v = None if valid is None else torch.from_numpy(pack_bitmap(valid)).to(_dev())
    return DeviceColumn(torch.from_numpy(vals).to(_dev()), v, torch.from_numpy(off).to(_dev()), None, strings), off


def _normalise(args):
    """(start, end) as Python slices them; end None = to the end of the row."""
    start, end = (args[0], None) if len(args) == 1 else args
    if start > 0 and end is None:
        start, end = 0, start
    return start, end


def _rows_expected(vals, valid, off, args, pad_width, pad_value):
    """Per row: Python's row[start:end], then the padding -- (values, validity, offsets)."""
    start, end = _normalise(args)
    out_v, out_ok, lens = [], [], []
    for i in range(len(off) - 1):
        row = vals[off[i]: off[i + 1]][start:end]
        ok = (np.ones(off[i + 1] - off[i], dtype=bool) if valid is None else valid[off[i]: off[i + 1]])[start:end]
        if pad_width is not None:
            k = pad_width - len(row)
            row = np.concatenate([row, np.full(k, pad_value).astype(vals.dtype)])
            ok = np.concatenate([ok, np.ones(k, dtype=bool)])
        out_v.append(row)
        out_ok.append(ok)
        lens.append(len(row))
    new_off = np.zeros(len(off), dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    cat = np.concatenate(out_v) if out_v else vals[:0]
    return cat.astype(vals.dtype), (np.concatenate(out_ok) if out_ok else np.zeros(0, bool)), new_off


def _vector_expected(off, args, pad_width):
    """The same slice with vectorised numpy, for frames too large for a Python loop: the new
    offsets, and per output leaf its source leaf (-1 = a padded leaf)."""
    start, end = _normalise(args)
    L = np.diff(off)
    a = np.clip(L + start, 0, None) if start < 0 else np.minimum(start, L)
    if end is None:
        e = L
    else:
        e = np.clip(L + end, 0, None) if end < 0 else np.minimum(end, L)
    cnt = np.clip(e - a, 0, None)
    width = cnt if pad_width is None else np.full(len(L), pad_width, dtype=np.int64)
    new_off = np.zeros(len(off), dtype=np.int64)
    np.cumsum(width, out=new_off[1:])
    total = int(new_off[-1])
    k = np.arange(total, dtype=np.int64) - np.repeat(new_off[:-1], width)
    src = np.repeat(off[:-1] + a, width) + k
    if pad_width is not None:
        src[k >= np.repeat(cnt, width)] = -1
    return new_off, src


def _check(got, exp_vals, exp_ok, exp_off, had_bitmap, name=""):
    from nvtabular_amd.device import pack_bitmap

    assert got.offsets.dtype == torch.int64
    np.testing.assert_array_equal(got.offsets.cpu().numpy(), exp_off, err_msg=name)
    data = got.data.cpu().numpy()
    assert data.dtype == exp_vals.dtype and len(data) == len(exp_vals), name
    np.testing.assert_array_equal(data.view(np.uint8), exp_vals.view(np.uint8), err_msg=name)
    if not had_bitmap:
        assert got.valid is None, name
        return
    assert got.valid is not None and got.valid.dtype == torch.uint8, name
    raw = got.valid.cpu().numpy()
    assert len(raw) == (len(exp_vals) + 63) // 64 * 8, name
    np.testing.assert_array_equal(raw, pack_bitmap(exp_ok), err_msg=name)   # bits past the end are 0


def _slice(frame, names, args, pad=False, pad_value=0.0):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    return ops.ListSlice(*args, pad=pad, pad_value=pad_value).transform(nvt.ColumnSelector(names), frame)


def _mixed_lengths(rng, n, max_elements):
    lens = rng.integers(0, 41, n)
    lens[rng.random(n) < 0.2] = 0
    lens[rng.random(n) < 0.1] = 1
    lens[rng.random(n) < 0.1] = max_elements
    lens[:4] = [0, 1, max_elements, max_elements + 7]
    return lens.astype(np.int64)


@pytest.mark.parametrize("bitmap", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("args", SLICES, ids=str)
def test_list_slice_matrix(args, pad, dt, bitmap):
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    if pad and args in UNBOUNDED:
        with pytest.raises(ValueError):
            ops.ListSlice(*args, pad=True)
        return
    rng = np.random.default_rng(zlib.crc32(repr((args, pad, np.dtype(dt).name, bitmap)).encode()))
    op = ops.ListSlice(*args, pad=pad, pad_value=3.0)
    lens = _mixed_lengths(rng, 3000, op.max_elements or 10)
    vals = _values(dt, int(lens.sum()), rng)
    valid = (rng.random(len(vals)) < 0.8) if bitmap else None
    col, off = _list_column(vals, lens, valid)
    got = _slice(DeviceFrame({"c": col}), ["c"], args, pad, 3.0)["c"]
    exp = _rows_expected(vals, valid, off, args, op.max_elements if pad else None, 3.0)
    _check(got, *exp, bitmap, f"{args} pad={pad}")
    # the vectorised restatement used by the large cases agrees with the per-row one
    v_off, v_src = _vector_expected(off, args, op.max_elements if pad else None)
    np.testing.assert_array_equal(v_off, exp[2])
    v_vals = np.where(v_src >= 0, vals[np.clip(v_src, 0, None)], np.array(3.0).astype(vals.dtype))
    np.testing.assert_array_equal(v_vals.view(np.uint8), exp[0].view(np.uint8))


@pytest.mark.parametrize("pad", [False, True])
def test_list_slice_empty_and_all_empty(pad):
    from nvtabular_amd.device import DeviceFrame

    for n in (0, 5000):
        vals = np.zeros(0, dtype=np.float32)
        col, off = _list_column(vals, np.zeros(n, dtype=np.int64), np.zeros(0, dtype=bool))
        got = _slice(DeviceFrame({"c": col}), ["c"], (-4,), pad, 1.5)["c"]
        exp = _rows_expected(vals, np.zeros(0, dtype=bool), off, (-4,), 4 if pad else None, 1.5)
        _check(got, *exp, True, f"n={n}")
        assert len(got) == n


def _skewed(rng):
    lens = np.concatenate([[10_000_000], np.zeros(1_000_000, dtype=np.int64), rng.integers(1, 31, 1_000_000)])
    return lens.astype(np.int64)


@pytest.mark.parametrize("args, pad", [((-20,), False), ((-20,), True), ((1, -1), False), ((10,), True)], ids=str)
def test_list_slice_skewed_frame(args, pad):
    """One row of 10 M leaves, 1 M empty rows, then 1 M rows of 1-30 leaves."""
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    rng = np.random.default_rng(7)
    lens = _skewed(rng)
    total = int(lens.sum())
    a = rng.integers(-(2 ** 62), 2 ** 62, total).astype(np.int64)
    b = rng.standard_normal(total).astype(np.float32)
    ok = rng.random(total) < 0.9
    ca, off = _list_column(a, lens)
    cb, _ = _list_column(b, lens, ok)
    cb.offsets = ca.offsets
    got = _slice(DeviceFrame({"a": ca, "b": cb}), ["a", "b"], args, pad, -1.0)
    width = ops.ListSlice(*args, pad=pad).max_elements if pad else None
    new_off, src = _vector_expected(off, args, width)
    safe = np.clip(src, 0, None)
    _check(got["a"], np.where(src >= 0, a[safe], np.int64(-1)), None, new_off, False, "a")
    _check(got["b"], np.where(src >= 0, b[safe], np.float32(-1.0)).astype(np.float32),
           np.where(src >= 0, ok[safe], True), new_off, True, "b")
    assert got["a"].offsets is got["b"].offsets


def test_list_slice_string_leaves():
    from nvtabular_amd.device import DeviceFrame

    rows = [["a", "b", "c", "d"], [], ["e"], ["f", "a", "g"], ["h", "i", "j", "k", "l", "m"]] * 300
    df = pd.DataFrame({"s": rows})
    frame = DeviceFrame.from_pandas(df)
    assert frame["s"].strings is not None
    out = _slice(frame, ["s"], (-3,))
    assert out["s"].strings is frame["s"].strings
    got = out.to_pandas()["s"]
    for g, r in zip(got, rows):
        assert list(g) == r[-3:]
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    with pytest.raises(NotImplementedError):
        ops.ListSlice(-3, pad=True).transform(nvt.ColumnSelector(["s"]), frame)


def test_list_slice_pandas_in_pandas_out_and_fill_carried():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    rng = np.random.default_rng(3)
    rows = [list(rng.integers(0, 100, int(k))) for k in rng.integers(0, 9, 500)]
    rows[0] = [1, 2, 3, 4, 5, 6, 7]
    df = pd.DataFrame({"x": rows, "y": np.arange(500)})
    out = ops.ListSlice(1, 4, pad=True, pad_value=9).transform(nvt.ColumnSelector(["x"]), df)
    assert isinstance(out, pd.DataFrame) and list(out.columns) == ["x"]
    for g, r in zip(out["x"], rows):
        assert list(g) == (r[1:4] + [9] * 3)[:3]
    # a pending FillMissing constant travels with the column
    vals = np.arange(10, dtype=np.int64)
    col, off = _list_column(vals, np.array([4, 0, 6]), np.arange(10) % 3 != 0)
    col.fill = 5.0
    got = _slice(DeviceFrame({"c": col}), ["c"], (2,))["c"]
    assert got.fill == 5.0
    _check(got, *_rows_expected(vals, np.arange(10) % 3 != 0, off, (2,), None, 0), True)


@pytest.mark.parametrize("pad, grow", [(False, (1, 1, 1)), (True, (0, 1, 0))])
def test_list_slice_plan_sharing_and_counters(pad, grow):
    """Columns that share an offsets tensor are planned once, move in one launch and come back
    sharing one offsets tensor; the padded path reads nothing back."""
    from nvtabular_amd import kernels as K
    from nvtabular_amd.device import DeviceFrame

    rng = np.random.default_rng(11)
    lens = _mixed_lengths(rng, 4000, 20)
    total = int(lens.sum())
    a, off = _list_column(_values(np.int64, total, rng), lens)
    b, _ = _list_column(_values(np.int32, total, rng), lens)
    okc = rng.random(total) < 0.7
    c, _ = _list_column(_values(np.float32, total, rng), lens, okc)
    b.offsets = c.offsets = a.offsets
    frame = DeviceFrame({"a": a, "b": b, "c": c})
    before = {k: K.STATS.get(k, 0) for k in ("list_plan", "list_slice_many", "list_readback")}
    out = _slice(frame, ["a", "b", "c"], (-20,), pad, 0.0)
    after = {k: K.STATS.get(k, 0) for k in before}
    assert tuple(after[k] - before[k] for k in ("list_plan", "list_slice_many", "list_readback")) == grow
    assert out["a"].offsets is out["b"].offsets and out["b"].offsets is out["c"].offsets
    for name, col, ok in (("a", a, None), ("b", b, None), ("c", c, okc)):
        exp = _rows_expected(col.data.cpu().numpy(), ok, off, (-20,), 20 if pad else None, 0.0)
        _check(out[name], *exp, ok is not None, name)
    # a column with offsets of its own gets a plan of its own
    d, _ = _list_column(_values(np.int64, total, rng), lens)
    frame["d"] = d
    before = K.STATS.get("list_slice_many", 0)
    out = _slice(frame, ["a", "d"], (-20,), pad, 0.0)
    assert K.STATS.get("list_slice_many", 0) - before == 2
    assert out["a"].offsets is not out["d"].offsets


def test_list_slice_300m_leaves():
    """300 M int64 leaves (2.4 GB in, 2.35 GB out): byte offsets pass 2^31 on both sides."""
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    n = 3_000_000
    lens = 50 + (np.arange(n, dtype=np.int64) % 101)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    assert total > 299_000_000 and total * 8 > 2 ** 31
    data = torch.arange(total, dtype=torch.int64, device=_dev()) * 2654435761 + 12345
    col = DeviceColumn(data, None, torch.from_numpy(off).to(_dev()))
    got = _slice(DeviceFrame({"c": col}), ["c"], (1, -1))["c"]
    new_off, src = _vector_expected(off, (1, -1), None)
    assert int(new_off[-1]) * 8 > 2 ** 31
    np.testing.assert_array_equal(got.offsets.cpu().numpy(), new_off)
    out = got.data.cpu().numpy()
    del got, data, col
    src *= 2654435761
    src += 12345
    assert out.shape == src.shape
    assert np.array_equal(out, src)


# ---- ValueCount -------------------------------------------------------------------------------------
def test_value_count_fit_multi_partition():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceColumn, DeviceFrame
    from nvtabular_amd.schema import ColumnSchema, Schema

    rng = np.random.default_rng(5)
    parts, la, lb = [], [], []
    for p, n in enumerate((5000, 0, 1, 70_000)):
        lens_a = rng.integers(3, 50, n).astype(np.int64)
        lens_b = rng.integers(0, 9, n).astype(np.int64) + (2 if p == 0 else 0)
        a, _ = _list_column(np.zeros(int(lens_a.sum()), dtype=np.int32), lens_a)
        a2, _ = _list_column(np.zeros(int(lens_a.sum()), dtype=np.float32), lens_a)
        a2.offsets = a.offsets
        b, _ = _list_column(np.zeros(int(lens_b.sum()), dtype=np.int64), lens_b)
        flat = DeviceColumn(torch.zeros(n, dtype=torch.int64, device=_dev()))
        parts.append(DeviceFrame({"a": a, "a2": a2, "b": b, "flat": flat}))
        la.append(lens_a)
        lb.append(lens_b)
    la, lb = np.concatenate(la), np.concatenate(lb)
    op = ops.ValueCount()
    sel = nvt.ColumnSelector(["a", "a2", "b", "flat"])
    stats = op.fit(sel, parts).compute()
    op.fit_finalize(stats)
    exp_a = {"value_count": {"min": int(la.min()), "max": int(la.max())}}
    assert op.stats == {"a": exp_a, "a2": exp_a,
                        "b": {"value_count": {"min": int(lb.min()), "max": int(lb.max())}}}
    for v in op.stats.values():
        assert type(v["value_count"]["min"]) is int and type(v["value_count"]["max"]) is int
    assert op.transform(sel, parts[0]) is parts[0]
    schema = Schema([ColumnSchema("a", np.int32, is_list=True, is_ragged=True),
                     ColumnSchema("a2", np.float32, is_list=True, is_ragged=True),
                     ColumnSchema("b", np.int64, is_list=True, is_ragged=True), ColumnSchema("flat", np.int64)])
    out = op.compute_output_schema(schema, sel)
    assert out["a"].properties["value_count"] == exp_a["value_count"] and out["a"].is_ragged
    assert out["flat"].properties["value_count"] == {"min": 0, "max": None}
    op.clear()
    assert op.stats == {}
    # equal lengths: not ragged
    c, _ = _list_column(np.zeros(40, dtype=np.int32), np.full(10, 4))
    op.fit_finalize(op.fit(nvt.ColumnSelector(["c"]), [DeviceFrame({"c": c})]).compute())
    assert op.stats == {"c": {"value_count": {"min": 4, "max": 4}}}
    one = op.compute_output_schema(Schema([ColumnSchema("c", np.int32, is_list=True, is_ragged=True)]),
                                   nvt.ColumnSelector(["c"]))["c"]
    assert one.is_list and not one.is_ragged


# ---- DifferenceLag ----------------------------------------------------------------------------------
def _lag_expected(x, x_ok, keys, shift):
    """keys: [(values as an object / numeric array, non-null mask)]."""
    n = len(x)
    i = np.arange(n)
    j = i - shift
    inside = (j >= 0) & (j < n)
    jj = np.clip(j, 0, max(n - 1, 0))
    ok = inside & x_ok & x_ok[jj]
    for kv, kok in keys:
        ok &= kok & kok[jj] & (kv == kv[jj])
    with np.errstate(invalid="ignore", over="ignore"):
        if x.dtype == np.float32:
            d = x - x[jj]
        else:
            d = (x.astype(np.float64) - x[jj].astype(np.float64)).astype(np.float32)
    return np.where(ok, d, np.float32(np.nan)).astype(np.float32)


def _assert_lag_equal(got, exp, name=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == exp.shape, name
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=name)
    m = ~np.isnan(exp)
    np.testing.assert_array_equal(got[m].view(np.uint32), exp[m].view(np.uint32), err_msg=name)


def _sessions(rng, n, mean=6):
    """A grouped key column: runs of equal ids."""
    ids = np.cumsum(rng.random(n) < 1.0 / mean).astype(np.int64)
    return ids


@pytest.mark.parametrize("n", [1, 5, 100_000])
def test_difference_lag_shifts_and_dtypes(n):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap

    rng = np.random.default_rng(n)
    user = _sessions(rng, n)
    cols = {
        "i64": (rng.integers(2 ** 60 - 1000, 2 ** 60 + 1000, n).astype(np.int64) + user * 3),
        "i32": rng.integers(-(2 ** 31), 2 ** 31 - 1, n).astype(np.int32),
        "f32": (rng.standard_normal(n) * 1e3).astype(np.float32),
        "f64": rng.standard_normal(n) * 1e10,
    }
    for name in ("f32", "f64"):
        cols[name][rng.random(n) < 0.05] = np.nan
        cols[name][rng.random(n) < 0.05] = np.inf
        cols[name][rng.random(n) < 0.02] = -np.inf
    ok = rng.random(n) < 0.85
    frame = DeviceFrame({k: DeviceColumn(torch.from_numpy(v).to(_dev())) for k, v in cols.items()})
    frame["i64m"] = DeviceColumn(frame["i64"].data, torch.from_numpy(pack_bitmap(ok)).to(_dev()))
    frame["user"] = DeviceColumn(torch.from_numpy(user).to(_dev()))
    shifts = list(dict.fromkeys([1, -1, 2, -3, 0, n, -n, n + 5, -(n + 5), 2 ** 40]))
    op = ops.DifferenceLag("user", shift=shifts)
    names = ["i64", "i32", "f32", "f64", "i64m"]
    from nvtabular_amd import kernels as K

    before = K.STATS.get("difference_lag_many", 0)
    out = op.transform(nvt.ColumnSelector(names), frame)
    assert K.STATS.get("difference_lag_many", 0) - before == 1   # every output from ONE launch
    assert out.columns == [f"{c}_difference_lag_{s}" for c in names for s in shifts]
    all_ok = np.ones(n, dtype=bool)
    for c in names:
        x = cols["i64"] if c == "i64m" else cols[c]
        for s in shifts:
            col = out[f"{c}_difference_lag_{s}"]
            assert col.valid is None and col.offsets is None
            exp = _lag_expected(x, ok if c == "i64m" else all_ok, [(user, all_ok)], s)
            _assert_lag_equal(col.data, exp, f"{c} shift {s}")
    if n > 1000:   # the float64-first rule is visible: int64 subtraction would give other bits
        exact = (cols["i64"][1:] - cols["i64"][:-1]).astype(np.float32)
        same = user[1:] == user[:-1]
        got = out["i64_difference_lag_1"].data.cpu().numpy()[1:]
        assert (got[same] != exact[same]).any()


def test_difference_lag_matches_pandas_expression():
    """The reference's pandas formula on a small frame: (x - x.shift(s)) masked by the partition
    test, cast to float32."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(9)
    n = 4000
    df = pd.DataFrame({
        "user": _sessions(rng, n),
        "ts": rng.integers(2 ** 60, 2 ** 60 + 10 ** 6, n).astype(np.int64),
        "v": rng.standard_normal(n),
        "w": rng.integers(-1000, 1000, n).astype(np.int32),
    })
    out = ops.DifferenceLag(["user"], shift=[1, -1, 3]).transform(nvt.ColumnSelector(["ts", "v", "w"]), df)
    assert isinstance(out, pd.DataFrame)
    for s in (1, -1, 3):
        mask = (df["user"] == df["user"].shift(s)).to_numpy()
        for c in ("ts", "v", "w"):
            exp = (df[c] - df[c].shift(s)).to_numpy(dtype=np.float64)
            exp = np.where(mask, exp, np.nan).astype(np.float32)
            _assert_lag_equal(out[f"{c}_difference_lag_{s}"].to_numpy(), exp, f"{c} {s}")


def test_difference_lag_three_partition_columns():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    rng = np.random.default_rng(21)
    n = 60_000
    user = _sessions(rng, n, 12)
    words = np.array(["web", "app", "tv", None], dtype=object)
    chan = words[(np.cumsum(rng.random(n) < 0.15) + rng.integers(0, 2, 1)) % 4]
    day = np.cumsum(rng.random(n) < 0.1).astype(np.float64)
    day_null = rng.random(n) < 0.03
    x = rng.integers(0, 2 ** 40, n).astype(np.int64)
    df = pd.DataFrame({
        "user": user,
        "chan": chan,
        "day": pd.array(day.astype(np.int64), dtype="Int64"),
        "x": x,
    })
    df.loc[day_null, "day"] = pd.NA
    frame = DeviceFrame.from_pandas(df)
    assert frame["chan"].strings is not None and frame["day"].valid is not None
    op = ops.DifferenceLag(["user", "chan", "day"], shift=[1, -2])
    out = op.transform(nvt.ColumnSelector(["x"]), frame)
    chan_ok = np.array([c is not None for c in chan])
    chan_cmp = np.where(chan_ok, chan, "").astype(str)
    keys = [(user, np.ones(n, bool)), (chan_cmp, chan_ok), (day, ~day_null)]
    for s in (1, -2):
        _assert_lag_equal(out[f"x_difference_lag_{s}"].data, _lag_expected(x, np.ones(n, bool), keys, s), str(s))
    with pytest.raises(NotImplementedError):
        ops.DifferenceLag(["user", "chan", "day", "x", "user"]).transform(nvt.ColumnSelector(["x"]), frame)


def test_difference_lag_10m_rows_and_pending_fill():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceColumn, DeviceFrame, pack_bitmap

    rng = np.random.default_rng(2)
    n = 10_000_000
    user = _sessions(rng, n, 8).astype(np.int32)
    ts = np.cumsum(rng.integers(0, 1000, n)).astype(np.int64) + 2 ** 58
    ok = rng.random(n) < 0.9
    frame = DeviceFrame({
        "user": DeviceColumn(torch.from_numpy(user).to(_dev())),
        "ts": DeviceColumn(torch.from_numpy(ts).to(_dev())),
        "q": DeviceColumn(torch.from_numpy(ts).to(_dev()), torch.from_numpy(pack_bitmap(ok)).to(_dev()),
                          None, 7.0),   # a pending FillMissing constant counts as the value
    })
    out = ops.DifferenceLag("user", shift=[1, -1]).transform(nvt.ColumnSelector(["ts", "q"]), frame)
    all_ok = np.ones(n, dtype=bool)
    filled = np.where(ok, ts, 7)
    for s in (1, -1):
        _assert_lag_equal(out[f"ts_difference_lag_{s}"].data, _lag_expected(ts, all_ok, [(user, all_ok)], s))
        _assert_lag_equal(out[f"q_difference_lag_{s}"].data, _lag_expected(filled, all_ok, [(user, all_ok)], s))


# ---- the session pipeline -----------------------------------------------------------------------------
def test_session_pipeline_through_workflow():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(17)
    n = 2_000_000
    df = pd.DataFrame({
        "user_id": rng.integers(0, 60_000, n).astype(np.int64),
        "item_id": (rng.zipf(1.2, n) % 50_000).astype(np.int64),
        "ts": rng.integers(0, 1_000_000, n).astype(np.int64),
    }).sort_values(["user_id", "ts"], kind="stable").reset_index(drop=True)

    def graph(with_slice):
        feats = ["item_id", "ts"] >> ops.Categorify()
        lag = ["ts"] >> ops.DifferenceLag(partition_cols=["user_id"], shift=[1, -1])
        groups = (feats + lag + ["user_id"]) >> ops.Groupby(
            groupby_cols=["user_id"], sort_cols=["ts"], aggs={"item_id": ["list", "count"], "ts": ["list"]})
        lists = groups["item_id_list", "ts_list"]
        if with_slice:
            return lists >> ops.ListSlice(-20, pad=True) >> ops.ValueCount()
        return lists

    ds = nvt.Dataset(df)
    base_wf = nvt.Workflow(graph(False))
    base = base_wf.fit_transform(ds).to_ddf().compute()
    wf = nvt.Workflow(graph(True))
    wf.fit(ds)
    out = wf.transform(ds).to_ddf().compute()
    assert list(out.columns) == ["item_id_list", "ts_list"] and len(out) == len(base) > 50_000
    for c in ("item_id_list", "ts_list"):
        lens = base[c].map(len).to_numpy()
        assert lens.max() > 20 and lens.min() < 20   # both the cut and the padding are exercised
        exp = np.zeros((len(base), 20), dtype=np.asarray(base[c].iloc[0]).dtype)
        for i, row in enumerate(base[c]):
            tail = np.asarray(row)[-20:]
            exp[i, : len(tail)] = tail
        got = np.stack([np.asarray(r) for r in out[c]])
        assert got.dtype == exp.dtype
        np.testing.assert_array_equal(got, exp)
        sch = wf.output_schema[c]
        assert sch.properties["value_count"] == {"min": 20, "max": 20}
        assert sch.is_list and not sch.is_ragged
    # the lag columns of the same graph, on their own
    lag_out = nvt.Workflow(["ts"] >> ops.DifferenceLag(partition_cols=["user_id"], shift=[1, -1])) \
        .fit_transform(ds).to_ddf().compute()
    ones = np.ones(n, dtype=bool)
    for s in (1, -1):
        exp = _lag_expected(df["ts"].to_numpy(), ones, [(df["user_id"].to_numpy(), ones)], s)
        _assert_lag_equal(lag_out[f"ts_difference_lag_{s}"].to_numpy(), exp)


# ---- paths the C interface promises ---------------------------------------------------------------------
def test_list_slice_nonzero_first_offset_and_40_columns():
    """offsets[0] != 0 (leaf 0 of the values is the leaf offsets[0] names), and more columns than
    one launch's descriptor batch (NVT_LIST_MAX_COLS = 32)."""
    from nvtabular_amd import _lib
    from nvtabular_amd.device import DeviceFrame

    rng = np.random.default_rng(41)
    lens = _mixed_lengths(rng, 5000, 7)
    total = int(lens.sum())
    cols, off, host = {}, None, {}
    shared = None
    for k in range(_lib.LIST_MAX_COLS + 8):
        dt = DTYPES[k % len(DTYPES)]
        vals = _values(dt, total, rng)
        ok = (rng.random(total) < 0.8) if k % 3 == 0 else None
        col, off = _list_column(vals, lens, ok)
        if shared is None:
            shared = col.offsets + 12345   # a sliced Arrow array: the offsets do not start at 0
        col.offsets = shared
        cols[f"c{k}"], host[f"c{k}"] = col, (vals, ok)
    frame = DeviceFrame(cols)
    for args, pad in (((-7,), False), ((2, 9), True)):
        out = _slice(frame, list(cols), args, pad, 1.0)
        for name, (vals, ok) in host.items():
            exp = _rows_expected(vals, ok, off, args, 7 if pad else None, 1.0)
            _check(out[name], *exp, ok is not None, f"{name} {args}")
        assert all(out[name].offsets is out["c0"].offsets for name in cols)


def test_difference_lag_40_outputs_numpy_shift_bool_partition():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(43)
    n = 30_000
    user = _sessions(rng, n)
    flag = (np.cumsum(rng.random(n) < 0.3) % 2).astype(bool)   # a bool partition column: by value
    xs = {f"x{k}": rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int64) for k in range(5)}
    frame = DeviceFrame({k: DeviceColumn(torch.from_numpy(v).to(_dev())) for k, v in xs.items()})
    frame["user"] = DeviceColumn(torch.from_numpy(user).to(_dev()))
    frame["flag"] = DeviceColumn(torch.from_numpy(flag).to(_dev()))
    shifts = [np.int64(1), np.int32(-1), 2, -2, 3, -3, 5, -7]
    op = ops.DifferenceLag(["user", "flag"], shift=shifts)
    assert op.shifts == [1, -1, 2, -2, 3, -3, 5, -7] and all(type(s) is int for s in op.shifts)
    assert ops.DifferenceLag("user", shift=np.int64(3)).shifts == [3]
    out = op.transform(nvt.ColumnSelector(list(xs)), frame)   # 40 outputs: two descriptor batches
    assert len(out.columns) == 40
    ones = np.ones(n, dtype=bool)
    for name, x in xs.items():
        for s in op.shifts:
            exp = _lag_expected(x, ones, [(user, ones), (flag, ones)], s)
            _assert_lag_equal(out[f"{name}_difference_lag_{s}"].data, exp, f"{name} {s}")


def test_value_count_shared_in_one_partition_only():
    """Two columns with offsets of their own in the first partition and ONE offsets tensor in the
    second: each keeps its own lengths from the first."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame

    la, lb, lc = np.array([1, 2, 3]), np.array([10, 11, 12]), np.array([5, 6, 5, 6])
    a1, _ = _list_column(np.zeros(int(la.sum()), dtype=np.int32), la)
    b1, _ = _list_column(np.zeros(int(lb.sum()), dtype=np.int32), lb)
    a2, _ = _list_column(np.zeros(int(lc.sum()), dtype=np.int32), lc)
    b2, _ = _list_column(np.zeros(int(lc.sum()), dtype=np.int32), lc)
    b2.offsets = a2.offsets
    parts = [DeviceFrame({"a": a1, "b": b1}), DeviceFrame({"a": a2, "b": b2})]
    for order in (parts, parts[::-1]):
        op = ops.ValueCount()
        op.fit_finalize(op.fit(nvt.ColumnSelector(["a", "b"]), order).compute())
        assert op.stats == {"a": {"value_count": {"min": 1, "max": 6}},
                            "b": {"value_count": {"min": 5, "max": 12}}}


def test_encode_keeps_ordering_buffers_until_the_call_is_enqueued(monkeypatch, tmp_path):
    """A vocabulary that an internal stream is still ordering keeps its scratch, counts and source
    list while the descriptors of nvt_encode_many are filled (the outputs of the other columns are
    allocated in between and must not land on them) and lets them go behind the call."""
    import nvtabular_amd as nvt
    from nvtabular_amd import _lib, ops
    from nvtabular_amd import kernels as K
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(47)
    n = 2_000_000
    host = {c: rng.integers(0, 300_000, n).astype(np.int32) * 3 for c in ("c", "d", "e")}
    frame = DeviceFrame({k: DeviceColumn(torch.from_numpy(v).to(_dev())) for k, v in host.items()})
    lib = _lib.load()
    tabs, held = [], []
    fill, call = K.EncodeTable.fill_encode_desc, lib.nvt_encode_many

    def spy_fill(self, *args):
        was = self.pending
        fill(self, *args)
        if was:
            tabs.append(self)
            held.append(self.sort_tmp is not None and self._counts is not None)

    def spy_call(descs, k, stream):
        held.extend(t.sort_tmp is not None and t._counts is not None for t in tabs)
        return call(descs, k, stream)

    monkeypatch.setattr(K.EncodeTable, "fill_encode_desc", spy_fill)
    monkeypatch.setattr(lib, "nvt_encode_many", spy_call)
    # (artifacts deferred, as in bench.py: nothing reads the vocabularies between fit and transform)
    wf = nvt.Workflow(list(host) >> ops.Categorify(out_path=str(tmp_path), defer_artifacts=True))
    wf.fit(nvt.Dataset(frame))
    out = wf.transform(frame)
    assert tabs, "no vocabulary was still being ordered when the encode was enqueued"
    assert held and all(held)
    assert all(t.sort_tmp is None and t._counts is None and t._src is None for t in tabs)
    for c, v in host.items():   # and the labels are right: frequency order, ties by key
        keys, counts = np.unique(v, return_counts=True)
        order = np.lexsort((keys, -counts))
        label = np.empty(len(keys), dtype=np.int64)
        label[order] = np.arange(len(keys)) + 3
        np.testing.assert_array_equal(out[c].data.cpu().numpy(), label[np.searchsorted(keys, v)])
