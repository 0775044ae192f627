"""List columns through Dataset.to_parquet's hand-written PLAIN writer on the device: the level
kernels (nvt_pqlist_*) against the numpy reference byte for byte, then whole files read back with
pyarrow and with this package."""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import pq_list_reference as R

pytestmark = pytest.mark.gpu

PAGE = 64
GUARD = 64
PLAIN = "nvtabular_amd plain writer"


def dev():
    return torch.device("cuda:0")


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return off


def _bitmap(valid):
    from nvtabular_amd.device import pack_bitmap

    return torch.from_numpy(pack_bitmap(np.asarray(valid, dtype=bool))).to(dev())


def _check(off, valids, r0=0, r1=None, page=PAGE, first=0):
    """pack_levels of rows [r0, r1) against the reference: page table, rep bytes, def bytes and
    non-null counts of every column, guard bytes and the unused tail of every buffer untouched.
    ``first``: offsets[0] (the offsets are shifted by it: leaf 0 of the bitmaps is that leaf)."""
    from nvtabular_amd import kernels_parquet_list as KPL

    off = np.asarray(off, dtype=np.int64)
    r1 = len(off) - 1 if r1 is None else r1
    d_off = torch.from_numpy(off + first).to(dev())
    bitmaps = [None if v is None else _bitmap(v) for v in valids]
    dl = KPL.pack_levels(d_off, r0, r1, bitmaps, int(off[-1]), page, guard=GUARD)
    lt = dl.read_back()
    torch.cuda.synchronize()
    ref = [R.list_pages(off, v, r0, r1, page) for v in valids]
    pages = ref[0]
    assert lt.npages == len(pages)
    np.testing.assert_array_equal(lt.row0, [p["row0"] for p in pages])
    np.testing.assert_array_equal(lt.rows, [p["rows"] for p in pages])
    np.testing.assert_array_equal(lt.slot0, [p["slot0"] for p in pages])
    np.testing.assert_array_equal(lt.slots, [p["slots"] for p in pages])
    np.testing.assert_array_equal(lt.leaves, [p["leaves"] for p in pages])
    assert lt.total_slots == sum(p["slots"] for p in pages)
    assert (lt.leaf_lo, lt.leaf_hi) == (int(off[r0]), int(off[r1]))
    rep = dl.rep.cpu().numpy()
    defs = [d.cpu().numpy() for d in dl.defs]
    for j, pj in enumerate(ref):
        st = dl.stream_of[j]
        np.testing.assert_array_equal(lt.nonnull[st], [p["nonnull"] for p in pj], err_msg=f"column {j}")
        for p, page_ref in enumerate(pj):
            a, b = int(lt.rep_at[p]), int(lt.def_at[p])
            assert rep[a: a + len(page_ref["rep"])].tobytes() == page_ref["rep"], (j, p)
            assert defs[st][b: b + len(page_ref["dfn"])].tobytes() == page_ref["dfn"], (j, p)
    # nothing outside what the table names: guards, and the buffers behind the bytes in use
    meta_raw, rep_raw, defs_raw = dl.raw
    for raw, used in [(meta_raw, None), (rep_raw, lt.rep_bytes)] + [(r, lt.def_bytes) for r in defs_raw]:
        h = raw.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[-GUARD:] == 0xA5).all()
        if used is not None:
            assert (h[GUARD + used: -GUARD] == 0xA5).all()
    return dl, lt


@pytest.fixture(scope="module")
def mixed():
    """Lengths 0..5, a row of more than three pages, 3000 consecutive empty rows, empty rows first and
    last; two bitmaps with 10 % / 50 % null leaves."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(0, 6, 1500), np.zeros(3000, dtype=np.int64), rng.integers(0, 6, 1500)])
    lens[0] = lens[-1] = 0
    lens[700] = 3 * PAGE + 17
    off = _offsets(lens)
    leaves = int(off[-1])
    return off, rng.random(leaves) >= 0.1, rng.random(leaves) >= 0.5


@pytest.mark.parametrize("lens", [[0], [1], [7], [3, 0, 3], [8], [4, 4], [9], [0] * 9, [5, 0, 0, 2],
                                  [PAGE], [PAGE + 1], [0, PAGE - 1, 1]])
def test_smallest_streams(lens):
    """1, 7, 8 and 9 slots and the sizes around one page: whole-word stores must not show."""
    off = _offsets(lens)
    rng = np.random.default_rng(len(lens) * 131 + int(off[-1]))
    _check(off, [None, rng.random(int(off[-1])) >= 0.3])


def test_mixed_rows_pages_and_sharing(mixed):
    """Pages whose slot count is no multiple of 8, dropped pages, three columns that share the
    offsets: ONE plan, one repetition stream, one definition stream for the columns without a
    bitmap and one per bitmap."""
    from nvtabular_amd import kernels as K

    off, v1, v2 = mixed
    before = dict(K.STATS)
    dl, lt = _check(off, [None, v1, None, v2])
    assert K.STATS.get("pqlist_plan", 0) - before.get("pqlist_plan", 0) == 1
    assert K.STATS.get("pqlist_readback", 0) - before.get("pqlist_readback", 0) == 1
    assert dl.stream_of == [0, 1, 0, 2] and len(dl.defs) == 3
    assert (lt.slots % 8 != 0).any() and lt.npages < -(-lt.total_slots // PAGE)
    assert lt.slots.max() > 3 * PAGE


def test_empty_run_past_the_lds_stage(mixed):
    """3000 empty rows are 3000 slots in a row: with pages of 4096 slots a 2048-slot tile spans more
    rows than the LDS stage holds and takes the global-memory search; with pages of 64 slots every
    tile is staged.  Both against the reference."""
    off, v1, _ = mixed
    _check(off, [None, v1], 1400, 4600, page=PAGE)
    _check(off, [None, v1], 1400, 4600, page=4096)
    _check(off, [v1], page=1 << 20)      # one page, many tiles


def test_row_range_starting_inside_a_bitmap_byte(mixed):
    off, v1, _ = mixed
    lens = np.diff(off)
    lens[:2] = [3, 2]
    off = _offsets(lens)
    v = np.resize(v1, int(off[-1]))
    assert off[1] == 3
    _check(off, [v, None], 1, 900)        # the first leaf of the range is bit 3
    _check(off, [v], 1, 2)                # one row
    _check(off, [v, None], 0, 900, first=11)   # offsets[0] != 0: leaf 11 is bit 0 of the bitmap


def test_null_leaves_at_page_edges():
    """All leaves null; a null leaf first and last in a page."""
    lens = np.full(40, 16)                # pages of exactly 64 slots, 4 rows each
    off = _offsets(lens)
    leaves = int(off[-1])
    edges = np.ones(leaves, dtype=bool)
    edges[0::PAGE] = False
    edges[PAGE - 1::PAGE] = False
    _, lt = _check(off, [np.zeros(leaves, dtype=bool), edges, None])
    assert (lt.slots == PAGE).all() and lt.npages == 10


def test_more_columns_than_one_launch_takes(mixed):
    from nvtabular_amd import _lib

    off, _, _ = mixed
    rng = np.random.default_rng(9)
    off = off[:1201]
    valids = [rng.random(int(off[-1])) >= 0.2 for _ in range(_lib.PQLIST_MAX_COLS + 1)]
    dl, _ = _check(off, valids)
    assert len(dl.defs) == _lib.PQLIST_MAX_COLS + 1


def test_offsets_outside_the_leaves_are_refused():
    """The buffers are sized from the leaves the columns hold: offsets that name more are an error,
    nothing is written past the buffers."""
    from nvtabular_amd import _lib
    from nvtabular_amd import kernels_parquet_list as KPL

    off = torch.from_numpy(_offsets([1000, 2000, 3000])).to(dev())
    dl = KPL.pack_levels(off, 0, 3, [None], 10, PAGE, guard=GUARD)
    with pytest.raises(_lib.NvtHipError, match="do not fit"):
        dl.read_back()
    torch.cuda.synchronize()
    for raw in (dl.raw[1], dl.raw[2][0]):
        assert (raw.cpu().numpy() == 0xA5).all()


# ---- whole files --------------------------------------------------------------------------------------
def _frame(rows=5000, seed=3):
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, rows)
    lens[0] = lens[-1] = 0
    lens[rows // 2] = 300
    off = _offsets(lens)
    leaves = int(off[-1])
    a = rng.integers(-2**62, 2**62, leaves).astype(np.int64)
    a_ok = rng.random(leaves) >= 0.1
    b = rng.normal(size=leaves).astype(np.float32)
    b[rng.random(leaves) < 0.05] = np.nan
    x = rng.normal(size=rows).astype(np.float32)
    x_ok = rng.random(rows) >= 0.2
    d_off = torch.from_numpy(off).to(dev())
    t = lambda v: torch.from_numpy(v).to(dev())
    return DeviceFrame({
        "id": DeviceColumn(t(rng.permutation(rows).astype(np.int64))),
        "a": DeviceColumn(t(a), _bitmap(a_ok), d_off),
        "x": DeviceColumn(t(x), _bitmap(x_ok)),
        "b": DeviceColumn(t(b), None, d_off),
    })


def _columns(table, by=None):
    """{column: (offsets or None, validity, value bits)} of an Arrow table, rows ordered by `by`."""
    if by is not None:
        table = table.take(pa.array(np.argsort(np.asarray(table.column(by)), kind="stable")))
    out = {}
    for name in table.column_names:
        arr = table.column(name).combine_chunks()
        off = None
        if pa.types.is_list(arr.type) or pa.types.is_large_list(arr.type):
            assert arr.null_count == 0
            off = np.asarray(arr.offsets, dtype=np.int64)
            off = off - off[0]
            arr = arr.flatten()
        ok = ~np.asarray(arr.is_null())
        vals = np.asarray(arr.fill_null(0))
        out[name] = (off, ok, np.where(ok, vals.view(f"u{vals.dtype.itemsize}"), 0))
    return out


def _assert_same(got, exp):
    assert list(got) == list(exp)
    for name in exp:
        for g, e, what in zip(got[name], exp[name], ("offsets", "validity", "value bits")):
            if e is None:
                assert g is None, (name, what)
            else:
                np.testing.assert_array_equal(g, e, err_msg=f"{name}: {what}")


@pytest.mark.parametrize("rows, k", [(5000, None), (5000, 3), (40, 50)])
@pytest.mark.parametrize("shuffle", [None, "PER_PARTITION"])
def test_to_parquet_list_columns_end_to_end(tmp_path, monkeypatch, rows, k, shuffle):
    """Row groups of 1000 rows and pages of 64 slots; k = 3 cuts the partition at arbitrary rows; k = 50
    is more files than rows, so most pieces have no row and must still be files pyarrow reads."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import kernels as K
    from nvtabular_amd.io import Shuffle

    from nvtabular_amd import parquet_plain as PP

    monkeypatch.setattr(nio, "PLAIN_ROW_GROUP", 1000)
    monkeypatch.setattr(PP, "PAGE_VALUES", PAGE)      # many pages per chunk, one of them the 300-leaf row's
    frame = _frame(rows)
    exp = _columns(frame.to_arrow(), by="id")
    out = str(tmp_path / "out")
    before = dict(K.STATS)
    nvt.Dataset(frame).to_parquet(out, out_files_per_proc=k,
                                  shuffle=getattr(Shuffle, shuffle) if shuffle else None)
    files = sorted(f for f in os.listdir(out) if f.endswith(".parquet"))
    assert len(files) == (k or 1)
    for f in files:
        assert pq.read_metadata(os.path.join(out, f)).created_by == PLAIN
    if shuffle is None and k is None:
        # "a" and "b" share their offsets: one plan and one read-back per row group of 1000 rows
        assert K.STATS.get("pqlist_plan", 0) - before.get("pqlist_plan", 0) == 5
        assert K.STATS.get("pqlist_readback", 0) - before.get("pqlist_readback", 0) == 5
    by_index = sorted(files, key=lambda f: int(f.split("_")[1].split(".")[0]))
    table = pa.concat_tables([pq.read_table(os.path.join(out, f)) for f in by_index])
    got = _columns(table, by="id")
    _assert_same(got, exp)
    if shuffle is None:
        _assert_same(_columns(table), _columns(frame.to_arrow()))     # row order kept
    else:
        assert not np.array_equal(np.asarray(table.column("id")), frame["id"].data.cpu().numpy())
    assert os.path.exists(os.path.join(out, "_metadata"))
    assert pq.read_metadata(os.path.join(out, "_metadata")).num_rows == len(frame)
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(out).to_iter()])
    _assert_same(_columns(back, by="id"), exp)


@pytest.mark.parametrize("change", ["dtype", "list_column_gone"])
def test_schema_change_between_partitions_leaves_no_file(tmp_path, change):
    """Two partitions of 100 rows go to part_0; the second does not have the file's schema (int32 for
    int64, or a list column missing): its flush raises and the footer-less file is removed."""
    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    t = lambda v: torch.from_numpy(v).to(dev())
    first = {"a": DeviceColumn(t(np.arange(100, dtype=np.int64)))}
    second = {"a": DeviceColumn(t(np.arange(100, dtype=np.int32 if change == "dtype" else np.int64)))}
    if change == "list_column_gone":
        first["l"] = DeviceColumn(t(np.arange(200, dtype=np.int64)), None, t(_offsets([2] * 100)))
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="differs from the schema"):
        nvt.Dataset([DeviceFrame(first), DeviceFrame(second)]).to_parquet(out, out_files_per_proc=1)
    assert not [f for f in os.listdir(out) if f.endswith(".parquet")]


def test_statistics_of_list_columns(tmp_path):
    """min / max over the non-null leaves, null_count = slots - non-null leaves."""
    import nvtabular_amd as nvt

    frame = _frame(rows=1200, seed=8)
    out = str(tmp_path / "out")
    nvt.Dataset(frame).to_parquet(out, statistics=True)
    md = pq.read_metadata(os.path.join(out, "part_0.parquet"))
    exp = _columns(frame.to_arrow())
    names = [md.schema.column(j).path for j in range(md.num_columns)]
    assert names == ["id", "a.list.element", "x", "b.list.element"]
    off, ok, bits = exp["a"]
    slots = int(np.maximum(np.diff(off), 1).sum())
    st = md.row_group(0).column(1).statistics
    vals = bits.view(np.int64)[ok]
    assert md.row_group(0).column(1).num_values == slots
    assert (st.min, st.max, st.null_count) == (int(vals.min()), int(vals.max()), slots - int(ok.sum()))


def test_session_pipeline_to_parquet(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = np.random.default_rng(17)
    n = 20_000
    df = pd.DataFrame({
        "user_id": rng.integers(0, 3000, n).astype(np.int64),
        "item_id": rng.integers(0, 5000, n).astype(np.int64),
        "ts": rng.integers(0, 1_000_000, n).astype(np.int64),
    }).sort_values(["user_id", "ts"], kind="stable").reset_index(drop=True)
    groups = ["user_id", "item_id", "ts"] >> ops.Groupby(
        groupby_cols=["user_id"], sort_cols=["ts"], aggs={"item_id": ["list", "first", "count"], "ts": ["list"]})
    lists = groups["item_id_list", "ts_list"] >> ops.ListSlice(-5)
    wf = nvt.Workflow(lists + groups["user_id", "item_id_first", "item_id_count"])
    ds = nvt.Dataset(df)
    wf.fit(ds)
    exp = pa.concat_tables([p.to_arrow() for p in wf.transform(ds).to_iter()])
    assert pa.types.is_large_list(exp.schema.field("item_id_list").type) and exp.num_rows > 1000
    out = str(tmp_path / "out")
    wf.transform(ds).to_parquet(out)
    files = sorted(f for f in os.listdir(out) if f.endswith(".parquet"))
    assert files and all(pq.read_metadata(os.path.join(out, f)).created_by == PLAIN for f in files)
    back = pa.concat_tables([p.to_arrow() for p in nvt.Dataset(out).to_iter()])
    assert back.column_names == exp.column_names
    _assert_same(_columns(back, by="user_id"), _columns(exp, by="user_id"))
    lens = np.diff(_columns(back)["item_id_list"][0])
    assert lens.max() == 5 and lens.min() < 5


def test_what_still_goes_to_pyarrow(tmp_path, monkeypatch):
    """String leaves, a dtypes= entry naming a list column, a codec, Shuffle.PER_WORKER with
    out_files_per_proc and NVT_PLAIN_PARQUET=0: pyarrow's writer, as before."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio

    def created_by(ds, name, **kw):
        out = str(tmp_path / name)
        ds.to_parquet(out, **kw)
        files = sorted(f for f in os.listdir(out) if f.endswith(".parquet"))
        assert files
        return [pq.read_metadata(os.path.join(out, f)).created_by for f in files], \
            pa.concat_tables([pq.read_table(os.path.join(out, f)) for f in files])

    strings = pd.DataFrame({"s": [["a", "bc"], [], ["d"]], "y": np.arange(3)})
    made, table = created_by(nvt.Dataset(strings), "strings")
    assert all(m != PLAIN for m in made)
    assert table.column("s").to_pylist() == [["a", "bc"], [], ["d"]]

    frame = _frame(rows=500, seed=4)
    exp = _columns(frame.to_arrow())
    # a cast of a list column is not taken by the PLAIN writer; pyarrow's cast, which the request
    # then reaches as it always did, has no list -> number conversion and says so
    with pytest.raises(pa.ArrowNotImplementedError, match="large_list"):
        nvt.Dataset(frame).to_parquet(str(tmp_path / "cast"), dtypes={"b": "float64"})
    assert not [f for f in os.listdir(tmp_path / "cast") if f.endswith(".parquet")]
    made, table = created_by(nvt.Dataset(frame), "cast_flat", dtypes={"x": "float64"})
    assert all(m == PLAIN for m in made) and table.schema.field("x").type == pa.float64()
    _assert_same({c: v for c, v in _columns(table).items() if c != "x"}, {c: v for c, v in exp.items() if c != "x"})

    for name, kw in (("codec", {"compression": "snappy"}),
                     ("worker", {"shuffle": nio.Shuffle.PER_WORKER, "out_files_per_proc": 2})):
        made, table = created_by(nvt.Dataset(frame), name, **kw)
        assert all(m != PLAIN for m in made) and table.num_rows == 500
    monkeypatch.setattr(nio, "PLAIN_PARQUET", False)
    made, table = created_by(nvt.Dataset(frame), "off")
    assert all(m != PLAIN for m in made)
    _assert_same(_columns(table), exp)
