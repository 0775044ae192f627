"""Dataset(engine="csv") on the device against pandas.read_csv (keep_default_na=False,
na_values=[""], float_precision="round_trip") and Python's float / int.  Files are a few KiB to
1 MiB (the tile-scan step needs 256 tiles of 4 KiB)."""
import glob
import io
import os

import numpy as np
import pandas as pd
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import _lib, ops

pytestmark = pytest.mark.gpu

TILE, STEP = _lib.CSV_TILE, _lib.CSV_SCAN_STEP
PD = {"int64": "Int64", "int32": "Int32", "float64": np.float64, "float32": np.float32, "string": str}
FIXED = ["1e23", "8.98846567431158e307", "4.9e-324", "2.2250738585072011e-308", "1e-400", "1e400", "-0.0",
         "0.1234567890123456789", "9007199254740993", "1E5", "+1.5", ".5", "5.", "12345678901234567890123.5",
         "0.000000000000000000000000000012345678901234567890"]   # (the last two take the host slow path)


# pandas itself refuses "1e400" in a float64 column (and, with keep_default_na=False, "nan"): the
# frames compared with pandas leave those out, test_float_specials_against_python_float has them
FIXED_PANDAS = [t for t in FIXED if t != "1e400"]


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text if isinstance(text, bytes) else text.encode("utf-8"))
    return str(p)


def pandas_frame(text, dtypes, **kw):
    raw = text if isinstance(text, bytes) else text.encode("utf-8")
    return pd.read_csv(io.BytesIO(raw), keep_default_na=False, na_values=[""], float_precision="round_trip",
                       dtype={c: PD[d] for c, d in dtypes.items()}, **kw)


def frames(ds, **kw):
    return list(ds.to_iter(**kw))


def column_arrays(parts, name):
    """(values, valid mask, strings or None) of a column over all partitions."""
    vals, masks, strs = [], [], []
    for f in parts:
        col = f[name]
        n = len(col)
        vals.append(col.data.cpu().numpy())
        m = col.valid_mask_host()
        masks.append(np.ones(n, dtype=bool) if m is None else m)
        if col.strings is not None:
            strs.append(col.to_pandas().to_numpy())
    return np.concatenate(vals), np.concatenate(masks), (np.concatenate(strs) if strs else None)


def assert_equals_pandas(parts, exp, dtypes, columns=None):
    cols = list(columns) if columns is not None else list(dtypes)
    for f in parts:
        assert f.columns == cols
    assert sum(len(f) for f in parts) == len(exp)
    for c in cols:
        vals, mask, strs = column_arrays(parts, c)
        want = exp[c]
        d = dtypes[c]
        if d == "string":
            assert strs is not None, c
            np.testing.assert_array_equal(mask, want.notna().to_numpy(), err_msg=c)
            assert [s for s, m in zip(strs, mask) if m] == want[want.notna()].tolist(), c
            assert all(s is None for s, m in zip(strs, mask) if not m), c
        elif d.startswith("int"):
            assert vals.dtype == np.dtype(d), c
            np.testing.assert_array_equal(mask, want.notna().to_numpy(), err_msg=c)
            np.testing.assert_array_equal(vals[mask], want[want.notna()].to_numpy(dtype=d), err_msg=c)
        else:
            assert vals.dtype == np.dtype(d), c
            w = want.to_numpy()
            # pandas has one NaN for "empty" and for the text nan: an invalid row must be NaN there,
            # and a valid row is bit-equal (NaN for NaN)
            assert np.isnan(w[~mask]).all(), c
            u = np.uint64 if d == "float64" else np.uint32
            both = mask & ~np.isnan(w)
            np.testing.assert_array_equal(vals[both].view(u), w[both].view(u), err_msg=c)
            assert np.isnan(vals[mask & np.isnan(w)]).all(), c


def quote_field(v, sep=",", force=False):
    if force or sep in v or '"' in v:
        return '"' + v.replace('"', '""') + '"'
    return v


STRINGS = ["plain", "with,comma", 'say "hi"', "", "naïve ✓ 日本", "NA", "null", "x", ",", '"',
           "tab\there", "a" * 37]


def mixed_text(n, seed=0, sep=",", eol="\n", header=True, last_eol=True):
    """n rows of (i64 with negatives and empties, i32, f64 from repr of random doubles and the fixed
    list, f32, string) -> (text, dtypes)."""
    rng = np.random.default_rng(seed)
    dtypes = {"a": "int64", "b": "int32", "x": "float64", "y": "float32", "s": "string"}
    lines = [sep.join(dtypes)] if header else []
    bits = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    for i in range(n):
        a = "" if rng.random() < 0.2 else str(int(rng.integers(-2 ** 63, 2 ** 63 - 1, endpoint=True)))
        if i == 0:
            a = str(-2 ** 63)
        b = "" if rng.random() < 0.1 else str(int(rng.integers(-2 ** 31, 2 ** 31 - 1, endpoint=True)))
        r = rng.random()
        if r < 0.1:
            x = ""
        elif r < 0.3:
            x = FIXED_PANDAS[int(rng.integers(len(FIXED_PANDAS)))]
        elif r < 0.6:
            x = repr(float(bits[i])) if np.isfinite(bits[i]) else "7"
        else:
            x = repr(float(rng.standard_normal() * 10.0 ** int(rng.integers(-20, 20))))
        if rng.random() < 0.1 and x:
            x = '"' + x + '"'     # quotes around a numeric field are stripped
        y = "" if rng.random() < 0.1 else repr(float(rng.standard_normal() * 10.0 ** int(rng.integers(-10, 10))))
        s = STRINGS[int(rng.integers(len(STRINGS)))].replace(",", sep)
        s = '""' if (s == "" and rng.random() < 0.5) else quote_field(s, sep, force=rng.random() < 0.2 and s != "")
        lines.append(sep.join([a, b, x, y, s]))
    text = eol.join(lines) + (eol if last_eol else "")
    return text, dtypes


# ---- row counts: the validity-word edges -----------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_row_counts(tmp_path, n):
    text, dtypes = mixed_text(n, seed=n)
    p = write(tmp_path, "t.csv", text)
    ds = nvt.Dataset(p, dtypes=dtypes)
    parts = frames(ds)
    assert len(parts) == 1 and len(parts[0]) == n
    assert_equals_pandas(parts, pandas_frame(text, dtypes), dtypes)
    if n == 0:
        f = parts[0]
        assert [f[c].data.dtype for c in dtypes] == [torch.int64, torch.int32, torch.float64, torch.float32,
                                                     torch.int64]
        assert f["s"].strings == {}
    for c in ("a", "b"):   # validity is stored in whole words, bits past the last row zero
        v = parts[0][c].valid
        if n:
            assert v.numel() == (n + 63) // 64 * 8
            bits = np.unpackbits(v.cpu().numpy(), bitorder="little")
            assert not bits[n:].any()


# ---- tile edges -----------------------------------------------------------------------------------
def padded_rows(total, seed=0, first=0):
    """Rows "i,text\\n" of exactly ``total`` bytes, quoted fields with separators among them."""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, first
    while True:
        body = "y" * int(rng.integers(0, 30))
        if rng.random() < 0.3:
            body = '"' + body + ',"",' + '"'
        row = f"{i},{body}\n"
        if size + len(row) + 48 > total:
            break
        out.append(row)
        size += len(row)
        i += 1
    last = f"{i},"
    out.append(last + "z" * (total - size - len(last) - 1) + "\n")
    text = "".join(out)
    assert len(text) == total
    return text


TWO = {"i": "int64", "t": "string"}


def check_two(tmp_path, text, **kw):
    p = write(tmp_path, "e.csv", text)
    parts = frames(nvt.Dataset(p, names=list(TWO), dtypes=TWO, **kw))
    exp = pandas_frame(text, TWO, names=list(TWO), header=None)
    assert_equals_pandas(parts, exp, TWO)
    return parts


@pytest.mark.parametrize("size", [TILE - 1, TILE, TILE + 1])
def test_file_sizes_around_one_tile(tmp_path, size):
    check_two(tmp_path, padded_rows(size, seed=size))


@pytest.mark.parametrize("row", ['12345,"ab,cd"\n', '7,"ab,cd""e"\n', "7777777,abcdef\n"])
@pytest.mark.parametrize("lead", range(1, 9))
def test_field_straddles_a_tile_edge(tmp_path, row, lead):
    # the row starts `lead` bytes before the tile edge: every byte of '12345,"ab' (the opening quote
    # among them, lead = 7) is once the last byte of the first tile
    text = padded_rows(TILE - lead, seed=lead) + row + padded_rows(300, seed=1, first=10 ** 6)
    if lead == 7 and row.startswith("12345"):
        assert text[TILE - 1] == '"' and text[TILE - 2] == ","
    check_two(tmp_path, text)


@pytest.mark.parametrize("size", [(STEP - 1) * TILE, STEP * TILE, STEP * TILE + 1, STEP * TILE + 300])
def test_tile_scan_step_edges(tmp_path, size):
    # W - 1, W and W + 1 tiles (W + 1 twice: one byte and 300 bytes in the last tile); a quoted field
    # with separators lies across the last tile edge that has 200 bytes behind it -- for the last
    # size that is the edge between the two steps of the scan, which the parity has to cross
    edge = (size - 200) // TILE * TILE
    head = padded_rows(edge - 5, seed=size % 97)
    mid = '1,"q,""r"",s"\n'
    text = head + mid + padded_rows(size - len(head) - len(mid), seed=3, first=10 ** 6)
    assert len(text) == size
    parts = check_two(tmp_path, text)
    assert len(parts) == 1


# ---- the mixed frame and the format variants ------------------------------------------------------
def test_mixed_frame(tmp_path):
    text, dtypes = mixed_text(3000, seed=11)
    p = write(tmp_path, "m.csv", text)
    parts = frames(nvt.Dataset(p, dtypes=dtypes))
    assert_equals_pandas(parts, pandas_frame(text, dtypes), dtypes)


def test_float_specials_against_python_float(tmp_path):
    # (1e-40 ... : subnormal as float32, the double is rounded once and not flushed to zero)
    fields = FIXED + ["nan", "NaN", "inf", "-inf", "Infinity", "-nan", "", "1e22", "123456789012345678e-40", '"2.5"',
                      "1e-40", "-1.1754942e-38", "1.401298464324817e-45", "7.006492321624085e-46", "7.1e-46"]
    text = "x\n" + "\n".join(fields) + "\n"
    p = write(tmp_path, "f.csv", text)
    for d, u in (("float64", np.uint64), ("float32", np.uint32)):
        (f,) = frames(nvt.Dataset(p, dtypes={"x": d}))
        vals, mask, _ = column_arrays([f], "x")
        with np.errstate(over="ignore"):     # (8.98846567431158e307 is inf as a float32)
            want = np.array([float(t.strip('"')) if t else np.nan for t in fields], dtype=np.float64).astype(d)
        np.testing.assert_array_equal(mask, np.array([t != "" for t in fields]))
        finite = ~np.isnan(want)
        np.testing.assert_array_equal(vals[finite].view(u), want[finite].view(u))
        assert np.isnan(vals[~finite]).all()


@pytest.mark.parametrize("variant", ["tsv", "crlf", "no_trailing_newline", "crlf_no_trailing_newline"])
def test_format_variants(tmp_path, variant):
    sep = "\t" if variant == "tsv" else ","
    eol = "\r\n" if variant.startswith("crlf") else "\n"
    text, dtypes = mixed_text(300, seed=5, sep=sep, eol=eol, last_eol="no_trailing" not in variant)
    p = write(tmp_path, "v.tsv" if sep == "\t" else "v.csv", text)
    parts = frames(nvt.Dataset(p, sep=sep, dtypes=dtypes))
    assert_equals_pandas(parts, pandas_frame(text, dtypes, sep=sep), dtypes)


def test_crlf_last_column_float32_on_the_host_slow_path(tmp_path):
    # quoted 25-digit values in the last column of a CRLF file: the device parser declines them, the
    # host parses the text that is left without the '\r' and the quotes, and float32 rounds that double
    rng = np.random.default_rng(12)
    digits = ["".join(map(str, rng.integers(0, 10, 25))) for _ in range(150)]
    cells = ['"%s.%s"' % (d[:i % 24 + 1], d[i % 24 + 1:]) for i, d in enumerate(digits)]
    cells[3], cells[70], cells[149] = "", '"-1234567890123456789012345"', "0.1000000000000000055511151"
    text = "a,y\r\n" + "".join(f"{i},{c}\r\n" for i, c in enumerate(cells))
    dtypes = {"a": "int64", "y": "float32"}
    p = write(tmp_path, "slow.csv", text)
    from nvtabular_amd import kernels as K

    before = K.STATS.get("csv_slow_fields", 0)
    parts = frames(nvt.Dataset(p, dtypes=dtypes))
    assert K.STATS.get("csv_slow_fields", 0) - before == 149
    assert_equals_pandas(parts, pandas_frame(text, dtypes), dtypes)
    vals, mask, _ = column_arrays(parts, "y")
    want = np.array([float(c.strip('"')) if c else np.nan for c in cells], dtype=np.float64).astype(np.float32)
    np.testing.assert_array_equal(vals[mask].view(np.uint32), want[mask].view(np.uint32))
    assert mask.sum() == 149 and not mask[3]


def test_headerless_with_names(tmp_path):
    text, dtypes = mixed_text(200, seed=6, header=False)
    p = write(tmp_path, "h.csv", text)
    exp = pandas_frame(text, dtypes, names=list(dtypes), header=None)
    assert_equals_pandas(frames(nvt.Dataset(p, names=list(dtypes), dtypes=dtypes)), exp, dtypes)
    assert_equals_pandas(frames(nvt.Dataset(p, names=list(dtypes), header=None, dtypes=dtypes)), exp, dtypes)


def test_columns_pruning(tmp_path):
    text, dtypes = mixed_text(200, seed=7)
    p = write(tmp_path, "p.csv", text)
    exp = pandas_frame(text, dtypes)
    ds = nvt.Dataset(p, dtypes=dtypes)
    assert_equals_pandas(frames(ds, columns=["s", "b"]), exp, dtypes, columns=["s", "b"])
    assert_equals_pandas(frames(ds, columns=["x"]), exp, dtypes, columns=["x"])


def test_all_empty_column_and_inference(tmp_path):
    text = "a,e,s\n" + "".join(f"{i},,{'' if i % 3 else 'v%d' % i}\n" for i in range(130))
    p = write(tmp_path, "e.csv", text)
    ds = nvt.Dataset(p)
    dtypes = {"a": "int64", "e": "float64", "s": "string"}
    assert ds._csv.dtypes == dtypes
    parts = frames(ds)
    assert_equals_pandas(parts, pandas_frame(text, dtypes), dtypes)
    assert not column_arrays(parts, "e")[1].any()
    for d in ("int32", "string"):
        dt = dict(dtypes, e=d)
        parts = frames(nvt.Dataset(p, dtypes=dt))
        assert not column_arrays(parts, "e")[1].any()
        assert_equals_pandas(parts, pandas_frame(text, dt), dt)


def test_single_column_file(tmp_path):
    for d, vals in (("int64", ["5", "-7", "0", "123456789012"]), ("string", ["a", '"b,c"', "d", "NA"]),
                    ("float64", ["1.5", "inf", "-2e5", "3"])):
        text = "only\n" + "\n".join(vals * 20) + "\n"
        p = write(tmp_path, f"s_{d}.csv", text)
        dt = {"only": d}
        assert_equals_pandas(frames(nvt.Dataset(p, dtypes=dt)), pandas_frame(text, dt), dt)


def test_partitions_cut_mid_line(tmp_path):
    text, dtypes = mixed_text(400, seed=8)
    p = write(tmp_path, "big.csv", text)
    ds = nvt.Dataset(p, dtypes=dtypes, part_size=len(text) // 7)
    assert 5 <= ds.npartitions <= 8
    cuts = [b for _, _, b in ds._csv.ranges[:-1]]
    header = ds._csv.ranges[0][1]
    assert any((b - header) % (len(text) // 7) for b in cuts)      # nominal boundaries fell mid-line
    parts = frames(ds)
    assert len(parts) == ds.npartitions
    assert_equals_pandas(parts, pandas_frame(text, dtypes), dtypes)
    # a shard takes every world-th partition
    mine = frames(ds, shard=(1, 3))
    assert [len(f) for f in mine] == [len(f) for f in parts[1::3]]


def test_two_files_each_with_a_header(tmp_path):
    d = tmp_path / "dir"
    d.mkdir()
    t1, dtypes = mixed_text(50, seed=1)
    t2, _ = mixed_text(70, seed=2)
    write(d, "a.csv", t1)
    write(d, "b.csv", t2)
    parts = frames(nvt.Dataset(str(d), dtypes=dtypes))
    exp = pd.concat([pandas_frame(t1, dtypes), pandas_frame(t2, dtypes)], ignore_index=True)
    assert_equals_pandas(parts, exp, dtypes)


# ---- errors: ordinary returns read from the state block -----------------------------------------------
def raises(tmp_path, text, dtypes, *words, **kw):
    p = write(tmp_path, "bad.csv", text)
    ds = nvt.Dataset(p, dtypes=dtypes, **kw)
    with pytest.raises(ValueError) as e:
        frames(ds)
    msg = str(e.value)
    for w in (p,) + words:
        assert w in msg, (w, msg)
    return msg


AB = {"a": "int64", "b": "int64"}


def test_field_count_errors(tmp_path):
    raises(tmp_path, "a,b\n1,2\n3\n4,5\n", AB, "row 1 ", "2 fields")
    raises(tmp_path, "a,b\n1,2\n3,4\n5,6,7\n8,9\n", AB, "row 2 ", "2 fields")
    raises(tmp_path, "a,b\n1,2\n3,4,5\n6\n", AB, "row 1 ", "2 fields")          # the totals balance
    raises(tmp_path, "a,b\n1,2\n\n3,4\n", AB, "row 1 ", "2 fields")              # a blank line is a row
    rows = "".join(f"{i},{i}\n" for i in range(1500))                            # the bad row is in the second tile
    assert len(rows) > 2 * TILE
    raises(tmp_path, "a,b\n" + rows + "7\n" + rows, AB, "row 1500 ")


def test_value_errors(tmp_path):
    msg = raises(tmp_path, "a,b\n1,2\n3,x1\n4,zz\n", AB, "row 1,", "column 'b'", "dtypes", "int64")
    assert "'x1'" in msg
    raises(tmp_path, "a,b\n1,2\n3,4\n5,1.0\n", AB, "row 2,", "column 'b'", "dtypes")
    raises(tmp_path, "a,b\n9223372036854775807,2\n9223372036854775808,4\n", AB, "row 1,", "column 'a'", "does not fit")
    raises(tmp_path, "a,b\n-9223372036854775808,2\n1,-9223372036854775809\n", AB, "row 1,", "column 'b'", "does not fit")
    raises(tmp_path, "a,b\n1,2147483647\n1,2147483648\n", {"a": "int64", "b": "int32"}, "row 1,", "column 'b'",
           "does not fit int32")
    raises(tmp_path, "a,b\n1,2\n3, 4\n", AB, "row 1,", "column 'b'")                      # whitespace is kept
    raises(tmp_path, "a,b\n1,2.5\n3,1.5x\n", {"a": "int64", "b": "float64"}, "row 1,", "column 'b'", "float64")
    raises(tmp_path, "a,b\n1,2.5\n3,abc\n", {"a": "int64", "b": "float32"}, "row 1,", "column 'b'", "float32")
    # a pruned column is not parsed: its text does not matter
    p = write(tmp_path, "ok.csv", "a,b\n1,2\n3,x1\n")
    (f,) = frames(nvt.Dataset(p, dtypes=AB), columns=["a"])
    assert column_arrays([f], "a")[0].tolist() == [1, 3]


def test_quote_errors(tmp_path):
    st = {"a": "int64", "s": "string"}
    raises(tmp_path, 'a,s\n1,u\n2,"x\ny"\n3,z\n', st, "row 1:", "quoted")          # a newline inside quotes
    raises(tmp_path, 'a,s\n1,u\n2,v\n3,"x\n', st, "row 2:", "quote")                # never closed
    raises(tmp_path, 'a,s\n1,u\n2,v\n3,w"\n', st, "quote")                          # a stray quote
    # inside a quoted field a quote has to be doubled
    raises(tmp_path, 'a,s\n1,"u""v"\n2,"a"b"c"\n3,z\n', st, "row 1,", "column 's'", "not doubled")


def test_some_dtypes_given_the_rest_inferred(tmp_path):
    text = "a,b,s,x\n" + "".join(f"{'' if i % 5 == 1 else i - 40},{i},{'' if i % 7 == 2 else 'v%d' % (i % 9)},"
                                 f"{'' if i % 4 == 3 else i / 8}\n" for i in range(100))
    p = write(tmp_path, "some.csv", text)
    ds = nvt.Dataset(p, dtypes={"a": "int64"})
    dtypes = {"a": "int64", "b": "int64", "s": "string", "x": "float64"}
    assert ds._csv.dtypes == dtypes
    parts = frames(ds)
    assert_equals_pandas(parts, pandas_frame(text, dtypes), dtypes)
    assert parts[0]["a"].data.dtype == torch.int64 and not column_arrays(parts, "a")[1].all()


# ---- end to end --------------------------------------------------------------------------------------
def workflow_text(n=2000, seed=3):
    rng = np.random.default_rng(seed)
    cat = rng.zipf(1.5, n) % 40
    words = np.array(["w%d" % k for k in range(25)] + ['q,"%d"' % k for k in range(5)])
    s = words[rng.zipf(1.3, n) % len(words)]
    x = rng.lognormal(1, 1.5, n)
    lines = ["c,s,x"]
    for i in range(n):
        lines.append(f"{cat[i]},{quote_field(str(s[i]))},{'' if rng.random() < 0.2 else repr(float(x[i]))}")
    return "\n".join(lines) + "\n", {"c": "int64", "s": "string", "x": "float64"}


def test_workflow_equals_the_pandas_route(tmp_path):
    text, dtypes = workflow_text()
    p = write(tmp_path, "w.csv", text)
    df = pd.read_csv(p, keep_default_na=False, na_values=[""], float_precision="round_trip",
                     dtype={"c": np.int64, "s": str, "x": np.float64})

    def run(ds, tag):
        cats = ["c", "s"] >> ops.Categorify(out_path=str(tmp_path / tag))
        conts = ["x"] >> ops.FillMissing() >> ops.Normalize()
        return nvt.Workflow(cats + conts).fit_transform(ds).to_ddf().compute()

    ds = nvt.Dataset(p, dtypes=dtypes, part_size=len(text) // 3)
    assert ds.npartitions >= 3
    # the pandas route gets the same rows per partition, so both sides add up in the same order
    cuts = np.concatenate([[0], np.cumsum([len(f) for f in ds.to_iter(columns=["c"])])])
    assert cuts[-1] == len(df)
    got = run(ds, "csv")
    want = run(nvt.Dataset([df.iloc[a:b].reset_index(drop=True) for a, b in zip(cuts[:-1], cuts[1:])]), "pandas")
    assert list(got.columns) == list(want.columns) and len(got) == len(df)
    for c in ("c", "s"):
        np.testing.assert_array_equal(got[c].to_numpy(), want[c].to_numpy(), err_msg=c)
    np.testing.assert_array_equal(got["x"].to_numpy().view(np.uint64), want["x"].to_numpy().view(np.uint64))


def test_to_parquet_round_trip(tmp_path):
    text, dtypes = workflow_text(n=700, seed=4)
    p = write(tmp_path, "w.csv", text)
    out = str(tmp_path / "pq")
    nvt.Dataset(p, dtypes=dtypes, part_size=len(text) // 2).to_parquet(out)
    files = sorted(glob.glob(os.path.join(out, "part_*.parquet")), key=lambda f: int(f.split("_")[-1].split(".")[0]))
    got = pd.concat([pd.read_parquet(f) for f in files], ignore_index=True)
    want = pd.read_csv(p, keep_default_na=False, na_values=[""], float_precision="round_trip",
                       dtype={"c": np.int64, "s": str, "x": np.float64})
    assert list(got.columns) == ["c", "s", "x"] and len(got) == len(want)
    np.testing.assert_array_equal(got["c"].to_numpy(dtype=np.int64), want["c"].to_numpy())
    np.testing.assert_array_equal(got["x"].to_numpy(dtype=np.float64).view(np.uint64),
                                  want["x"].to_numpy().view(np.uint64))
    assert got["s"].tolist() == want["s"].tolist()


def test_torch_loader_over_a_csv_dataset(tmp_path):
    from nvtabular_amd.loader.torch import TorchAsyncItr

    n = 1000
    text = "c,x,label\n" + "".join(f"{i % 17},{i / 4},{i % 2}\n" for i in range(n))
    p = write(tmp_path, "l.csv", text)
    ds = nvt.Dataset(p, part_size=len(text) // 4)
    assert ds.npartitions >= 4
    it = TorchAsyncItr(ds, cats=["c"], conts=["x"], labels=["label"], batch_size=96)
    assert len(it) == -(-n // 96)
    rows, xs = 0, []
    for x, y in it:
        rows += len(y)
        xs.append(x["x"].cpu().numpy().reshape(-1))
    assert rows == n
    np.testing.assert_array_equal(np.sort(np.concatenate(xs)), (np.arange(n) / 4).astype(np.float32))
