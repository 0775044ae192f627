"""The host half of the CSV engine (nvtabular_amd/csv_text.py) and the scalar number parsers of
nvt_csv_parse.hpp through their host entry points.  Runs without a GPU."""
import ctypes as C
import os
import struct

import numpy as np
import pandas as pd
import pytest

from nvtabular_amd import _lib, csv_text
from nvtabular_amd.io import Dataset

OK, DECLINED, INVALID, OVERFLOW = 0, 1, 2, 3


# ---- engine selection and option errors ---------------------------------------------------------
def _write(path, text):
    with open(path, "wb") as f:
        f.write(text.encode() if isinstance(text, str) else text)
    return str(path)


@pytest.mark.parametrize("suffix", [".csv", ".tsv", ".txt"])
def test_engine_by_suffix(tmp_path, suffix):
    p = _write(tmp_path / ("a" + suffix), "x,y\n1,2\n")
    ds = Dataset(p)
    assert ds.engine == "csv" and ds.npartitions == 1
    assert ds.schema.column_names == ["x", "y"]
    assert getattr(ds, "_pieces", None) is None     # (the loader counts rows through the generic branch)


def test_engine_by_argument_directory_and_glob(tmp_path):
    p = _write(tmp_path / "data.dat", "x,y\n1,2\n")
    assert Dataset(p, engine="csv").engine == "csv"
    d = tmp_path / "dir"
    d.mkdir()
    _write(d / "b.csv", "x,y\n3,4\n")
    _write(d / "a.csv", "x,y\n1,2\n")
    ds = Dataset(str(d))
    assert ds.engine == "csv" and ds.npartitions == 2
    assert [os.path.basename(f) for f in ds._csv.files] == ["a.csv", "b.csv"]
    assert Dataset(str(d / "*.csv")).npartitions == 2
    assert Dataset([str(d / "b.csv"), str(d / "a.csv")]).npartitions == 2


def test_parquet_selection_is_unchanged(tmp_path):
    p = str(tmp_path / "t.parquet")
    pd.DataFrame({"x": [1, 2, 3]}).to_parquet(p)
    for engine in (None, "parquet"):
        ds = Dataset(p, engine=engine)
        assert getattr(ds, "_pieces", None) is not None and ds.npartitions == 1
    with pytest.raises(Exception):   # a text file forced through the parquet reader still fails
        Dataset(_write(tmp_path / "a.csv", "x\n1\n"), engine="parquet")


def test_directory_with_parquet_files_stays_parquet(tmp_path):
    # stray text beside the part files (also one that sorts first) does not change the engine
    d = tmp_path / "pq"
    d.mkdir()
    pd.DataFrame({"x": [1, 2, 3]}).to_parquet(str(d / "part_0.parquet"))
    _write(d / "notes.txt", "not,a\ntable\n")
    _write(d / "keys.csv", "k\n1\n")
    assert csv_text.select_engine(str(d), None) is None
    ds = Dataset(str(d))
    assert ds.engine is None and getattr(ds, "_pieces", None) is not None and ds.npartitions == 1
    assert ds.schema.column_names == ["x"]
    # without a parquet file the first file of the sorted listing decides
    e = tmp_path / "other"
    e.mkdir()
    _write(e / "a.bin", b"\x00\x01")
    _write(e / "b.csv", "k\n1\n")
    assert csv_text.select_engine(str(e), None) is None
    (e / "a.bin").unlink()
    assert csv_text.select_engine(str(e), None) == "csv"
    # asked for by name, the text files of the mixed directory are read
    assert [os.path.basename(f) for f in Dataset(str(d), engine="csv")._csv.files] == ["keys.csv", "notes.txt"]


def test_option_errors(tmp_path):
    p = _write(tmp_path / "a.csv", "x,y\n1,2\n")
    with pytest.raises(ValueError, match="names"):
        Dataset(p, header=None)
    for name in ("a.csv.gz", "a.tsv.bz2"):
        with pytest.raises(NotImplementedError, match="[Cc]ompressed"):
            Dataset(_write(tmp_path / name, b"\x1f\x8b"))
    with pytest.raises(NotImplementedError, match="[Cc]ompressed"):
        Dataset(_write(tmp_path / "b.gz", b"\x1f\x8b"), engine="csv")
    for bad in ("12 parsecs", "MB", -5, 0, "2GB", (1 << 30) + 1):
        with pytest.raises(ValueError, match="part_size"):
            Dataset(p, part_size=bad)
    with pytest.raises(ValueError, match="sep"):
        Dataset(p, sep="||")
    with pytest.raises(ValueError, match="header"):
        Dataset(p, header=3)
    with pytest.raises(TypeError, match="dtype"):
        Dataset(p, dtypes={"x": "datetime64[ns]"})
    with pytest.raises(ValueError, match="unknown column"):
        Dataset(p, dtypes={"zz": "int64"})


def test_bool_inference_raises_type_error(tmp_path):
    p = _write(tmp_path / "a.csv", "x,flag\n1,True\n2,False\n")
    with pytest.raises(TypeError, match="flag.*dtypes"):
        Dataset(p)
    ds = Dataset(p, dtypes={"flag": "string"})
    assert ds._csv.dtypes["flag"] == "string"


def test_part_size_strings():
    assert csv_text.parse_size("128MB") == 128 * 10 ** 6
    assert csv_text.parse_size("1 KiB") == 1024
    assert csv_text.parse_size("4k") == 4000
    assert csv_text.parse_size(4096) == 4096
    assert csv_text.parse_size(None) == 128 << 20


# ---- cut points -----------------------------------------------------------------------------------
def _ten_kib(newline_at_end=True):
    rng = np.random.default_rng(3)
    lines, size = [], len("alpha,beta\n")
    while size < 10240:
        line = "%d,%s" % (rng.integers(0, 10 ** 6), "x" * int(rng.integers(0, 40)))
        lines.append(line)
        size += len(line) + 1
    body = "\n".join(lines) + ("\n" if newline_at_end else "")
    return "alpha,beta\n" + body


@pytest.mark.parametrize("newline_at_end", [True, False])
@pytest.mark.parametrize("part_size", [1024, 4096, 1 << 20])
def test_cut_points(tmp_path, part_size, newline_at_end):
    text = _ten_kib(newline_at_end).encode()
    p = _write(tmp_path / "t.csv", text)
    ds = Dataset(p, part_size=part_size)
    ranges = ds._csv.ranges
    header = len(b"alpha,beta\n")
    assert ds.npartitions == len(ranges)
    assert ranges[0][1] == header                                  # header bytes excluded
    assert ranges[-1][2] == len(text)
    for (f, a, b), (_, a2, _) in zip(ranges, ranges[1:]):
        assert b == a2                                             # the ranges tile the file
    for f, a, b in ranges:
        assert f == p and b > a
        assert text[b - 1:b] == b"\n" or (b == len(text) and not newline_at_end)
    if part_size >= len(text):
        assert len(ranges) == 1
    else:
        # cut i is the first line end at or after nominal boundary i (lines here are under 64 bytes)
        k = -(-(len(text) - header) // part_size)
        assert len(ranges) in (k - 1, k)       # (k - 1: the last boundary's line is the file's last)
        for i, (_, a, b) in enumerate(ranges[:-1], start=1):
            assert header + i * part_size <= b < header + i * part_size + 64
    # what is uploaded always ends in a newline
    for i in range(len(ranges)):
        buf, n = ds._csv.read_range(i, pinned=False)
        assert n == ranges[i][2] - ranges[i][1] + (i == len(ranges) - 1 and not newline_at_end)
        assert bytes(buf[n - 1:n]) == b"\n"
        assert bytes(buf[:ranges[i][2] - ranges[i][1]]) == text[ranges[i][1]:ranges[i][2]]


def test_header_only_file_and_headerless(tmp_path):
    ds = Dataset(_write(tmp_path / "h.csv", "a,b\n"))
    assert ds.npartitions == 1 and ds._csv.ranges[0][1] == ds._csv.ranges[0][2]
    ds = Dataset(_write(tmp_path / "n.csv", "1,2\n3,4\n"), names=["p", "q"])
    assert ds._csv.ranges == [(str(tmp_path / "n.csv"), 0, 8)]
    assert ds.schema.column_names == ["p", "q"]
    ds = Dataset(_write(tmp_path / "q.csv", '"a,1","b ""x"""\r\n1,2\r\n'))
    assert ds.schema.column_names == ["a,1", 'b "x"']
    assert ds._csv.ranges[0][1] == len('"a,1","b ""x"""\r\n')


# ---- dtype inference ------------------------------------------------------------------------------
def test_dtype_inference_from_the_sample(tmp_path):
    p = _write(tmp_path / "a.csv", "i,f,s,e,n\n1,1.5,abc,,NA\n-2,,x,,null\n,3,,,\n")
    ds = Dataset(p)
    assert ds._csv.dtypes == {"i": "float64", "f": "float64", "s": "string", "e": "float64", "n": "string"}
    p = _write(tmp_path / "b.csv", "i,f,s\n1,1.5,abc\n-2,2,x\n")
    ds = Dataset(p, dtypes={"f": np.float32})
    assert ds._csv.dtypes == {"i": "int64", "f": "float32", "s": "string"}
    sch = ds.schema
    assert sch["i"].dtype == np.int64 and sch["f"].dtype == np.float32 and sch["s"].dtype == object
    ds = Dataset(p, dtypes={"i": "int32", "s": str, "f": "float64"})
    assert ds._csv.dtypes == {"i": "int32", "f": "float64", "s": "string"}


def test_some_dtypes_given_the_rest_inferred(tmp_path):
    # an empty field in a column NAMED int64 is a null of this engine, not an inference failure
    p = _write(tmp_path / "p.csv", "a,b,c,d\n1,2,x,1.5\n,3,y,\n7,,z,2\n")
    ds = Dataset(p, dtypes={"a": "int64"})
    assert ds._csv.dtypes == {"a": "int64", "b": "float64", "c": "string", "d": "float64"}
    ds = Dataset(p, dtypes={"a": "int64", "b": "int32", "d": np.float32})
    assert ds._csv.dtypes == {"a": "int64", "b": "int32", "c": "string", "d": "float32"}
    # a named column's text does not have to look like its type in the sample either
    p = _write(tmp_path / "q.csv", "a,b\nabc,2\n,3\n")
    assert Dataset(p, dtypes={"a": "float64"})._csv.dtypes == {"a": "float64", "b": "int64"}


def test_inference_sample_is_cut_at_a_line_end(tmp_path):
    # the 64 KiB sample ends in the middle of a line whose first field is not a number yet
    rows = ["%d,%d" % (i, i) for i in range(20000)]
    p = _write(tmp_path / "big.csv", "a,b\n" + "\n".join(rows) + "\nlast,1\n")
    assert Dataset(p)._csv.dtypes == {"a": "int64", "b": "int64"}


# ---- scalar parsers -------------------------------------------------------------------------------
def _f64(lib, text):
    out = C.c_double()
    b = text.encode()
    rc = lib.nvt_csv_parse_f64_host(b, len(b), C.byref(out))
    return rc, struct.pack("<d", out.value)


def _random_doubles():
    """200 000 doubles: 80 000 normal, 80 000 uniform in bit pattern (the finite ones of a larger
    draw), 40 000 subnormal."""
    rng = np.random.default_rng(20240611)
    normal = rng.standard_normal(80_000) * 10.0 ** rng.integers(-30, 30, 80_000)
    bits = rng.integers(0, 1 << 64, 81_000, dtype=np.uint64).view(np.float64)
    bits = bits[np.isfinite(bits)][:80_000]
    sub = rng.integers(1, 1 << 52, 40_000, dtype=np.uint64).view(np.float64)
    sub = np.where(rng.random(40_000) < 0.5, sub, -sub)
    return np.concatenate([normal, bits, sub])


def test_parse_f64_repr_of_random_doubles():
    lib = _lib.load()
    vals = _random_doubles()
    assert len(vals) == 200_000
    declined = 0
    out = C.c_double()
    for v in vals.tolist():
        b = repr(v).encode()
        rc = lib.nvt_csv_parse_f64_host(b, len(b), C.byref(out))
        if rc == DECLINED:
            declined += 1
            continue
        assert rc == OK, (b, rc)
        assert struct.pack("<d", out.value) == struct.pack("<d", float(b)), b
    share = declined / len(vals)
    print(f"declined {declined} of {len(vals)} ({share:.4%})")   # (profiles/csv_notes.md quotes it)
    assert share <= 0.01


FIXED = ["1e23", "8.98846567431158e307", "4.9e-324", "2.2250738585072011e-308", "1e-400", "1e400", "-0.0",
         "0.1234567890123456789", "9007199254740993", "1E5", "+1.5", ".5", "5."]


def test_parse_f64_fixed_list():
    lib = _lib.load()
    for t in FIXED + ["0", "-0", "00012.50", "1e22", "1e-22", "9007199254740992e3", "2.5e-5", "123456789012345678e-40",
                      "1.7976931348623157e308", "1.7976931348623159e308", "2.4703282292062327e-324",
                      "2.4703282292062328e-324", "inf", "-inf", "Infinity", "nan", "NaN", "-nan", "+INF"]:
        rc, got = _f64(lib, t)
        assert rc in (OK, DECLINED), t
        if rc == OK:
            assert got == struct.pack("<d", float(t)), t
    assert _f64(lib, "1e23")[0] == OK and _f64(lib, "4.9e-324")[0] == OK     # Eisel-Lemire takes these
    assert _f64(lib, "12345678901234567890123")[0] == DECLINED               # more than 19 digits
    for t in ["", "-", "+", ".", "e5", "1e", "1e+", "1.2.3", "12a", " 1", "1 ", "0x10", "1_0", "in", "nanx", "--1",
              "1,5"]:
        assert _f64(lib, t)[0] == INVALID, t


def test_parse_i64():
    lib = _lib.load()
    out = C.c_int64()

    def parse(t):
        b = t.encode()
        return lib.nvt_csv_parse_i64_host(b, len(b), C.byref(out)), out.value

    for t in [str(-2 ** 63), str(2 ** 63 - 1), "+7", "-0", "0", "0000123", "-000", "42"]:
        assert parse(t) == (OK, int(t)), t
    for t in [str(2 ** 63), str(-2 ** 63 - 1), "99999999999999999999999999", str(2 ** 64), str(2 ** 64 + 5)]:
        assert parse(t)[0] == OVERFLOW, t
    for t in ["", "1.0", "12a", "-", "+", " 1", "1 ", "0x1", "1e3", "99999999999999999999999999x"]:
        assert parse(t)[0] == INVALID, t
