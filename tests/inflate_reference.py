"""Helpers of the snappy-inflate tests (no test module: the tests import it): snappy copy elements,
the parquet files the reader tests share, and which of a file's data pages the device route takes,
counted from the page headers."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from nvtabular_amd import parquet_plain as PP
from nvtabular_amd.parquet_thrift import _TReader

NUMBER_COLUMNS = ("i32", "i64", "f32", "f64", "ts", "i16")


def copy1(length, offset):
    """4 .. 11 bytes from 1 .. 2047 back."""
    assert 4 <= length <= 11 and 0 <= offset < 2048
    return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xFF])


def copy2(length, offset, width=2):
    """1 .. 64 bytes, the offset in ``width`` = 2 or 4 bytes."""
    assert 1 <= length <= 64 and 0 <= offset < (1 << 8 * width)
    return bytes([width // 2 + 1 | ((length - 1) << 2)]) + offset.to_bytes(width, "little")


def copy4(length, offset):
    return copy2(length, offset, 4)


def out_len(body):
    """The bytes a bare element stream produces, by its tags alone."""
    at = n = 0
    while at < len(body):
        tag = body[at]
        kind, hi = tag & 3, tag >> 2
        if kind == 0:
            k = max(0, hi - 59)
            m = (int.from_bytes(body[at + 1: at + 1 + k], "little") if k else hi) + 1
            at += 1 + k + m
            n += m
        else:
            at += (2, 3, 5)[kind - 1]
            n += 4 + (hi & 7) if kind == 1 else hi + 1
    return n


def table(rows, nullable, seed=3, with_nulls=()):
    """The number columns of NUMBER_COLUMNS; the columns named in ``with_nulls`` hold nulls."""
    rng = np.random.default_rng(seed)
    cols = {
        "i32": (rng.integers(-50, 50, rows).astype(np.int32), pa.int32()),
        "i64": (np.minimum(rng.zipf(1.3, rows), 1 << 40).astype(np.int64), pa.int64()),
        "f32": (rng.normal(size=rows).astype(np.float32), pa.float32()),
        "f64": ((rng.integers(0, 64, rows) / 8).astype(np.float64), pa.float64()),
        "ts": ((rng.integers(0, 50, rows) * 86_400_000_000 + 1_600_000_000_000_000).astype("datetime64[us]"),
               pa.timestamp("us")),
        "i16": (rng.integers(-300, 300, rows).astype(np.int16), pa.int16()),
    }
    arrays, fields = [], []
    for name, (v, t) in cols.items():
        mask = rng.random(rows) < 0.2 if name in with_nulls else None
        arrays.append(pa.array(v, type=t, mask=mask))
        fields.append(pa.field(name, t, nullable=nullable or name in with_nulls))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def eligible_pages(path):
    """{column: data pages of its SNAPPY chunks that are PLAIN and known to hold no nulls}, from the
    page headers: a required column; a v2 header with num_nulls 0 that is compressed; a v1 header whose
    statistics say null_count 0, or without them the chunk's footer null_count 0."""
    pf = PP.PlainParquetFile(path)
    raw = open(path, "rb").read()
    out = {}
    for j, name in enumerate(pf.names):
        n = 0
        for rg in pf.row_groups:
            cc = rg["columns"][j]
            at, rows = cc["offset"], 0
            while rows < cc["num_values"]:
                r = _TReader(raw, at)
                h = r.struct()
                at = r.p + h[3]
                v1, v2 = h.get(5), h.get(8)
                if v1 is None and v2 is None:
                    continue
                rows += (v1 or v2)[1]
                if v1 is not None:
                    nulls = (v1.get(5) or {}).get(3, cc["null_count"] if cc["null_count"] >= 0 else None)
                    ok = v1[2] == 0 and (pf.max_def[j] == 0 or nulls == 0)
                else:
                    ok = v2[4] == 0 and v2.get(7, True) and (pf.max_def[j] == 0 or v2[2] == 0)
                n += bool(ok and cc["codec"] == 1 and pf.dtypes[j] != PP.BOOL_DTYPE)
        out[name] = n
    return out


def write(path, version, nullable, rows=5000, **kw):
    """``table`` written by pyarrow without dictionaries, snappy, 4 KiB pages, two row groups."""
    t = table(rows, nullable, with_nulls=kw.pop("with_nulls", ()))
    opts = dict(compression="snappy", use_dictionary=False, data_page_size=4096, data_page_version=version,
                row_group_size=rows // 2)
    opts.update(kw)
    pq.write_table(t, path, **opts)
    return pq.read_table(path)
