"""The parquet files of the string-column reader tests (test_parquet_string_host.py,
test_gpu_parquet_strings.py): about 6000 rows each, a string column "s" beside an int64 column "x"
and a float64 column "f" with nulls.  CASES[name] = (table builder, pq.write_table keywords)."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

N = 6000
SMALL_DICT = dict(row_group_size=2500, dictionary_pagesize_limit=1024, data_page_size=2048)


def _distinct(rng, n):
    """Mostly distinct 8-character strings (a few repeats)."""
    ids = rng.integers(0, 4 * n, n)
    return [f"{int(v):08x}" for v in ids]


def _nulls(values, pattern):
    if pattern == "seventh":
        return [None if i % 7 == 3 else v for i, v in enumerate(values)]
    if pattern == "group":   # rows 2000 .. 3999: one whole row group at row_group_size=2000
        return [None if 2000 <= i < 4000 else v for i, v in enumerate(values)]
    return list(values)


def table(strings, typ=pa.string(), nullable=True, seed=0):
    rng = np.random.default_rng(seed)
    n = len(strings)
    f = rng.normal(size=n)
    fmask = rng.random(n) < 0.1
    schema = pa.schema([pa.field("x", pa.int64()), pa.field("s", typ, nullable=nullable), pa.field("f", pa.float64())])
    return pa.table({"x": pa.array(rng.integers(0, 1000, n), type=pa.int64()), "s": pa.array(strings, type=typ),
                     "f": pa.array(f, mask=fmask)}, schema=schema)


def _contents(rng):
    pool = ["", "a", "größe", "日本語のテキスト", "🙂🙃", "x" * 300, "tail "]
    vals = [pool[int(i)] for i in rng.integers(0, len(pool), N)]
    vals[1234] = "L" * 70_000
    vals[0] = ""
    return vals


def _build():
    rng = np.random.default_rng(11)
    five = [("alpha", "be", "gamma-gamma", "", "δ")[int(i)] for i in rng.integers(0, 5, N)]
    distinct = _distinct(rng, N)
    return {
        "default": (table(_nulls(five, "seventh")), {}),
        "default_distinct": (table(distinct), {}),
        "plain_uncompressed": (table(_nulls(distinct, "seventh")), dict(use_dictionary=False, compression=None)),
        "page_v2": (table(_nulls(distinct, "seventh")), dict(data_page_version="2.0")),
        "small_dict_v1": (table(distinct), dict(SMALL_DICT, data_page_version="1.0")),
        "small_dict_v2": (table(_nulls(distinct, "seventh")), dict(SMALL_DICT, data_page_version="2.0")),
        "many_pages": (table(_nulls(five, "seventh")), dict(data_page_size=512, row_group_size=2500)),
        "null_group": (table(_nulls(distinct, "group")), dict(row_group_size=2000)),
        "contents": (table(_nulls(_contents(rng), "seventh"), typ=pa.large_string()), dict(row_group_size=2500)),
        "constant": (table(["same"] * N, nullable=False), dict(row_group_size=2500)),
        "long_runs": (table(sorted(five)), dict(row_group_size=2500, compression=None)),
        "required": (table(distinct, nullable=False), dict(row_group_size=2500)),
    }


CASES = _build()


def write(name, path):
    t, kw = CASES[name]
    pq.write_table(t, path, **kw)
    return t
