"""filter_terms_reference.py against pyarrow: for a 200-row table with nulls, NaN, +-0.0 and
INT64_MIN / INT64_MAX in the column types int32, int64, float32, float64, bool, string and
timestamp[ms], every operator and 200 seeded random DNFs keep exactly the rows
``pyarrow.parquet.read_table(filters=...)`` keeps.  The members of ``in`` on the float32 column are
exactly representable in float32 (pyarrow narrows the set, the reference widens the column).  Also:
the mask words and tile counts of ``plan``, and that the package's own typing of the same DNFs
(filters.validate) loses nothing: evaluating its normalised terms gives the same rows."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import filter_terms_reference as R

N = 200
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def make_table(n=N, seed=5):
    rng = np.random.default_rng(seed)
    i32 = rng.integers(-5, 6, n).astype(np.int32)
    i64 = rng.integers(-3, 4, n).astype(np.int64)
    i64[:4] = [I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
    f32 = (rng.integers(-8, 9, n) * 0.25).astype(np.float32)
    f32[5:9] = [np.nan, -0.0, 0.0, np.float32(0.1)]
    f64 = rng.integers(-8, 9, n) * 0.1
    f64[9:13] = [np.nan, -0.0, 0.0, 1e300]
    b = rng.random(n) < 0.5
    s = np.array([["a", "b", "", "zebra", "é"][k] for k in rng.integers(0, 5, n)], dtype=object)
    ts = (np.datetime64("2024-01-01", "ms") + rng.integers(0, 6, n) * np.timedelta64(12, "h")).astype("datetime64[ms]")
    cols = {"i32": i32, "i64": i64, "f32": f32, "f64": f64, "b": b, "s": s, "ts": ts}
    valid = {name: rng.random(n) >= 0.15 for name in cols}
    valid["i64"][:4] = True
    valid["f32"][5:9] = True
    valid["f64"][9:13] = True
    return cols, valid


def arrow_table(cols, valid):
    arrays = {"row": pa.array(np.arange(len(cols["i32"]), dtype=np.int64))}
    for name, vals in cols.items():
        mask = ~valid[name]
        if name == "s":
            arrays[name] = pa.array(vals, type=pa.string(), mask=mask)
        elif name == "ts":
            arrays[name] = pa.array(vals, type=pa.timestamp("ms"), mask=mask)
        else:
            arrays[name] = pa.array(vals, mask=mask)
    return pa.table(arrays)


CONSTANTS = {
    "i32": [-5, 0, 3, 5, 7],
    "i64": [I64_MIN, I64_MAX, -1, 0, 2, I64_MIN + 1],
    "f32": [-0.0, 0.0, 0.25, -1.5, 2.0, 0.1, 0.5],
    "f64": [-0.0, 0.0, 0.1, -0.30000000000000004, 0.5, 1e300, 2],
    "b": [True, False],
    "s": ["a", "", "zebra", "é", "nope"],
    "ts": [pd.Timestamp("2024-01-01"), pd.Timestamp("2024-01-02 12:00"), np.datetime64("2024-01-03", "ms"),
           pd.Timestamp("2030-01-01")],
}
# `in` members: exactly representable in the column's type, and no zeros in the float sets (pyarrow's
# is_in matches a zero by its sign bit; here a member is compared as ==, where -0.0 == 0.0)
MEMBERS = dict(CONSTANTS, f32=[0.25, -1.5, 2.0, 0.5, -2.0], f64=[0.1, -0.30000000000000004, 0.5, 1e300, 2],
               i64=[I64_MIN, I64_MAX, -1, 0, 2],
               ts=[pd.Timestamp("2024-01-01"), pd.Timestamp("2024-01-02 12:00"), pd.Timestamp("2024-01-03"),
                   pd.Timestamp("2030-01-01")])   # (pyarrow builds one array of a set: one type)
ORDERED = ("<", "<=", ">", ">=")


def ops_of(name):
    return [op for op in R.OPS if not (name == "s" and op in ORDERED)]


def random_term(rng):
    name = list(CONSTANTS)[rng.integers(0, len(CONSTANTS))]
    ops = ops_of(name)
    op = ops[rng.integers(0, len(ops))]
    if op in ("in", "not in"):
        pool = MEMBERS[name]
        k = int(rng.integers(0, len(pool) + 1))
        value = [pool[i] for i in rng.permutation(len(pool))[:k]]
        if not value:
            value = [pool[0]] if op == "not in" else []
    else:
        pool = CONSTANTS[name]
        value = pool[rng.integers(0, len(pool))]
    return (name, op, value)


def random_dnf(rng):
    return [[random_term(rng) for _ in range(rng.integers(1, 4))] for _ in range(rng.integers(1, 4))]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    cols, valid = make_table()
    path = str(tmp_path_factory.mktemp("filter_ref") / "t.parquet")
    pq.write_table(arrow_table(cols, valid), path, row_group_size=64)
    return path, {name: (cols[name], valid[name]) for name in cols}


def pyarrow_rows(path, dnf):
    # (pyarrow types an empty list as a set of nulls, which it casts to numbers but not to strings)
    dnf = [[(c, op, pa.array([], pa.string()) if c == "s" and op == "in" and len(v) == 0 else v)
            for c, op, v in conj] for conj in dnf]
    return pq.read_table(path, filters=dnf, columns=["row"]).column("row").to_numpy()


def check(path, cols, dnf):
    want = pyarrow_rows(path, dnf)
    got = np.flatnonzero(R.keep_mask(dnf, cols, N))
    np.testing.assert_array_equal(got, want, err_msg=repr(dnf))


@pytest.mark.parametrize("name", list(CONSTANTS))
def test_every_operator_matches_pyarrow(data, name):
    path, cols = data
    for op in ops_of(name):
        if op in ("in", "not in"):
            values = [MEMBERS[name], MEMBERS[name][:1], MEMBERS[name][1:3]] + ([[]] if op == "in" else [])
        else:
            values = CONSTANTS[name]
        for value in values:
            check(path, cols, [[(name, op, value)]])


def test_nan_constant_and_signed_zero(data):
    path, cols = data
    for name in ("f32", "f64"):
        check(path, cols, [[(name, "!=", float("nan"))]])
        check(path, cols, [[(name, "==", float("nan"))]])
        check(path, cols, [[(name, "==", -0.0)]])
        check(path, cols, [[(name, ">=", 0.0), (name, "<=", -0.0)]])


def test_random_dnfs_match_pyarrow(data):
    path, cols = data
    rng = np.random.default_rng(2024)
    kept_some = 0
    for _ in range(200):
        dnf = random_dnf(rng)
        check(path, cols, dnf)
        kept_some += bool(R.keep_mask(dnf, cols, N).any())
    assert kept_some > 100


def test_the_package_types_the_same_filters(data):
    """filters.validate turns constants into the host domain (ints for bools and datetimes, sorted
    distinct sets): its terms, evaluated by the reference on the same domain, keep the same rows."""
    from nvtabular_amd import filters as F
    from nvtabular_amd.schema import Schema

    path, cols = data
    schema = Schema.from_frame(pq.read_schema(path))
    dom = dict(cols)
    dom["ts"] = (cols["ts"][0].view(np.int64), cols["ts"][1])
    dom["b"] = (cols["b"][0].astype(np.int64), cols["b"][1])
    rng = np.random.default_rng(7)
    for _ in range(200):
        dnf = random_dnf(rng)
        flt = F.validate(F.normalize(dnf), schema)
        np.testing.assert_array_equal(R.keep_mask(flt.as_tuples(), dom, N), R.keep_mask(dnf, cols, N), err_msg=repr(dnf))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17])
def test_plan_words_and_counts(n):
    rng = np.random.default_rng(n)
    keep = rng.random(n) < 0.4
    words, counts = R.plan(keep)
    nt = (n + 2047) // 2048
    assert words.shape == (nt * 32,) and counts.shape == (nt,)
    for i in range(nt * 2048):
        bit = (int(words[i // 64]) >> (i % 64)) & 1
        assert bit == (int(keep[i]) if i < n else 0)
        if n > 4096 and i > 200:
            break
    got = np.unpackbits(words.view(np.uint8), bitorder="little")
    np.testing.assert_array_equal(got[:n], keep)
    assert not got[n:].any()
    np.testing.assert_array_equal(counts, [keep[t * 2048: (t + 1) * 2048].sum() for t in range(nt)])
