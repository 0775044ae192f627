"""hive_reference.py pinned against pandas.factorize, and the segment encoding of
nvtabular_amd/hive.py pinned against the directories pyarrow.parquet.write_to_dataset makes."""
import os

import numpy as np
import pandas as pd
import pytest

import hive_reference as R
from nvtabular_amd import hive

STRINGS = ["a/b", "x=y", "p%q r", "é", "", None]
INTS = [1, -3, None]


def _factorize(keys):
    codes, uniques = pd.factorize(pd.Series(list(keys), dtype=object), use_na_sentinel=False)
    first = np.array([int(np.flatnonzero(codes == l)[0]) for l in range(len(uniques))], dtype=np.uint32)
    return codes.astype(np.uint32), first


@pytest.mark.parametrize("case", ["one", "interleaved", "nulls", "pairs", "random"])
def test_labels_are_first_appearance_ranks(case):
    rng = np.random.default_rng(7)
    nkeys, words = 1, None
    if case == "one":
        tags, nulls = np.array([5] * 9, dtype=np.uint64), np.zeros(9, np.uint8)
    elif case == "interleaved":
        tags, nulls = np.array([9, 3, 9, 7, 3, 0, 7, 2 ** 63, 0], dtype=np.uint64), np.zeros(9, np.uint8)
    elif case == "nulls":   # null rows are one key whatever their tag; a non-null row with that tag is another
        tags = np.array([4, 1, 4, 8, 1, 8, 4], dtype=np.uint64)
        nulls = np.array([0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    elif case == "pairs":
        nkeys = 2
        a, b = rng.integers(0, 5, 200), rng.integers(0, 4, 200)
        words = np.stack([a, b]).astype(np.uint64)
        tags, nulls = (a * 1000003 + b).astype(np.uint64), np.zeros(200, np.uint8)
    else:
        tags, nulls = rng.integers(0, 300, 5000).astype(np.uint64), (rng.random(5000) < 0.1).astype(np.uint8)
    keys = [("null",) if (nkeys == 1 and nl) else (int(t),) for t, nl in zip(tags, nulls)]
    want_label, want_first = _factorize(keys)
    label, first, D, status = R.key_labels(tags, nulls, words, nkeys)
    assert status == 0 and D == len(want_first)
    np.testing.assert_array_equal(label, want_label)
    np.testing.assert_array_equal(first, want_first)
    fl, ff, fD, _ = R.key_labels_fast(tags, nulls, nkeys)
    np.testing.assert_array_equal(fl, want_label)
    np.testing.assert_array_equal(ff, want_first)
    assert fD == D


def test_status_words():
    tags = np.arange(R.LABEL_MAX + 1, dtype=np.uint64)
    assert R.key_labels(tags, np.zeros(len(tags), np.uint8))[2:] == (R.LABEL_MAX + 1, 1)
    assert R.key_labels_fast(tags, np.zeros(len(tags), np.uint8))[2:] == (R.LABEL_MAX + 1, 1)
    assert R.key_labels(tags[:-1], np.zeros(R.LABEL_MAX, np.uint8))[2:] == (R.LABEL_MAX, 0)
    # equal tags, different words: a fingerprint collision
    words = np.array([[1, 1, 2], [7, 7, 7]], dtype=np.uint64)
    assert R.key_labels(np.array([3, 3, 3], np.uint64), np.zeros(3, np.uint8), words, 2)[3] == 2
    # equal tags and words, different null bits
    words = np.array([[1, 1, 1], [7, 7, 7]], dtype=np.uint64)
    assert R.key_labels(np.array([3, 3, 3], np.uint64), np.array([0, 2, 0], np.uint8), words, 2)[3] == 2
    assert R.key_labels(np.array([3, 3, 3], np.uint64), np.zeros(3, np.uint8), words, 2)[3] == 0


@pytest.mark.parametrize("values, typ", [(STRINGS, "string"), (INTS, "int64")])
def test_segments_are_pyarrows(tmp_path, values, typ):
    import pyarrow as pa
    import pyarrow.parquet as pq

    table = pa.table({"k": pa.array(values, type=pa.string() if typ == "string" else pa.int64()),
                      "x": pa.array(range(len(values)), type=pa.int64())})
    pq.write_to_dataset(table, str(tmp_path), partition_cols=["k"])
    made = sorted(d for d in os.listdir(tmp_path) if os.path.isdir(tmp_path / d))
    assert made == sorted(hive.dir_name(["k"], [v]) for v in values)
    for v in values:
        key, seg = hive.parse_dir(hive.dir_name(["k"], [v]))
        assert key == "k"
        assert hive.decode_segment(seg) == (None if v is None else str(v))
    assert hive.encode_segment("a/b") == "a%2Fb" and hive.encode_segment("x=y") == "x%3Dy"
    assert hive.encode_segment("é") == "%C3%A9" and hive.encode_segment("") == ""
    assert hive.encode_segment(None) == "__HIVE_DEFAULT_PARTITION__"
    assert hive.parse_dir("part_0.parquet") is None and hive.parse_dir("=x") is None
    assert hive.parse_dir("k=") == ("k", "")
