"""count_reference.py pinned to the pandas oracle (no GPU): ``count_ref`` equals the oracle's
top-level groupby-size on nullable int32 / int64 frames (nulls and the smallest integer of the type
among the keys), ``merge_ref`` its mid-level groupby over several partitions, and the (count
descending, key ascending) order of the reference's list the oracle's stable vocabulary order.
The kernel-level tests of test_gpu_count_kernels.py compare the device with these references."""
import numpy as np
import pandas as pd
import pytest

import count_reference as R
import oracle as O

OPTS = O.GroupbyOptions(col_groups=[["c"]], agg_list=["size"], name_sep="_")


def _column(dtype, n, seed, sentinel=True):
    """(keys, validity): zipf over a pool that holds the extremes of the type; poison under nulls."""
    rng = np.random.default_rng(seed)
    i = np.iinfo(dtype)
    pool = np.concatenate([rng.integers(i.min + 1, i.max, 60), [0, -1, 1, i.max]]).astype(dtype)
    if sentinel:
        pool = np.append(pool, np.array([i.min], dtype))
    keys = pool[np.minimum(rng.zipf(1.3, n) - 1, pool.size - 1)]
    if sentinel:
        keys[::41] = i.min
    valid = rng.random(n) >= 0.15
    bad = np.flatnonzero(~valid)
    keys[bad[0::3]] = pool[0]          # a key of the column
    keys[bad[1::3]] = i.min            # the smallest integer
    keys[bad[2::3]] = 77               # anything
    return keys, valid


def _frame(keys, valid):
    """A nullable integer column (exact for every int64, unlike float64 with NaN)."""
    arr = pd.array(keys, dtype="Int32" if keys.dtype == np.int32 else "Int64")
    arr[~valid] = pd.NA
    return pd.DataFrame({"c": arr})


def _split(gb):
    """oracle groupby frame -> (keys int64 ascending, sizes int64, null size)."""
    null = gb["c"].isna()
    nulls = int(gb.loc[null, "c_size"].sum())
    body = gb[~null].sort_values("c")
    return body["c"].to_numpy(dtype=np.int64), body["c_size"].to_numpy(dtype=np.int64), nulls


@pytest.mark.parametrize("sentinel", [False, True], ids=["plain", "sentinel"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
def test_count_ref_equals_the_oracles_top_level_groupby(dtype, sentinel):
    keys, valid = _column(dtype, 700, 3 + sentinel, sentinel)
    gb = O.top_level_groupby(_frame(keys, valid), OPTS)[0]
    ek, ec, en = _split(gb)
    k, c, nulls = R.count_ref(keys, valid)
    assert k.dtype == dtype and c.dtype == np.int64
    R.list_mismatch(k.astype(np.int64), c, ek, ec, f"{np.dtype(dtype).name} sentinel={sentinel}")
    assert nulls == en == int((~valid).sum()) and nulls > 0
    assert (np.iinfo(dtype).min in k) == sentinel            # under a valid bit only when asked for
    assert int(c.sum()) + nulls == keys.size
    # no bitmap = all valid; an all-null column has no keys
    k2, c2, n2 = R.count_ref(keys, None)
    assert n2 == 0 and int(c2.sum()) == keys.size
    k3, c3, n3 = R.count_ref(keys, np.zeros(keys.size, bool))
    assert k3.size == 0 and c3.size == 0 and n3 == keys.size


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
def test_merge_ref_equals_the_oracles_mid_level_groupby(dtype):
    parts, lists, nulls = [], [], 0
    for p in range(4):
        keys, valid = _column(dtype, 300 + 50 * p, 20 + p)
        parts.append(O.top_level_groupby(_frame(keys, valid), OPTS)[0])
        k, c, nn = R.count_ref(keys, valid)
        lists.append((k, c))
        nulls += nn
    ek, ec, en = _split(O.mid_level_groupby(parts, ["c"], OPTS))
    k, c = R.merge_ref(lists)
    R.list_mismatch(k.astype(np.int64), c, ek, ec, f"merge {np.dtype(dtype).name}")
    assert en == nulls
    # weights: a merge of merges is the merge of everything
    k2, c2 = R.merge_ref([R.merge_ref(lists[:2]), R.merge_ref(lists[2:])])
    R.list_mismatch(k2, c2, k, c, "merge of merges")
    assert R.merge_ref([])[0].size == 0


def test_vocab_order_equals_the_oracles_stable_order():
    keys, valid = _column(np.int32, 900, 7)
    gb = O.top_level_groupby(_frame(keys, valid), OPTS)[0]
    ordered, null_size = O.order_uniques(gb, ["c"], tie_break="stable")
    k, c, nulls = R.count_ref(keys, valid)
    vk, vc = R.vocab_order_ref(k, c)
    np.testing.assert_array_equal(vk.astype(np.int64), ordered["c"].to_numpy(dtype=np.int64))
    np.testing.assert_array_equal(vc, ordered["c_size"].to_numpy(dtype=np.int64))
    assert int(null_size) == nulls
    assert np.unique(c).size < c.size                       # ties: the key order decides


def test_count_ref_weights_and_histogram_rules():
    keys = np.array([5, 5, -2**31, 9, 5, 9, 7], np.int32)
    valid = np.array([1, 1, 1, 1, 0, 1, 1], bool)
    w = np.array([2**40, 2**40, 3, 2**62, 11, 2**62 - 1, 1], np.int64)
    k, c, nulls = R.count_ref(keys, valid, w)
    assert k.tolist() == [-2**31, 5, 7, 9] and c.tolist() == [3, 2**41, 1, 2**63 - 1] and nulls == 11
    with pytest.raises(AssertionError):
        R.count_ref(keys, valid, w + (keys == 9))             # 2^63: the reference refuses to wrap
    counts = np.array([1, 254, 255, 256, 2**40, 1], np.int64)
    h = R.class_hist_ref(counts)
    assert h.size == 256 and h[1] == 2 and h[254] == 1 and h[255] == 3 and int(h.sum()) == 6
    assert R.n_big_ref(counts) == 3 and R.n_big_ref(counts[:2]) == 0
    with pytest.raises(AssertionError, match="first at key 7"):
        R.list_mismatch(k, c + (k == 7), k, c, "case")
    with pytest.raises(AssertionError, match="1 missing"):
        R.list_mismatch(k[1:], c[1:], k, c, "case")
