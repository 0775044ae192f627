"""order_reference.py pinned on the CPU (no GPU): ``vocab_order_ref`` equals the two stable
``sort_values`` of the reference's vocabulary order in pandas (by key, then by count descending),
``positions_ref`` is its inverse permutation, ``class_hist_ref`` a plain loop over the counts, and
``labels_ref`` a dictionary lookup.  The kernel-level tests of test_gpu_order_kernels.py compare the
device with these references."""
import numpy as np
import pandas as pd
import pytest

import order_reference as R

I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def _list(dtype, n, seed):
    """A duplicate-free key list in random order with the extremes of the type, and counts with
    heavy ties, the class boundaries and values beyond 32 bits."""
    rng = np.random.default_rng(seed)
    i = np.iinfo(dtype)
    keys = np.unique(np.concatenate([rng.integers(i.min, i.max, n, dtype=np.int64), [i.min, i.max, 0, -1, 1]]))
    keys = rng.permutation(keys).astype(dtype)
    counts = np.minimum(rng.zipf(1.5, keys.size), 300).astype(np.int64)
    counts[:8] = [254, 255, 256, 255, 2**32, 2**40, 2**32 + 1, 254]
    return keys, counts


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
def test_vocab_order_ref_equals_two_stable_sort_values(dtype):
    keys, counts = _list(dtype, 700, 5)
    df = pd.DataFrame({"c": keys, "c_size": counts})
    df = df.sort_values("c", kind="stable", ignore_index=True)
    df = df.sort_values("c_size", ascending=False, kind="stable", ignore_index=True)
    vk, vc = R.vocab_order_ref(keys, counts)
    assert vk.dtype == dtype and vc.dtype == np.int64
    R.first_mismatch(vk, df["c"].to_numpy(), "vocabulary order")
    R.first_mismatch(vc, df["c_size"].to_numpy(), "ordered counts")
    assert np.unique(counts).size < counts.size // 4               # ties: the key order decides
    assert vc[0] == 2**40 and vc[1] == 2**32 + 1 and vc[2] == 2**32
    # the order does not depend on the order of the list
    p = np.random.default_rng(6).permutation(keys.size)
    vk2, vc2 = R.vocab_order_ref(keys[p], counts[p])
    R.first_mismatch(vk2, vk, "order of a permuted list")
    R.first_mismatch(vc2, vc, "counts of a permuted list")
    # positions_ref: entry i of the list sits at position pos[i] of the order
    pos = R.positions_ref(keys, counts)
    assert pos.dtype == np.int32 and np.array_equal(np.sort(pos), np.arange(keys.size))
    R.first_mismatch(vk[pos], keys, "positions_ref")
    assert R.vocab_order_ref(keys[:0], counts[:0])[0].size == 0 and R.positions_ref(keys[:0], counts[:0]).size == 0


def test_class_hist_ref_rules():
    counts = np.array([1, 0, -7, 254, 255, 256, 2**40, 1, 1, 2**32, 253], np.int64)
    h = R.class_hist_ref(counts)
    exp = np.zeros(256, np.int32)
    for c in counts.tolist():
        exp[min(max(c, 0), 255)] += 1
    assert h.dtype == np.int32 and h.shape == (256,)
    np.testing.assert_array_equal(h, exp)
    assert h[0] == 2 and h[1] == 3 and h[253] == 1 and h[254] == 1 and h[255] == 4 == R.n_big_ref(counts)
    assert int(R.class_hist_ref(counts[:0]).sum()) == 0


def test_labels_ref_rules():
    vk = np.array([9, I32_MAX, -4, 0, 7], np.int32)                # an ordered vocabulary without the smallest key
    keys = np.array([7, 8, I32_MIN, I32_MAX, I32_MAX - 1, -4, -5, 9, 9, 0], np.int32)
    got = R.labels_ref(keys, vk, 3)
    lookup = {int(k): 3 + j for j, k in enumerate(vk)}
    assert got.dtype == np.int64
    assert got.tolist() == [lookup.get(int(k), -1) for k in keys] == [7, -1, -1, 4, -1, 5, -1, 3, 3, 6]
    # the smallest key of the type is a key like any other
    vk2 = np.array([5, I32_MIN, 6], np.int32)
    assert R.labels_ref(np.array([I32_MIN, I32_MIN + 1, 6], np.int32), vk2, 10).tolist() == [11, -1, 12]
    # int64 keys that differ only above bit 32
    vk3 = np.array([5, 5 + (1 << 32), 5 - (1 << 32), np.iinfo(np.int64).min], np.int64)
    assert R.labels_ref(np.array([5 + (1 << 32), 5 + (2 << 32), np.iinfo(np.int64).min, 5]), vk3, 0).tolist() \
        == [1, -1, 3, 0]
    assert R.labels_ref(keys, vk[:0], 3).tolist() == [-1] * keys.size
    assert R.labels_ref(keys[:0], vk, 3).size == 0
    with pytest.raises(AssertionError, match="twice"):
        R.labels_ref(keys, np.array([1, 2, 1], np.int32), 0)


def test_labels_ref_agrees_with_vocab_order_ref():
    keys, counts = _list(np.int32, 500, 9)
    vk, _ = R.vocab_order_ref(keys, counts)
    R.first_mismatch(R.labels_ref(keys, vk, 3), 3 + R.positions_ref(keys, counts).astype(np.int64),
                     "labels of the vocabulary's own keys")
