"""encode_reference.py pinned to the pandas oracle (no GPU): the oracle's Categorify fit +
transform on small frames equals ``encode_ref`` fed with the vocabulary file the oracle wrote, and
``hash_bucket_ref`` equals the oracle's HashBucket / HashedCross.  The kernel-level tests of
test_gpu_encode_kernels.py compare the device with these references."""
import numpy as np
import pandas as pd
import pytest

import encode_reference as R
import oracle as O

I32_MIN, I64_MIN = np.iinfo(np.int32).min, np.iinfo(np.int64).min


def _frames(dtype, nulls, sentinel, seed):
    """(fit frame, transform frame, transform keys, transform validity).  A column with nulls
    is float64 in pandas, so its keys are chosen exactly representable there."""
    rng = np.random.default_rng(seed)
    lo = I32_MIN if dtype == "int32" else I64_MIN
    if dtype == "int32":
        pool = np.concatenate([rng.integers(-2**31 + 1, 2**31 - 1, 40), [0, -1, 2**31 - 1, 7, 8]]).astype(np.int64)
    else:
        pool = np.concatenate([rng.integers(-2**40, 2**40, 40) * 2**12, [0, -1, 2**62, 2**32 + 5, 5]]).astype(np.int64)
    if sentinel:
        pool = np.append(pool, lo)
    fit = pool[np.minimum(rng.zipf(1.3, 600) - 1, pool.size - 1)]
    if sentinel:
        fit[::50] = lo
    unseen = np.array([3, -9, 123456, 2**30 + 1] + ([] if sentinel else [lo]), dtype=np.int64)
    tr = np.concatenate([pool[rng.integers(0, pool.size, 300)], unseen, fit[:50]])
    rng.shuffle(tr)
    out = []
    for x, p in ((fit, 0.1), (tr, 0.2)):
        null = rng.random(x.size) < p if nulls else np.zeros(x.size, bool)
        if nulls:
            col = x.astype(np.float64)
            assert (col.astype(np.int64) == x).all()
            col[null] = np.nan
        else:
            col = x.astype(dtype)
        out.append((pd.DataFrame({"c": col}), x.astype(dtype), ~null))
    return out[0][0], out[1][0], out[1][1], out[1][2]


@pytest.mark.parametrize("num_buckets", [None, 7])
@pytest.mark.parametrize("sentinel", [False, True], ids=["plain", "sentinel"])
@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_encode_ref_equals_the_oracle(tmp_path, dtype, nulls, sentinel, num_buckets):
    fit, tr, keys, valid = _frames(dtype, nulls, sentinel, 11 + 2 * nulls + sentinel)
    paths = O.categorify_fit([fit], ["c"], str(tmp_path), tie_break="stable", num_buckets=num_buckets)
    exp = O.categorify_transform(tr, ["c"], paths, num_buckets=num_buckets)["c"].to_numpy()
    vocab = pd.read_parquet(paths["c"])
    vk = vocab["c"].to_numpy().astype(np.int64)
    first = int(vocab.index[0])
    assert first == O.OOV_OFFSET + (num_buckets or 1)
    lo = I32_MIN if dtype == "int32" else I64_MIN
    assert (lo in vk) == sentinel and (lo in keys[valid])          # the sentinel key is in the rows either way
    # garbage under the nulls: a key of the vocabulary, the sentinel key, anything
    poison = keys.copy()
    idx = np.flatnonzero(~valid)
    poison[idx[0::3]] = vk[0]
    poison[idx[1::3]] = lo
    poison[idx[2::3]] = 77
    for out_dtype in (np.int64, np.int32):
        got = R.encode_ref(poison, valid if nulls else None, vk, first, O.NULL_OFFSET, O.OOV_OFFSET,
                           num_buckets or 0, out_dtype)
        R.first_mismatch(got, exp.astype(out_dtype), f"{dtype} nulls={nulls} sentinel={sentinel} nb={num_buckets}")
    found = R.found_mask(keys, valid, vk)
    assert found.any() and (~found & valid).any() and (not nulls or (~valid).any())


def test_encode_ref_first_occurrence_and_bucket_rules():
    vk = np.array([5, I32_MIN, 9, 5, I32_MIN, 7], dtype=np.int32)      # 5 and the sentinel key twice
    keys = np.array([5, 9, 7, I32_MIN, 6, 5], dtype=np.int32)
    valid = np.array([1, 1, 1, 1, 1, 0], bool)
    got = R.encode_ref(keys, valid, vk, 10, 1, 2, 0, np.int64)
    np.testing.assert_array_equal(got, [10, 12, 15, 11, 2, 1])
    # num_buckets 0 and 1: the bare oov label; > 1: + hash % buckets
    for nb in (0, 1):
        assert R.encode_ref(keys[4:5], None, vk, 10, 1, 2, nb, np.int32)[0] == 2
    for nb in (2, 7, 2**31 - 1):
        h = int(O.nvt_hash32(np.array([6]))[0])
        assert R.encode_ref(keys[4:5], None, vk, 10, 1, 2, nb, np.int64)[0] == 2 + h % nb
    # an empty vocabulary, no rows
    assert R.encode_ref(keys, None, vk[:0], 3, 1, 2, 0, np.int64).tolist() == [2] * 6
    assert R.encode_ref(keys[:0], None, vk, 3, 1, 2, 0, np.int32).size == 0


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_hash_bucket_ref_equals_the_oracle(dtype):
    rng = np.random.default_rng(5)
    n = 500
    a = rng.integers(-1000, 1000, n).astype(dtype)
    b = (rng.integers(-2**40, 2**40, n) if dtype == "int64" else rng.integers(-2**31, 2**31 - 1, n)).astype(dtype)
    a[:3] = [0, 1, -1]
    b[:3] = [0, np.iinfo(dtype).min, np.iinfo(dtype).max]
    null = rng.random(n) < 0.2
    fa = a.astype(np.float64)                           # (a column with nulls is float64 in pandas)
    fa[null] = np.nan
    df = pd.DataFrame({"a": fa, "b": b})
    for nb in (1, 2, 7, 2**31 - 1):
        exp = O.hash_bucket_op(df.copy(), {"a": nb, "b": nb})       # (it writes into its frame)
        np.testing.assert_array_equal(R.hash_bucket_ref(np.where(null, 12345, a).astype(dtype), ~null, nb),
                                      exp["a"].to_numpy().astype(np.int32))
        np.testing.assert_array_equal(R.hash_bucket_ref(b, None, nb), exp["b"].to_numpy().astype(np.int32))
        # the XOR chain of a hashed cross: the hash of the columns in front goes in as xor_in
        carry = R.hash64_ref(np.where(null, -1, a).astype(dtype), ~null)
        cross = O.hashed_cross(df, ["a", "b"], nb)["a_X_b"].to_numpy()
        np.testing.assert_array_equal(R.hash_bucket_ref(b, None, nb, xor_in=carry.view(np.int64)), cross)
