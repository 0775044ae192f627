"""Plain numpy references of Categorify's counting step (groupby-size of a key column, the
weighted merge of partial lists, and what the one-pass vocabulary ordering reads from a count
list), for the kernel-level tests of csrc/nvt_count_lds.hip, nvt_count_part.hip, nvt_hot_sample.hip,
nvt_range_count.hip, nvt_sort_count.hip and nvt_count.hip (test_gpu_count_kernels.py).  test_count_reference.py pins
them to the pandas oracle on the CPU.  Nothing here shares code with the device side: the counts
are ``np.unique`` + ``np.add.at`` on uint64, checked against 2^63 so that the reference itself
cannot wrap.
"""
import numpy as np

from encode_reference import first_mismatch, pack_bits  # noqa: F401  (re-exported for the tests)


def count_ref(keys, valid, weights=None):
    """(keys ascending, counts int64, nulls) of a key column.

    * ``valid`` is a bool array or None (all rows valid); a null row adds its weight (1 without
      weights) to ``nulls`` and nothing else, whatever bytes lie under it;
    * the smallest integer of the key type is a key like any other (it sorts first);
    * sums are exact: accumulated in uint64, and every total is asserted to be below 2^63.
    """
    keys = np.asarray(keys)
    n = keys.size
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, dtype=bool)
    assert ok.shape == keys.shape
    if weights is None:
        w = np.ones(n, np.uint64)
    else:
        w = np.asarray(weights)
        assert w.shape == keys.shape and (w.size == 0 or int(w.min()) >= 0)
        w = w.astype(np.uint64)
    # no total can wrap uint64 (and every total is asserted to be below 2^63 further down)
    total = (int((w >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int((w & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
    assert total < 2**64, "the reference would wrap"
    nulls = int(w[~ok].sum(dtype=np.uint64))
    assert nulls < 2**63
    kk, ww = keys[ok], w[ok]
    order = np.argsort(kk, kind="stable")
    kk, ww = kk[order], ww[order]
    uniq, start = np.unique(kk, return_index=True)
    sums = np.add.reduceat(ww, start) if uniq.size else np.zeros(0, np.uint64)   # uint64 sums per run
    assert sums.dtype == np.uint64
    assert sums.size == 0 or int(sums.max()) < 2**63
    return uniq.astype(keys.dtype), sums.astype(np.int64), int(nulls)


def class_hist_ref(counts) -> np.ndarray:
    """int64[256] histogram of min(count, 255): the input of the one-pass vocabulary ordering."""
    c = np.asarray(counts).astype(np.int64)
    return np.bincount(np.minimum(c, 255), minlength=256).astype(np.int64)


def n_big_ref(counts) -> int:
    """Entries whose count is at or above 255."""
    return int((np.asarray(counts).astype(np.int64) >= 255).sum())


def merge_ref(lists):
    """Sum of the counts per key over several (keys, counts) lists -> (keys ascending, counts)."""
    lists = [(np.asarray(k), np.asarray(c)) for k, c in lists]
    if not lists:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    wide = np.int64 if any(k.dtype == np.int64 for k, _ in lists) else lists[0][0].dtype
    keys = np.concatenate([k.astype(wide) for k, _ in lists])
    counts = np.concatenate([c.astype(np.int64) for _, c in lists])
    k, c, _ = count_ref(keys, None, counts)
    return k, c


def vocab_order_ref(keys, counts):
    """(count descending, key ascending): the order of the vocabulary file."""
    keys, counts = np.asarray(keys), np.asarray(counts)
    o = np.lexsort((keys, -counts.astype(np.int64)))
    return keys[o], counts[o]


def list_mismatch(got_k, got_c, exp_k, exp_c, what: str) -> None:
    """Two key-ordered (keys, counts) lists are equal; the message names the case, the first
    differing key and both counts."""
    got_k, got_c, exp_k, exp_c = (np.asarray(a) for a in (got_k, got_c, exp_k, exp_c))
    assert got_k.dtype == exp_k.dtype, f"{what}: key dtype {got_k.dtype}, expected {exp_k.dtype}"
    if got_k.shape == exp_k.shape and (got_k == exp_k).all():
        bad = np.flatnonzero(got_c != exp_c)
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} of {exp_k.size} counts differ, first at key {exp_k[i]} "
                                 f"(entry {i}): got {got_c[i]}, expected {exp_c[i]}")
        return
    missing = np.setdiff1d(exp_k, got_k)
    extra = np.setdiff1d(got_k, exp_k)
    if missing.size or extra.size:
        raise AssertionError(f"{what}: {got_k.size} keys, expected {exp_k.size}; {missing.size} missing "
                             f"(first {missing[:1]}), {extra.size} unexpected (first {extra[:1]})")
    first_mismatch(got_k, exp_k, what + ": key order")
