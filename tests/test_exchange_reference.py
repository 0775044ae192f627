"""exchange_reference.py against independent formulations, on the CPU: the owner against
dist._range_owner, the histogram against np.bincount, words against shifts written out by hand."""
import numpy as np
import pytest
import torch

import exchange_reference as R

I32 = np.iinfo(np.int32)


def _col(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    k = rng.integers(lo, hi + 1, n).astype(np.int32)
    return k, rng.integers(1, 1000, n).astype(np.int64)


def test_ranges():
    a, b = _col(1, 50, -40, 90), _col(2, 1, 7, 7)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int64))
    zeros = (np.array([3, 4], np.int32), np.zeros(2, np.int64))
    edge = (np.array([I32.min, I32.max], np.int32), np.array([2 ** 31 - 1, 2 ** 31 - 1], np.int64))
    got = R.ranges([a, empty, b, zeros, edge])
    assert got.dtype == np.int64
    assert got.tolist() == [[-int(a[0].min()), int(a[0].max()), int(a[1].sum())], list(R.EMPTY),
                            [-7, 7, int(b[1][0])], list(R.EMPTY), [2 ** 31, 2 ** 31 - 1, 2 ** 32 - 2]]


@pytest.mark.parametrize("lo,hi", [(0, 999), (-500, 12), (I32.min, I32.max), (5, 5), (-3, 4)])
@pytest.mark.parametrize("G", [1, 2, 3, 8, 64])
def test_owner_and_hist(lo, hi, G):
    from nvtabular_amd.dist import _range_owner

    k, c = _col(G, 777, lo, hi)
    k[:2] = (lo, hi)
    width = -(-(hi - lo + 1) // G)
    exp = _range_owner(torch.from_numpy(k.astype(np.int64)), lo, hi, G).numpy()
    got = R.owner(k, lo, width, G)
    np.testing.assert_array_equal(got, exp)
    assert got.min() >= 0 and got.max() <= G - 1 and (np.diff(got[np.argsort(k, kind="stable")]) >= 0).all()
    k2, c2 = _col(G + 100, 300, lo, hi)
    mat = R.hist([(k, c), (k2, c2)], [lo, lo], [width, width], G)
    np.testing.assert_array_equal(mat[:, 0], np.bincount(exp, minlength=G))
    exp2 = _range_owner(torch.from_numpy(k2.astype(np.int64)), lo, hi, G).numpy()
    np.testing.assert_array_equal(mat[:, 1], np.bincount(exp2, minlength=G))


def test_words():
    keys = np.array([0, 1, -1, I32.min, I32.max, 5], dtype=np.int32)
    cnts = np.array([0, 1, 2 ** 31 - 1, 2 ** 31 - 1, 7, 3], dtype=np.int64)
    w = R.pack_words(keys, cnts)
    assert w.dtype == np.int64
    assert w.tolist() == [0, (1 << 32) | 1, ((2 ** 31 - 1) << 32) | 0xFFFFFFFF, ((2 ** 31 - 1) << 32) | 0x80000000,
                          (7 << 32) | 0x7FFFFFFF, (3 << 32) | 5]
    k, c = R.unpack_words(w)
    assert k.dtype == np.int32 and c.dtype == np.int64
    np.testing.assert_array_equal(k, keys)
    np.testing.assert_array_equal(c, cnts)
    # a count of 2^31 and above leaves the word: bit 31 returns as the sign, higher bits are lost
    k, c = R.unpack_words(R.pack_words([9, 9, 9], [2 ** 31, 2 ** 32 + 5, 2 ** 32 - 1]))
    assert k.tolist() == [9, 9, 9] and c.tolist() == [-2 ** 31, 5, -1]


def test_pack_ordered_and_unpack():
    G, lo, width = 3, [-10, 0], [7, 4]
    cols = [(np.arange(-10, 10, dtype=np.int32), np.arange(1, 21, dtype=np.int64)),
            (np.array([0, 3, 4, 11, 30], np.int32), np.array([5, 6, 7, 8, 9], np.int64))]
    mat = R.hist(cols, lo, width, G)
    assert mat.tolist() == [[7, 2], [7, 1], [6, 2]]
    start = np.zeros_like(mat)
    start.ravel()[1:] = np.cumsum(mat.ravel())[:-1]                  # (owner, column) groups side by side
    first_row = np.cumsum(mat, axis=0) - mat
    out = R.pack_ordered(cols, lo, width, G, first_row, start, 25, -1)
    exp = []
    for g in range(G):
        for j, (k, c) in enumerate(cols):
            sel = R.owner(k, lo[j], width[j], G) == g
            exp += R.pack_words(k[sel], c[sel]).tolist()
    assert out.tolist() == exp
    # back: segments (owner-major, column-minor) to column-major lists; one empty segment
    seg_off = np.concatenate([[0], np.cumsum(mat.ravel())])
    dst = np.zeros_like(mat)
    col_at = [0, 20]
    for j in range(2):
        dst[:, j] = col_at[j] + first_row[:, j]
    keys, cnts = np.full(25, -7, np.int32), np.full(25, -7, np.int64)
    R.unpack(out, seg_off, dst.ravel(), keys, cnts)
    assert keys.tolist() == cols[0][0].tolist() + cols[1][0].tolist()
    assert cnts.tolist() == cols[0][1].tolist() + cols[1][1].tolist()
    extra, xo = np.arange(25, dtype=np.int32), np.full(27, -7, np.int32)
    keys2, cnts2 = np.full(27, -7, np.int32), np.full(27, -7, np.int64)
    R.unpack(out, [0, 7, 7, 25], [1, 0, 9], keys2, cnts2, extra, xo)
    assert xo.tolist() == [-7] + list(range(7)) + [-7] + list(range(7, 25))
    assert keys2[1:8].tolist() == R.unpack_words(out[:7])[0].tolist() and keys2[0] == keys2[8] == -7
