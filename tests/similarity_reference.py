"""Plain float64 restatement of ColumnSimilarity's definition (ISSUE / DESIGN "ColumnSimilarity"), on
dense matrices: fine at test sizes.  Not a test module."""
import math

import numpy as np


def weights(row, col, data, shape, metric, merge_first=False):
    """Dense float64 [shape] of the prepared weights.  Entry by entry: tf-idf counts every stored
    entry of a column, the norm sums w^2 over the entries (exactly: math.fsum), and only then equal
    (row, col) pairs are added up.  ``merge_first=True`` is the WRONG order (duplicates summed before
    weighting), kept so that a test can show its inputs tell the two apart."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    w = np.asarray(data, dtype=np.float64).copy()
    if merge_first:
        dense = np.zeros(shape)
        np.add.at(dense, (row, col), w)
        row, col = np.nonzero(dense)
        w = dense[row, col]
    if metric == "tfidf":
        w = w * np.log(float(shape[0]) / np.bincount(col, minlength=shape[1])[col])
    if metric in ("tfidf", "cosine"):
        sq = [[] for _ in range(shape[0])]
        for r, x in zip(row, w):
            sq[r].append(x * x)
        norm = np.array([math.sqrt(math.fsum(s)) if s else 1.0 for s in sq])
        w = w / norm[row]
    dense = np.zeros(shape)
    np.add.at(dense, (row, col), w)
    stored = np.zeros(shape, dtype=bool)
    stored[row, col] = True
    return dense, stored


def similarity(a, b, left, right, a_null=None, b_null=None):
    """(sim, L, S) per data row for ``left = (dense, stored)`` and ``right``: the dot product of row
    a[i] of left and row b[i] of right, L = the columns stored on both sides, S = sum |a_k b_k| over
    them.  NaN where an id is null or outside its matrix."""
    k = min(left[0].shape[1], right[0].shape[1])   # a column only one matrix has matches nothing
    (lw, ls), (rw, rs) = (m[:, :k] for m in left), (m[:, :k] for m in right)
    n = len(a)
    sim, L, S = np.full(n, np.nan), np.zeros(n), np.zeros(n)
    for i in range(n):
        x, y = int(a[i]), int(b[i])
        if (a_null is not None and a_null[i]) or (b_null is not None and b_null[i]):
            continue
        if not (0 <= x < lw.shape[0] and 0 <= y < rw.shape[0]):
            continue
        both = ls[x] & rs[y]
        prod = lw[x, both] * rw[y, both]
        sim[i], L[i], S[i] = math.fsum(prod), both.sum(), math.fsum(np.abs(prod))
    return sim, L, S


def assert_within_bound(got, ref, exact=False):
    sim, L, S = ref
    got = np.asarray(got, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(sim))
    ok = ~np.isnan(sim)
    if exact:
        np.testing.assert_array_equal(got[ok], sim[ok])
        return
    err, bound = np.abs(got[ok] - sim[ok]), (L[ok] + 16) * 2.0 ** -52 * S[ok]
    worst = int(np.argmax(err - bound)) if err.size else 0
    assert (err <= bound).all(), (worst, err[worst], bound[worst], L[ok][worst])
