"""Plain numpy references for the continuous-column kernels (nvtabular_amd/csrc/nvt_cont.hip and
the hash-bucket kernel), written for clarity, one operation at a time.

Every function takes ``(values, null, parameters)``: ``values`` a numpy array in the column's
dtype, ``null`` a bool array (True = the row's validity bit is clear) or None.  The slot under a
null row holds arbitrary bytes and must not influence any result.  test_cont_reference.py pins
these functions to the pandas oracle on the CPU; test_gpu_cont_kernels.py compares the kernels
with them element by element."""
import math

import numpy as np

import oracle as O


def null_rows(x, null):
    """Rows the kernels treat as missing: validity bit clear, or NaN in a float column."""
    x = np.asarray(x)
    m = np.zeros(x.shape, dtype=bool) if null is None else np.asarray(null, dtype=bool).copy()
    if x.dtype.kind == "f":
        m |= np.isnan(x)
    return m


def pack_bits(valid_bool):
    """Arrow validity bitmap (LSB first) of a bool array, padded to whole bytes."""
    return np.packbits(np.asarray(valid_bool, dtype=bool), bitorder="little")


# ---- moments -------------------------------------------------------------------------------
def moment_terms(x, null, fill=None):
    """float64 value of every row that counts: the fill for missing rows when there is one,
    those rows skipped otherwise."""
    x = np.asarray(x)
    m = null_rows(x, null)
    v = np.where(m, 0, x).astype(np.float64)
    if fill is None:
        return v[~m]
    v[m] = float(fill)
    return v


def moments(x, null, fill=None):
    """(count as int, sum, sum of squares), the two sums correctly rounded (math.fsum)."""
    v = moment_terms(x, null, fill)
    return int(v.size), math.fsum(v.tolist()), math.fsum((v * v).tolist())


def finalize_moments(count, total, sq):
    """(mean, std) as moments.py:89-116 finishes them, every operation rounded once."""
    count, total, sq = float(count), np.float64(total), np.float64(sq)
    if count == 0:
        return float("nan"), float("nan")
    with np.errstate(all="ignore"):
        var = sq - total * total / count
        var = var / max(count - 1.0, 1.0)
        if count - 1.0 == 0:
            var = np.float64("nan")
        std = float(np.sqrt(var)) if var == var and var >= 0 else float("nan")
        return float(total / count), std


# ---- min / max ------------------------------------------------------------------------------
def minmax(x, null, prev=None):
    """(min, max) as float64 over the rows that are neither null nor NaN; NaN when none is left.
    ``prev`` = an earlier (min, max) pair to fold in (NaN = empty)."""
    x = np.asarray(x)
    v = np.where(null_rows(x, null), 0, x).astype(np.float64)[~null_rows(x, null)]
    lo = [float(v.min())] if v.size else []
    hi = [float(v.max())] if v.size else []
    if prev is not None:
        lo += [float(prev[0])] if prev[0] == prev[0] else []
        hi += [float(prev[1])] if prev[1] == prev[1] else []
    return (min(lo) if lo else float("nan")), (max(hi) if hi else float("nan"))


# ---- FillMissing + Normalize ------------------------------------------------------------------
def fill_normalize(x, null, fill, do_norm, shift, scale, out_dtype):
    """-> (out, filled).  ``filled`` is 1 exactly on null-or-NaN rows.

    do_norm = False: pure fill in the output type; an integer column stays exact; a missing row
    without a fill is NaN (float output) or 0 (integer output: the caller keeps the bitmap).
    do_norm = True: (v - shift) / scale, ``scale <= 0`` = subtract only.  float32 INPUT: both
    operations in float32 (normalize.py:79-84: the Python float operands are weak scalars), then
    converted; every other input: float64 arithmetic."""
    x = np.asarray(x)
    out_dtype = np.dtype(out_dtype)
    m = null_rows(x, null)
    filled = m.astype(np.uint8)
    safe = np.where(m, 0, x).astype(x.dtype)      # never look at the slot under a null
    with np.errstate(all="ignore"):
        if not do_norm:
            out = safe.astype(out_dtype)
            if fill is not None:
                out[m] = out_dtype.type(fill)
            elif out_dtype.kind == "f":
                out[m] = np.nan
            else:
                out[m] = 0
            return out, filled
        assert out_dtype.kind == "f"
        work = np.float32 if x.dtype == np.float32 else np.float64
        v = safe.astype(work)
        v[m] = work(fill) if fill is not None else work("nan")
        v = v - work(shift)
        if scale > 0:
            v = v / work(scale)
        return v.astype(out_dtype), filled


# ---- Clip / LogOp -------------------------------------------------------------------------------
def clip(x, null, fill, vmin, vmax, out_dtype):
    """clip.py:49-55 after an optional fill: assign the bound only where the comparison is true.
    Integer in -> the same integer type out is done in that type (a value inside the bounds is
    never changed); everything else compares in float64 and converts.  Missing rows without a
    fill: NaN (float output) / 0 (integer output)."""
    x = np.asarray(x)
    out_dtype = np.dtype(out_dtype)
    m = null_rows(x, null)
    exact = x.dtype.kind == "i" and out_dtype == x.dtype
    work = x.dtype if exact else np.dtype(np.float64)
    v = np.where(m, 0, x).astype(work)
    if fill is not None:
        v[m] = work.type(fill)
    if vmin is not None:
        v[v < work.type(vmin)] = work.type(vmin)
    if vmax is not None:
        v[v > work.type(vmax)] = work.type(vmax)
    with np.errstate(all="ignore"):
        out = v.astype(out_dtype)
    if fill is None:
        out[m] = np.nan if out_dtype.kind == "f" else 0
    return out


def log_argument(x, null, fill, vmin, vmax):
    """float32(v) + float32(1) for the clipped value v (logop.py:43-53 computes in float32);
    NaN on missing rows without a fill."""
    v = clip(x, null, fill, vmin, vmax, np.float64)
    with np.errstate(all="ignore"):
        return v.astype(np.float32) + np.float32(1)


def log1p_f32(x, null, fill=None, vmin=None, vmax=None):
    """The float64 logarithm of the float32 argument."""
    with np.errstate(all="ignore"):
        return np.log(log_argument(x, null, fill, vmin, vmax).astype(np.float64))


# ---- Bucketize ----------------------------------------------------------------------------------
def bucketize(x, null, boundaries):
    """np.digitize(x, b, right=False) as int32; null / NaN rows get len(b)."""
    x = np.asarray(x)
    b = np.asarray(boundaries, dtype=np.float64)
    m = null_rows(x, null)
    v = np.where(m, 0, x).astype(np.float64)
    out = np.digitize(v, b, right=False).astype(np.int32)
    out[m] = len(b)
    return out


# ---- JoinGroupby / TargetEncoding row-wise joins (the formulas of the kernel comments) ------------
def gather(src, group, miss, out_dtype):
    """out[i] = src[group[i]] for group >= 0, ``miss`` otherwise; float64, then converted (C
    conversion: integers truncate towards zero)."""
    src = np.asarray(src, dtype=np.float64)
    group = np.asarray(group, dtype=np.int64)
    v = np.full(group.shape, float(miss), dtype=np.float64)
    hit = group >= 0
    v[hit] = src[group[hit]]
    with np.errstate(all="ignore"):
        return v.astype(out_dtype)


def te_apply(group_all, group_fold, sum_all, cnt_all, sum_fold, cnt_fold, p, y_mean):
    """target_encoding.py:340-374 in float64 -> (value, s, c, formula rows).  Without folds:
    (sum_all[g] + p * y_mean) / (cnt_all[g] + p) for g >= 0.  With folds (group_fold given): rows
    with g >= 0 and f >= 0 take ((sum_all[g] - sum_fold[f]) + p * y_mean) / ((cnt_all[g] -
    cnt_fold[f]) + p).  Every other row: y_mean.  ``s`` and ``c`` are returned for the bound."""
    g = np.asarray(group_all, dtype=np.int64)
    n = g.size
    use = g >= 0
    if group_fold is not None:
        f = np.asarray(group_fold, dtype=np.int64)
        use &= f >= 0
    s = np.zeros(n, dtype=np.float64)
    c = np.zeros(n, dtype=np.float64)
    s[use] = np.asarray(sum_all, dtype=np.float64)[g[use]]
    ci = np.zeros(n, dtype=np.int64)
    ci[use] = np.asarray(cnt_all, dtype=np.int64)[g[use]]
    if group_fold is not None:
        s[use] = s[use] - np.asarray(sum_fold, dtype=np.float64)[f[use]]
        ci[use] = ci[use] - np.asarray(cnt_fold, dtype=np.int64)[f[use]]
    c = ci.astype(np.float64)
    out = np.full(n, float(y_mean), dtype=np.float64)
    with np.errstate(all="ignore"):
        prod = np.float64(p) * np.float64(y_mean)
        out[use] = (s[use] + prod) / (c[use] + np.float64(p))
    return out, s, c, use


def te_apply_folds(group_all, fold, kfold, sum_all, cnt_all, sum_fold, cnt_fold, p, y_mean):
    """Dense fold statistics: entry g * kfold + fold[i] belongs to (group g, fold of row i); a pair
    with fold count 0 has no rows and is the reference's unmatched merge (y_mean)."""
    g = np.asarray(group_all, dtype=np.int64)
    n = g.size
    idx = np.where(g >= 0, g, 0) * int(kfold) + np.asarray(fold, dtype=np.int64)
    cf = np.where(g >= 0, np.asarray(cnt_fold, dtype=np.int64)[idx] if n else 0, 0)
    use = (g >= 0) & (cf > 0)
    s = np.zeros(n, dtype=np.float64)
    c = np.zeros(n, dtype=np.float64)
    s[use] = np.asarray(sum_all, dtype=np.float64)[g[use]] - np.asarray(sum_fold, dtype=np.float64)[idx[use]]
    c[use] = (np.asarray(cnt_all, dtype=np.int64)[g[use]] - cf[use]).astype(np.float64)
    out = np.full(n, float(y_mean), dtype=np.float64)
    with np.errstate(all="ignore"):
        prod = np.float64(p) * np.float64(y_mean)
        out[use] = (s[use] + prod) / (c[use] + np.float64(p))
    return out, s, c, use


def te_bound(s, c, p, y_mean):
    """The compiler may fuse ``s + p * y_mean`` into one FMA.  Fused or not, numerator and quotient
    are each within a few roundings of the exact value: 4 * 2**-53 * (|s| + |p * y_mean|) /
    |c + p| absolute covers both forms."""
    with np.errstate(all="ignore"):
        return 4 * 2.0**-53 * (np.abs(s) + abs(float(p) * float(y_mean))) / np.abs(c + float(p))


# ---- small ones ---------------------------------------------------------------------------------
def widen(x):
    x = np.asarray(x)
    return (x.view(np.uint8) if x.dtype == np.bool_ else x).astype(np.int64)


def popcount(valid_bool):
    return int(np.count_nonzero(np.asarray(valid_bool, dtype=bool)))


def hash64(keys, null, xor_in=None):
    """DESIGN.md section 4 hash; a null row hashes as key 0 whatever its slot holds."""
    k = np.asarray(keys).astype(np.int64)
    if null is not None:
        k = np.where(np.asarray(null, dtype=bool), 0, k)
    h = O.nvt_hash64(k)
    return h if xor_in is None else h ^ np.asarray(xor_in).view(np.uint64)


def hash_bucket(keys, null, num_buckets, xor_in=None):
    h = hash64(keys, null, xor_in)
    return ((h >> np.uint64(32)) % np.uint64(num_buckets)).astype(np.int32)


# ---- comparisons used by both test files -------------------------------------------------------
def assert_bits_equal(got, exp, what=""):
    """Same dtype, same NaN positions, and the same bits everywhere else (so -0.0 != +0.0)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    if got.dtype.kind == "f":
        gn, en = np.isnan(got), np.isnan(exp)
        bad = np.flatnonzero(gn != en)
        assert bad.size == 0, f"{what}: NaN positions differ at rows {bad[:8]} (got {got[bad[:8]]}, expected {exp[bad[:8]]})"
        iv = np.int32 if got.dtype == np.float32 else np.int64
        g, e = np.where(gn, 0, got).astype(got.dtype).view(iv), np.where(en, 0, exp).astype(exp.dtype).view(iv)
    else:
        g, e = got, exp
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, (
        f"{what}: {bad.size} of {got.size} elements differ, first rows {bad[:8]}: "
        f"got {got[bad[:8]]!r}, expected {exp[bad[:8]]!r}")
