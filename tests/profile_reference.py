"""Plain numpy / pandas references for the column-profile and narrowing-cast kernels
(nvtabular_amd/csrc/nvt_profile.hip) and the operators on top of them, one operation at a time.
``null`` is a bool array (True = validity bit clear) or None, as in cont_reference.py."""
import math

import numpy as np

import cont_reference as R

INT64_MAX, INT64_MIN = 2**63 - 1, -(2**63)


def profile(x, null, sums=True):
    """dict(rows, valid, min, max, sum, sumsq) of one column: counts as ints; min / max over the rows
    that are neither null nor NaN -- exact Python ints for an integer column, floats (by VALUE:
    R.minmax) for a float column, None when no row is left; the sums correctly rounded (fsum).
    ``sums=False`` leaves the two sums None: data that holds +-inf has no correctly rounded sum."""
    x = np.asarray(x)
    m = R.null_rows(x, null)
    if sums:
        cnt, tot, sq = R.moments(x, null)
    else:
        cnt, tot, sq = int((~m).sum()), None, None
    if cnt == 0:
        lo = hi = None
    elif x.dtype.kind == "f":
        lo, hi = R.minmax(x, null)
    else:
        v = x[~m]
        lo, hi = int(v.min()), int(v.max())
    return dict(rows=int(x.size), valid=cnt, min=lo, max=hi, sum=tot, sumsq=sq)


def zero_signs(x, null):
    """(min is -0.0, max is +0.0) candidates of a float column: the kernel orders -0.0 below +0.0,
    so a zero minimum is -0.0 exactly when a -0.0 counts and a zero maximum is +0.0 exactly when a
    +0.0 counts -- wherever they sit.  (numpy's min / max return whichever zero they meet first.)"""
    x = np.asarray(x)
    v = x[~R.null_rows(x, null)]
    zeros = v[v == 0]
    return bool(np.signbit(zeros).any()), bool((~np.signbit(zeros)).any())


def float_bits(v):
    return np.array([v], dtype=np.float64).view(np.int64)[0]


def expected_float_extrema(x, null):
    """(min, max) of a float column as float64 with the zero signs the kernel's total order gives."""
    lo, hi = R.minmax(x, null)
    neg, pos = zero_signs(x, null)
    if lo == 0:
        lo = -0.0 if neg else 0.0
    if hi == 0:
        hi = 0.0 if pos else -0.0
    return lo, hi


def sum_bound(x, null):
    """The order-independent bounds of _check_moments_bound (test_gpu_cont_kernels.py):
    |err| <= n * 2**-53 * fsum(|terms|) for the sum and for the sum of squares."""
    v = R.moment_terms(x, null)
    u = v.size * 2.0**-53
    return u * math.fsum(np.abs(v).tolist()), u * math.fsum((v * v).tolist())


def merge_profiles(a, b):
    """Two profile dicts folded as the accumulators fold (counts added, extrema by min / max)."""
    def pick(f, p, q):
        return q if p is None else p if q is None else f(p, q)
    return dict(rows=a["rows"] + b["rows"], valid=a["valid"] + b["valid"],
                min=pick(min, a["min"], b["min"]), max=pick(max, a["max"], b["max"]),
                sum=a["sum"] + b["sum"], sumsq=a["sumsq"] + b["sumsq"])
