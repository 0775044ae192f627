"""Kernel-level matrix for the radix select (nvtabular_amd/csrc/nvt_select.hip), driven through
``kernels_select.select_median_many`` on torch tensors.

The reference for every value is numpy / pandas on the host: ``np.sort`` of the participating
values for ``lo`` and ``hi`` (ranks (m - 1) // 2 and m // 2) and
``pandas.Series(participating).quantile(0.5, interpolation="linear")`` for the median.  ``m``,
``lo``, ``hi`` and the median are compared with ``==`` (both NaN for an empty column): for floats
that is bit equality except for the sign of a zero, which ``np.sort`` does not order (-0.0 == +0.0)
-- the zero-sign case asserts on the KEYS instead.  Values are finite and |x| < 1e300, so the
interpolation cannot overflow; integer columns may wrap in ``hi - lo`` exactly as pandas does.

"Uniform random float64" of the candidate-path case means uniform over the finite bit patterns
below 1e300: the top digit of a float64 key is its sign and the upper exponent bits, so only data
spread over the exponents puts ~n / 2048 rows into a top-digit bin.  Uniform(0, 1) data has half
of its rows in the median's bin ([0.5, 2) is one bin) and takes the full passes; it is checked
too, for its values.
"""
import math

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

NP = {"int32": np.int32, "int64": np.int64, "float32": np.float32, "float64": np.float64}
SIZES = [0, 1, 2, 3, 63, 64, 65, 4097]


@pytest.fixture(scope="module")
def KS():
    from nvtabular_amd import kernels_select

    return kernels_select


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bitmap(mask):
    from nvtabular_amd.device import pack_bitmap

    return dev(pack_bitmap(np.asarray(mask, dtype=bool)))


def chunk(data, mask=None, fill=None):
    return (dev(data), None if mask is None else bitmap(mask), fill)


def random_values(dtype, n, rng):
    """Finite values over the whole range of the type (|x| < 1e300), both signs, repeats."""
    if dtype == "float64":
        a = rng.standard_normal(n) * 10.0 ** rng.integers(-200, 200, n)
    elif dtype == "float32":
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    elif dtype == "int32":
        a = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    else:
        a = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    a = a.astype(NP[dtype])
    if n > 8:   # some repeats, so that lo == hi happens too
        a[rng.integers(0, n, n // 4)] = a[0]
    return a


def participating(data, mask, fill):
    ok = np.ones(len(data), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    if data.dtype.kind == "f":
        ok &= ~np.isnan(data)
    if fill is not None:
        return np.where(ok, data, data.dtype.type(fill)).astype(data.dtype)
    return data[ok]


def reference(data, mask=None, fill=None):
    part = participating(data, mask, fill)
    m = len(part)
    if m == 0:
        return 0, None, None, float("nan")
    s = np.sort(part)
    med = pd.Series(part).dropna().quantile(0.5, interpolation="linear")
    return m, s[(m - 1) // 2], s[m // 2], float(med)


def check(got, ref, what=""):
    m, lo, hi, med = got
    rm, rlo, rhi, rmed = ref
    assert m == rm, (what, m, rm)
    if rm == 0:
        assert lo is None and hi is None and math.isnan(med), (what, got)
        return
    assert lo.dtype == rlo.dtype and hi.dtype == rhi.dtype, (what, lo.dtype, rlo.dtype)
    assert lo == rlo and hi == rhi, (what, lo, rlo, hi, rhi)
    assert isinstance(med, float) and med == rmed, (what, med, rmed, float.hex(med), float.hex(rmed))


def one(KS, data, mask=None, fill=None, **kw):
    return KS.select_median_many([[chunk(data, mask, fill)]], **kw)[0]


# ---- dtypes and shapes -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
@pytest.mark.parametrize("n", SIZES)
def test_every_dtype_and_size(KS, dtype, n):
    rng = np.random.default_rng(1000 + n)
    data = random_values(dtype, n, rng)
    check(one(KS, data), reference(data), f"{dtype} n={n}")


# ---- nulls, NaN, pending fill ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
@pytest.mark.parametrize("n", [3, 65, 4097])
def test_bitmap_with_nulls(KS, dtype, n):
    rng = np.random.default_rng(2000 + n)
    data = random_values(dtype, n, rng)
    mask = rng.random(n) >= 0.3
    got = one(KS, data, mask)
    check(got, reference(data, mask), f"{dtype} n={n}")
    assert got.m == int(mask.sum())


@pytest.mark.parametrize("dtype", list(NP))
@pytest.mark.parametrize("n", [1, 64, 4097])
def test_all_rows_null(KS, dtype, n):
    data = random_values(dtype, n, np.random.default_rng(3))
    got = one(KS, data, np.zeros(n, dtype=bool))
    assert got.m == 0 and got.lo is None and got.hi is None and math.isnan(got.median)
    assert got.path == KS.PATH_NONE


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("with_bitmap", [False, True])
def test_nan_rows_do_not_count(KS, dtype, with_bitmap):
    rng = np.random.default_rng(4)
    n = 4097
    data = random_values(dtype, n, rng)
    data[rng.random(n) < 0.25] = np.nan
    mask = (rng.random(n) >= 0.3) if with_bitmap else None   # NaN under set bits among them
    got = one(KS, data, mask)
    check(got, reference(data, mask), dtype)
    assert got.m < n
    # only NaN: nothing takes part
    allnan = np.full(65, np.nan, dtype=NP[dtype])
    assert one(KS, allnan).m == 0 and math.isnan(one(KS, allnan).median)


@pytest.mark.parametrize("dtype", list(NP))
@pytest.mark.parametrize("n", [2, 65, 4097])
def test_pending_fill_counts_for_the_null_rows(KS, dtype, n):
    rng = np.random.default_rng(5000 + n)
    data = random_values(dtype, n, rng)
    mask = rng.random(n) >= 0.3
    fill = -7 if dtype.startswith("int") else 0.5
    if dtype.startswith("float"):
        data[rng.random(n) < 0.1] = np.nan     # NaN rows are filled too
    got = one(KS, data, mask, fill)
    check(got, reference(data, mask, fill), f"{dtype} n={n}")
    assert got.m == n
    # more than half of the rows null: the fill constant IS the median
    mostly = rng.random(n) >= 0.8
    mostly[:1] = False
    got = one(KS, data, mostly, fill)
    check(got, reference(data, mostly, fill), f"{dtype} n={n} mostly null")


@pytest.mark.parametrize("dtype", ["float32", "float64", "int64"])
def test_nan_fill_constant_fills_nothing(KS, dtype):
    """A pending fill of NaN leaves the null rows null: they do not take part (pandas' dropna drops
    them after such a fillna)."""
    rng = np.random.default_rng(7)
    data = random_values(dtype, 1001, rng)
    mask = rng.random(1001) >= 0.3
    got = one(KS, data, mask, float("nan"))
    check(got, reference(data, mask), dtype)
    assert got.m == int(mask.sum())


def test_fractional_fill_of_an_integer_column(KS):
    """An integer column whose pending fill is not an integer takes part as the float64 column the
    fill makes of it."""
    rng = np.random.default_rng(6)
    data = rng.integers(-50, 50, 1001).astype(np.int64)
    mask = rng.random(1001) >= 0.6
    got = one(KS, data, mask, 0.5)
    ref = reference(np.where(mask, data.astype(np.float64), 0.5))
    check(got, ref)


# ---- key order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_negative_and_positive_zero_are_neighbouring_keys(KS, dtype):
    t = NP[dtype]
    data = np.array([3.0, -0.0, -2.0, 0.0], dtype=t)
    got = one(KS, data)
    assert got.m == 4
    k_neg, k_pos = KS.key_of(t(-0.0), t), KS.key_of(t(0.0), t)
    assert k_neg + 1 == k_pos
    assert got.key_lo == k_neg and got.key_hi == k_pos
    assert np.signbit(got.lo) and not np.signbit(got.hi) and got.lo == 0 and got.hi == 0
    assert got.median == 0.0
    # ... and the whole order around them: ranks 0 .. 5 of [-inf side .. +inf side]
    order = np.array([-5.0, -np.finfo(t).tiny, -0.0, 0.0, np.finfo(t).tiny, 5.0], dtype=t)
    keys = [KS.key_of(v, t) for v in order]
    assert keys == sorted(keys) and len(set(keys)) == 6
    for v in order:
        assert KS.value_of(KS.key_of(v, t), t).tobytes() == v.tobytes()


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_int_min_and_int_max(KS, dtype):
    t = NP[dtype]
    info = np.iinfo(t)
    for vals in ([info.min, info.max], [info.min, info.min, info.max], [info.max, info.min, info.max, info.min],
                 [info.min], [info.max], [info.min, -1, 0, info.max], [info.max, 0, info.min]):
        data = np.array(vals, dtype=t)
        with np.errstate(over="ignore"):
            ref = reference(data)
        check(one(KS, data), ref, f"{dtype} {vals}")
    assert KS.key_of(info.min, t) == 0 and KS.key_of(info.max, t) == 2 ** (8 * t().itemsize) - 1


def test_float64_lowest_mantissa_bit_decides_on_the_last_pass(KS):
    a = np.float64(1.5)
    b = np.nextafter(a, 2.0)
    assert KS.key_of(b, np.float64) - KS.key_of(a, np.float64) == 1
    for na, nb in ((2, 2), (3, 4), (4, 3), (1, 1), (500, 501), (501, 500), (700, 700)):
        data = np.array([a] * na + [b] * nb)
        np.random.default_rng(na).shuffle(data)
        got = one(KS, data)
        check(got, reference(data), f"{na} x a, {nb} x b")
    got = one(KS, np.array([b, a, b, a]))
    assert got.lo == a and got.hi == b and got.key_hi - got.key_lo == 1


def test_int64_top_bits_decide_on_pass_0(KS):
    rng = np.random.default_rng(8)
    low = np.int64(0x0012_3456_789A_BCDE) & np.int64((1 << 53) - 1)
    top = rng.integers(-1024, 1024, 4097).astype(np.int64)      # the top 11 bits, signed
    data = (top << np.int64(53)) | low
    assert len(np.unique(data >> np.int64(53))) > 1000
    with np.errstate(over="ignore"):
        check(one(KS, data), reference(data))
        check(one(KS, data[:64]), reference(data[:64]))


# ---- the two ranks in different bins -------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
def test_ranks_straddle_a_top_digit_boundary(KS, dtype):
    t = NP[dtype]
    data = np.array([-1, 1], dtype=t)
    got = one(KS, data)
    check(got, reference(data))
    assert got.median == 0.0
    # different top digits: the prefixes part on pass 0
    top = 8 * t().itemsize - 11
    assert got.key_lo >> top != got.key_hi >> top
    rng = np.random.default_rng(9)
    vals = random_values(dtype, 2048, rng)
    if dtype.startswith("int"):
        vals = vals >> t(2)      # (room for the negation and the - 1)
    neg = -np.abs(vals) - t(1)
    data = np.concatenate([neg, -neg]).astype(t)      # 2048 below zero, 2048 above: ranks 2047 | 2048
    rng.shuffle(data)
    got = one(KS, data)
    check(got, reference(data))
    assert got.lo < 0 < got.hi


# ---- the two paths ---------------------------------------------------------------------------------
def uniform_bits_float64(n, rng):
    out = np.empty(0)
    while len(out) < n:
        a = rng.integers(0, 2**64, 2 * n, dtype=np.uint64).view(np.float64)
        out = np.concatenate([out, a[np.isfinite(a) & (np.abs(a) < 1e300)]])
    return out[:n]


@pytest.fixture(scope="module")
def big_uniform():
    data = uniform_bits_float64(200_000, np.random.default_rng(10))
    return data, reference(data)


def test_candidate_path(KS, big_uniform):
    data, ref = big_uniform
    got = one(KS, data)
    check(got, ref)
    assert got.path == KS.PATH_CAND
    # the same column with the candidate path switched off: all the full passes, the same result
    full = one(KS, data, allow_candidates=False)
    check(full, ref)
    assert full.path == KS.PATH_FULL


@pytest.mark.parametrize("dtype", ["float64", "int32"])
def test_full_pass_path(KS, dtype):
    rng = np.random.default_rng(11)
    n = 200_000
    if dtype == "float64":
        data = rng.uniform(-1e6, 1e6, n)
    else:
        data = rng.integers(-1000, 100_000, n).astype(np.int32)
    data[rng.permutation(n)[: n * 6 // 10]] = 0     # 120 000 equal rows: above the candidate cap
    got = one(KS, data)
    check(got, reference(data))
    assert got.path == KS.PATH_FULL
    assert got.lo == 0 and got.hi == 0


def test_uniform_unit_interval(KS):
    data = np.random.default_rng(12).uniform(0.0, 1.0, 200_000)
    got = one(KS, data)
    check(got, reference(data))
    print("uniform(0, 1), 200 000 rows: path", got.path)


def test_candidate_path_with_ranks_in_two_bins(KS):
    """lo and hi in different top-digit bins, both small: the candidates of both bins are gathered."""
    rng = np.random.default_rng(13)
    neg = -np.abs(uniform_bits_float64(50_000, rng))
    pos = np.abs(uniform_bits_float64(50_000, rng))
    data = np.concatenate([neg, pos])
    rng.shuffle(data)
    got = one(KS, data)
    check(got, reference(data))
    assert got.path == KS.PATH_CAND and got.lo < 0 < got.hi


# ---- chunks and batches -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
def test_three_unequal_chunks_one_empty(KS, dtype):
    rng = np.random.default_rng(14)
    data = random_values(dtype, 5000, rng)
    mask = rng.random(5000) >= 0.3
    cuts = [(0, 1237), (1237, 1237), (1237, 5000)]
    # (bitmaps start at bit 0 of every chunk: they are cut from the row masks, not from the bytes)
    chunks = [chunk(data[a:b], mask[a:b]) for a, b in cuts]
    got = KS.select_median_many([chunks])[0]
    check(got, reference(data, mask))
    # chunks with and without a bitmap, in another order
    chunks = [chunk(data[1237:]), chunk(data[:0]), chunk(data[:1237], mask[:1237])]
    full_mask = np.concatenate([np.ones(5000 - 1237, dtype=bool), mask[:1237]])
    check(KS.select_median_many([chunks])[0], reference(np.concatenate([data[1237:], data[:1237]]), full_mask))


def test_mixed_batch_equals_single_calls(KS, big_uniform):
    rng = np.random.default_rng(15)
    cols = []
    for dtype, n in (("float32", 4097), ("int64", 63), ("float64", 30_001), ("int32", 1), ("int64", 0)):
        data = random_values(dtype, n, rng)
        mask = rng.random(n) >= 0.3 if n > 1 else None
        cols.append((data, mask, None))
    cols[2] = (np.concatenate([big_uniform[0][:30_000], [np.nan]]), None, 0.25)
    together = KS.select_median_many([[chunk(*c)] for c in cols])
    assert len(together) == 5
    for c, got in zip(cols, together):
        alone = one(KS, *c)
        check(got, reference(*c))
        assert tuple(alone)[:1] == tuple(got)[:1] and alone.key_lo == got.key_lo and alone.key_hi == got.key_hi
        assert alone.path == got.path
    assert together[4].m == 0 and together[3].m == 1
    # more columns than one launch takes (NVT_SELECT_MAX_COLS = 32)
    many = [random_values("int32", 100 + i, rng) for i in range(35)]
    for data, got in zip(many, KS.select_median_many([[chunk(d)] for d in many])):
        check(got, reference(data))
    assert KS.select_median_many([]) == []
    assert KS.select_median_many([[]])[0].m == 0
