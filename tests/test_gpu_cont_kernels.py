"""Kernel-level matrix for the continuous-column kernels (nvtabular_amd/csrc/nvt_cont.hip) and
the hash-bucket kernel: the ``K.*`` wrappers called directly on torch tensors, every element
compared with the plain references of cont_reference.py (which test_cont_reference.py pins to the
pandas oracle on the CPU).

What "equal" means: bit for bit (NaN positions compared separately, the sign of a zero
included), except where a comment derives a bound: the moments of general float data, float32
log, and the target-encoding formula.

Excluded, by name:
* moments of +-inf / +-max data: the sums are inf or NaN depending on the summation order, in
  any implementation; the moments data holds finite values below 1e30 (denormals included).
* the SIGN of a zero minimum / maximum: -0.0 == +0.0, and which of the two a parallel reduction
  keeps depends on its order; min / max are compared by value and by NaN-ness.
* gather into an integer output is given finite in-range sources only: converting NaN or an
  out-of-range double to an integer is undefined in C.
"""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import cont_reference as R
import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
         100_003]

# One size per code shape that needs a SECOND trip of the grid-stride loop and then ends inside
# a partial unrolled block and a scalar tail.  stream_grid(work, per_block, blocks_per_cu) caps a
# grid at 256 CUs * blocks_per_cu blocks of kBlock = 256 threads (4 waves of 64).
# widen_stream (4-byte in, 8-byte out): stream_grid(.., .., 8) = 2048 blocks * 4 waves, a wave
# takes U = 4 runs of 128 elements per trip -> 2048 * 4 * 4 * 128 = 4 194 304 elements a trip.
# One more run (the first of an unrolled group of 4) and 3 tail elements:
BIG_WIDEN = 4_194_304 + 128 + 3
# 16-byte vector path, VEC = 4 (4-byte in, 4-byte out): 2048 blocks * 256 lanes * 4 elements =
# 2 097 152 a trip; 5 more vectors and a 3-element tail:
BIG_VEC4 = 2_097_152 + 4 * 5 + 3
# the same with VEC = 2 (8-byte in): 2048 * 256 * 2 = 1 048 576 a trip; 5 vectors and 1 element:
BIG_VEC2 = 1_048_576 + 2 * 5 + 1
# moments: stream_grid(.., .., 4) = 1024 blocks; a lane takes U = 4 vectors a trip, one grid
# stride (1024 * 256 vectors) apart -> 1024 * 256 * 4 * VEC elements a trip.  The second trip gets
# one full slot (1024 * 256 vectors), 7 vectors of the second slot, and a tail:
BIG_MOM4 = 1024 * 256 * 4 * 4 + 1024 * 256 * 4 + 4 * 7 + 3
BIG_MOM8 = 1024 * 256 * 4 * 2 + 1024 * 256 * 2 + 2 * 7 + 1
# min / max: 1024 blocks * 256 lanes * VEC = 4 (float32), no unrolling; 5 vectors and a tail:
BIG_MINMAX = 1024 * 256 * 4 + 4 * 5 + 3
# bucketize: stream_grid(n, 1024, 8) = 2048 blocks * 256 lanes, one element each:
BIG_BUCKET = 2048 * 256 + 77
# popcount: stream_grid(n / 8 + 1, 4096) = 2048 blocks * 256 lanes, one BYTE each; 5 more bytes
# and a 3-bit tail:
BIG_POPCOUNT = 8 * (2048 * 256 + 5) + 3

NP = {"float32": np.float32, "float64": np.float64, "int32": np.int32, "int64": np.int64}
TT = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "int64": torch.int64}
TS_NS = 1_700_000_000_123_456_789


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def edges(dtype):
    if dtype in ("float32", "float64"):
        f = np.finfo(NP[dtype])
        return np.array([0.0, -0.0, np.inf, -np.inf, f.smallest_subnormal, -f.smallest_subnormal, f.tiny,
                         f.max, -f.max, np.nan, 1.0, -1.0, 0.5, -2.0, 3.0], dtype=NP[dtype])
    i = np.iinfo(NP[dtype])
    e = [0, 1, -1, i.min, i.max, 2**31 - 1, -(2**31), 7, -300]
    if dtype == "int64":
        e += [2**53 + 1, -(2**53 + 1), TS_NS, 2**53, 2**62 + 1]
    return np.array(e, dtype=NP[dtype])


def values(dtype, n, rng, finite=False):
    """Random data with the edge values at the front, at the end and at random rows."""
    if dtype.startswith("float"):
        x = (rng.normal(size=n) * 50).astype(NP[dtype])
    else:
        x = rng.integers(-300, 300, n).astype(NP[dtype])
    e = edges(dtype)
    if finite:
        e = e[np.isfinite(e.astype(np.float64)) & (np.abs(e.astype(np.float64)) < 1e30)]
    if n:
        k = min(n, e.size)
        x[:k] = e[:k]
        x[n - k:] = e[e.size - k:]
        pos = rng.integers(0, n, min(n, 4 * e.size))
        x[pos] = e[rng.integers(0, e.size, pos.size)]
    return x


def patterns(n, rng):
    """(name, null mask or None).  None = no bitmap is passed at all."""
    out = [("no-bitmap", None), ("all-valid", np.zeros(n, bool)), ("all-null", np.ones(n, bool)),
           ("random30", rng.random(n) < 0.3), ("alternating", np.arange(n) % 2 == 1)]
    first = np.zeros(n, bool)
    first[:1] = True
    last = np.zeros(n, bool)
    last[n - 1:] = True
    return out + [("row0-null", first), ("last-null", last)]


def garbage(x, null, rng):
    """Arbitrary bytes in the slot under a null: NaN and huge values."""
    x = x.copy()
    if null is None or not null.any():
        return x
    idx = np.flatnonzero(null)
    if x.dtype.kind == "f":
        x[idx[0::2]] = np.nan
        x[idx[1::2]] = np.finfo(x.dtype).max
    else:
        x[idx[0::2]] = np.iinfo(x.dtype).max
        x[idx[1::2]] = np.iinfo(x.dtype).min
    return x


def bitmap(null):
    return None if null is None else dev(R.pack_bits(~null))


def cases(dtype, seed, sizes=SIZES, finite=False):
    """Every size x every validity pattern: (label, values, null, device values, device bitmap)."""
    rng = np.random.default_rng(seed)
    for n in sizes:
        base = values(dtype, n, rng, finite)
        for name, null in patterns(n, rng):
            x = garbage(base, null, rng)
            yield f"{dtype} n={n} {name}", x, null, dev(x), bitmap(null)


# ---------------------------------------------------------------------------------------------
# fill / fill + normalize
# ---------------------------------------------------------------------------------------------
FN_PAIRS = [(i, o) for o in ("float64", "float32") for i in ("float32", "float64", "int32", "int64")] + [
    ("int32", "int32"), ("int64", "int64")]
# (fill, do_norm, shift, scale); scale 0 = subtract only
FN_MODES_FILL = [(None, False, 0.0, 1.0), (7, False, 0.0, 1.0), (-3, False, 0.0, 1.0)]
FN_MODES_NORM = [(None, True, 1.25, 2.5), (0.5, True, -3.0, 0.1), (0, True, 0.75, 0.0)]


def _check_fill_norm(K, label, x, null, dx, dv, mode, out_dtype):
    fill, do_norm, shift, scale = mode
    got, filled = K.fill_normalize(dx, dv, fill, do_norm, shift, scale, TT[out_dtype], want_filled_mask=True)
    exp, exp_filled = R.fill_normalize(x, null, fill, do_norm, shift, scale, NP[out_dtype])
    what = f"{label} -> {out_dtype} mode={mode}"
    R.assert_bits_equal(host(filled).astype(np.uint8), exp_filled, what + " filled")
    R.assert_bits_equal(host(got), exp, what)


@pytest.mark.parametrize("pair", FN_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_fill_normalize(K, pair):
    """float64 arithmetic is two separately rounded IEEE operations (no contraction is possible
    between a subtraction and a division), float32 input the same in float32: bit-exact."""
    i, o = pair
    modes = FN_MODES_FILL + (FN_MODES_NORM if o.startswith("float") else [])
    for label, x, null, dx, dv in cases(i, 101):
        for mode in modes:
            _check_fill_norm(K, label, x, null, dx, dv, mode, o)
    # without the mask the values are the same
    x = values(i, 1000, np.random.default_rng(1))
    got, none = K.fill_normalize(dev(x), None, 7, False, 0.0, 1.0, TT[o])
    assert none is None
    R.assert_bits_equal(host(got), R.fill_normalize(x, None, 7, False, 0.0, 1.0, NP[o])[0])


@pytest.mark.parametrize("pair,n", [(("float32", "float64"), BIG_WIDEN), (("int32", "float32"), BIG_VEC4),
                                    (("float64", "float64"), BIG_VEC2)], ids=["widen", "vec4", "vec2"])
def test_fill_normalize_second_grid_trip(K, pair, n):
    i, o = pair
    rng = np.random.default_rng(7)
    x = values(i, n, rng)
    null = rng.random(n) < 0.3
    x = garbage(x, null, rng)
    _check_fill_norm(K, f"{i} n={n} random30", x, null, dev(x), bitmap(null), (0.5, True, 1.25, 2.5), o)


def test_fill_normalize_rejects(K):
    from nvtabular_amd._lib import NvtHipError

    x = dev(np.arange(64, dtype=np.int32))
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.fill_normalize(x, None, 0, False, 0.0, 1.0, torch.int64)          # int32 -> int64
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.fill_normalize(x, None, 0, True, 0.0, 1.0, torch.int32)           # normalised integers
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.fill_normalize(x.to(torch.uint8), None, 0, False, 0.0, 1.0, torch.float64)
    with pytest.raises(TypeError, match="float16"):
        K.fill_normalize(x.to(torch.float16), None, 0, False, 0.0, 1.0, torch.float64)
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.fill_normalize_many([(x.to(torch.float32), None, 0, False, 0.0, 1.0, torch.int32, False)])
    with pytest.raises(NvtHipError, match="normalised output"):
        K.fill_normalize_many([(x, None, 0, True, 0.0, 1.0, torch.int32, False)])
    # an integer fill constant travels as a double: it must be an integer the column type holds
    # and at most 2**53 in magnitude
    x64 = x.to(torch.int64)
    for bad in (2**53 + 1, -(2**53) - 1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="fill"):
            K.fill_normalize(x64, None, bad, False, 0.0, 1.0, torch.int64)
        with pytest.raises(ValueError, match="fill"):
            K.fill_normalize_many([(x64, None, bad, False, 0.0, 1.0, torch.int64, False)])
    with pytest.raises(ValueError, match="fill"):
        K.fill_normalize(x, None, 2**31, False, 0.0, 1.0, torch.int32)
    for ok in (2**53, -(2**53)):
        null = np.arange(64) % 2 == 0
        got, _ = K.fill_normalize(x64, bitmap(null), ok, False, 0.0, 1.0, torch.int64)
        R.assert_bits_equal(host(got), R.fill_normalize(host(x64), null, ok, False, 0.0, 1.0, np.int64)[0])


# ---------------------------------------------------------------------------------------------
# clip / log
# ---------------------------------------------------------------------------------------------
CL_PAIRS = FN_PAIRS[:8] + [("int32", "int32"), ("int64", "int64")]
# (fill, min, max): min only, max only, both, bounds no value reaches, fill outside the bounds
CLIP_MODES = [(None, 0, None), (None, None, 3), (None, -2, 3), (0, -2, 3), (50, -2, 3), (-50, 0, None)]


def _unreached(dtype):
    if dtype == "int32":
        return (None, -(2**31), 2**31 - 1)
    if dtype == "int64":
        return (None, -(2**53), 2**53)     # the largest an integer clip takes: only |x| > 2**53 is reached
    return (None, -np.inf, np.inf)


def _check_clip(K, label, x, null, dx, dv, mode, out_dtype):
    fill, lo, hi = mode
    got = K.clip_log(dx, dv, fill, lo, hi, False, TT[out_dtype])
    exp = R.clip(x, null, fill, lo, hi, NP[out_dtype])
    R.assert_bits_equal(host(got), exp, f"clip {label} -> {out_dtype} mode={mode}")


def _check_log(K, label, x, null, dx, dv, mode, out_dtype):
    fill, lo, hi = mode
    got = host(K.clip_log(dx, dv, fill, lo, hi, True, TT[out_dtype]))
    assert got.dtype == NP[out_dtype]
    arg = R.log_argument(x, null, fill, lo, hi)
    exp = R.log1p_f32(x, null, fill, lo, hi)
    what = f"log {label} -> {out_dtype} mode={mode}"
    # exact at the special points: log(1) = 0, log(0) = -inf, log(< 0) = NaN, log(inf) = inf,
    # missing = NaN
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=what)
    for point, val in ((arg == 1, 0.0), (arg == 0, -np.inf), (arg == np.inf, np.inf)):
        assert (got[point] == val).all(), what
    fin = np.isfinite(exp)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=what)
    # the project's float32 log bound (test_gpu_parity.test_fill_clip_log_vs_oracle) against the
    # float64 logarithm of the float32 argument
    np.testing.assert_allclose(got[fin].astype(np.float64), exp[fin], rtol=2e-6, atol=1e-7, err_msg=what)


@pytest.mark.parametrize("pair", CL_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_clip(K, pair):
    i, o = pair
    for label, x, null, dx, dv in cases(i, 202):
        for mode in CLIP_MODES + [_unreached(i)]:
            _check_clip(K, label, x, null, dx, dv, mode, o)


@pytest.mark.parametrize("pair", CL_PAIRS[:8], ids=lambda p: f"{p[0]}-{p[1]}")
def test_log(K, pair):
    i, o = pair
    for label, x, null, dx, dv in cases(i, 303):
        for mode in [(None, None, None), (0, 0, None), (None, -2, 3)]:
            _check_log(K, label, x, null, dx, dv, mode, o)


def test_clip_int64_values_beyond_2_53_pass_through(K):
    """Clip(min_value=0) on int64: values inside the bounds are not touched (clip.py:49-55)."""
    x = np.array([2**53 + 1, TS_NS, 2**63 - 1, -5, -(2**63), 2**62 + 1, -(2**53) - 1], dtype=np.int64)
    exp = O.clip_transform(pd.DataFrame({"x": x}), ["x"], min_value=0)["x"].to_numpy()
    got = host(K.clip_log(dev(x), None, None, 0, None, False, torch.int64))
    R.assert_bits_equal(got, exp, "Clip(min_value=0) on int64")
    exp = O.clip_transform(pd.DataFrame({"x": x}), ["x"], max_value=10)["x"].to_numpy()
    R.assert_bits_equal(host(K.clip_log(dev(x), None, None, None, 10, False, torch.int64)), exp)
    # INT32_MIN / MAX survive an int32 clip whose bounds are the type's own limits
    x32 = edges("int32")
    got = host(K.clip_log(dev(x32), None, None, -(2**31), 2**31 - 1, False, torch.int32))
    R.assert_bits_equal(got, x32)


@pytest.mark.parametrize("pair,n", [(("int32", "float64"), BIG_WIDEN), (("int32", "int32"), BIG_VEC4),
                                    (("int64", "int64"), BIG_VEC2)], ids=["widen", "vec4", "vec2"])
def test_clip_second_grid_trip(K, pair, n):
    i, o = pair
    rng = np.random.default_rng(8)
    x = values(i, n, rng)
    null = rng.random(n) < 0.3
    x = garbage(x, null, rng)
    _check_clip(K, f"{i} n={n} random30", x, null, dev(x), bitmap(null), (5, -2, 3), o)


def test_clip_log_rejects(K):
    from nvtabular_amd._lib import NvtHipError

    x = dev(np.arange(64, dtype=np.int32))
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.clip_log(x, None, None, 0, None, False, torch.int64)
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.clip_log(x, None, None, 0, None, True, torch.int32)               # log into integers
    with pytest.raises(NvtHipError, match="unsupported dtype combination"):
        K.clip_log(x.to(torch.uint8), None, None, 0, None, False, torch.float64)
    with pytest.raises(TypeError, match="float16"):
        K.clip_log(x, None, None, 0, None, False, torch.float16)
    # integer clip: a bound or fill the column type cannot take exactly is refused, not rounded
    x64 = x.to(torch.int64)
    for bad in (2**53 + 1, -(2**53) - 1, 0.5, float("nan")):
        with pytest.raises(ValueError, match="min_value"):
            K.clip_log(x64, None, None, bad, None, False, torch.int64)
        with pytest.raises(ValueError, match="max_value"):
            K.clip_log(x64, None, None, None, bad, False, torch.int64)
        with pytest.raises(ValueError, match="fill"):
            K.clip_log(x64, None, bad, 0, None, False, torch.int64)
    # a bound every value of the type is beyond cannot be stored in the type ...
    with pytest.raises(ValueError, match="min_value"):
        K.clip_log(x, None, None, 2**31, None, False, torch.int32)
    with pytest.raises(ValueError, match="max_value"):
        K.clip_log(x, None, None, None, -(2**31) - 1, False, torch.int32)
    with pytest.raises(ValueError, match="min_value"):
        K.clip_log(x64, None, None, float("inf"), None, False, torch.int64)
    with pytest.raises(ValueError, match="fill"):
        K.clip_log(x, None, 2**31, 0, None, False, torch.int32)
    # ... one at or beyond the end of the type clips nothing, as in the reference (clip.py:49-55)
    e32, e64 = edges("int32"), edges("int64")
    for lo, hi in ((-(2**31), 2**31 - 1), (-(2**53), 2**53), (float("-inf"), float("inf")), (None, 1e10)):
        R.assert_bits_equal(host(K.clip_log(dev(e32), None, None, lo, hi, False, torch.int32)), e32)
    for lo, hi in ((-(2**63), 2**63 - 1), (float("-inf"), float("inf")), (-(2**70), 2**70)):
        R.assert_bits_equal(host(K.clip_log(dev(e64), None, None, lo, hi, False, torch.int64)), e64)
    # the same bounds are fine for a float64 output
    got = host(K.clip_log(x64, None, None, 0.5, 2**53 + 1, False, torch.float64))
    R.assert_bits_equal(got, R.clip(host(x64), None, None, 0.5, 2**53 + 1, np.float64))


# ---------------------------------------------------------------------------------------------
# moments, min / max
# ---------------------------------------------------------------------------------------------
def _int_valued(dtype, n, rng):
    """Integer-valued data, |x| < 2**20 and small enough that n * x**2 < 2**53: every partial sum
    is exact in float64, so count, sum and sum of squares are exact whatever the order."""
    mag = int(min(2**20, math.isqrt(2**53 // max(n, 1)))) - 1
    return rng.integers(-mag, mag + 1, n).astype(NP[dtype])


def _moments(K, dx, dv, fill, start=None):
    out3 = torch.zeros(3, dtype=torch.float64, device="cuda") if start is None else start
    K.moments_accumulate(dx, dv, out3, fill)
    return out3


def _check_moments_exact(K, label, x, null, fill):
    dx, dv = dev(x), bitmap(null)
    out3 = _moments(K, dx, dv, fill)
    cnt, tot, sq = R.moments(x, null, fill)
    R.assert_bits_equal(host(out3), np.array([cnt, tot, sq], dtype=np.float64), f"moments {label} fill={fill}")
    # out3 += : a second pass doubles every exact sum
    got2 = host(_moments(K, dx, dv, fill, out3))
    if 2 * sq < 2.0**53:
        R.assert_bits_equal(got2, np.array([2 * cnt, 2 * tot, 2 * sq], dtype=np.float64), f"moments += {label}")


def _check_moments_bound(K, label, x, null, fill):
    got = host(_moments(K, dev(x), bitmap(null), fill))
    cnt, tot, sq = R.moments(x, null, fill)
    v = R.moment_terms(x, null, fill)
    assert got[0] == cnt, label
    # the textbook bound for summing n terms in ANY order: (n - 1) additions of relative error
    # 2**-53 each, plus the rounding of the product (the square) -> n * 2**-53 * sum(|terms|)
    u = cnt * 2.0**-53
    assert abs(got[1] - tot) <= u * math.fsum(np.abs(v).tolist()), (label, got[1], tot)
    assert abs(got[2] - sq) <= u * math.fsum((v * v).tolist()), (label, got[2], sq)


@pytest.mark.parametrize("dtype", list(NP))
def test_moments(K, dtype):
    rng = np.random.default_rng(404)
    for n in SIZES:
        xi = _int_valued(dtype, n, rng)
        xg = values(dtype, n, rng, finite=True)
        if dtype == "int64":
            xg = np.where(np.abs(xg.astype(np.float64)) > 2.0**40, xg >> 24, xg)   # keep x**2 finite and summable
        for name, null in patterns(n, rng):
            for fill in (None, 3.0):
                xa = garbage(xi, null, rng)
                if dtype.startswith("float") and n > 5:
                    xa[5] = np.nan                      # NaN under a set validity bit
                _check_moments_exact(K, f"{dtype} n={n} {name}", xa, null, fill)
                _check_moments_bound(K, f"{dtype} n={n} {name}", garbage(xg, null, rng), null, fill)


@pytest.mark.parametrize("dtype,n", [("float32", BIG_MOM4), ("int64", BIG_MOM8)], ids=["4-byte", "8-byte"])
def test_moments_second_grid_trip(K, dtype, n):
    rng = np.random.default_rng(9)
    x = _int_valued(dtype, n, rng)
    null = rng.random(n) < 0.3
    _check_moments_exact(K, f"{dtype} n={n} random30", garbage(x, null, rng), null, None)
    _check_moments_exact(K, f"{dtype} n={n} random30", garbage(x, null, rng), null, 3.0)


def _check_minmax(K, label, x, null, prev, dx=None, dv=None):
    out2 = torch.tensor([7.0, -7.0] if prev is None else list(prev), dtype=torch.float64, device="cuda")
    dx, dv = (dev(x), bitmap(null)) if dx is None else (dx, dv)
    K.minmax_accumulate(dx, dv, out2, first=prev is None)
    got, exp = host(out2), np.array(R.minmax(x, null, prev))
    if x.size == 0:
        exp = np.array([7.0, -7.0] if prev is None else list(prev))   # n == 0 leaves out2 alone
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=label)
    np.testing.assert_array_equal(got, exp, err_msg=label)   # by value: see "Excluded" above


@pytest.mark.parametrize("dtype", list(NP))
def test_minmax(K, dtype):
    rng = np.random.default_rng(505)
    nan = float("nan")
    for n in SIZES:
        base = values(dtype, n, rng)
        plain = (rng.normal(size=n) * 50).astype(NP[dtype])       # the edges do not hide the data
        for name, null in patterns(n, rng):
            for x in (garbage(base, null, rng), garbage(plain, null, rng)):
                dx, dv = dev(x), bitmap(null)
                for prev in (None, (nan, nan), (-1e300, 1e300), (1e300, -1e300), (nan, 5.0)):
                    _check_minmax(K, f"minmax {dtype} n={n} {name} prev={prev}", x, null, prev, dx, dv)
    # the extreme value in EVERY position of a block-sized column: each lane and wave is heard
    for pos in list(range(0, 1024, 37)) + [1023]:
        x = np.zeros(1024, dtype=NP[dtype])
        x[pos] = 9
        x[1023 - pos] = -9 if pos != 1023 - pos else 9
        _check_minmax(K, f"minmax {dtype} peak at {pos}", x, None, None)


def test_minmax_second_grid_trip(K):
    rng = np.random.default_rng(10)
    x = (rng.normal(size=BIG_MINMAX) * 50).astype(np.float32)
    x[-2], x[-9] = 1e6, -1e6                      # the extremes sit in the tail / the last vectors
    null = rng.random(BIG_MINMAX) < 0.3
    null[-2] = null[-9] = False
    _check_minmax(K, "minmax big", garbage(x, null, rng), null, None)


def test_moments_minmax_reject(K):
    from nvtabular_amd._lib import NvtHipError

    out3 = torch.zeros(3, dtype=torch.float64, device="cuda")
    x16 = torch.zeros(64, dtype=torch.float16, device="cuda")
    with pytest.raises(TypeError, match="float16"):
        K.moments_accumulate(x16, None, out3)
    with pytest.raises(TypeError, match="float16"):
        K.moments_many([(x16, None, None, out3)])
    with pytest.raises(TypeError, match="float16"):
        K.minmax_accumulate(x16, None, out3[:2], first=True)
    with pytest.raises(NvtHipError, match="unsupported dtype"):
        K.minmax_accumulate(torch.zeros(64, dtype=torch.uint8, device="cuda"), None, out3[:2], first=True)
    assert host(out3).tolist() == [0.0, 0.0, 0.0]
    # a bool column is counted as 0 / 1 (widened first)
    b = np.arange(100) % 3 == 0
    K.moments_accumulate(dev(b), None, out3)
    assert host(out3).tolist() == [100.0, float(b.sum()), float(b.sum())]


# ---------------------------------------------------------------------------------------------
# the batched forms
# ---------------------------------------------------------------------------------------------
MANY_LENGTHS = [100_003, 1, 513, 0, 4097, 30_011, 129, 70_001]


def _many_columns(ncols, rng):
    """Columns of mixed dtypes and lengths, a zero-length column in the middle."""
    cols = []
    for c in range(ncols):
        dtype = list(NP)[c % 4]
        n = MANY_LENGTHS[c % len(MANY_LENGTHS)] if c != ncols // 2 else 0
        if ncols == 1:
            n = 30_011
        x = values(dtype, n, rng, finite=True)
        null = None if c % 3 == 0 else rng.random(n) < 0.3
        cols.append((dtype, garbage(x, null, rng), null, None if c % 2 else 1.5))
    return cols


@pytest.mark.parametrize("ncols", [1, 32, 33, 40])
def test_moments_many_bit_identical_to_single(K, ncols):
    """nvt_cont.hip: a batched column keeps the grid and the block-to-row mapping of the
    single-column kernel, "so the partial sums -- and therefore the results -- are bit-identical"."""
    cols = _many_columns(ncols, np.random.default_rng(606 + ncols))
    acc = torch.zeros(ncols, 3, dtype=torch.float64, device="cuda")
    items, single = [], []
    for c, (dtype, x, null, fill) in enumerate(cols):
        dx, dv = dev(x), bitmap(null)
        items.append((dx, dv, fill, acc[c]))
        single.append(host(_moments(K, dx, dv, fill)))
    K.moments_many(items)
    got = host(acc)
    for c, (dtype, x, null, fill) in enumerate(cols):
        R.assert_bits_equal(got[c], single[c], f"moments_many column {c} of {ncols} ({dtype}, n={x.size})")
        assert got[c][0] == R.moments(x, null, fill)[0]


def _fn_items(cols, with_mask=True):
    outs = ["float64", "float32"]
    items = []
    for c, (dtype, x, null, fill) in enumerate(cols):
        o = outs[c % 2]
        mode = FN_MODES_NORM[c % 3] if c % 5 else (7, False, 0.0, 1.0)
        if not mode[1] and dtype.startswith("int") and c % 2:
            o = dtype                                         # pure fill, integers stay integers
        items.append((dev(x), bitmap(null), mode[0], mode[1], mode[2], mode[3], TT[o], with_mask))
    return items


@pytest.mark.parametrize("ncols", [1, 32, 33, 40])
def test_fill_normalize_many_bit_identical_to_single(K, ncols):
    cols = _many_columns(ncols, np.random.default_rng(707 + ncols))
    items = _fn_items(cols)
    outs = K.fill_normalize_many(items)
    assert len(outs) == ncols
    for c, (item, (out, filled)) in enumerate(zip(items, outs)):
        dx, dv, fill, do_norm, shift, scale, odt, _ = item
        one, one_filled = K.fill_normalize(dx, dv, fill, do_norm, shift, scale, odt, want_filled_mask=True)
        what = f"fill_normalize_many column {c} of {ncols} ({cols[c][0]} -> {odt}, n={dx.numel()})"
        R.assert_bits_equal(host(out), host(one), what)
        R.assert_bits_equal(host(filled), host(one_filled), what + " filled")
        exp, _ = R.fill_normalize(cols[c][1], cols[c][2], fill, do_norm, shift, scale, host(out).dtype)
        R.assert_bits_equal(host(out), exp, what + " vs reference")


@pytest.mark.parametrize("i,o", [("float32", "float64"), ("float64", "float32"), ("int32", "float32"),
                                 ("int64", "float64")])
def test_fill_normalize_many_device_moments(K, i, o):
    """The ``moments`` pointer: mean / std finished on the device from {count, sum, sum of
    squares} give the bits of the host-finished pair (ops/normalize.py finalize_moments)."""
    from nvtabular_amd.ops.normalize import finalize_moments

    rng = np.random.default_rng(808)
    x = values(i, 4099, rng, finite=True)
    null = rng.random(x.size) < 0.3
    x = garbage(x, null, rng)
    dx, dv = dev(x), bitmap(null)
    const = np.full(x.size, 3, dtype=NP[i])
    trios = [host(_moments(K, dx, dv, 0.5)).tolist(),          # the column's own moments
             [0.0, 0.0, 0.0],                                   # count 0: mean and std NaN
             [1.0, 4.0, 16.0],                                  # count 1: std NaN -> subtract only
             host(_moments(K, dev(const), None, None)).tolist(),  # constant: std 0 -> subtract only
             [10.0, 5.0, 1e-3]]                                 # negative variance: std NaN
    for trio in trios:
        mean, _, std = finalize_moments(*trio)
        scale = std if std > 0 else 0.0
        m = torch.tensor(trio, dtype=torch.float64, device="cuda")
        (a, _), = K.fill_normalize_many([(dx, dv, 0.5, True, 0.0, 0.0, TT[o], False, m)])
        (b, _), = K.fill_normalize_many([(dx, dv, 0.5, True, mean, scale, TT[o], False)])
        R.assert_bits_equal(host(a), host(b), f"device moments {trio} {i}->{o}")
        exp, _ = R.fill_normalize(x, null, 0.5, True, mean, scale, NP[o])
        R.assert_bits_equal(host(a), exp, f"device moments {trio} {i}->{o} vs reference")
        rm, rs = R.finalize_moments(*trio)
        R.assert_bits_equal(np.array([mean, std]), np.array([rm, rs]))


# ---------------------------------------------------------------------------------------------
# bucketize
# ---------------------------------------------------------------------------------------------
def _boundary_sets(dtype):
    t = NP[dtype] if dtype.startswith("float") else np.float64
    b15 = float(t(1.5))
    sets = [[], [0.0], [-2.0, 0.0, 3.0], [-np.inf, -1.0, 0.0, 0.0, 0.0, 1.0, 1.0, np.inf],
            [float(np.nextafter(t(b15), t(0))), b15, float(np.nextafter(t(b15), t(2)))]]
    return sets, np.sort(np.random.default_rng(1).normal(size=8192) * 100)


def _with_boundary_neighbours(x, b):
    """Values equal to a boundary and one ulp (of the COLUMN type) to either side of it."""
    x = x.copy()
    fin = [v for v in b if np.isfinite(v)][:4]
    if x.dtype.kind == "f":
        near = [w for v in fin for w in (np.nextafter(x.dtype.type(v), x.dtype.type(-np.inf)), x.dtype.type(v),
                                         np.nextafter(x.dtype.type(v), x.dtype.type(np.inf)))]
    else:
        near = [w for v in fin for w in (int(math.floor(v)), int(math.floor(v)) + 1, int(math.ceil(v)) - 1)]
    k = min(len(near), max(x.size - 2, 0))
    x[1:1 + k] = near[:k]
    return x


@pytest.mark.parametrize("dtype", list(NP))
def test_bucketize(K, dtype):
    sets, b8192 = _boundary_sets(dtype)
    dsets = [(b, dev(np.array(b, dtype=np.float64))) for b in sets + [b8192.tolist()]]
    for label, x, null, dx, dv in cases(dtype, 909):
        for b, db in dsets:
            xb = _with_boundary_neighbours(x, b)
            got = host(K.bucketize(dev(xb), dv, db))
            R.assert_bits_equal(got, R.bucketize(xb, null, b), f"bucketize {label} nb={len(b)}")


def test_bucketize_second_grid_trip_and_limit(K):
    from nvtabular_amd._lib import NvtHipError

    rng = np.random.default_rng(11)
    x = values("float32", BIG_BUCKET, rng)
    null = rng.random(x.size) < 0.3
    b = [-50.0, -1.0, 0.0, 2.5, 60.0]
    got = host(K.bucketize(dev(garbage(x, null, rng)), bitmap(null), dev(np.array(b))))
    R.assert_bits_equal(got, R.bucketize(x, null, b), "bucketize big")
    with pytest.raises(NvtHipError, match="8192"):
        K.bucketize(dev(x[:100]), None, dev(np.arange(8193, dtype=np.float64)))
    with pytest.raises(NvtHipError, match="unsupported dtype"):
        K.bucketize(dev(np.zeros(100, dtype=np.uint8)), None, dev(np.array(b)))
    with pytest.raises(TypeError, match="float16"):
        K.bucketize(torch.zeros(64, dtype=torch.float16, device="cuda"), None, dev(np.array(b)))


# ---------------------------------------------------------------------------------------------
# gather / te_apply / te_apply_folds
# ---------------------------------------------------------------------------------------------
def _groups(n, ngroups, rng):
    g = rng.integers(-1, ngroups, n).astype(np.int64)
    if n > 2:
        g[0], g[-1] = -1, ngroups - 1
    return g


@pytest.mark.parametrize("out", list(NP))
def test_gather(K, out):
    from nvtabular_amd._lib import NvtHipError

    rng = np.random.default_rng(111)
    if out.startswith("float"):
        src = np.concatenate([edges("float64"), rng.normal(size=50) * 1e3])
        miss = float("nan")
    else:
        src = np.concatenate([[0.0, -0.0, 1.5, -1.5, 2.0**31 - 1, -(2.0**31), 0.999, -0.999], rng.normal(size=50) * 1e3])
        miss = 0.0
    for n in SIZES + [BIG_BUCKET]:
        g = _groups(n, src.size, rng)
        got = host(K.gather(dev(src), dev(g), miss, TT[out]))
        R.assert_bits_equal(got, R.gather(src, g, miss, NP[out]), f"gather -> {out} n={n}")
    with pytest.raises(NvtHipError, match="unsupported out dtype"):
        K.gather(dev(src), dev(_groups(10, 5, rng)), 0.0, torch.uint8)
    with pytest.raises(TypeError, match="float16"):
        K.gather(dev(src), dev(_groups(10, 5, rng)), 0.0, torch.float16)


def _check_te(got, out, exp, s, c, use, p, y_mean, what):
    assert got.dtype == NP[out], what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=what)
    fin = np.isfinite(exp)
    # non-finite results (0 / 0, x / 0) must be the reference's exactly
    np.testing.assert_array_equal(got[~fin & ~np.isnan(exp)], exp[~fin & ~np.isnan(exp)].astype(NP[out]), err_msg=what)
    # rows that take y_mean are exact
    R.assert_bits_equal(got[~use], np.full(int((~use).sum()), y_mean).astype(NP[out]), what + " y_mean rows")
    bound = np.zeros(exp.size)
    bound[use] = R.te_bound(s[use], c[use], p, y_mean)      # FMA or not: see cont_reference.te_bound
    if out == "float32":
        bound = bound + 2.0**-24 * np.abs(exp)              # one more rounding: float64 -> float32
        big = fin & (np.abs(exp) > np.finfo(np.float32).max)
        fin = fin & ~big
        assert np.isinf(got[big]).all(), what               # beyond float32: the conversion gives inf
    m = fin & use
    err = np.abs(got[m].astype(np.float64) - exp[m])
    assert (err <= bound[m]).all(), (what, float(err.max()), np.flatnonzero(err > bound[m])[:5])


def _te_tables(ngroups, rng):
    cnt_all = rng.integers(1, 50, ngroups).astype(np.int64)
    sum_all = (rng.normal(size=ngroups) * cnt_all).round(3)
    return sum_all, cnt_all


@pytest.mark.parametrize("out", ["float32", "float64"])
@pytest.mark.parametrize("p", [20.0, 0.0, 0.3])
def test_te_apply(K, out, p):
    rng = np.random.default_rng(121)
    ngroups, y_mean = 37, 0.3712
    sum_all, cnt_all = _te_tables(ngroups, rng)
    # sparse fold statistics, one entry per group here; entries 0..3 hold the WHOLE group (fold
    # count = group count: a count of 0 in the denominator), entry 1 with a non-zero sum left
    cnt_fold = np.minimum(rng.integers(0, 5, ngroups), cnt_all).astype(np.int64)
    sum_fold = (rng.normal(size=ngroups) * cnt_fold).round(3)
    cnt_fold[:4] = cnt_all[:4]
    sum_fold[:4] = sum_all[:4]
    sum_fold[1] = sum_all[1] - 2.5
    d = [dev(a) for a in (sum_all, cnt_all, sum_fold, cnt_fold)]
    for n in SIZES + [BIG_BUCKET]:
        g = _groups(n, ngroups, rng)
        if n > 8:
            g[1:5] = [0, 1, 2, 3]
        gf = np.where(rng.random(n) < 0.2, -1, g)        # an unseen (fold, key) pair -> y_mean
        if n > 8:
            gf[1:5] = g[1:5]
        got = host(K.te_apply(dev(g), None, d[0], d[1], None, None, p, y_mean, TT[out]))
        exp, s, c, use = R.te_apply(g, None, sum_all, cnt_all, None, None, p, y_mean)
        _check_te(got, out, exp, s, c, use, p, y_mean, f"te_apply p={p} n={n}")
        got = host(K.te_apply(dev(g), dev(gf), d[0], d[1], d[2], d[3], p, y_mean, TT[out]))
        exp, s, c, use = R.te_apply(g, gf, sum_all, cnt_all, sum_fold, cnt_fold, p, y_mean)
        if p == 0 and n > 8:
            assert np.isnan(exp[1]) and np.isinf(exp[2])          # 0 / 0 and 2.5 / 0
        _check_te(got, out, exp, s, c, use, p, y_mean, f"te_apply folds p={p} n={n}")


@pytest.mark.parametrize("out", ["float32", "float64"])
@pytest.mark.parametrize("p", [20.0, 0.0])
@pytest.mark.parametrize("kfold", [2, 5, 256])
def test_te_apply_folds(K, out, p, kfold):
    rng = np.random.default_rng(131)
    ngroups, y_mean = 23, -1.625
    sum_all, cnt_all = _te_tables(ngroups, rng)
    cnt_fold = rng.integers(0, 3, ngroups * kfold).astype(np.int64)       # fold counts of 0 included
    cnt_fold[0] = cnt_all[0]             # (group 0, fold 0) holds the whole group: c = 0
    cnt_fold[kfold] = cnt_all[1]         # (group 1, fold 0) as well, with a sum left over
    sum_fold = (rng.normal(size=ngroups * kfold) * cnt_fold).round(3)
    sum_fold[0] = sum_all[0]
    sum_fold[kfold] = sum_all[1] + 1.25
    d = [dev(a) for a in (sum_all, cnt_all, sum_fold, cnt_fold)]
    for n in SIZES + [BIG_BUCKET]:
        g = _groups(n, ngroups, rng)
        fold = rng.integers(0, kfold, n).astype(np.uint8)
        if n > 8:
            g[1:3], fold[1:3] = [0, 1], [0, 0]
        got = host(K.te_apply_folds(dev(g), dev(fold), kfold, d[0], d[1], d[2], d[3], p, y_mean, TT[out]))
        exp, s, c, use = R.te_apply_folds(g, fold, kfold, sum_all, cnt_all, sum_fold, cnt_fold, p, y_mean)
        if p == 0 and n > 8:
            assert np.isnan(exp[1]) and np.isinf(exp[2])
        _check_te(got, out, exp, s, c, use, p, y_mean, f"te_apply_folds kfold={kfold} p={p} n={n}")


def test_te_apply_rejects(K):
    from nvtabular_amd._lib import NvtHipError

    g = dev(np.zeros(16, dtype=np.int64))
    s, c = dev(np.ones(4)), dev(np.ones(4, dtype=np.int64))
    fold = dev(np.zeros(16, dtype=np.uint8))
    with pytest.raises(NvtHipError, match="f32/f64"):
        K.te_apply(g, None, s, c, None, None, 1.0, 0.5, torch.int32)
    with pytest.raises(NvtHipError, match="f32/f64"):
        K.te_apply_folds(g, fold, 2, s, c, dev(np.ones(8)), dev(np.ones(8, dtype=np.int64)), 1.0, 0.5, torch.int64)
    with pytest.raises(TypeError, match="float16"):
        K.te_apply(g, None, s, c, None, None, 1.0, 0.5, torch.float16)
    with pytest.raises(NvtHipError, match="kfold"):
        K.te_apply_folds(g, fold, 1, s, c, s, c, 1.0, 0.5, torch.float32)


# ---------------------------------------------------------------------------------------------
# widen, popcount, hash bucket
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64", "uint8", "bool"])
def test_widen_i64(K, dtype):
    rng = np.random.default_rng(141)
    for n in SIZES + [BIG_BUCKET]:
        if dtype == "bool":
            x = rng.random(n) < 0.5
        elif dtype == "uint8":
            x = rng.integers(0, 256, n).astype(np.uint8)
        else:
            x = values(dtype, n, rng)
        R.assert_bits_equal(host(K.widen_i64(dev(x))), R.widen(x), f"widen {dtype} n={n}")


def test_widen_rejects(K):
    from nvtabular_amd._lib import NvtHipError

    with pytest.raises(NvtHipError, match="unsupported dtype"):
        K.widen_i64(torch.zeros(64, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError, match="int16"):
        K.widen_i64(torch.zeros(64, dtype=torch.int16, device="cuda"))


def test_popcount(K):
    rng = np.random.default_rng(151)
    for n in SIZES + [BIG_POPCOUNT]:
        for name, null in patterns(n, rng):
            if null is None:
                assert K.popcount(None, n) == n
                continue
            bits = R.pack_bits(~null)
            if bits.size:                  # bits past n in the last byte are arbitrary
                bits[-1] |= (0xFF << (n & 7)) & 0xFF if n & 7 else 0
            assert K.popcount(dev(bits), n) == R.popcount(~null), f"popcount n={n} {name}"


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_hash_bucket(K, dtype):
    """Both kernels (the vectorised one and the XOR-chain one) x bitmap x size edges."""
    for label, x, null, dx, dv in cases(dtype, 161):
        rng = np.random.default_rng(x.size)
        for nb in (1, 1000, 2**31 - 1):
            got, none = K.hash_bucket(dx, nb, valid=dv)
            assert none is None
            R.assert_bits_equal(host(got), R.hash_bucket(x, null, nb), f"hash_bucket {label} nb={nb}")
        xin = rng.integers(-(2**63), 2**63 - 1, x.size, dtype=np.int64)
        got, h = K.hash_bucket(dx, 1000, xor_in=dev(xin), want_hash=True, valid=dv)
        R.assert_bits_equal(host(h).view(np.uint64), R.hash64(x, null, xin), f"hash64 {label}")
        R.assert_bits_equal(host(got), R.hash_bucket(x, null, 1000, xin), f"hash_bucket xor {label}")


def test_hash_bucket_second_grid_trip_and_rejects(K):
    from nvtabular_amd._lib import NvtHipError

    rng = np.random.default_rng(171)
    # stream_grid(n / 4 + 1, 512) = 2048 blocks * 256 lanes * 4 keys = 2 097 152 a trip
    x = values("int32", BIG_VEC4, rng)
    null = rng.random(x.size) < 0.3
    got, _ = K.hash_bucket(dev(garbage(x, null, rng)), 1000, valid=bitmap(null))
    R.assert_bits_equal(host(got), R.hash_bucket(x, null, 1000), "hash_bucket big")
    with pytest.raises(NvtHipError, match="num_buckets"):
        K.hash_bucket(dev(x[:64]), 0)


# ---------------------------------------------------------------------------------------------
# the operators on bool columns (widened first, like LogOp and Bucketize)
# ---------------------------------------------------------------------------------------------
def _bool_frame(n=1003):
    rng = np.random.default_rng(181)
    b = pd.array(rng.random(n) < 0.4, dtype="boolean")
    b[rng.random(n) < 0.25] = pd.NA
    return pd.DataFrame({"b": b}), pd.DataFrame({"b": b.astype("Int64")})


def _run(graph, gdf):
    import nvtabular_amd as nvt

    return nvt.Workflow(graph).fit_transform(nvt.Dataset(gdf)).to_ddf().compute()


def test_bool_columns_through_the_operators():
    """A nullable boolean column is 0 / 1 in int64 for the continuous operators.  The oracle is
    asked on the boolean frame where pandas computes on it, on the same frame as Int64 where
    pandas refuses (a 0 fill or a subtraction on 'boolean')."""
    from nvtabular_amd import ops

    bdf, idf = _bool_frame()
    na = bdf["b"].isna().to_numpy()
    # Clip: the oracle on the boolean frame changes nothing for min_value=0
    got = _run(["b"] >> ops.Clip(min_value=0), bdf)["b"]
    ref = O.clip_transform(bdf, ["b"], min_value=0)["b"]
    np.testing.assert_array_equal(got.isna().to_numpy(), na)
    np.testing.assert_array_equal(got[~na].to_numpy(dtype="int64"), ref[~na].to_numpy(dtype="int64"))
    got = _run(["b"] >> ops.Clip(max_value=0), bdf)["b"]
    ref = O.clip_transform(idf, ["b"], max_value=0)["b"]
    np.testing.assert_array_equal(got[~na].to_numpy(dtype="int64"), ref[~na].to_numpy(dtype="int64"))
    # FillMissing, output directly (DeviceColumn.materialize) and with the binary column
    got = _run(["b"] >> ops.FillMissing(1), bdf)["b"]
    ref = O.fill_missing(idf.copy(), ["b"], 1)["b"]
    np.testing.assert_array_equal(got.to_numpy(dtype="int64"), ref.to_numpy(dtype="int64"))
    got = _run(["b"] >> ops.FillMissing(0, add_binary_cols=True), bdf)
    ref = O.fill_missing(idf.copy(), ["b"], 0, add_binary_cols=True)
    np.testing.assert_array_equal(got["b"].to_numpy(dtype="int64"), ref["b"].to_numpy(dtype="int64"))
    np.testing.assert_array_equal(got["b_filled"].to_numpy(dtype=bool), ref["b_filled"].to_numpy(dtype=bool))
    # Normalize: the oracle takes the boolean frame
    got = _run(["b"] >> ops.Normalize(), bdf)["b"].to_numpy(dtype="float64")
    mom = O.custom_moments([bdf], ["b"])
    ref = O.normalize_transform(bdf, ["b"], mom["mean"].to_dict(), mom["std"].to_dict())["b"]
    R.assert_bits_equal(got, ref.to_numpy(dtype="float64", na_value=np.nan), "Normalize on boolean")
    # NormalizeMinMax
    got = _run(["b"] >> ops.NormalizeMinMax(), bdf)["b"].to_numpy(dtype="float64")
    mins, maxs = O.minmax_fit([idf], ["b"])
    ref = O.minmax_transform(idf, ["b"], mins, maxs)["b"]
    R.assert_bits_equal(got, ref.to_numpy(dtype="float64", na_value=np.nan), "NormalizeMinMax on boolean")
