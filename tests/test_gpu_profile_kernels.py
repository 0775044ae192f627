"""nvt_col_profile_many and nvt_cast_many through ``K.col_profile_many`` / ``K.cast_many``, against the
numpy references of profile_reference.py / cont_reference.py.

Float min / max are compared bit for bit.  ``R.minmax`` gives their VALUE; the sign of a zero
result is fixed by the kernel's total order (-0.0 below +0.0: min is -0.0 when a -0.0 counts, max
is +0.0 when a +0.0 counts), where numpy returns whichever zero it meets first.

Sums: exact (bit-equal to math.fsum) for integer-valued data whose sums stay below 2**53, where
every partial sum is exact whatever the order; for general finite data within the bound for
summing n terms in any order, |err| <= n * 2**-53 * fsum(|terms|) (derived in
test_gpu_cont_kernels._check_moments_bound)."""
import math

import numpy as np
import pytest
import torch

import cont_reference as R
import profile_reference as PR
from test_gpu_cont_kernels import BIG_MOM4, BIG_MOM8, NP, TT, bitmap, dev, garbage, host, patterns, values

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025]
CAST_SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 4097]


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


def _int_valued(dtype, n, rng):
    mag = int(min(2**20, math.isqrt(2**53 // max(n, 1)))) - 1
    return rng.integers(-mag, mag + 1, n).astype(NP[dtype])


def _run(K, cols, acc=None):
    """cols: [(device x, device bitmap)] -> (accumulator tensor, decoded rows)."""
    dts = [x.dtype for x, _ in cols]
    acc = K.new_profile_acc(dts, "cuda") if acc is None else acc
    K.col_profile_many([(x, v, acc[i]) for i, (x, v) in enumerate(cols)])
    return acc, K.profile_rows(host(acc), dts)


def _check_counts_extrema(label, got, x, null, sums=False):
    exp = PR.profile(x, null, sums)
    assert (got["rows"], got["valid"]) == (exp["rows"], exp["valid"]), label
    if x.dtype.kind == "i":
        assert got["min"] == exp["min"] and got["max"] == exp["max"], (label, got, exp)
        assert got["min"] is None or (isinstance(got["min"], int) and isinstance(got["max"], int)), label
    elif exp["valid"] == 0:
        assert got["min"] is None and got["max"] is None, label
    else:
        lo, hi = PR.expected_float_extrema(x, null)
        assert PR.float_bits(got["min"]) == PR.float_bits(lo), (label, got["min"], lo)
        assert PR.float_bits(got["max"]) == PR.float_bits(hi), (label, got["max"], hi)
    return exp


def _check_exact(label, got, x, null):
    exp = _check_counts_extrema(label, got, x, null, sums=True)
    assert PR.float_bits(got["sum"]) == PR.float_bits(exp["sum"]), (label, got["sum"], exp["sum"])
    assert PR.float_bits(got["sumsq"]) == PR.float_bits(exp["sumsq"]), (label, got["sumsq"], exp["sumsq"])


def _check_bound(label, got, x, null):
    exp = _check_counts_extrema(label, got, x, null, sums=True)
    bs, bq = PR.sum_bound(x, null)
    assert abs(got["sum"] - exp["sum"]) <= bs, (label, got["sum"], exp["sum"], bs)
    assert abs(got["sumsq"] - exp["sumsq"]) <= bq, (label, got["sumsq"], exp["sumsq"], bq)


def _tame(dtype, x):
    """General finite data whose squares stay finite and summable (as test_moments does)."""
    if dtype == "int64":
        return np.where(np.abs(x.astype(np.float64)) > 2.0**40, x >> 24, x)
    return x


@pytest.mark.parametrize("dtype", list(NP))
def test_profile_sizes_and_null_patterns(K, dtype):
    """Cases 1-4: every size x every validity pattern; the columns of one size go in ONE call."""
    rng = np.random.default_rng(71)
    for n in SIZES:
        xi, xe, xg = _int_valued(dtype, n, rng), values(dtype, n, rng), _tame(dtype, values(dtype, n, rng, finite=True))
        batch = []
        for name, null in patterns(n, rng):
            a = garbage(xi, null, rng)
            if dtype.startswith("float") and n > 5:
                a[5] = np.nan                                   # NaN under a set validity bit
            batch.append((f"{dtype} n={n} {name} int-valued", a, null, _check_exact))
            batch.append((f"{dtype} n={n} {name} edges", garbage(xe, null, rng), null, _check_counts_extrema))
            batch.append((f"{dtype} n={n} {name} general", garbage(xg, null, rng), null, _check_bound))
        acc, rows = _run(K, [(dev(x), bitmap(null)) for _, x, null, _ in batch])
        for (label, x, null, check), got in zip(batch, rows):
            check(label, got, x, null)
        if n == 0:   # a call with n == 0 leaves the accumulators untouched
            assert torch.equal(acc.cpu(), K.new_profile_acc([TT[dtype]] * len(batch), "cpu"))


@pytest.mark.parametrize("dtype", list(NP))
def test_profile_second_grid_trip(K, dtype):
    """The kernel keeps the loop of the moments kernel (1024 blocks, 4 vectors per lane and trip), so
    the sizes that force its second trip are BIG_MOM4 / BIG_MOM8 of test_gpu_cont_kernels.py (the
    BIG_MINMAX of test_minmax_second_grid_trip fits in one trip of this loop)."""
    n = BIG_MOM4 if dtype in ("float32", "int32") else BIG_MOM8
    rng = np.random.default_rng(72)
    x = _int_valued(dtype, n, rng) // 2                       # (halved: room for the two extremes below)
    x[-2], x[-9] = 60_000, -60_000                            # the extremes sit in the tail / the last vectors
    null = rng.random(n) < 0.3
    null[-2] = null[-9] = False
    x = garbage(x, null, rng)
    _, rows = _run(K, [(dev(x), bitmap(null))])
    _check_exact(f"{dtype} big", rows[0], x, null)


def test_profile_exact_int64_and_float_edges(K):
    """Case 3: values a double accumulator would round, every lane heard, the zeros' signs."""
    big = np.array([2**53 + 1, -(2**53) - 1, 5, -7, 0], dtype=np.int64)
    full = np.array([2**63 - 1, -(2**63), 2**53 + 1, -(2**53) - 1], dtype=np.int64)
    cols = [big, full, big[:1], big[1:2], np.array([2**63 - 1], dtype=np.int64), np.array([-(2**63)], dtype=np.int64)]
    for pos in list(range(0, 1024, 37)) + [1023]:
        x = np.zeros(1024, dtype=np.int64)
        x[pos], x[1023 - pos] = 2**53 + 1, -(2**53) - 1
        cols.append(x)
    _, rows = _run(K, [(dev(x), None) for x in cols])
    for x, got in zip(cols, rows):
        assert got["min"] == int(x.min()) and got["max"] == int(x.max()) and isinstance(got["min"], int), (x[:4], got)
        assert got["rows"] == got["valid"] == x.size
    for dt in (np.float32, np.float64):
        tiny = np.finfo(dt).smallest_subnormal
        cases = [np.array([0.0, -0.0], dt), np.array([-0.0, 0.0], dt), np.array([0.0, 0.0], dt),
                 np.array([-0.0, -0.0], dt), np.array([np.inf, -np.inf, 1.0], dt), np.array([np.inf], dt),
                 np.array([-np.inf, np.nan], dt), np.array([tiny, -tiny, 0.0], dt), np.array([tiny, 2 * tiny], dt),
                 np.array([np.nan, np.nan], dt), np.concatenate([np.zeros(700, dt), -np.zeros(1, dt), np.zeros(323, dt)])]
        _, rows = _run(K, [(dev(x), None) for x in cases])
        for x, got in zip(cases, rows):
            _check_counts_extrema(f"{dt.__name__} {x[:3]}", got, x, None)
    # a zero that is only present under a null does not count
    x, null = np.array([-0.0, 0.0, 0.0], np.float64), np.array([True, False, False])
    _, rows = _run(K, [(dev(x), bitmap(null))])
    assert PR.float_bits(rows[0]["min"]) == PR.float_bits(0.0)


@pytest.mark.parametrize("dtype", list(NP))
def test_profile_accumulates_across_calls(K, dtype):
    """Case 5: x[:k] then x[k:] into the same accumulators."""
    rng = np.random.default_rng(73)
    n = 1025
    null = rng.random(n) < 0.3
    for make, check in ((_int_valued, _check_exact), (lambda d, m, r: _tame(d, values(d, m, r, finite=True)), _check_bound)):
        x = garbage(make(dtype, n, rng), null, rng)
        _, whole = _run(K, [(dev(x), bitmap(null))])
        for k in (0, 1, n - 1):
            acc = K.new_profile_acc([TT[dtype]], "cuda")
            for lo, hi in ((0, k), (k, n)):
                _run(K, [(dev(x[lo:hi]), bitmap(null[lo:hi]))], acc)
            got = K.profile_rows(host(acc), [TT[dtype]])[0]
            for key in ("rows", "valid", "min", "max"):
                assert got[key] == whole[0][key] or (key in ("min", "max") and PR.float_bits(got[key]) == PR.float_bits(whole[0][key])), (k, key)
            check(f"{dtype} split at {k}", got, x, null)
    # folding into accumulators that already hold wider extrema keeps them
    acc = K.new_profile_acc([TT[dtype]], "cuda")
    _run(K, [(dev(np.array([-900, 900], NP[dtype])), None)], acc)
    _run(K, [(dev(np.array([1, 2, 3], NP[dtype])), None)], acc)
    got = K.profile_rows(host(acc), [TT[dtype]])[0]
    assert (got["rows"], got["valid"], got["min"], got["max"], got["sum"]) == (5, 5, -900, 900, 6.0)


def test_profile_batch_of_33_and_element_aligned_heads(K):
    """Case 6: one more column than a batch, mixed dtypes and lengths; slices that start one element in."""
    rng = np.random.default_rng(74)
    lengths = [100_003, 1, 513, 0, 4097, 30_011, 129, 70_001]
    cols = []
    for c in range(33):
        dtype = list(NP)[c % 4]
        n = lengths[c % len(lengths)]
        null = None if c % 3 == 0 else rng.random(n) < 0.3
        cols.append((dev(garbage(_tame(dtype, values(dtype, n, rng, finite=True)), null, rng)), bitmap(null)))
    acc, _ = _run(K, cols)
    for c, col in enumerate(cols):
        single, _ = _run(K, [col])
        assert torch.equal(acc[c], single[0]), f"column {c} of 33"
    heads = []
    for dtype in NP:
        for n in (1, 5, 257, 4099):
            base = dev(_tame(dtype, values(dtype, n + 1, rng, finite=True)))
            null = rng.random(n) < 0.3
            heads.append((base[1:], base[1:].clone(), bitmap(null)))
            assert base[1:].data_ptr() % 16 != 0 and heads[-1][1].data_ptr() % 16 == 0
    a, _ = _run(K, [(s, v) for s, _, v in heads])
    b, _ = _run(K, [(f, v) for _, f, v in heads])
    assert torch.equal(a, b)


def test_profile_rejects(K):
    acc = K.new_profile_acc([torch.float32], "cuda")
    with pytest.raises(TypeError, match="float16"):
        K.col_profile_many([(torch.zeros(8, dtype=torch.float16, device="cuda"), None, acc[0])])
    with pytest.raises(TypeError, match="int8"):
        K.col_profile_many([(torch.zeros(8, dtype=torch.int8, device="cuda"), None, acc[0])])
    assert torch.equal(acc.cpu(), K.new_profile_acc([torch.float32], "cpu"))
    # a bool column is profiled as 0 / 1
    b = np.arange(100) % 3 == 0
    acc = K.new_profile_acc([torch.int64], "cuda")
    K.col_profile_many([(dev(b), None, acc[0])])
    got = K.profile_rows(host(acc), [torch.int64])[0]
    assert (got["valid"], got["min"], got["max"], got["sum"]) == (100, 0, 1, float(b.sum()))


# ---- casts ------------------------------------------------------------------------------------------------
CAST_PAIRS = [("int32", "int8"), ("int32", "int16"), ("int64", "int8"), ("int64", "int16"), ("int64", "int32"),
              ("float64", "float32")]
NPC = {**NP, "int8": np.int8, "int16": np.int16}
TTC = {**TT, "int8": torch.int8, "int16": torch.int16}


def _cast_values(src, n, rng):
    if src == "float64":
        f32 = np.finfo(np.float32)
        half = (np.float64(np.float32(1.0)) + np.float64(np.nextafter(np.float32(1.0), np.float32(2.0)))) / 2
        e = np.array([np.nan, np.inf, -np.inf, 1e39, -1e39, float(f32.max) * (1 + 2.0**-25), half, -half,
                      1.0 + 2.0**-24 + 2.0**-50, float(f32.smallest_subnormal), float(f32.smallest_subnormal) * 0.5,
                      -float(f32.tiny) * 0.75, 5e-324, 1e-50, 0.0, -0.0, float(f32.max)], dtype=np.float64)
        x = rng.normal(size=n) * 10.0 ** rng.integers(-45, 40, n)
    else:
        e = []
        for t in (np.int8, np.int16, np.int32, np.int64):
            i = np.iinfo(t)
            e += [i.min, i.max] + ([i.min - 1, i.max + 1] if t != np.int64 else [])
        e = np.array([v for v in e if np.iinfo(NPC[src]).min <= v <= np.iinfo(NPC[src]).max], dtype=NPC[src])
        info = np.iinfo(NPC[src])
        x = rng.integers(info.min, info.max, n, dtype=NPC[src], endpoint=True)
    if n:
        k = min(n, e.size)
        x[:k] = e[:k]
        x[n - k:] = e[e.size - k:]
        pos = rng.integers(0, n, min(n, 2 * e.size))
        x[pos] = e[rng.integers(0, e.size, pos.size)]
    return x.astype(NPC[src])


@pytest.mark.parametrize("pair", CAST_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_cast_matches_numpy_astype(K, pair):
    """Case 7: every size, aligned and element-aligned source, in ONE call; sentinel behind every output."""
    src, dst = pair
    rng = np.random.default_rng(75)
    width = np.dtype(NPC[dst]).itemsize
    items, exp = [], []
    for n in CAST_SIZES + ([4096 * 64 + 17] if pair == ("int64", "int8") else []):
        for head in (0, 1):
            x = _cast_values(src, n + head, rng)
            d = dev(x)[head:]
            assert head == 0 or n == 0 or d.data_ptr() % 16 != 0
            buf = torch.full((n * width + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            items.append((d, TTC[dst], buf[: n * width].view(TTC[dst])))
            with np.errstate(over="ignore"):
                exp.append((x[head:].astype(NPC[dst]), buf, n))
    outs = K.cast_many(items)
    for (want, buf, n), out, item in zip(exp, outs, items):
        assert out is item[2]
        got = host(out)
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got.view(f"u{width}"), want.view(f"u{width}"), err_msg=f"{pair} n={n}")
        assert host(buf[n * width:]).tolist() == [0xA5] * 16, f"{pair} n={n}: bytes behind the output"
    # an output that is only element-aligned takes the scalar way: same values, nothing behind it touched
    x = _cast_values(src, 65, rng)
    buf = torch.full((65 * width + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[width: 66 * width].view(TTC[dst])
    assert out.data_ptr() % 16 != 0
    K.cast_many([(dev(x), TTC[dst], out)])
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(host(out).view(f"u{width}"), x.astype(NPC[dst]).view(f"u{width}"))
    assert set(host(buf[:width]).tolist()) == {0xA5} and set(host(buf[66 * width:]).tolist()) == {0xA5}
    # the driver allocates the output itself; the same dtype is a no-op
    x = dev(_cast_values(src, 1000, rng))
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(host(K.cast_many([(x, TTC[dst])])[0]), host(x).astype(NPC[dst]))
    assert K.cast_many([(x, TTC[src])])[0] is x


def test_cast_rejects(K):
    """Case 8: widening, int <-> float and unknown dtypes raise; nothing is launched or written."""
    from nvtabular_amd._lib import NvtHipError

    out = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    for src, dst in [(torch.int32, torch.int64), (torch.int64, torch.float32), (torch.float64, torch.int32),
                     (torch.float32, torch.float64), (torch.float32, torch.int8)]:
        with pytest.raises(NvtHipError, match="unsupported cast"):
            K.cast_many([(torch.zeros(8, dtype=src, device="cuda"), dst, out.view(dst)[:8])])
    for src, dst in [(torch.int64, torch.uint8), (torch.float16, torch.float32), (torch.bool, torch.int8)]:
        with pytest.raises(TypeError, match="unsupported cast"):
            K.cast_many([(torch.zeros(8, dtype=src, device="cuda"), dst)])
    assert host(out).tolist() == [7] * 64
