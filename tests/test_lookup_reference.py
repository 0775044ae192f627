"""lookup_reference.py pinned on the CPU (no GPU): ``jg_stats`` equals ``pandas.groupby(...).agg``
(count / sum / min / max / mean bit for bit, var / std within the bound of pandas' own two-pass
evaluation), ``te_values`` equals the oracle's TargetEncoding fit + transform bit for bit on exact
data and lies within the bound of ``te_values_exact``, ``position`` equals a dict lookup in Python
integers (int64 subtractions that overflow included), ``read_image`` / ``build_image`` equal a
record written by hand with ``struct``, and ``check_keydir`` refuses each way a directory can be
wrong.  test_gpu_lookup_kernels.py compares the device with the key and record references; the
value references wait for a kernel-level test of the record builders."""
import struct
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import lookup_reference as R
import oracle as O

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)


# ---------------------------------------------------------------------------------------------
# jg_stats
# ---------------------------------------------------------------------------------------------
def _jg_frame(seed, ngroups):
    """Integer-valued rows: sizes 1 .. 40 per group; every group of two or more rows is shifted so
    that |sum| <= n / 2 (the reference's sum * sum / n is then small against its sumsq and takes no
    part in a cancellation); two constant groups of 4 and 8 rows (variance exactly 0)."""
    rng = np.random.default_rng(seed)
    keys, vals = [], []
    for g in range(ngroups):
        n = int(rng.integers(1, 41)) if g >= 4 else (1, 2, 4, 8)[g]
        x = rng.integers(-1000, 1001, n).astype(np.float64)
        if g in (2, 3):
            x[:] = 37.0 + g
        elif n > 1:
            x -= np.round(x.mean())
        keys += [g * 3 - 5] * n
        vals += list(x)
    order = rng.permutation(len(keys))
    return pd.DataFrame({"k": np.array(keys)[order], "x": np.array(vals)[order]})


@pytest.mark.parametrize("seed,ngroups", [(1, 12), (2, 30)])
def test_jg_stats_equal_pandas(seed, ngroups):
    df = _jg_frame(seed, ngroups)
    assert 100 <= len(df) <= 900
    x = df["x"].to_numpy()
    assert np.all(x == np.round(x)) and np.abs(x).max() ** 2 * len(df) < 2**53     # exact sums of squares
    gb = df.groupby("k", sort=True)["x"]
    exp = gb.agg(["count", "sum", "min", "max", "mean", "var", "std"])
    count = exp["count"].to_numpy().astype(np.int64)
    sum_ = exp["sum"].to_numpy()
    sumsq = (df["x"] ** 2).groupby(df["k"], sort=True).sum().to_numpy()
    mn, mx = exp["min"].to_numpy(), exp["max"].to_numpy()
    for kind, dt in (("count", np.int64), ("count", np.int32), ("count", np.float32), ("sum", np.float64),
                     ("min", np.float64), ("max", np.float64), ("mean", np.float64)):
        got, free = R.jg_stats(count, sum_, sumsq, mn, mx, kind, dt)
        assert not free.any()
        assert R.bits_mismatch(got, exp[kind].to_numpy().astype(dt), what=kind) is None
    var, free = R.jg_stats(count, sum_, sumsq, None, None, "var", np.float64)
    std, free_s = R.jg_stats(count, sum_, sumsq, None, None, "std", np.float64)
    assert not free.any() and not free_s.any()
    one = count == 1
    assert one.any() and np.all(np.isnan(var[one])) and np.all(np.isnan(std[one]))
    assert np.all(np.isnan(exp["var"].to_numpy()[one])) and np.all(np.isnan(exp["std"].to_numpy()[one]))
    assert np.all(var[one].view(np.uint64) == 0x7FF8000000000000)
    many = ~one
    # premise of the bound: no cancellation in sumsq - sum * sum / n
    assert np.all((var[many] == 0) | (sum_[many] ** 2 / count[many] <= var[many] * (count[many] - 1)))
    for got, ref in ((var, exp["var"].to_numpy()), (std, exp["std"].to_numpy())):
        bound = (count[many] + 3) * 2.0**-53 * np.abs(ref[many])
        assert np.all(np.abs(got[many] - ref[many]) <= bound), (got[many], ref[many])
    assert (var[many] == 0).sum() >= 2                       # the constant groups
    # the output cast: once, from the float64 value
    v32, _ = R.jg_stats(count, sum_, sumsq, None, None, "var", np.float32)
    assert R.bits_mismatch(v32, var.astype(np.float32)) is None
    m_i, _ = R.jg_stats(count, sum_ * 0 + 7.0 * count + 3, None, None, None, "mean", np.int32)
    assert m_i.dtype == np.int32 and np.all(m_i == np.trunc((7.0 * count + 3) / count))


def test_jg_stats_negative_variance_and_undefined_casts():
    count = np.array([3, 2], np.int64)
    s = np.array([3.0, 2.0])
    ss = np.array([3.0 - 2.0**-40, 2.0])
    var, free = R.jg_stats(count, s, ss, None, None, "var", np.float64)
    assert var[0] < 0 and var[1] == 0 and not free.any()
    std, free = R.jg_stats(count, s, ss, None, None, "std", np.float64)
    assert np.isnan(std[0]) and std[1] == 0 and free.tolist() == [True, False]
    with pytest.raises(AssertionError):
        R.jg_stats(np.array([1], np.int64), s[:1], ss[:1], None, None, "var", np.int32)      # NaN -> int32
    with pytest.raises(AssertionError):
        R.jg_stats(count, s * 1e12, None, None, None, "sum", np.int32)                       # out of range


# ---------------------------------------------------------------------------------------------
# te_values
# ---------------------------------------------------------------------------------------------
def _dense_stats(fit, kfold):
    """totals [g] and dense fold statistics [g * kfold] of a fitted frame (columns k, y, __fold__)."""
    keys = np.sort(fit["k"].unique())
    pos = {int(k): i for i, k in enumerate(keys)}
    g = keys.size
    tc, ts = np.zeros(g, np.int64), np.zeros(g)
    fc, fs = np.zeros(g * max(kfold, 1), np.int64), np.zeros(g * max(kfold, 1))
    fold = fit["__fold__"].to_numpy() if kfold > 1 else np.zeros(len(fit), np.int64)
    for k, y, f in zip(fit["k"].to_numpy(), fit["y"].to_numpy(), fold):
        i = pos[int(k)]
        tc[i] += 1
        ts[i] += y
        fc[i * max(kfold, 1) + int(f)] += 1
        fs[i * max(kfold, 1) + int(f)] += y
    return keys, tc, ts, fc, fs


@pytest.mark.parametrize("kfold", [1, 3])
@pytest.mark.parametrize("p_smooth", [0, 20])
@pytest.mark.parametrize("exact", [True, False])
def test_te_values_equal_the_oracle(tmp_path, kfold, p_smooth, exact):
    rng = np.random.default_rng(100 * kfold + p_smooth + exact)
    n = 500
    k = rng.integers(0, 14, n).astype(np.int64) * 7 - 20
    if exact:       # multiples of 2^-6: sums, p * mean and the numerator are exact in float64
        y = rng.integers(-2**10, 2**10, n) / 64.0
        ym = 23 / 64.0
    else:
        y = rng.normal(size=n)
        ym = 0.37
    fit = pd.DataFrame({"k": k[:380], "y": y[:380]})
    stats, means = O.target_encoding_fit([fit], ["k"], ["y"], str(tmp_path), kfold=kfold, fold_seed=5,
                                         target_mean={"y": ym})
    df = pd.DataFrame({"k": np.concatenate([k[380:], [1000, -1000]])})               # two unseen keys
    ref = O.target_encoding_transform(df.copy(), ["k"], ["y"], stats, means, kfold=kfold, fold_seed=5,
                                      p_smooth=p_smooth, out_dtype=np.float64, target_mean={"y": ym})
    ref = ref["TE_k_y"].to_numpy()
    keys, tc, ts, fc, fs = _dense_stats(fit, kfold)
    if not exact:   # the oracle's sums, in its order of addition
        agg = pd.read_parquet(stats["k"])
        agg.columns = ["k", "count", "sum"]
        agg = agg.sort_values("k", ignore_index=True)
        assert np.array_equal(agg["k"].to_numpy(), keys) and np.array_equal(agg["count"].to_numpy(), tc)
        ts = agg["sum"].to_numpy().astype(np.float64)
        if kfold > 1:
            af = pd.read_parquet(stats["__fold___k"])
            af.columns = ["f", "k", "count", "sum"]
            at = np.searchsorted(keys, af["k"].to_numpy()) * kfold + af["f"].to_numpy().astype(np.int64)
            assert np.array_equal(fc[at], af["count"].to_numpy())
            fs[at] = af["sum"].to_numpy()
    kf = kfold if kfold > 1 else 0
    vals, free = R.te_values(tc, ts, fc if kf else None, fs if kf else None, kf, p_smooth, ym, np.float64)
    assert vals.shape == (keys.size, kf + 1)
    assert not free.any()                    # (no group with all its rows in one fold: the oracle fills those NaN)
    g = R.position((keys + 20).astype(np.int32), df["k"].to_numpy(), key_offset=-20)
    assert (g < 0).sum() == 2
    slot = 1 + O.add_fold(len(df), kfold, 5).astype(np.int64) if kf else np.zeros(len(df), np.int64)
    got = np.where(g >= 0, vals[np.maximum(g, 0), slot], ym)
    assert R.bits_mismatch(got, ref, what=f"kfold {kfold} p {p_smooth}") is None
    E, bound = R.te_values_exact(tc, ts, fc if kf else None, fs if kf else None, kf, p_smooth, ym, np.float64)
    assert R.te_outside(vals, E, bound) == []
    if exact:       # the premise of the exact family, and what follows from it
        for a in (ts, fs):
            assert np.all(a * 64 == np.round(a * 64)) and np.abs(a).max() < 2**20
        one_rounding = np.vectorize(lambda e: float(e), otypes=[np.float64])(E)      # Fraction -> nearest double
        assert R.bits_mismatch(vals, one_rounding, what="exact family") is None
    v32, _ = R.te_values(tc, ts, fc if kf else None, fs if kf else None, kf, p_smooth, ym, np.float32)
    assert R.bits_mismatch(v32, vals.astype(np.float32)) is None
    E32, b32 = R.te_values_exact(tc, ts, fc if kf else None, fs if kf else None, kf, p_smooth, ym, np.float32)
    assert R.te_outside(v32, E32, b32) == []


def test_te_values_slots_and_division_by_zero():
    tc = np.array([4, 3, 2], np.int64)
    ts = np.array([2.0, 6.0, 1.5])
    fc = np.array([4, 0, 1, 2, 2, 0], np.int64)              # group 0 and 2: every row in fold 0
    fs = np.array([2.0, 0.0, 1.0, 5.0, 2.5, 0.0])            # group 2: forged sums (x / 0)
    v, free = R.te_values(tc, ts, fc, fs, 2, 0.0, 0.25, np.float64)
    assert v[0, 0] == 0.5 and v[1, 0] == 2.0
    assert np.isnan(v[0, 1]) and free[0, 1] and v[0, 2] == 0.25                     # 0 / 0; no rows: the mean
    assert v[1, 1] == 2.5 and v[1, 2] == 1.0
    assert v[2, 1] == -np.inf and v[2, 2] == 0.25 and free.sum() == 1
    with pytest.raises(AssertionError):
        R.te_values_exact(tc, ts, fc, fs, 2, 0.0, 0.25, np.float64)
    # a value one ulp off the exact one lies inside the bound, one part in 2^40 does not
    E, b = R.te_values_exact(tc[1:2], ts[1:2], fc[2:4], fs[2:4], 2, 20.0, 0.37, np.float64)
    v, _ = R.te_values(tc[1:2], ts[1:2], fc[2:4], fs[2:4], 2, 20.0, 0.37, np.float64)
    assert R.te_outside(np.nextafter(v, 9.0), E, b) == []
    assert len(R.te_outside(v * (1 + 2.0**-40), E, b)) == 3
    assert abs(Fraction(float(v[0, 1])) - (Fraction(6.0) - Fraction(1.0) + 20 * Fraction(0.37)) / 22) <= b[0, 1]


# ---------------------------------------------------------------------------------------------
# position
# ---------------------------------------------------------------------------------------------
def _dict_lookup(ids, rows, valid, key_offset, null_group):
    where = {int(k): g for g, k in enumerate(ids)}
    out = []
    for i, r in enumerate(rows):
        if valid is not None and not valid[i]:
            out.append(null_group)
        else:
            out.append(where.get(int(r) - key_offset, -1))
    return np.array(out, np.int64)


def test_position_equals_a_dict_lookup():
    rng = np.random.default_rng(3)
    ids = np.unique(np.concatenate([rng.integers(I32.min, I32.max, 300), [I32.min, I32.max, 0]])).astype(np.int32)
    rows = np.concatenate([ids[rng.integers(0, ids.size, 500)], rng.integers(I32.min, I32.max, 200)]).astype(np.int32)
    valid = rng.random(rows.size) > 0.2
    for v, ng in ((None, -1), (valid, -1), (valid, ids.size)):
        np.testing.assert_array_equal(R.position(ids, rows, v, 0, ng), _dict_lookup(ids, rows, v, 0, ng))
    for off in (-7_000_000_000_000, 5_000_000_000, I64.max - 5, I64.min + 5, 2**31, -(2**31)):
        lo, hi = max(I64.min, off + I32.min), min(I64.max, off + I32.max)
        inside = [k for k in (ids.astype(object) + off) if lo <= k <= hi]
        rows = np.array(inside[:200] + [I64.min, I64.max, I64.min + 1, I64.max - 1, 0, -1, lo, hi]
                        + ([lo - 1] if lo > I64.min else []) + ([hi + 1] if hi < I64.max else []), np.int64)
        got = R.position(ids, rows, None, off)
        np.testing.assert_array_equal(got, _dict_lookup(ids, rows, None, off, -1))
        assert (got >= 0).sum() >= min(200, len(inside))
    # subtractions that overflow int64 miss; they must not wrap into the list
    ids = np.array([-2, -1, 0, 1, I32.max], np.int32)
    assert R.position(ids, np.array([I64.min, I64.max], np.int64), None, 1).tolist() == [-1, -1]
    assert R.position(ids, np.array([I64.max, I64.min], np.int64), None, -1).tolist() == [-1, -1]
    assert R.position(ids, np.array([I64.min], np.int64), None, I64.min).tolist() == [2]
    assert R.position(ids, np.array([I64.max, I64.max - 2], np.int64), None, I64.max - 1).tolist() == [3, 1]
    # one below and one above the window
    assert R.position(ids, np.array([10 + I32.max, 11 + I32.max, 10 + I32.min - 1], np.int64), None, 10).tolist() \
        == [4, -1, -1]
    with pytest.raises(AssertionError):
        R.position(np.array([1, 1], np.int32), rows)


def test_flat_positions():
    assert R.flat_positions([0, 0, 0, 5, 5, 6, 9]).tolist() == [0, 1, 2, 5, 6, 7, 9]


# ---------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------
def test_read_and_build_image_equal_records_written_by_hand():
    count = np.array([1, 2, 5], np.int64)
    s = [np.array([4.0, 3.0, 10.0])]
    ss = [np.array([16.0, 5.0, 30.0])]
    tc, ts = np.array([4, 3], np.int64), np.array([2.0, 6.0])
    fc, fs = np.array([3, 1, 0, 3], np.int64), np.array([1.5, 0.5, 0.0, 6.0])
    parts = [dict(kind="jg", groups=3, count=count, sum=s, sumsq=ss, mn=None, mx=None,
                  outputs=[("count", 0, np.int32, 0), ("mean", 0, np.float32, 4), ("var", 0, np.float64, 8)]),
             dict(kind="te", groups=2, tot_count=tc, tot_sum=ts, fold_count=fc, fold_sum=fs, kfold=2, p=1.0,
                  y_mean=0.5, dtype=np.float32, off=16)]
    img, free = R.build_image(parts, 4, 32)
    assert free == [] and img.size == 128
    nan = struct.pack("<Q", 0x7FF8000000000000)
    exp = b"".join([
        struct.pack("<if", 1, 4.0) + nan + struct.pack("<fff", 2.5 / 5, (0.5 + 0.5) / 2, (1.5 + 0.5) / 4) + bytes(4),
        struct.pack("<ifd", 2, 1.5, 0.5) + struct.pack("<fff", 6.5 / 4, 0.5, 0.5 / 1) + bytes(4),
        struct.pack("<ifd", 5, 2.0, 2.5) + bytes(16),
        bytes(32)])
    assert img.tobytes() == exp
    assert R.image_mismatch(img, np.frombuffer(exp, np.uint8), free, 32) is None
    bad = img.copy()
    bad[32 * 3 + 31] = 1
    assert "record 3 byte 31" in R.image_mismatch(bad, img, free, 32)
    # the mean from {count, sum}; a generated NaN is free in sign, not in being one
    p = dict(parts[1], moments=(3.0, 1.0), p=0.0, kfold=0, dtype=np.float64, off=24, tot_count=np.array([0, 1], np.int64),
             tot_sum=np.array([0.0, 1.0]))
    img2, free2 = R.build_image([p], 2, 32)
    assert len(free2) == 1 and free2[0][0].tolist() == [0] and free2[0][1] == 24
    flipped = img2.copy()
    flipped[31] ^= 0x80
    assert R.image_mismatch(flipped, img2, free2, 32) is None
    flipped[24:32] = 0
    assert "NaN expected" in R.image_mismatch(flipped, img2, free2, 32)
    with pytest.raises(AssertionError):
        R.build_image([dict(parts[1], groups=5)], 4, 32)
    # read_image
    g = np.array([1, -1, 0, 2], np.int64)
    assert R.read_image(img, 32, g, 0, 4, None, 0xFFFFFFFF11).tolist() == [2, 0xFFFFFF11, 1, 5]
    got = R.read_image(img, 32, g, 8, 8, None, 7)
    assert got.dtype == np.uint64 and got.view(np.float64)[[0, 3]].tolist() == [0.5, 2.5] and got[1] == 7
    assert got[2] == 0x7FF8000000000000
    fold = np.array([1, 0, 0, 1], np.uint8)
    got = R.read_image(img, 32, g, 16, 4, fold, 0).view(np.float32)
    assert got.tolist() == [0.5, 0.0, 0.5, 0.0]
    with pytest.raises(AssertionError):
        R.read_image(img, 32, g, 24, 4, fold, 0)              # slot 2 of offset 24 lies outside the record


# ---------------------------------------------------------------------------------------------
# check_keydir
# ---------------------------------------------------------------------------------------------
def _dir(ids, bucket_of, B):
    """A directory written from the definition, with an arbitrary monotone key -> bucket map."""
    n = ids.size
    b = np.array([bucket_of(int(k)) for k in ids])
    d = np.zeros((B + 1, 4), np.uint32)
    for q in range(B + 1):
        first = int(np.searchsorted(b, q, side="left"))
        nxt = int(np.searchsorted(b, q + 1, side="left")) if q < B else n
        ks = ids[first:nxt][:3].tolist()
        if not ks:
            ks = [int(ids[min(first, n - 1)])]
        ks += [ks[-1]] * (3 - len(ks))
        d[q] = [first] + [k & 0xFFFFFFFF for k in ks]
    return d.reshape(-1)


def test_check_keydir_accepts_the_definition_and_refuses_each_wrong_field():
    ids = np.array([I32.min, -50, -49, -48, -47, 3, 4, 900, I32.max], np.int32)
    B = 8
    d = _dir(ids, lambda k: (k - I32.min) * B >> 32, B)
    R.check_keydir(d, ids, B)
    R.check_keydir(d.view(np.int32), ids, B)                    # (as torch holds it)
    R.check_keydir(_dir(ids[:1], lambda k: 0, 3), ids[:1], 3)
    first = d.reshape(B + 1, 4)[:, 0]
    assert np.diff(np.append(first, ids.size)).max() >= 4       # a bucket of more than three keys
    assert (np.diff(first) == 0).any()                          # an empty bucket

    def broken(entry, word, value):
        bad = d.copy().reshape(B + 1, 4)
        bad[entry, word] = value
        return bad.reshape(-1)

    full = int(np.argmax(np.diff(np.append(first, ids.size))))
    empty = int(np.flatnonzero(np.diff(first) == 0)[0])
    cases = {"first[0]": broken(0, 0, 1), "first[8]": broken(B, 0, ids.size - 1),
             "first decreases": broken(B - 1, 0, ids.size + 1),
             "k0": broken(full, 1, 12345), "k1": broken(full, 2, 12345), "k2": broken(full, 3, 12345),
             "k0 of bucket %d" % empty: broken(empty, 1, int(ids[0]) & 0xFFFFFFFF),
             "k2 of bucket %d" % B: broken(B, 3, 5),
             "directory of": d[:-4]}
    for what, bad in cases.items():
        with pytest.raises(AssertionError, match=what.replace("[", r"\[").replace("]", r"\]")):
            R.check_keydir(bad, ids, B)
