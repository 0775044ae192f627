"""Plain numpy / Python references of the transform side of JoinGroupby and TargetEncoding
(csrc/nvt_flat_lookup.hip, csrc/nvt_keydir.hip, the per-row kernels of csrc/nvt_cont.hip).
test_lookup_reference.py pins them to pandas, to the oracle's TargetEncoding and to a dict lookup
on the CPU.  test_gpu_lookup_kernels.py compares the device with ``position``, ``read_image``,
``check_keydir`` and ``flat_positions``; the references of the VALUES (``jg_stats``, ``te_values``,
``te_values_exact``, ``build_image``) are what a kernel-level test of the four record builders has
to compare with -- no such test exists yet.  Nothing here shares code with the device side; the
contract followed is the one of include/nvt_hip.h ("flat range table", "Lookup images", "key
directory", nvt_te_apply*, nvt_gather_f64):

    position         key -> position in the ascending int32 key list, in Python integers
    jg_stats         the seven JoinGroupby statistics from the fit's accumulators, in float64 in
                     the documented order, then ONE cast to the output dtype
    te_values        TargetEncoding's (kfold + 1) values per group; te_values_exact the same as
                     exact rationals with a first-order rounding bound
    read_image       what a row receives from a packed record
    build_image      the whole byte image of the one-pass build
    check_keydir     the directory definition
    flat_positions   the layout rule of the flat table, p_i = max(h_i, p_(i-1) + 1)

NaN.  A NaN that is MOVED (a record byte, a miss value, the NaN of var at n == 1, which the header
fixes as the quiet NaN 0x7FF8000000000000) is compared bit for bit.  A NaN that an invalid operation
GENERATES -- 0 / 0 in a TargetEncoding value with p_smooth = 0, sqrt of a negative variance -- has
no sign or payload in IEEE 754 (section 6.3 leaves the sign of such a result open: x86 sets it,
other machines clear it), so the references report WHERE they generated one (``free`` masks) and a
test asks for a NaN there, whatever its bits.  Infinities and every other value keep their bits.
"""
from fractions import Fraction

import numpy as np

I32_MIN, I32_MAX = -(2**31), 2**31 - 1
KINDS = {"count": 0, "sum": 1, "mean": 2, "min": 3, "max": 4, "var": 5, "std": 6}   # include/nvt_hip.h
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def pack_bits(bits) -> np.ndarray:
    """Arrow validity bitmap (LSB first) of a boolean array, padded to whole 64-bit words."""
    bits = np.asarray(bits, dtype=bool)
    out = np.zeros((bits.size + 63) // 64 * 8, np.uint8)
    p = np.packbits(bits, bitorder="little")
    out[:p.size] = p
    return out


# ---------------------------------------------------------------------------------------------
# key -> position
# ---------------------------------------------------------------------------------------------
def position(ids, rows, valid=None, key_offset=0, null_group=-1) -> np.ndarray:
    """int64 position of every row's key in the ascending duplicate-free int32 list ``ids`` or -1.

    The list key is ``row - key_offset`` evaluated in Python integers (an int64 subtraction that
    overflows cannot wrap into the list); a value outside int32 misses; a row whose validity bit
    is cleared takes ``null_group`` whatever its bytes."""
    ids = np.asarray(ids)
    assert ids.dtype == np.int32 and ids.ndim == 1 and ids.size >= 1
    lst = ids.astype(np.int64)
    assert np.all(np.diff(lst) > 0), "the key list is ascending and duplicate-free"
    rows = np.asarray(rows)
    assert rows.dtype in (np.int32, np.int64)
    n = rows.size
    kv = rows.astype(object) - int(key_offset)                     # Python integers
    inside = np.fromiter((I32_MIN <= v <= I32_MAX for v in kv), bool, n)
    out = np.full(n, -1, np.int64)
    k = np.array([int(v) for v in kv[inside]], np.int64)
    pos = np.searchsorted(lst, k)
    pos_c = np.minimum(pos, lst.size - 1)
    out[inside] = np.where(lst[pos_c] == k, pos_c, -1)
    if valid is not None:
        out[~np.asarray(valid, dtype=bool)] = int(null_group)
    return out


def flat_positions(home) -> np.ndarray:
    """Slot of every entry of a flat table laid out from non-decreasing home slots:
    p_i = max(h_i, p_(i-1) + 1).  The reported displacement is max(p_i - h_i)."""
    home = np.asarray(home, dtype=np.int64)
    assert np.all(np.diff(home) >= 0)
    p = np.empty_like(home)
    last = -1
    for i, h in enumerate(home):
        last = max(int(h), last + 1)
        p[i] = last
    return p


def check_keydir(dir_words, ids, B) -> None:
    """The key directory of ``ids`` (ascending int32) with B buckets: uint32[4 * (B + 1)] entries
    {first, k0, k1, k2}; ``first`` runs monotone from 0 (entry 0) to n (entry B): bucket b holds
    the keys [first[b], first[b + 1]); k0..k2 are the bucket's first three keys, a shorter bucket
    repeats its last key, an empty one holds the next key of the list (the last key when there is
    none).  Raises AssertionError naming the first wrong field."""
    ids = np.asarray(ids)
    assert ids.dtype == np.int32
    n = ids.size
    d = np.asarray(dir_words)
    assert d.size == 4 * (B + 1), f"directory of {d.size} words for {B} buckets"
    d = d.view(np.uint32).reshape(B + 1, 4)
    first = d[:, 0].astype(np.int64)
    assert first[0] == 0, f"first[0] = {first[0]}"
    assert first[B] == n, f"first[{B}] = {first[B]}, {n} keys"
    down = np.flatnonzero(np.diff(first) < 0)
    assert down.size == 0, f"first decreases behind bucket {down[:1]}"
    cnt = np.diff(np.append(first, n))
    keys = d[:, 1:].view(np.int32)
    for j in range(3):
        # key j of the bucket, its last key when it is shorter, the list's next (or last) key when empty
        at = np.minimum(first + np.minimum(j, np.maximum(cnt - 1, 0)), n - 1)
        bad = np.flatnonzero(keys[:, j] != ids[at])
        assert bad.size == 0, (f"k{j} of bucket {bad[0]} (first {first[bad[0]]}, {cnt[bad[0]]} keys) is "
                               f"{keys[bad[0], j]}, expected {ids[at[bad[0]]]}")


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
def cast(x, out_dtype) -> np.ndarray:
    """ONE IEEE conversion float64 / int64 -> out dtype; to an integer type it truncates, and a
    NaN or a value out of range raises (the C ABI does not define those)."""
    out_dtype = np.dtype(out_dtype)
    x = np.asarray(x)
    with np.errstate(invalid="raise", over="ignore"):
        if out_dtype.kind == "i" and x.dtype.kind == "f":
            assert np.all(np.isfinite(x)), "NaN / inf to an integer type is undefined"
            info = np.iinfo(out_dtype)
            assert np.all((np.trunc(x) >= info.min) & (np.trunc(x) <= info.max)), "out of range"
        if out_dtype.kind == "i" and x.dtype.kind == "i":
            info = np.iinfo(out_dtype)
            assert np.all((x >= info.min) & (x <= info.max)), "out of range"
        return x.astype(out_dtype)


def jg_stats(count, sum_, sumsq, mn, mx, kind, out_dtype):
    """(values [groups] in out_dtype, free bool [groups]) of one statistic of one value column.

    count int64; sum / sumsq / mn / mx float64 or None when ``kind`` does not need them.  In
    float64, in this order: mean = sum / n; var = (sumsq - (sum * sum) / n) / max(n - 1, 1), the
    quiet NaN at n == 1; std = sqrt(var).  count converts from the integer itself.  ``free``:
    std of a negative variance (a generated NaN)."""
    kind = KINDS.get(kind, kind)
    count = np.asarray(count)
    assert count.dtype == np.int64
    free = np.zeros(count.size, bool)
    if kind == 0:
        return cast(count, out_dtype), free
    n = count.astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == 1:
            x = np.asarray(sum_, np.float64)
        elif kind == 2:
            x = np.asarray(sum_, np.float64) / n
        elif kind == 3:
            x = np.asarray(mn, np.float64)
        elif kind == 4:
            x = np.asarray(mx, np.float64)
        else:
            s1, s2 = np.asarray(sum_, np.float64), np.asarray(sumsq, np.float64)
            sq = s1 * s1
            num = s2 - sq / n
            dn = n - 1.0
            x = num / np.maximum(dn, 1.0)
            x = np.where(dn == 0.0, QNAN, x)
            if kind == 6:
                free = x < 0.0
                x = np.sqrt(x)
    return cast(x, out_dtype), free


def _te_terms(tot_count, tot_sum, fold_count, fold_sum, kfold):
    """[groups, kfold + 1] float64 of (S, s_f, C, c_f) with slot 0 = no fold (s_f = c_f = 0), and
    the bool ``rows`` = the slot's (group, fold) pair has rows (slot 0: always)."""
    C = np.asarray(tot_count)
    assert C.dtype == np.int64
    g = C.size
    S = np.asarray(tot_sum, np.float64)
    sf = np.zeros((g, kfold + 1))
    cf = np.zeros((g, kfold + 1))
    rows = np.ones((g, kfold + 1), bool)
    if kfold:
        fc = np.asarray(fold_count)
        assert fc.dtype == np.int64 and fc.size == g * kfold
        cf[:, 1:] = fc.reshape(g, kfold).astype(np.float64)
        sf[:, 1:] = np.asarray(fold_sum, np.float64).reshape(g, kfold)
        rows[:, 1:] = fc.reshape(g, kfold) > 0
    return np.broadcast_to(S[:, None], sf.shape), sf, np.broadcast_to(C.astype(np.float64)[:, None], sf.shape), cf, rows


def te_values(tot_count, tot_sum, fold_count, fold_sum, kfold, p, y_mean, out_dtype):
    """(values [groups, kfold + 1] in out_dtype, free bool of the same shape).  Slot 0 =
    (S + p * m) / (C + p); slot 1 + f = ((S - s_f) + p * m) / ((C - c_f) + p), or m where the
    (group, fold) pair has no rows.  kfold = 0: slot 0 only.  Every operation rounds on its own
    (no fused multiply-add).  ``free``: 0 / 0."""
    S, sf, C, cf, rows = _te_terms(tot_count, tot_sum, fold_count, fold_sum, kfold)
    p, m = np.float64(p), np.float64(y_mean)
    with np.errstate(all="ignore"):
        num = (S - sf) + p * m
        den = (C - cf) + p
        v = num / den
    free = rows & (num == 0.0) & (den == 0.0)
    v = np.where(rows, v, m)
    assert np.dtype(out_dtype).kind == "f"
    with np.errstate(all="ignore"):
        return v.astype(out_dtype), free


def te_values_exact(tot_count, tot_sum, fold_count, fold_sum, kfold, p, y_mean, out_dtype):
    """(E, bound): object arrays [groups, kfold + 1] of fractions.Fraction -- the values of
    te_values on the exact values of the float64 inputs, and the margin
        2^-52 * ((|S - s_f| + |p * m| + |num|) / |den| + 2 * |E|)   (+ 2^-24 * |E| for float32):
    about twice the first-order bound of the three roundings (subtraction, product or fused
    product-sum, division), which covers contracted and uncontracted code.  A slot without rows is
    m itself: its margin is the output cast alone.  den must not be 0."""
    S, sf, C, cf, rows = _te_terms(tot_count, tot_sum, fold_count, fold_sum, kfold)
    pf, mf = Fraction(float(p)), Fraction(float(y_mean))
    f32 = np.dtype(out_dtype) == np.float32
    E = np.empty(S.shape, object)
    bound = np.empty(S.shape, object)
    for idx in np.ndindex(*S.shape):
        if not rows[idx]:
            E[idx] = mf
            bound[idx] = abs(mf) * Fraction(1, 2**24) if f32 else Fraction(0)
            continue
        d = Fraction(float(S[idx])) - Fraction(float(sf[idx]))
        num = d + pf * mf
        den = Fraction(float(C[idx])) - Fraction(float(cf[idx])) + pf
        assert den != 0
        e = num / den
        b = Fraction(1, 2**52) * ((abs(d) + abs(pf * mf) + abs(num)) / abs(den) + 2 * abs(e))
        if f32:
            b += Fraction(1, 2**24) * abs(e)
        E[idx], bound[idx] = e, b
    return E, bound


def te_outside(got, E, bound):
    """Indices where a finite ``got`` lies further than ``bound`` from ``E`` (or is not finite)."""
    got = np.asarray(got)
    bad = []
    for idx in np.ndindex(*got.shape):
        x = float(got[idx])
        if not np.isfinite(x) or abs(Fraction(x) - E[idx]) > bound[idx]:
            bad.append(idx)
    return bad


# ---------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------
def read_image(image_bytes, stride, g, off, size, fold=None, miss_bits=0) -> np.ndarray:
    """uint32 / uint64 per row: the ``size`` (4 / 8) bytes at
    image[g][off + (fold is None ? 0 : (1 + fold[i]) * size)], ``miss_bits`` where g < 0."""
    img = np.asarray(image_bytes, np.uint8)
    g = np.asarray(g, np.int64)
    assert size in (4, 8) and off % size == 0
    at = np.full(g.size, off, np.int64)
    if fold is not None:
        at = at + (1 + np.asarray(fold).astype(np.int64)) * size
    hit = g >= 0
    assert np.all(at + size <= stride)
    start = np.where(hit, g, 0) * stride + at
    assert np.all(start[hit] + size <= img.size)
    word = img[start[:, None] + np.arange(size)[None, :]]
    ut = np.uint32 if size == 4 else np.uint64
    out = np.ascontiguousarray(word).view(ut).reshape(-1).copy()
    out[~hit] = ut(int(miss_bits) & ((1 << (8 * size)) - 1))
    return out


def _put(rec, free, groups, off, values, free_rows):
    values = np.ascontiguousarray(values)
    sz = values.dtype.itemsize
    assert off % sz == 0 and off + sz <= rec.shape[1], "value outside the record"
    rec[:groups, off:off + sz] = values.view(np.uint8).reshape(groups, sz)
    rows = np.flatnonzero(free_rows)
    if rows.size:
        free.append((rows, off, values.dtype))


def build_image(parts, records, stride, base=None):
    """(image uint8 [records * stride], free) of the one-pass build: every part writes its byte
    range of its first ``groups`` records, every other byte is zero -- or, with ``base`` (the
    image before the call), what it was: the per-operator builders nvt_jg_image / nvt_te_image
    leave the bytes outside their range alone.

    A JoinGroupby part: dict(kind="jg", groups, count, sum=[..], sumsq=[..] / None, mn, mx,
    outputs=[(statistic, value column, out dtype, byte offset)]); a TargetEncoding part:
    dict(kind="te", groups, tot_count, tot_sum, fold_count, fold_sum, kfold, p, y_mean, dtype,
    off[, moments=(count, sum)]) -- with ``moments`` the mean is sum / count correctly rounded.
    ``free``: [(record numbers, byte offset, dtype)] of generated NaNs (see the module docstring)."""
    if base is None:
        rec = np.zeros((records, stride), np.uint8)
    else:
        rec = np.array(base, np.uint8).reshape(records, stride)
    free = []
    for p in parts:
        g = int(p["groups"])
        assert g <= records, "a part with more groups than records"
        if g == 0:
            continue
        if p["kind"] == "jg":
            def col(name, j):
                arrs = p.get(name)
                return None if arrs is None or arrs[j] is None else np.asarray(arrs[j])[:g]
            for kind, j, dt, off in p["outputs"]:
                v, fr = jg_stats(np.asarray(p["count"])[:g], col("sum", j), col("sumsq", j), col("mn", j),
                                 col("mx", j), kind, dt)
                _put(rec, free, g, off, v, fr)
        else:
            kfold = int(p["kfold"])
            m = p["y_mean"]
            if p.get("moments") is not None:
                m = np.float64(p["moments"][1]) / np.float64(p["moments"][0])
            fc = None if not kfold else np.asarray(p["fold_count"])[:g * kfold]
            fs = None if not kfold else np.asarray(p["fold_sum"])[:g * kfold]
            v, fr = te_values(np.asarray(p["tot_count"])[:g], np.asarray(p["tot_sum"])[:g], fc, fs, kfold,
                              p["p"], m, p["dtype"])
            sz = v.dtype.itemsize
            for slot in range(kfold + 1):
                _put(rec, free, g, p["off"] + slot * sz, v[:, slot], fr[:, slot])
    return rec.reshape(-1), free


def image_mismatch(got, exp, free, stride):
    """None, or a message naming the first byte of ``got`` that differs from ``exp`` outside the
    generated NaNs of ``free`` / the first of those that is no NaN."""
    got = np.asarray(got, np.uint8).reshape(-1, stride)
    exp = np.asarray(exp, np.uint8).reshape(-1, stride)
    if got.shape != exp.shape:
        return f"{got.shape} records x bytes, expected {exp.shape}"
    open_ = np.zeros(exp.shape, bool)
    for rows, off, dt in free:
        sz = np.dtype(dt).itemsize
        open_[rows, off:off + sz] = True
        v = np.ascontiguousarray(got[rows, off:off + sz]).view(dt).reshape(-1)
        if not np.all(np.isnan(v)):
            r = rows[np.flatnonzero(~np.isnan(v))[0]]
            return f"record {r} offset {off}: a NaN expected, got {v[~np.isnan(v)][0]!r}"
    bad = np.argwhere((got != exp) & ~open_)
    if bad.size:
        r, b = bad[0]
        return (f"{len(bad)} bytes differ, first at record {r} byte {b}: got {got[r, b]:#04x}, expected "
                f"{exp[r, b]:#04x} (record got {got[r].tobytes().hex()} expected {exp[r].tobytes().hex()})")
    return None


def bits_mismatch(got, exp, free=None, what=""):
    """None, or a message: ``got`` and ``exp`` (same dtype and shape) differ in a bit outside
    ``free``, or ``got`` is no NaN somewhere inside it."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return f"{what}: {got.dtype}{got.shape}, expected {exp.dtype}{exp.shape}"
    ut = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = got.view(ut) != exp.view(ut)
    if free is not None:
        free = np.asarray(free, bool)
        if free.any() and not np.all(np.isnan(got[free])):
            return f"{what}: a NaN expected at {np.argwhere(free & ~np.isnan(got))[0]}"
        diff &= ~free
    if diff.any():
        i = tuple(np.argwhere(diff)[0])
        return (f"{what}: {int(diff.sum())} of {diff.size} differ, first at {i}: got {got[i]!r} "
                f"({int(got.view(ut)[i]):#x}), expected {exp[i]!r} ({int(exp.view(ut)[i]):#x})")
    return None
