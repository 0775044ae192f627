"""join_reference.py pinned to ``pandas.merge`` (no GPU): the composed reference
``canon -> group_rows -> probe -> exclusive_offsets -> expand -> gather`` equals
``left.merge(ext, how=...)`` in left-row order on frames of a few hundred rows, ``fmix64`` has the
documented known answers, and ``check_slots`` refuses the three ways a slot table can be wrong.  The
kernel-level tests of test_gpu_join_kernels.py compare the device with these references."""
import numpy as np
import pandas as pd
import pytest

import join_reference as R

INT, FLT = R.JOIN_INT, R.JOIN_FLOAT


def _pandas_col(values, valid):
    """A key component as pandas sees it: a cleared validity bit becomes NaN (the column float64)."""
    values = np.asarray(values)
    if valid is None:
        return values
    out = values.astype(np.float64)
    assert values.dtype.kind == "f" or (out.astype(np.int64)[valid] == values[valid]).all()
    out[~valid] = np.nan
    return out


def _check(left_keys, ext_keys, modes, how):
    """left_keys / ext_keys: (values, valid bool or None) per component.  Payload: the external row
    number (never null) and a float column with nulls; the left frame carries its row number."""
    nl, ne = len(left_keys[0][0]), len(ext_keys[0][0])
    rng = np.random.default_rng(nl * 1000 + ne)
    v = np.arange(ne, dtype=np.int64)
    w = rng.standard_normal(ne)
    w_valid = rng.random(ne) >= 0.25
    left = pd.DataFrame({f"k{j}": _pandas_col(*k) for j, k in enumerate(left_keys)})
    left["__r"] = np.arange(nl)
    ext = pd.DataFrame({f"k{j}": _pandas_col(*k) for j, k in enumerate(ext_keys)})
    ext["v"] = v
    ext["w"] = np.where(w_valid, w, np.nan)
    on = [f"k{j}" for j in range(len(modes))]
    # left-row order, external order within a key (pandas' inner merge does not always keep the latter
    # where -0.0 and 0.0 are one key; v is the external row number)
    exp = left.merge(ext, on=on, how=how).sort_values(["__r", "v"], kind="stable").reset_index(drop=True)

    left_row, ext_row, order, cols = R.join_ref(left_keys, ext_keys, modes, how == "inner", [(v, None), (w, w_valid)])
    (gv, gv_valid), (gw, gw_valid) = cols
    what = f"{how} {nl} x {ne} rows, modes {modes}"
    R.first_mismatch(left_row, exp["__r"].to_numpy().astype(np.int64), what + ": left rows")
    ev = exp["v"].to_numpy()
    R.first_mismatch(gv_valid, ~pd.isna(ev), what + ": matched")
    R.first_mismatch(gv[gv_valid], ev[gv_valid].astype(np.int64), what + ": external rows")
    R.first_mismatch(order[ext_row[ext_row >= 0]], gv[gv_valid], what + ": grouped positions")
    ew = exp["w"].to_numpy()
    R.first_mismatch(gw_valid, ~np.isnan(ew), what + ": payload validity")
    R.first_mismatch(gw[gw_valid], ew[gw_valid], what + ": payload values")
    assert not gw[ext_row < 0].any() and not gv[ext_row < 0].any(), what + ": the value of a miss is not 0"
    return exp


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("dup", [False, True], ids=["unique", "duplicates"])
def test_one_integer_key(how, dup):
    rng = np.random.default_rng(5 + dup)
    ek = rng.permutation(np.arange(0, 400, 2, dtype=np.int64))
    if dup:
        ek = rng.permutation(np.concatenate([ek, ek[::3], ek[::7], ek[::7]]))
    lk = rng.integers(-5, 405, 300).astype(np.int64)
    exp = _check([(lk, None)], [(ek, None)], (INT,), how)
    assert exp["v"].notna().any() and (how == "inner" or exp["v"].isna().any())
    if dup:
        assert exp["__r"].duplicated().any()


@pytest.mark.parametrize("how", ["left", "inner"])
def test_int32_against_int64_and_uint8(how):
    rng = np.random.default_rng(6)
    ek = np.concatenate([rng.permutation(np.arange(-100, 100, dtype=np.int64)), [2**31 - 1, -2**31, 2**40, 7, 7]])
    lk = np.concatenate([rng.integers(-120, 120, 250), [2**31 - 1, -2**31, -1]]).astype(np.int32)
    _check([(lk, None)], [(ek, None)], (INT,), how)
    lk8 = rng.integers(0, 256, 200).astype(np.uint8)      # 128 .. 255 are positive keys
    ek8 = np.arange(-128, 256, 3, dtype=np.int64)
    exp = _check([(lk8, None)], [(ek8, None)], (INT,), how)
    assert (exp["k0"] >= 128).any()


@pytest.mark.filterwarnings("ignore:You are merging on int and float columns")
@pytest.mark.parametrize("how", ["left", "inner"])
def test_float_with_nan_against_int(how):
    rng = np.random.default_rng(7)
    lk = rng.integers(0, 60, 300).astype(np.float64)
    lk[rng.random(300) < 0.2] = np.nan
    lk[::17] += 0.5
    ek = rng.permutation(np.concatenate([np.arange(0, 60, 2), np.arange(0, 60, 6)])).astype(np.int64)
    exp = _check([(lk, None)], [(ek, None)], (FLT,), how)
    if how == "left":
        assert exp["v"][np.isnan(exp["k0"])].isna().all()      # an integer table has no null key


@pytest.mark.parametrize("how", ["left", "inner"])
def test_nan_keys_match_nan_keys(how):
    rng = np.random.default_rng(8)
    lk = rng.integers(0, 20, 200).astype(np.float32)
    lk[rng.random(200) < 0.2] = np.nan
    ek = rng.integers(0, 30, 80).astype(np.float64)
    ek[[3, 40, 41]] = np.nan
    exp = _check([(lk, None)], [(ek, None)], (FLT,), how)
    assert exp["v"][np.isnan(exp["k0"])].notna().all()
    # the same nulls arriving by bitmap over integer garbage
    lv = ~np.isnan(lk)
    ev = ~np.isnan(ek)
    li = np.where(lv, lk, rng.integers(0, 20, 200)).astype(np.int32)
    ei = np.where(ev, ek, 0).astype(np.int64)                  # 0 is also a real key
    _check([(li, lv)], [(ei, ev)], (INT,), how)


@pytest.mark.parametrize("how", ["left", "inner"])
def test_negative_zero_matches_zero(how):
    lk = np.array([0.0, -0.0, 1.0, -1.0, np.nan, -0.0], dtype=np.float64)
    ek = np.array([-0.0, 1.0, 5.0], dtype=np.float32)
    exp = _check([(lk, None)], [(ek, None)], (FLT,), how)
    assert exp["v"].notna().sum() == 4
    ek = np.array([0.0, -0.0, 2.0], dtype=np.float64)          # both zeros on the external side: one key
    exp = _check([(lk, None)], [(ek, None)], (FLT,), how)
    assert exp["v"].notna().sum() == 6


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("nkeys", [2, 3])
def test_several_components_with_nulls_on_both_sides(how, nkeys):
    rng = np.random.default_rng(9 + nkeys)
    nl, ne = 400, 150

    def side(n):
        a = rng.integers(0, 4, n).astype(np.int64)
        b = rng.integers(0, 3, n).astype(np.float64)
        b[rng.random(n) < 0.25] = np.nan
        c = rng.integers(0, 3, n).astype(np.int32)
        cv = rng.random(n) >= 0.25
        c[~cv] = rng.integers(-9, 9, int((~cv).sum()))          # garbage under the nulls
        return [(a, None), (b, None), (c, cv)][:nkeys]

    modes = (INT, FLT, INT)[:nkeys]
    exp = _check(side(nl), side(ne), modes, how)
    null_key = exp[[f"k{j}" for j in range(1, nkeys)]].isna().any(axis=1)
    assert exp["v"][null_key].notna().any(), "no null key found its match"
    assert len(exp) > nl or how == "inner"
    # a permutation of the components is another key
    left = [(np.array([1, 2], np.int64), None), (np.array([2.0, 1.0]), None)]
    ext = [(np.array([2], np.int64), None), (np.array([1.0]), None)]
    lr, er, _, _ = R.join_ref(left, ext, (INT, FLT), True, [])
    assert lr.tolist() == [1] and er.tolist() == [0]


@pytest.mark.parametrize("how", ["left", "inner"])
def test_empty_tables(how):
    k = np.arange(10, dtype=np.int64)
    none = np.empty(0, np.int64)
    _check([(none, None)], [(k, None)], (INT,), how)
    _check([(k, None)], [(none, None)], (INT,), how)
    _check([(none, None)], [(none, None)], (INT,), how)
    f = np.empty(0, np.float64)
    _check([(k, None), (k.astype(np.float64), None)], [(none, None), (f, None)], (INT, FLT), how)


def test_canon_edges():
    nan = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF],
                   np.uint64).view(np.float64)
    w, nl = R.canon(nan, np.float64, FLT, None)
    assert nl.all() and not w.any()
    x = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324], np.float64)
    w, nl = R.canon(x, np.float64, FLT, None)
    assert not nl.any()
    assert w.tolist() == [0, 0, 0x7FF0000000000000, 0xFFF0000000000000, 1, 0x8000000000000001]
    w, _ = R.canon(np.array([1.1], np.float32), np.float32, FLT, None)
    assert w[0] == np.array([np.float64(np.float32(1.1))]).view(np.uint64)[0] != np.array([1.1]).view(np.uint64)[0]
    # int64 beyond 2^53 under JOIN_FLOAT: 2^53 and 2^53 + 1 are one key; by value they are two
    big = np.array([2**53, 2**53 + 1, -2**63, 2**63 - 1], np.int64)
    w, _ = R.canon(big, np.int64, FLT, None)
    assert w[0] == w[1] and w[3] == np.array([2.0**63]).view(np.uint64)[0]
    w, _ = R.canon(big, np.int64, INT, None)
    assert w.tolist() == [2**53, 2**53 + 1, 2**63, 2**63 - 1]
    w, _ = R.canon(np.array([-1], np.int32), np.int32, INT, None)
    assert w[0] == 2**64 - 1
    w, _ = R.canon(np.array([200, 255], np.uint8), np.uint8, INT, None)
    assert w.tolist() == [200, 255]
    w, _ = R.canon(np.array([200], np.uint8), np.uint8, FLT, None)
    assert w[0] == np.array([200.0]).view(np.uint64)[0]
    w, nl = R.canon(np.array([7, 8, 9], np.int64), np.int64, INT, np.array([True, False, True]))
    assert w.tolist() == [7, 0, 9] and nl.tolist() == [False, True, False]
    with pytest.raises(AssertionError):
        R.canon(np.array([1.0]), np.float64, INT, None)


def test_fmix64_known_answers():
    """The documented hash (murmur3 fmix64): the known answers of test_oracle_golden.py."""
    got = R.fmix64(np.array([0, 1, 2**64 - 1], np.uint64))
    assert got.tolist() == [0, 0xB456BCFC34C2CB2C, 0x64B5720B4B825F21]
    import oracle as O

    x = np.random.default_rng(0).integers(-2**63, 2**63 - 1, 1000)
    np.testing.assert_array_equal(R.fmix64(x.view(np.uint64)), O.nvt_hash64(x))
    assert R.home_slot(np.array([1], np.uint64), 64)[0] == 0xB456BCFC34C2CB2C & 63
    assert R.home_slot(np.array([1], np.uint64), 2)[0] == 0


def test_offsets_expand_gather():
    c = np.array([0, 0, 3, 0, 1, 0], np.uint32)
    off = R.exclusive_offsets(c)
    assert off.dtype == np.uint64 and off.tolist() == [0, 0, 0, 3, 3, 4]
    big = R.exclusive_offsets(np.array([2**31, 2**31, 5, 0], np.uint32))
    assert big.tolist() == [0, 2**31, 2**32, 2**32 + 5]
    left, ext = R.expand(off, np.array([9, 9, 20, 9, -1], np.int64), 4)
    assert left.tolist() == [2, 2, 2, 4] and ext.tolist() == [20, 21, 22, -1]
    vals, valid = R.gather([2, -1, 0, 2], np.array([5, 6, 7], np.int32), np.array([True, True, False]))
    assert vals.tolist() == [7, 0, 5, 7] and valid.tolist() == [False, False, True, False] and vals.dtype == np.int32
    vals, valid = R.gather([2, -1], np.array([5, 6, 7], np.uint8), None)
    assert vals.tolist() == [7, 0] and valid.tolist() == [True, False]


# ---------------------------------------------------------------------------------------------
# check_slots
# ---------------------------------------------------------------------------------------------
EMPTY = (-(1 << 63)) & R.MASK64


def _table(capacity, tags, first, count):
    """A sequential linear-probing insert on the host."""
    slots = np.zeros((capacity, 2), np.uint64)
    slots[:, 0] = np.uint64(EMPTY)
    for t, f, c in zip(tags, first, count):
        h = int(R.home_slot(np.uint64(t), capacity)[0])
        while slots[h, 0] != np.uint64(EMPTY):
            h = (h + 1) % capacity
        slots[h] = (t, f | (c << 32))
    return slots


def _case():
    rng = np.random.default_rng(12)
    tags = np.unique(rng.integers(0, 2**63, 40).astype(np.uint64))[:32]
    first = np.arange(32, dtype=np.uint32) * 3
    count = (1 + np.arange(32) % 5).astype(np.uint32)
    return tags, first, count, _table(64, tags.tolist(), first.tolist(), count.tolist())


def test_check_slots_accepts_any_insertion_order():
    tags, first, count, slots = _case()
    R.check_slots(slots, 64, EMPTY, tags, first, count)
    p = np.random.default_rng(1).permutation(32)
    other = _table(64, tags[p].tolist(), first[p].tolist(), count[p].tolist())
    R.check_slots(other, 64, EMPTY, tags, first, count)
    R.check_slots(other.view(np.int64), 64, EMPTY - (1 << 64), tags, first, count)   # int64 views, as torch holds them
    R.check_slots(_table(2, [], [], []), 2, EMPTY, [], [], [])


def test_check_slots_rejects_a_duplicated_tag():
    tags, first, count, slots = _case()
    free = np.flatnonzero(slots[:, 0] == np.uint64(EMPTY))
    used = np.flatnonzero(slots[:, 0] != np.uint64(EMPTY))
    slots[int(free[0])] = slots[int(used[0])]
    with pytest.raises(AssertionError, match="in slots"):
        R.check_slots(slots, 64, EMPTY, tags, first, count)


def test_check_slots_rejects_an_entry_behind_an_empty_slot():
    tags, first, count, slots = _case()
    p = int(np.flatnonzero(slots[:, 0] != np.uint64(EMPTY))[0])
    t = int(slots[p, 0])
    h = int(R.home_slot(np.uint64(t), 64)[0])
    # move the entry past the first empty slot behind its home
    q = h
    while slots[q, 0] != np.uint64(EMPTY):
        q = (q + 1) % 64
    q2 = (q + 1) % 64
    while slots[q2, 0] != np.uint64(EMPTY):
        q2 = (q2 + 1) % 64
    slots[q2] = slots[p]
    slots[p] = (EMPTY, 0)
    with pytest.raises(AssertionError, match="behind the empty slot"):
        R.check_slots(slots, 64, EMPTY, tags, first, count)


def test_check_slots_rejects_an_overwritten_empty_slot_and_wrong_contents():
    tags, first, count, slots = _case()
    free = int(np.flatnonzero(slots[:, 0] == np.uint64(EMPTY))[0])
    bad = slots.copy()
    bad[free, 1] = 1 << 32
    with pytest.raises(AssertionError, match="was overwritten"):
        R.check_slots(bad, 64, EMPTY, tags, first, count)
    bad = slots.copy()
    bad[free] = (12345, 0)                                     # a tag of no group
    with pytest.raises(AssertionError):
        R.check_slots(bad, 64, EMPTY, tags, first, count)
    used = int(np.flatnonzero(slots[:, 0] != np.uint64(EMPTY))[0])
    bad = slots.copy()
    bad[used, 1] += np.uint64(1)                               # first off by one
    with pytest.raises(AssertionError, match="first, count"):
        R.check_slots(bad, 64, EMPTY, tags, first, count)
    bad = slots.copy()
    bad[used] = (EMPTY, 0)                                     # a group that was never inserted
    with pytest.raises(AssertionError):
        R.check_slots(bad, 64, EMPTY, tags, first, count)
