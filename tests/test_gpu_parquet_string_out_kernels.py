"""nvt_pq_str_entry_ids / nvt_pq_byte_array_plan / nvt_pq_byte_array_fill on the device against
tests/pq_str_out_reference.py, byte for byte: ids and the count of absent surrogates, pos and page_at,
every byte of the body, the guard bytes around every output and the bytes nobody may touch."""
import numpy as np
import pytest
import torch

import pq_str_out_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64
I64 = np.iinfo(np.int64)
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17]


def dev():
    return torch.device("cuda:0")


def t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _guards_hold(raw, used=None):
    h = raw.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[-GUARD:] == 0xA5).all()
    if used is not None:
        assert (h[GUARD + used: -GUARD] == 0xA5).all()
    return h


def _check(strings, surrogates, page_start, short=0):
    """The three entries for the values ``surrogates`` of a column whose dict is ``strings``, cut into
    pages at ``page_start``; ``short``: out_bytes is that much smaller than the body."""
    from nvtabular_amd import kernels_parquet_str_out as KSO

    keys, offsets, chars, _ = R.entry_table(strings)
    surrogates = np.asarray(surrogates, dtype=np.int64)
    page_start = np.asarray(page_start, dtype=np.int64)
    m = surrogates.size
    d_keys, d_off, d_chars = t(keys), t(offsets), t(chars)
    bad = torch.zeros(1, dtype=torch.int64, device=dev())
    ids = KSO.entry_ids(d_keys, t(surrogates), bad)
    ref_ids, ref_bad = R.entry_ids(keys, surrogates)
    np.testing.assert_array_equal(ids.cpu().numpy(), ref_ids)
    assert int(bad.cpu()[0]) == ref_bad
    pos, page_at, (pos_raw, at_raw) = KSO.plan(ids, d_off, t(page_start), guard=GUARD)
    ref_pos, ref_at = R.plan(ref_ids, offsets, page_start)
    _guards_hold(pos_raw)
    _guards_hold(at_raw)
    np.testing.assert_array_equal(pos.cpu().numpy(), ref_pos)
    np.testing.assert_array_equal(page_at.cpu().numpy(), ref_at)
    total = int(ref_pos[-1])
    out, raw = KSO.fill(ids, d_off, d_chars, pos, total - short, guard=GUARD, room=total)
    want = np.full(total + 2 * GUARD, 0xA5, dtype=np.uint8)
    R.fill(ref_ids, offsets, chars, ref_pos, want[GUARD: GUARD + total], out_bytes=total - short)
    got = raw.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    return ref_ids, ref_pos


def _dict(rng, E, lengths=LENGTHS):
    keys = np.unique(rng.integers(-2**62, 2**62, 2 * E + 8))[:E]
    words = ["".join(chr(c) for c in rng.integers(97, 123, lengths[i % len(lengths)])) for i in range(E)]
    return dict(zip(keys.tolist(), words))


def _pages(m, rng):
    """Cut points with an empty page first, in the middle and last."""
    a, b = sorted(rng.integers(0, m + 1, 2).tolist())
    return [0, 0, a, a, b, m, m]


@pytest.mark.parametrize("E", [1, 2, 1000])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 4097])
def test_sizes(m, E):
    rng = np.random.default_rng(1000 * m + E)
    strings = _dict(rng, E)
    sur = rng.choice(np.array(list(strings), dtype=np.int64), m)
    _check(strings, sur, [0, m])
    _check(strings, sur, _pages(m, rng))


def test_every_source_and_destination_alignment():
    """Entries of 1, 2, 3, ... bytes: their chars start at every residue mod 4, and behind a 4-byte
    length so do the values in the body."""
    rng = np.random.default_rng(2)
    strings = _dict(rng, 40, lengths=list(range(1, 41)))
    _, offsets, _, _ = R.entry_table(strings)
    assert set((offsets[:-1] % 4).tolist()) == {0, 1, 2, 3}
    sur = np.array(sorted(strings) * 3 + sorted(strings)[::-1], dtype=np.int64)
    _, pos = _check(strings, sur, [0, 7, 7, len(sur)])
    assert set((pos[:-1] % 4).tolist()) == {0, 1, 2, 3}


def test_one_long_entry_between_short_ones():
    rng = np.random.default_rng(3)
    long = "".join(chr(c) for c in rng.integers(97, 123, 100_000))
    strings = {-5: "a", 7: long, 9: "b"}
    _check(strings, [-5, 7, 9, 9, 7, -5, -5], [0, 3, 7])


def test_key_extremes_same_entry_and_all_distinct():
    strings = dict(zip([I64.min, -1, 0, 1, I64.max], ["min", "minus one", "", "one", "max"]))
    rng = np.random.default_rng(4)
    _check(strings, rng.choice(np.array(list(strings), dtype=np.int64), 500), [0, 100, 500])
    _check(strings, np.full(300, I64.max, dtype=np.int64), [0, 300])          # every value the same entry
    many = _dict(rng, 1000)
    _check(many, rng.permutation(np.array(list(many), dtype=np.int64)), [0, 1000])   # every value another entry


def test_absent_surrogates_are_counted():
    strings = {10: "ten", 20: "twenty", 30: "thirty"}
    sur = np.array([10, 11, 30, I64.min, I64.max, 20, 25, 20], dtype=np.int64)
    ids, _ = _check(strings, sur, [0, 8])                # (an absent one is written as entry 0)
    assert list(ids) == [0, 0, 2, 0, 0, 1, 0, 1]


def test_a_buffer_one_byte_short_loses_only_the_last_value():
    rng = np.random.default_rng(6)
    strings = _dict(rng, 50)
    sur = rng.choice(np.array(list(strings), dtype=np.int64), 777)
    _check(strings, sur, [0, 777], short=1)
    _check({1: ""}, [1, 1, 1], [0, 3], short=1)          # (the last value is only its length)


def test_positions_past_four_gib():
    """4100 values of one entry of 2^20 bytes: pos passes 2^32 (the plan only; no body is made)."""
    from nvtabular_amd import kernels_parquet_str_out as KSO

    offsets = np.array([0, 1 << 20], dtype=np.int64)
    ids = np.zeros(4100, dtype=np.int32)
    pos, page_at = KSO.plan(t(ids), t(offsets), t(np.array([0, 4096, 4100], dtype=np.int64)))
    ref_pos, ref_at = R.plan(ids, offsets, [0, 4096, 4100])
    assert ref_pos[-1] > 1 << 32
    np.testing.assert_array_equal(pos.cpu().numpy(), ref_pos)
    np.testing.assert_array_equal(page_at.cpu().numpy(), ref_at)
