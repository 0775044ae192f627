"""The numpy restatement of the partition entries (tests/partition_reference.py) on hand-written
cases, and the balance of the chosen finaliser on sequential tags.  No GPU."""
import numpy as np

import partition_reference as R


def test_mix_matches_integer_arithmetic():
    tags = [0, 1, 2, 63, 1 << 32, (1 << 63) + 5, (1 << 64) - 1, 0x243F6A8885A308D3]
    got = R.mix(np.array(tags, dtype=np.uint64))
    assert [int(x) for x in got] == [R.mix_int(t) for t in tags]
    assert R.mix_int(0) == 0
    assert R.mix_int(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF   # splitmix64's first output from seed 0
    # signed tags (torch keeps them as int64) are the same bits
    np.testing.assert_array_equal(R.mix(np.array([-1], dtype=np.int64).view(np.uint64)), R.mix(np.array([R.M64], dtype=np.uint64)))


def test_partition_ids_by_hand():
    tags = np.array([0, 1, 2, 12345, (1 << 64) - 1], dtype=np.uint64)
    for P in (1, 2, 3, 8, 4096):
        want = [(((R.mix_int(int(t)) >> 32) * P) >> 32) for t in tags]
        got = R.partition_ids(tags, P)
        assert got.dtype == np.uint32 and got.tolist() == want
        assert got.max() < P
    assert R.partition_ids(tags, 1).tolist() == [0] * 5
    # equal tags, equal ids
    rep = R.partition_ids(np.array([7, 9, 7, 9, 7], dtype=np.uint64), 64)
    assert rep[0] == rep[2] == rep[4] and rep[1] == rep[3]


def test_plan_is_a_stable_counting_sort():
    pid = np.array([2, 0, 2, 1, 0, 2, 2], dtype=np.uint32)
    perm, counts = R.plan(pid, 4)
    assert perm.tolist() == [1, 4, 3, 0, 2, 5, 6]
    assert counts.tolist() == [2, 1, 4, 0]
    perm, counts = R.plan(np.zeros(0, dtype=np.uint32), 3)
    assert perm.tolist() == [] and counts.tolist() == [0, 0, 0]
    perm, counts = R.plan(np.array([1, 0] * 4, dtype=np.uint32), 2)   # strictly alternating
    assert perm.tolist() == [1, 3, 5, 7, 0, 2, 4, 6] and counts.tolist() == [4, 4]


def test_bitmaps_pad_with_zero_bits():
    assert R.pack_bits([]).tolist() == []
    assert R.pack_bits([True]).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    b = R.pack_bits([True] * 65)
    assert len(b) == 16 and b[:8].tolist() == [255] * 8 and b[8:].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    m = np.array([True, False, True, True, False, False, False, True, True])
    assert R.pack_bits(m).tolist()[:2] == [0b10001101, 1]
    np.testing.assert_array_equal(R.unpack_bits(R.pack_bits(m), 9), m)


def test_gather_by_hand():
    a = np.array([10, 11, 12, 13], dtype=np.int64)
    b = np.array([20, 21, 22], dtype=np.int64)
    a_valid = R.pack_bits([True, False, True, True])
    vals, bitmap = R.gather([(a, a_valid, [3, 1]), (b, None, [0, 2]), (a, a_valid, [1])], True)
    assert vals.tolist() == [13, 11, 20, 22, 11]
    assert bitmap.tolist() == [0b01101, 0, 0, 0, 0, 0, 0, 0]
    vals, bitmap = R.gather([(a, None, [0]), (b, None, [])], False)
    assert vals.tolist() == [10] and bitmap is None
    vals, bitmap = R.gather([], True)
    assert len(vals) == 0 and len(bitmap) == 0


def test_finaliser_balances_sequential_tags():
    """Tags 0 .. 2^16 - 1 are the worst case for a weak finaliser.  The binomial spread of 65 536
    keys over 8 (3) partitions is about 1 %; max / mean <= 1.5 only catches a degenerate mix."""
    tags = np.arange(1 << 16, dtype=np.uint64)
    for P in (8, 3):
        counts = np.bincount(R.partition_ids(tags, P), minlength=P)
        ratio = counts.max() / counts.mean()
        print(f"P={P}: counts {counts.tolist()} max/mean {ratio:.4f}")
        assert counts.sum() == 1 << 16 and counts.min() > 0
        assert ratio <= 1.5
