"""``nvt_count_col.out_slots``: the range path of the counting stage (csrc/nvt_range_count.hip,
rp_count_kernel) records, for every entry of the key-ordered list it emits, the slot of the dumped
range table that holds the entry.  Checked here at 256 buckets through ``K.DenseCountJob`` /
``K.dense_count_many``:

  * out_slots[i] is 0xFFFFFFFF exactly for the entry of the smallest int32 (it owns no slot);
  * otherwise the low word of table[out_slots[i]] is out_keys[i] and its high word is i;
  * the slots are pairwise distinct, and they hold every key the table holds;
  * key list and counts equal numpy's.

The column is built so that entries leave their home slots.  The map sends (span of the keys) / 2^22
keys to each home slot -- more than 256 keys here -- so a run of consecutive integers shares one or two
home slots and all but those are displaced (RUN keys per run, several runs).  The largest keys of the
type form such a run as well: their home is the last slot of the last bucket, so the run continues
into the kRpTail slots behind the bucket's table, which the test asserts from the slots themselves."""
import zlib

import numpy as np
import pytest
import torch

import count_reference as R
import encode_reference as ER

pytestmark = pytest.mark.gpu

LO, HI = np.iinfo(np.int32).min, np.iinfo(np.int32).max
SLOTS, TAIL, GUARD = 16384, 128, 64          # kRpSlots, kRpTail, kRpGuard
REGION = SLOTS + TAIL
RUN = 40
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def column(n_rows, n_spread, runs, sentinel, nulls, seed):
    """(keys, validity or None): n_spread keys spread over [0, 2^31) under a power law, `runs` runs of
    RUN consecutive integers, the run HI - RUN + 1 .. HI, one key that takes a tenth of the rows."""
    rng = np.random.default_rng(zlib.crc32(repr(seed).encode()))
    spread = ((np.arange(1, n_spread + 1, dtype=np.int64) * 2654435761 + 12345) % (2**31))
    starts = rng.integers(-2**31 + 1000, 2**31 - 1000 - RUN, runs)
    run_keys = (starts[:, None] + np.arange(RUN)[None, :]).ravel()
    top = HI - np.arange(RUN, dtype=np.int64)
    pool = np.unique(np.concatenate([spread, run_keys, top]))
    pool = pool[pool != LO]
    assert n_rows >= 2 * pool.size and pool.max() - pool.min() >= 2**30
    rows = np.concatenate([pool, pool[np.minimum(rng.zipf(1.3, n_rows - pool.size) - 1, pool.size - 1)]])
    rows[rng.random(n_rows) < 0.1] = pool[pool.size // 2]          # a repeated key
    rows[:pool.size] = pool                                          # every key at least once
    rows = rng.permutation(rows)
    valid = None
    if sentinel:
        rows[rng.integers(0, n_rows, 5)] = LO
    if nulls:
        valid = rng.random(n_rows) >= 0.1
        idx = np.flatnonzero(~valid)
        rows[idx[0::2]] = LO                                         # bytes under null rows: the sentinel,
        rows[idx[1::2]] = rng.integers(LO, HI, idx[1::2].size)       # and keys that occur nowhere else
    return rows.astype(np.int32), valid


CASES = [("a few thousand rows", 6000, 1500, 4, False, False),
         ("sentinel", 60_000, 8000, 30, True, False),
         ("sentinel and null rows", 200_000, 20_000, 60, True, True),
         ("null rows, no sentinel row", 60_000, 8000, 30, False, True)]


@pytest.mark.parametrize("what,n_rows,n_spread,runs,sentinel,nulls", CASES, ids=[c[0] for c in CASES])
def test_slots_of_the_range_path(K, what, n_rows, n_spread, runs, sentinel, nulls):
    keys, valid = column(n_rows, n_spread, runs, sentinel, nulls, what)
    job = K.DenseCountJob(dev(keys), None if valid is None else dev(ER.pack_bits(valid)), None, hint=20_000,
                          min_range_bits=8)
    job.path = K.PATH_RANGE
    before = K.STATS["count_relaunches"]
    k, c, n_null, info = K.dense_count_many([job])[0]
    assert K.STATS["count_relaunches"] == before and info["path"] == K.PATH_RANGE, info
    assert info["range_bits"] == 8 and info["range_table"] is not None and info["range_slots"] is not None
    ek, ec, en = R.count_ref(keys, valid, None)
    hk, hc = k.cpu().numpy(), c.cpu().numpy()
    R.list_mismatch(hk, hc, ek, ec, what)
    assert n_null == en
    has_lo = bool(ek.size and ek[0] == LO)
    assert has_lo == sentinel, what      # (the smallest int32 under null rows is not a key)

    slots = info["range_slots"].cpu().numpy().view(np.uint32).astype(np.int64)
    assert slots.size == hk.size
    n_slots = 256 * REGION + GUARD
    table = info["range_table"].cpu().numpy().view(np.uint64)
    assert table.size == n_slots
    none = slots == NONE
    np.testing.assert_array_equal(none, hk == LO, err_msg=f"{what}: 0xFFFFFFFF exactly for the smallest int32")
    assert int(none.sum()) == int(has_lo)
    at = np.flatnonzero(~none)
    s = slots[at]
    assert s.min() >= 0 and s.max() < 256 * REGION, (what, s.min(), s.max())
    assert np.unique(s).size == s.size, f"{what}: two entries share a slot"
    words = table[s]
    ER.first_mismatch((words & 0xFFFFFFFF).astype(np.uint32).view(np.int32), hk[at], what + ": key in the slot")
    ER.first_mismatch((words >> 32).astype(np.int64), at.astype(np.int64), what + ": position in the slot")
    # ... and the table holds nothing else
    occupied = (table & 0xFFFFFFFF) != 0x80000000
    assert int(occupied.sum()) == s.size and not occupied[256 * REGION:].any(), what
    # the run at the top of the type reached the slots behind its bucket's table
    assert (s % REGION >= SLOTS).any(), f"{what}: no entry in the kRpTail slots"
