"""nvt_pq_dict_build / nvt_pq_dict_pack on the device against tests/pq_dict_reference.py, bit for bit:
the dictionary, d, every packed byte with the pad bits and pad bytes, the guard bytes and the parts
of the buffers nobody may touch."""
import numpy as np
import pytest
import torch

import pq_dict_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64
I64 = np.iinfo(np.int64)


def dev():
    return torch.device("cuda:0")


def _check(values, page_start, max_entries=None):
    """encode() of the values cut at page_start against the reference -> the DeviceDict."""
    from nvtabular_amd import kernels_parquet_dict as KPD

    values = np.ascontiguousarray(values)
    page_start = np.asarray(page_start, dtype=np.int64)
    kw = {} if max_entries is None else dict(max_entries=max_entries)
    dd = KPD.encode(torch.from_numpy(values).to(dev()), torch.from_numpy(page_start).to(dev()), guard=GUARD, **kw)
    (d, overflow, ps), = KPD.read_back_states([dd])
    torch.cuda.synchronize()
    dic, W, nv, packed = R.encode(values, page_start)
    assert overflow == 0 and d == len(dic)
    np.testing.assert_array_equal(ps, page_start)
    dict_raw, packed_raw, state_raw = [r.cpu().numpy() for r in dd.raw]
    for raw in (dict_raw, packed_raw, state_raw):
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    got = dict_raw[GUARD:-GUARD].view(values.dtype)
    np.testing.assert_array_equal(got[:d], dic)
    assert (dict_raw[GUARD + d * values.itemsize: -GUARD] == 0xA5).all()     # nothing behind the d entries
    body = packed_raw[GUARD:-GUARD]
    assert body[:len(packed)].tobytes() == packed
    assert (body[len(packed):] == 0xA5).all()                               # nothing behind the last page's padding
    return dd


def _pages(n, rng, k):
    """k + 1 ascending cut points of n values: not multiples of 8 or of the tile, some pages empty."""
    cuts = np.sort(rng.integers(0, n + 1, size=max(k - 1, 0)))
    ps = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    if k >= 3:
        ps[2] = ps[1]                                                       # a page of 0 values
    return ps


@pytest.mark.parametrize("dt", [np.int32, np.int64])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_sizes(n, dt):
    rng = np.random.default_rng(n)
    values = rng.integers(-50, 50, size=n).astype(dt)
    _check(values, [0, n])
    _check(values, _pages(n, rng, 5))


@pytest.mark.parametrize("dt", [np.int32, np.int64])
@pytest.mark.parametrize("W", [1, 2, 3, 7, 8, 9, 16])
def test_widths(W, dt):
    """d = 2^(W-1) + 1 distinct values need exactly W bits (W = 1: two values)."""
    d = 2 if W == 1 else (1 << (W - 1)) + 1
    rng = np.random.default_rng(W)
    info = np.iinfo(dt)
    base = np.unique(rng.integers(info.min, info.max, size=2 * d + 8, dtype=dt))[:d]
    values = np.concatenate([base, rng.choice(base, size=2100)])[rng.permutation(d + 2100)]
    assert R.index_width(len(np.unique(values))) == W
    _check(values, _pages(len(values), rng, 4))


@pytest.mark.parametrize("dt,d,W", [(np.int32, (1 << 16) + 1, 17), (np.int64, (1 << 16) + 1, 17),
                                    (np.int64, (1 << 17) + 1, 18), (np.int64, (1 << 19) + 1, 20)])
def test_wide_indices(dt, d, W):
    """Indices wider than 16 bits: 2^16 + 1 distinct values are the first to need 17 bits, 2^17 + 1
    need 18 and 2^19 + 1 need 20, the widest index a dictionary of 2^20 entries has."""
    assert R.index_width(d) == W
    rng = np.random.default_rng(W)
    values = (rng.permutation(d).astype(np.int64) * 7919 - 12345).astype(dt)    # d distinct values, unordered
    assert len(np.unique(values)) == d
    _check(values, [0, 2049, 2049, d - 3, d])


def test_all_values_equal_and_extremes():
    _check(np.full(3000, -7, dtype=np.int64), [0, 11, 3000])
    _check(np.full(100, np.iinfo(np.int32).min, dtype=np.int32), [0, 100])
    rng = np.random.default_rng(1)
    ext = np.array([I64.min, -1, 0, I64.max], dtype=np.int64)
    _check(rng.choice(ext, size=4099), [0, 5, 2100, 4099])
    _check(np.array([I64.max], dtype=np.int64), [0, 1])                        # the table's empty marker alone
    ext32 = np.array([np.iinfo(np.int32).min, -1, 0, np.iinfo(np.int32).max], dtype=np.int32)
    _check(rng.choice(ext32, size=777), [0, 777])


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_values_that_share_a_home_slot(dt):
    """Hundreds of distinct values whose home slot in the table is the same one (and the slots next to
    it): long probe sequences in build and pack."""
    from nvtabular_amd import kernels_parquet_dict as KPD

    n = 3000
    nslots = KPD.table_slots(n)
    cand = np.arange(-2_000_000, 2_000_000, dtype=dt)
    home = KPD.home_slot(cand, nslots)
    crowd = np.concatenate([cand[home == h][:150] for h in (5, 6, nslots - 1)])  # (the last slot wraps around)
    assert len(crowd) >= 300 and len(np.unique(KPD.home_slot(crowd, nslots))) == 3
    rng = np.random.default_rng(2)
    values = rng.choice(crowd, size=n).astype(dt)
    assert KPD.table_slots(len(values)) == nslots
    _check(values, [0, 1000, n])


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_overflow_leaves_the_outputs_alone(dt):
    """17 distinct values at max_entries = 16: overflow is set, nothing is packed and the dictionary
    buffer (16 entries) keeps its guards."""
    from nvtabular_amd import kernels_parquet_dict as KPD

    rng = np.random.default_rng(3)
    values = rng.permutation(np.repeat(np.arange(17, dtype=dt) * 1000 - 8000, 300))
    dd = KPD.encode(torch.from_numpy(values).to(dev()), torch.tensor([0, 2500, len(values)], device=dev()),
                    max_entries=16, guard=GUARD)
    (d, overflow, _), = KPD.read_back_states([dd])
    torch.cuda.synchronize()
    assert overflow & 1
    dict_raw, packed_raw, state_raw = [r.cpu().numpy() for r in dd.raw]
    assert dict_raw.size == 16 * values.itemsize + 2 * GUARD                 # no room past 16 entries ...
    for raw in (dict_raw, packed_raw, state_raw):
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()  # ... and nothing written there
    assert (packed_raw == 0xA5).all()                                        # the packed buffer is untouched
    # 16 distinct values at the same limit are a dictionary
    _check(values[values != values.max()], [0, 100, 4800], max_entries=16)


def test_a_bad_page_table_writes_nothing():
    from nvtabular_amd import kernels_parquet_dict as KPD

    values = torch.arange(100, device=dev(), dtype=torch.int64) % 7
    for ps in ([0, 60, 50, 100], [0, 101], [-1, 100]):
        dd = KPD.encode(values, torch.tensor(ps, device=dev()), guard=GUARD)
        (d, overflow, _), = KPD.read_back_states([dd])
        torch.cuda.synchronize()
        assert d == 7 and overflow == 2
        assert (dd.raw[1].cpu().numpy() == 0xA5).all()
