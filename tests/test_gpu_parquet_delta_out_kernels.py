"""kernels_parquet_delta_out.encode against tests/delta_reference.py: every page's region decodes to the
page's values, has the reference's length, zero width bytes for absent miniblocks, and no store leaves
the output buffers.  The chunk rule runs on the device, so every cut ends with a page of FILL constant
values: the chunk then pays whatever the pages under test hold."""
import numpy as np
import pytest
import torch

import delta_reference as R

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 1024
# values per page: none, header only, one delta, one / two miniblocks, exactly one block, one block and
# one delta, several blocks with a short last one, and a cut of different pages around an empty one
CUTS = [[0], [1], [2], [33], [34], [129], [130], [128 * 3 + 20], [130, 0, 35, 128 * 3 + 20]]


def _data(kind, n, dt):
    info, rng, k = np.iinfo(dt), np.random.default_rng(n), np.arange(n)
    if kind == "constant":                 # all widths 0
        return np.full(n, 7, dtype=dt)
    if kind == "arithmetic":               # widths 0, min_delta != 0
        return (1000 - 3 * k).astype(dt)
    if kind == "steps":                    # small random steps
        return np.cumsum(rng.integers(-5, 60, n)).astype(dt)
    if kind == "minmax":                   # wrap-around: the deltas are -1 and +1 modulo 2^bits; 10-byte first value
        return np.where(k % 2 == 0, info.min, info.max).astype(dt)
    if kind == "fullwidth":                # deltas alternate type-max / type-min: width 32 / 64, 10-byte min_delta
        with np.errstate(over="ignore"):
            return np.cumsum(np.where(k % 2 == 0, info.max, info.min).astype(dt), dtype=dt)
    assert kind == "wide"                  # one wide miniblock (deltas 39 .. 60) among constant ones
    v = np.full(n, -5, dtype=dt)
    v[40:61] = rng.integers(info.min, info.max, len(v[40:61]), dtype=dt)
    return v


def _encode(vals, counts):
    """-> (the DeviceDelta after its read-back, the host's packed buffer with its guards)"""
    from nvtabular_amd import kernels_parquet_delta_out as KDO

    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dev = torch.device("cuda:0")
    dl = KDO.encode(torch.from_numpy(vals).to(dev), torch.from_numpy(starts).to(dev), guard=GUARD)
    raw = [r.cpu().numpy() for r in dl.raw]
    for r in raw:
        assert (r[:GUARD] == 0xA5).all() and (r[-GUARD:] == 0xA5).all(), "a store outside the output buffer"
    device_pays = int(dl.table[1])
    dl.take_words([dl.table.cpu().numpy(), starts])   # (raises when the host's verdict is not the device's)
    assert dl.pays == bool(device_pays)
    return dl, raw[0]


@pytest.mark.parametrize("kind", ["constant", "arithmetic", "steps", "minmax", "fullwidth", "wide"])
@pytest.mark.parametrize("counts", CUTS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_regions_match_the_reference(dt, counts, kind):
    bits = 8 * np.dtype(dt).itemsize
    counts = counts + [FILL]
    vals = np.concatenate([_data(kind, c, dt) for c in counts[:-1]] + [np.zeros(FILL, dtype=dt)])
    dl, raw = _encode(vals, counts)
    assert dl.pays
    packed = raw[GUARD: len(raw) - GUARD]
    assert dl.used <= len(packed) and (dl.at % 16 == 0).all()
    for p, (a, n, lo) in enumerate(zip(dl.at, dl.lengths, dl.starts)):
        page, region = vals[lo: lo + counts[p]], packed[a: a + n]
        ref = np.frombuffer(R.encode(page, bits), dtype=np.uint8)
        assert n == len(ref), (p, n, len(ref))
        np.testing.assert_array_equal(R.decode(region.tobytes(), bits), page, err_msg=f"page {p}")
        # the reference writes 0xFF as the width of a miniblock that holds no delta, the device 0; all else is equal
        deltas = max(counts[p] - 1, 0)
        absent = (4 - -(-(deltas % 128 or 128) // 32)) if deltas else 0
        diff = np.flatnonzero(region != ref)
        assert len(diff) == absent and (ref[diff] == 0xFF).all() and (region[diff] == 0).all(), (p, diff)
        if p + 1 < len(dl.at):   # the bytes up to the next region are not written
            assert (packed[a + n: dl.at[p + 1]] == 0xA5).all()
    assert (packed[dl.at[-1] + dl.lengths[-1]:] == 0xA5).all()


@pytest.mark.parametrize("dt", [np.int32, np.int64])
@pytest.mark.parametrize("pays", [False, True])
def test_the_chunk_rule_runs_on_the_device(dt, pays):
    """A full-range random chunk leaves the packed buffer unwritten; an arithmetic one fills it."""
    info, counts = np.iinfo(dt), [1000, 0, 1300]
    vals = (np.arange(2300) * 17).astype(dt) if pays else \
        np.random.default_rng(5).integers(info.min, info.max, 2300, dtype=dt)
    dl, raw = _encode(vals, counts)
    assert dl.pays == pays
    if not pays:
        assert (raw == 0xA5).all()
        return
    for a, n, lo, c in zip(dl.at, dl.lengths, dl.starts, counts):
        region = raw[GUARD + a: GUARD + a + n]
        np.testing.assert_array_equal(R.decode(region.tobytes(), 8 * np.dtype(dt).itemsize), vals[lo: lo + c])
