"""nvt_snappy_plan_many / nvt_snappy_compress_many / nvt_snappy_gather_many on the device, called
through kernels_snappy: every fragment's stream decodes (tests/snappy_reference.py, no copy in front
of the fragment) to exactly its source bytes, every page's dense stream behind its varint is
decompressed by pyarrow to the page's bytes, the reported sizes are the stream lengths, the bytes
behind every stream and around every buffer stay untouched, and two runs give the same bytes.

Two caps keep a parse that finds nothing from passing: n >= 4096 zero bytes take at most n / 16
bytes (a copy of 64 bytes costs 3), and the int64 label fixture at most 2.0 x what pyarrow's codec
makes of the same bytes (pyarrow 25.0.0: 76,587 of 262,144 bytes; the CPU model of the parse:
103,728, 1.35 x; a literal-only stream: 3.4 x)."""
import numpy as np
import pyarrow as pa
import pytest
import torch

import snappy_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64
FRAG = 32768
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 4095, FRAG - 1, FRAG, FRAG + 1, 3 * FRAG + 7]


def dev():
    return torch.device("cuda:0")


def _region(data, cuts=None, unit=1, elem=8, shift=0):
    """(Region, the region's bytes, page cuts in bytes): ``cuts`` in units of ``unit``; ``shift``: the
    byte offset of the region in its allocation."""
    from nvtabular_amd import kernels_snappy as KS

    data = bytes(data)
    assert len(data) % unit == 0
    cuts = [0, len(data) // unit] if cuts is None else list(cuts)
    buf = np.zeros(shift + len(data) + 8, dtype=np.uint8)
    buf[shift: shift + len(data)] = np.frombuffer(data, dtype=np.uint8)
    src = torch.from_numpy(buf).to(dev())[shift: shift + len(data)]
    ps = torch.tensor(cuts, dtype=torch.int64, device=dev())
    room = KS.SLOT_BYTES * KS.max_frags(len(data), len(cuts) - 1)
    return KS.Region(src, ps, unit, elem, room), data, [c * unit for c in cuts]


def _run(specs, slot_cap=None):
    from nvtabular_amd import kernels_snappy as KS

    ds = KS.compress([s[0] for s in specs], slot_cap or KS.SLOT_BYTES, guard=GUARD)
    got = KS.read_back(ds, release=False)
    torch.cuda.synchronize()
    return ds, got


def _host(ds):
    return dict(table=ds.frag_table.cpu().numpy(), size=ds.frag_size.cpu().numpy(), pos=ds.frag_pos.cpu().numpy(),
                slots=ds.slots.cpu().numpy(), dense=[d.cpu().numpy() for d in ds.dense],
                raw=[[x.cpu().numpy() for x in grp] if isinstance(grp, list) else [grp.cpu().numpy()]
                     for grp in ds.raw])


def _guards_hold(h):
    for grp in h["raw"]:
        for raw in grp:
            assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()


def _check(specs, ds, got, h):
    """Everything the module's docstring promises, for one call; -> the total of every region."""
    from nvtabular_amd import kernels_snappy as KS

    _guards_hold(h)
    cap = ds.slot_cap
    codec = pa.Codec("snappy")
    totals = []
    for i, ((region, data, cuts), ps) in enumerate(zip(specs, got)):
        assert ps.error == 0
        base, nf = ds.frag_base[i], KS.max_frags(len(data), len(cuts) - 1)
        recs = h["table"][base: base + nf]
        used = recs[recs[:, 1] > 0]
        assert len(used) == ps.frags and (used[:, 3] == i).all()
        per_page = np.zeros(len(cuts) - 1, dtype=np.int64)
        covered = 0
        for e in range(base, base + nf):
            at, ln, page, _ = (int(x) for x in h["table"][e])
            size = int(h["size"][e])
            slot = h["slots"][e * cap: (e + 1) * cap]
            assert (slot[size:] == 0xA5).all()            # nothing behind the stream
            if ln == 0:
                assert size == 0
                continue
            assert 0 < ln <= FRAG and cuts[page] <= at and at + ln <= cuts[page + 1]   # never straddles a page
            assert (at - cuts[page]) % FRAG == 0
            assert R.decode_elements(slot[:size].tobytes(), ln, floor=0) == data[at: at + ln]
            per_page[page] += size
            covered += ln
        assert covered == len(data)
        np.testing.assert_array_equal(ps.sizes, per_page)
        assert ps.total == int(per_page.sum())
        assert int(h["pos"][base + nf] - h["pos"][base]) == ps.total
        dense, at = h["dense"][i], 0
        for p, c in enumerate(per_page.tolist()):
            U = cuts[p + 1] - cuts[p]
            stream = dense[at: at + c].tobytes()
            if U:
                assert codec.decompress(R.varint(U) + stream, decompressed_size=U).to_pybytes() == data[cuts[p]: cuts[p + 1]]
            else:
                assert c == 0
            at += c
        assert (dense[ps.total:] == 0xA5).all()           # nothing behind the last page
        totals.append(ps.total)
    return totals


def _go(specs):
    ds, got = _run(specs)
    h = _host(ds)
    totals = _check(specs, ds, got, h)
    ds2, got2 = _run(specs)
    h2 = _host(ds2)
    assert h["slots"].tobytes() == h2["slots"].tobytes() and h["size"].tobytes() == h2["size"].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(h["dense"], h2["dense"]))
    assert [g.total for g in got] == [g.total for g in got2]
    return totals


def _period(n, k, rng):
    unit = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    return (unit * (n // k + 1))[:n]


@pytest.mark.parametrize("n", SIZES)
def test_region_sizes_and_contents(n):
    """One call, one region per content: zeros, random bytes, periods 1 / 3 / 5 / 7 (overlapping copies)."""
    rng = np.random.default_rng(n)
    contents = [bytes(n), rng.bytes(n)] + [_period(n, k, rng) for k in (1, 3, 5, 7)]
    totals = _go([_region(c, elem=4 if i % 2 else 8) for i, c in enumerate(contents)])
    if n >= 4096:
        assert totals[0] <= n // 16, (totals[0], n)       # zeros: 64 bytes per 3-byte copy


def test_page_tables():
    rng = np.random.default_rng(7)
    vals = np.minimum(rng.zipf(1.3, 3000), 50000).astype(np.int64)
    big = rng.integers(0, 4, 3 * FRAG + 7, dtype=np.uint8).tobytes()
    n = len(vals)
    specs = [
        _region(vals.tobytes(), [0, n], unit=8),                                   # one page
        _region(vals[:700].tobytes(), list(range(701)), unit=8),                   # pages of one value
        _region(vals.tobytes(), [0, 1000, 1000, n], unit=8),                       # an empty page between two full ones
        _region(vals.tobytes(), [0, 0, n, n], unit=8),                             # empty pages first and last
        _region(big, [0, FRAG + 5, 2 * FRAG + 100, len(big)], unit=1, elem=4),     # pages that are no multiple of FRAG
        _region(big, [0, FRAG, 2 * FRAG, 3 * FRAG, len(big)], unit=1, elem=4),     # pages of exactly one fragment
    ]
    specs += [_region(big[:5000 + s], [0, 17, 4099, 5000 + s], unit=1, elem=4, shift=s) for s in (1, 2, 3)]
    _go(specs)


def test_more_columns_than_one_launch_takes():
    rng = np.random.default_rng(8)
    specs = [_region(np.minimum(rng.zipf(1.3, 500 + 37 * i), 5000).astype(np.int64).tobytes(), unit=8)
             for i in range(19)]
    _go(specs)


@pytest.mark.parametrize("m", [64, 65, 67, 1000])
def test_match_lengths(m):
    """A stretch of m random bytes stands twice, the byte behind its second copy differs."""
    rng = np.random.default_rng(m)
    a = bytearray(rng.bytes(6000))
    a[3000: 3000 + m] = a[100: 100 + m]
    a[3000 + m] = a[100 + m] ^ 0xFF
    (total,) = _go([_region(bytes(a), elem=8)])
    assert total <= len(a) - m + 3 * ((m + 63) // 64) + 8 + 64   # the copy was found (at most one window late)


def test_match_across_a_fragment_boundary():
    """The repeated stretch runs across the boundary: each fragment copies only from itself."""
    rng = np.random.default_rng(11)
    a = bytearray(rng.bytes(FRAG + 3000))
    a[FRAG - 150: FRAG + 150] = a[1000: 1300]
    a[FRAG + 500: FRAG + 800] = a[FRAG - 400: FRAG - 100]      # its source lies in the fragment before
    _go([_region(bytes(a), elem=8), _region(bytes(FRAG - 2) + bytes(a[:FRAG + 2]), elem=4)])


def test_label_fixture_and_its_cap():
    lab = np.minimum(np.random.default_rng(0).zipf(1.3, 32768), 50000).astype(np.int64)
    srt = np.sort(np.random.default_rng(1).choice(1 << 40, 32768, replace=False)).astype(np.int64)
    specs = [_region(lab.tobytes(), [0, 10000, 32768], unit=8, elem=8),
             _region(lab.astype(np.int32).tobytes(), unit=4, elem=4),
             _region(srt.tobytes(), unit=8, elem=8)]
    totals = _go(specs)
    ref = [len(pa.Codec("snappy").compress(s[1])) for s in specs]
    print("snappy fixtures (raw, device, pyarrow):", [(len(s[1]), t, r) for s, t, r in zip(specs, totals, ref)])
    assert totals[0] <= 2.0 * ref[0], (totals[0], ref[0])


def test_a_short_slot_sets_the_error_word_and_stays_inside():
    from nvtabular_amd import _lib

    rng = np.random.default_rng(12)
    specs = [_region(rng.bytes(5000), elem=8), _region(bytes(5000), elem=8)]
    ds, got = _run(specs, slot_cap=64)
    h = _host(ds)
    _guards_hold(h)
    assert got[0].error == _lib.SNAPPY_ERR_SLOT and got[1].error == _lib.SNAPPY_ERR_SLOT
    assert h["slots"].size == 64 * 4


def test_a_region_that_does_not_fit_its_dense_buffer_is_not_moved():
    from nvtabular_amd import kernels_snappy as KS

    rng = np.random.default_rng(13)
    r, data, cuts = _region(rng.bytes(5000), elem=8)
    z, zdata, zcuts = _region(bytes(5000), elem=8)
    ds = KS.compress([KS.Region(r.src, r.page_start, 1, 8, None), KS.Region(z.src, z.page_start, 1, 8, None)], guard=GUARD)
    got = KS.read_back(ds, release=False)
    torch.cuda.synchronize()
    h = _host(ds)
    _guards_hold(h)
    assert got[0].error == 0 and got[0].total > 5000 and (h["dense"][0] == 0xA5).all()
    assert got[1].error == 0 and got[1].total < 5000
    assert R.decode_elements(h["dense"][1][: got[1].total].tobytes(), 5000) == zdata
