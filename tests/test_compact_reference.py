"""compact_reference.py against boolean indexing, Python list slicing and bit tests written out one
row at a time, on the CPU."""
import numpy as np
import pytest

import compact_reference as R


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_plan(n):
    rng = np.random.default_rng(n)
    keep = rng.random(n) < 0.4
    words, counts, base = R.plan(keep)
    nt = (n + 2047) // 2048
    assert words.dtype == np.uint64 and len(words) == nt * 32
    assert counts.dtype == base.dtype == np.uint32 and len(counts) == nt and len(base) == nt + 1
    for i in range(nt * 2048):
        assert ((int(words[i // 64]) >> (i % 64)) & 1) == (i < n and bool(keep[i]))
    for t in range(nt):
        assert counts[t] == keep[t * 2048: (t + 1) * 2048].sum()
        assert base[t] == keep[: t * 2048].sum()
    assert base[nt] == keep.sum()
    assert R.plan_layout(n) == (0, nt * 256, nt * 256 + (nt + 1) * 4)


def test_dropna_keep():
    rng = np.random.default_rng(1)
    n = 300
    f = rng.standard_normal(n)
    f[::7] = np.nan
    g = rng.standard_normal(n).astype(np.float32)
    g[5::11] = np.nan
    i = rng.integers(0, 9, n)
    vi, vf = rng.random(n) < 0.8, rng.random(n) < 0.9
    got = R.dropna_keep([(f, vf), (g, None), (i, vi), (i, None), (None, vi)], n)
    exp = [bool(vf[r] and f[r] == f[r] and g[r] == g[r] and vi[r]) for r in range(n)]
    assert got.tolist() == exp
    assert R.dropna_keep([], 3).tolist() == [True] * 3


@pytest.mark.parametrize("first", [0, 11])
def test_list_keep_and_offsets(first):
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 9, 200)
    lens[rng.random(200) < 0.3] = 0
    rows = [list(rng.integers(0, 100, k)) for k in lens]
    off = first + np.concatenate([[0], np.cumsum(lens)])
    leaves = np.array([v for r in rows for v in r], dtype=np.int64)
    for keep in (rng.random(200) < 0.5, np.zeros(200, bool), np.ones(200, bool)):
        kept = [r for r, k in zip(rows, keep) if k]
        lk = R.list_keep(off, keep)
        assert len(lk) == len(leaves)
        assert R.compact(leaves, lk).tolist() == [v for r in kept for v in r]
        new_off = R.list_offsets(off, keep)
        assert new_off.dtype == np.int64 and new_off[0] == 0 and len(new_off) == len(kept) + 1
        flat = R.compact(leaves, lk)
        assert [flat[new_off[j]: new_off[j + 1]].tolist() for j in range(len(kept))] == [list(map(int, r)) for r in kept]


def test_pack_bits():
    assert R.pack_bits([1, 0, 0, 0, 0, 0, 0, 0, 0, 1]).tolist() == [1, 2, 0, 0, 0, 0, 0, 0]
    assert R.pack_bits(np.ones(64, bool)).tolist() == [255] * 8
    assert R.pack_bits([]).size == 0
