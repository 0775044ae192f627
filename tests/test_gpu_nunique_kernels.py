"""``K.seg_nunique`` (csrc/nvt_seg_nunique.hip) called directly on torch tensors and compared,
exactly, with the numpy reference of nunique_reference.py (np.unique per group), which
test_nunique_reference.py pins to pandas on the CPU.

Kernels reached: nu_key_kernel<float | double | int32 | int64 | uint8> (bool through the uint8
view), sort_words_bits on 8 / 32 / 32 + 32 key bits and on the bits of the group id,
nu_repack_kernel (high key half, group id), nu_count_kernel.

Sizes, from the constants of the .hip files.  The sorts work in tiles of kS2Tile = T = 4096 words
(there is no LDS tier with a tile of its own): the main frame holds groups of 1, 2, 63, 64, 65,
T - 1, T, T + 1 and 3 T + 5 rows, the first one (T rows) and the last one end exactly on a tile
edge, the others cross the edges or lie inside a tile.  nu_count_kernel: stream_grid(n, 1024, 8)
workgroups of 4 waves, each wave walks roundup64(ceil(n / nwaves)) words in rows of 64; at the main
frame's 28 709 words that is 116 waves with chunks of 256 words, so runs cross rows and chunks,
and the two large single-group frames (200 003 words: 784 waves, chunks of 256) carry one run
through every chunk.  The group id takes one radix pass below 256 groups, two below 65 536, three
from there on: 9 + 1, 5 000 and 70 000 groups.
"""
import numpy as np
import pytest
import torch

import nunique_reference as R

pytestmark = pytest.mark.gpu

T = 4096
I64 = np.iinfo(np.int64)
DTYPES = ["float32", "float64", "int32", "int64", "uint8", "bool"]


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(K, words, ngroups, vals, valid):
    """K.seg_nunique on host columns -> host int64[V, G]."""
    out = K.seg_nunique(dev(words.view(np.int64)), ngroups, [dev(v) for v in vals],
                        [None if ok is None else dev(R.pack_bits(ok)) for ok in valid])
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(vals), ngroups)
    return out.cpu().numpy()


def layout(rng, sizes, trailing=0):
    """Words of groups 0 .. len(sizes) - 1 with the given sizes, in group order, over a random
    permutation of the rows (a group's rows come in any order), followed by `trailing` words of
    null keys (group = ngroups, the marker of nvt_order_rows, and beyond)."""
    ngroups = len(sizes)
    group = np.repeat(np.arange(ngroups), sizes)
    if trailing:
        group = np.concatenate([group, ngroups + (np.arange(trailing) % 2) * 5])
    return R.words_of(group, rng.permutation(group.size)), ngroups


def column(rng, n, dtype, card):
    """n values of `dtype` drawn from about `card` distinct ones; floats with ~10 % NaN."""
    if dtype == "bool":
        return rng.random(n) < 0.5
    if dtype == "uint8":
        return rng.integers(0, min(card, 256), n).astype(np.uint8)
    if dtype.startswith("float"):
        v = (rng.integers(-card // 2, card // 2 + 1, n) / 4).astype(dtype)
        v[rng.random(n) < 0.1] = np.nan
        return v
    if dtype == "int64":                              # both halves of the key differ
        return (rng.integers(-card // 2, card // 2 + 1, n) * ((1 << 33) + 3)).astype(np.int64)
    return rng.integers(-card // 2, card // 2 + 1, n).astype(dtype)


MAIN_SIZES = [T, 1, 2, 63, 64, 65, T - 1, T + 1, 3 * T + 5, 7 * T - (6 * T + 200)]


@pytest.fixture(scope="module")
def main_frame():
    rng = np.random.default_rng(1)
    assert sum(MAIN_SIZES) == 7 * T and sum(MAIN_SIZES[:1]) == T
    words, ngroups = layout(rng, MAIN_SIZES, trailing=37)
    n = words.size
    cols = {}
    for dt in DTYPES:
        v = column(rng, n, dt, 300)
        ok = rng.random(n) >= 0.2
        cols[dt] = (v, ok)
    return words, ngroups, cols


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_sizes_around_the_tile(K, main_frame, dtype, nulls):
    words, ngroups, cols = main_frame
    v, ok = cols[dtype]
    ok = ok if nulls else None
    exp = R.seg_nunique(words, ngroups, [v], [ok])
    assert exp.max() > 1 or dtype == "bool"
    np.testing.assert_array_equal(run(K, words, ngroups, [v], [ok]), exp)


@pytest.mark.parametrize("ngroups,hi", [(5_000, 3), (70_000, 2)])
def test_many_small_groups(K, ngroups, hi):
    rng = np.random.default_rng(ngroups)
    sizes = rng.integers(1, hi + 1, ngroups)
    words, _ = layout(rng, sizes, trailing=11)
    n = words.size
    vals = [column(rng, n, "int64", 3), column(rng, n, "float32", 4), column(rng, n, "int32", 2)]
    valid = [None, rng.random(n) >= 0.3, None]
    exp = R.seg_nunique(words, ngroups, vals, valid)
    assert set(np.unique(exp)) >= {0, 1, 2}
    np.testing.assert_array_equal(run(K, words, ngroups, vals, valid), exp)


def test_groups_without_a_counting_entry_and_edge_values(K):
    """Group 0: all null; 1: all NaN; 2: -0.0 / +0.0 / +-inf; 3: ordinary; 4: no rows at all."""
    rng = np.random.default_rng(2)
    sizes = [70, 70, 70, 70, 0]
    words, ngroups = layout(rng, sizes)
    group = (words >> np.uint64(32)).astype(np.int64)
    row = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
    f = np.empty(280, np.float64)
    ok = np.ones(280, bool)
    f[row[group == 0]] = rng.integers(0, 5, 70)
    ok[row[group == 0]] = False
    f[row[group == 1]] = np.nan
    f[row[group == 2]] = np.resize([-0.0, 0.0, np.inf, -np.inf, np.inf, 1.0, 0.0], 70)
    f[row[group == 3]] = np.resize([1.5, 2.5, -1.5], 70)
    exp = R.seg_nunique(words, ngroups, [f, f.astype(np.float32)], [ok, ok])
    assert exp.tolist() == [[0, 0, 4, 3, 0]] * 2
    np.testing.assert_array_equal(run(K, words, ngroups, [f, f.astype(np.float32)], [ok, ok]), exp)


def test_int64_values_at_the_ends_of_the_range_are_distinct(K):
    """INT64_MAX / INT64_MAX - 1 and INT64_MIN / INT64_MIN + 1, interleaved in row order: an image
    that ties a pair (nvt_sort_key_u64's does) would leave the pair interleaved after a stable
    sort and count every change between them."""
    ends = [I64.max, I64.max - 1, I64.min, I64.min + 1]
    v = np.resize(np.array(ends, np.int64), 1000)
    words = R.words_of(np.repeat([0, 1], 500))        # rows in order: the pairs alternate
    exp = R.seg_nunique(words, 2, [v], [None])
    assert exp.tolist() == [[4, 4]]
    np.testing.assert_array_equal(run(K, words, 2, [v], [None]), exp)
    only_max = np.resize(np.array(ends[:2], np.int64), 1000)
    only_min = np.resize(np.array(ends[2:], np.int64), 1000)
    assert run(K, words, 2, [only_max, only_min], [None, None]).tolist() == [[2, 2], [2, 2]]


@pytest.mark.parametrize("shape", ["equal", "distinct"])
def test_one_large_group(K, shape):
    rng = np.random.default_rng(3)
    n = 200_003
    words, ngroups = layout(rng, [n])
    if shape == "equal":
        vals = [np.full(n, -7.25, np.float64), np.full(n, I64.min, np.int64), np.full(n, 200, np.uint8)]
        exp = [[1], [1], [1]]
    else:
        with np.errstate(over="ignore"):              # x -> a x mod 2^64 is a bijection (a odd)
            i64 = ((rng.permutation(n).astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        vals = [rng.permutation(n).astype(np.float64) - n / 2, i64, rng.permutation(n).astype(np.int32)]
        exp = [[n], [n], [n]]
    assert R.seg_nunique(words, ngroups, vals, [None] * 3).tolist() == exp
    assert run(K, words, ngroups, vals, [None] * 3).tolist() == exp


@pytest.mark.parametrize("ncols,calls", [(8, 1), (11, 2)])
def test_columns_per_call(K, main_frame, ncols, calls):
    """8 columns are one call of the C entry point, 11 go through the binding as 8 + 3."""
    words, ngroups, cols = main_frame
    names = [DTYPES[j % len(DTYPES)] for j in range(ncols)]
    vals = [cols[dt][0] for dt in names]
    valid = [cols[dt][1] if j % 2 else None for j, dt in enumerate(names)]
    exp = R.seg_nunique(words, ngroups, vals, valid)
    before = K.STATS.get("seg_nunique_calls", 0)
    got = run(K, words, ngroups, vals, valid)
    assert K.STATS["seg_nunique_calls"] == before + calls
    np.testing.assert_array_equal(got, exp)


def test_nothing_to_do(K):
    empty = np.zeros(0, np.uint64)
    v = np.zeros(0, np.int64)
    assert run(K, empty, 3, [v, v], [None, None]).tolist() == [[0, 0, 0]] * 2
    assert tuple(run(K, empty, 0, [v], [None]).shape) == (1, 0)
    words = R.words_of(np.zeros(5, np.int64))         # rows of null keys only: ngroups = 0
    assert tuple(run(K, words, 0, [np.arange(5)], [None]).shape) == (1, 0)
    assert tuple(run(K, words, 1, [], []).shape) == (0, 1)


def test_output_beyond_the_groups_stays_untouched(K, main_frame):
    """The C entry point itself: out is [ncols][ngroups]; a further row of ngroups entries and a
    canary behind it keep their pattern (the frame ends in words of groups ngroups and ngroups + 5)."""
    import ctypes as C

    from nvtabular_amd import _lib
    from nvtabular_amd._lib import check

    words, ngroups, cols = main_frame
    names = ["int64", "float32"]
    vals = [dev(cols[dt][0]) for dt in names]
    bitmaps = [dev(R.pack_bits(cols[dt][1])) for dt in names]
    w = dev(words.view(np.int64))
    lib = _lib.load()
    need = C.c_uint64()
    check(lib.nvt_seg_nunique_ws_bytes(words.size, C.byref(need)), "ws")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    pattern = -0x0123456789ABCDEF
    out = torch.full((3 * ngroups + 64,), pattern, dtype=torch.int64, device="cuda")
    out[:2 * ngroups] = 0
    vd = (C.c_int * 2)(*[K.dtype_code(v.dtype) for v in vals])
    check(lib.nvt_seg_nunique(w.data_ptr(), words.size, ngroups, _lib.ptr_array([v.data_ptr() for v in vals]),
                              vd, _lib.ptr_array([b.data_ptr() for b in bitmaps]), 2, out.data_ptr(),
                              ws.data_ptr(), K.stream_ptr()), "nvt_seg_nunique")
    got = out.cpu().numpy()
    exp = R.seg_nunique(words, ngroups, [cols[dt][0] for dt in names], [cols[dt][1] for dt in names])
    np.testing.assert_array_equal(got[:2 * ngroups].reshape(2, ngroups), exp)
    assert (got[2 * ngroups:] == pattern).all()
