"""Kernel-level matrix for nvt_key_labels (nvtabular_amd/csrc/nvt_key_labels.hip).  The entry point is
called through ``_lib.load()`` on buffers this file owns and compared bit for bit with
hive_reference.py (pinned on the CPU by test_hive_reference.py).  ``label``, ``first_row`` and
``state`` lie between two 64-byte guards of 0xA5 that must be intact afterwards; the entries of
``first_row`` from D on still hold 0xA5.

Branch -> the case that reaches it (T = nvt_key_labels_tile_rows(); a workgroup owns whole tiles, and
up to 256 T rows every workgroup owns exactly one).

  one workgroup, partial waves and tiles    n in {1, 63, 64, 65, T - 1, T}                      test_sizes
  two and more workgroups merge the same    n = T + 1, 3 T + 5                                   test_sizes
  keys into the global table
  a workgroup walks several tiles           n = 513 T + 3                                        test_several_tiles_per_workgroup
  n = 0: nothing is written                                                                     test_no_rows
  D = 1, 2, 4095, 4096; first rows not      random 64-bit tags, the keys' first rows in a        test_cardinalities
  sorted by tag; a key's first row in       shuffled block at the front, the rest of the rows
  another workgroup than most of its rows   drawn from all keys over 8+ workgroups
  local / global fill limit: status 1       D = 4097 on 3 x 4097 rows (a workgroup sees up to    test_too_many_keys
                                            2048 keys: the global count trips), and 4097 keys
                                            inside one workgroup's rows (the local count trips)
  probe chains: tags that agree in their    k << 13, k << 32 and runs of consecutive integers,   test_colliding_tags
  low or high bits                          4096 keys each
  the empty-slot marker as a tag            2^63 (= INT64_MIN), 0, -1, INT64_MAX in one input    test_marker_tags
  nkeys = 1: the null key                   null rows with arbitrary tags; a non-null row with   test_null_key
                                            a null row's tag is another key
  nkeys = 2: null bits in the fingerprint   (null, 5) against (5, null) through nvt_join_hash    test_pair_with_nulls
  nkeys = 2: collision check, status 2      equal tags with different words / null bits          test_collision_status
  no result depends on timing               two calls on one multi-workgroup input               test_two_runs_agree
  the driver                                int32 / int64 / uint8 keys, string surrogates and    test_driver
                                            a key pair through kernels_labels.key_labels
  argument checks                           tests/test_hive_cabi.py (no GPU)

Left out: timing (tools/hive_rate.py); n at 2^31 and above (the labels are 4 bytes a row and the
row index is compared as 32 bits only against n < 2^32, which the entry checks)."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

import hive_reference as R
from kernel_buffers import Guarded, Lib, dev

pytestmark = pytest.mark.gpu

POISON32 = np.frombuffer(b"\xA5" * 4, dtype=np.uint32)[0]
POISON64 = np.frombuffer(b"\xA5" * 8, dtype=np.uint64)[0]
MARKER = np.uint64(1 << 63)


@pytest.fixture(scope="module")
def L():
    yield Lib()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def T(L):
    return L.lib.nvt_key_labels_tile_rows()


def run(L, tags, nulls, words=None, nkeys=1):
    """nvt_key_labels into poisoned outputs -> (label uint32[n], first_row uint32[4096], state uint64[2])."""
    tags = np.ascontiguousarray(tags, dtype=np.uint64)
    n = len(tags)
    d_tags, d_nulls = dev(tags.view(np.int64)), dev(np.ascontiguousarray(nulls, dtype=np.uint8))
    d_words = dev(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)) if words is not None else None
    label, first, state = Guarded(n * 4), Guarded(R.LABEL_MAX * 4), Guarded(16)
    need = C.c_uint64()
    assert L.lib.nvt_key_labels_ws_bytes(n, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    L.call("nvt_key_labels", d_tags.data_ptr() if n else None, d_nulls.data_ptr() if n else None,
           None if d_words is None else d_words.data_ptr(), nkeys, n, label.ptr, first.ptr, state.ptr, ws.data_ptr(),
           need.value)
    return label.read(np.uint32, "label").copy(), first.read(np.uint32, "first_row").copy(), \
        state.read(np.uint64, "state").copy()


def check(L, tags, nulls, words=None, nkeys=1, fast=False):
    want = R.key_labels_fast(tags, nulls, nkeys) if fast else R.key_labels(tags, nulls, words, nkeys)
    label, first, state = run(L, tags, nulls, words, nkeys)
    want_label, want_first, D, status = want
    assert status == 0 and state.tolist() == [D, 0]
    np.testing.assert_array_equal(label, want_label)
    np.testing.assert_array_equal(first[:D], want_first)
    assert (first[D:] == POISON32).all(), "first_row was written from D on"
    return D


def test_sizes(L, T):
    rng = np.random.default_rng(11)
    for n in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        tags = rng.integers(0, 37, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        nulls = (rng.random(n) < 0.05).astype(np.uint8)
        check(L, tags, nulls)


def test_several_tiles_per_workgroup(L, T):
    rng = np.random.default_rng(19)
    n = 513 * T + 3                      # more than 256 tiles: three tiles per workgroup
    tags = rng.integers(0, 1000, n).astype(np.uint64) << np.uint64(40)
    tags[: n // 2] &= np.uint64(0xFF << 40)   # most keys first appear in the second half
    check(L, tags, (rng.random(n) < 0.001).astype(np.uint8), fast=True)


def test_no_rows(L):
    label, first, state = run(L, np.zeros(0, np.uint64), np.zeros(0, np.uint8))
    assert len(label) == 0 and (first == POISON32).all() and (state == POISON64).all()


@pytest.mark.parametrize("D", [1, 2, 4095, 4096])
def test_cardinalities(L, T, D):
    rng = np.random.default_rng(D)
    keys = rng.integers(0, 2 ** 63, D, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, D).astype(np.uint64) << 63)
    keys = np.unique(keys)
    keys = keys[keys != MARKER]
    assert len(keys) == D
    n = max(4 * D, 8 * T + 7)
    tags = np.concatenate([rng.permutation(keys), keys[rng.integers(0, D, n - D)]])
    assert check(L, tags, np.zeros(n, np.uint8), fast=True) == D


def test_too_many_keys(L, T):
    D = R.LABEL_MAX + 1
    rng = np.random.default_rng(3)
    spread = rng.permutation(np.tile(np.arange(D, dtype=np.uint64) * 7 + 1, 3))      # 3 x 4097 rows, 7 workgroups
    # 513 tiles: a workgroup owns three, and the first one's rows hold all 4097 keys
    within = np.concatenate([np.arange(D, dtype=np.uint64), np.zeros(513 * T - D, np.uint64)])
    for tags in (spread, within):
        label, first, state = run(L, tags, np.zeros(len(tags), np.uint8))   # (the guards are checked by run)
        assert state[1] == 1


@pytest.mark.parametrize("kind", ["shl13", "shl32", "runs"])
def test_colliding_tags(L, kind):
    rng = np.random.default_rng(5)
    k = np.arange(R.LABEL_MAX, dtype=np.uint64)
    if kind == "shl13":
        keys = k << np.uint64(13)
    elif kind == "shl32":
        keys = k << np.uint64(32)
    else:   # four runs of 1024 consecutive integers, one of them ending at 2^64 - 1
        keys = np.concatenate([np.arange(1024, dtype=np.uint64) + np.uint64(b) for b in
                               (0, 1 << 20, (1 << 63) + 1, (1 << 64) - 1024)])
    tags = np.concatenate([rng.permutation(keys), rng.permutation(keys)])
    assert check(L, tags, np.zeros(len(tags), np.uint8), fast=True) == R.LABEL_MAX


def test_marker_tags(L, T):
    rng = np.random.default_rng(9)
    keys = np.array([1 << 63, 0, (1 << 64) - 1, (1 << 63) - 1, 12345], dtype=np.uint64)
    assert keys[0] == MARKER and keys.view(np.int64)[0] == np.iinfo(np.int64).min
    for n in (300, 2 * T + 3):
        tags = keys[rng.integers(0, len(keys), n)]
        assert check(L, tags, np.zeros(n, np.uint8)) == len(keys)
        check(L, tags, (rng.random(n) < 0.3).astype(np.uint8))            # ... and next to the null key
        check(L, tags, np.zeros(n, np.uint8), np.stack([tags, tags]), 2)  # the same tags under nkeys = 2


def test_null_key(L, T):
    rng = np.random.default_rng(13)
    n = 2 * T + 100
    tags = rng.integers(0, 6, n).astype(np.uint64)
    nulls = (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)
    tags[:4], nulls[:4] = [3, 3, 4, 3], [0, 1, 7, 0]   # row 1 opens the null key; rows 0 and 3 are the key 3
    D = check(L, tags, nulls)
    assert D == 7
    label, _, _ = run(L, tags, nulls)
    assert label[:4].tolist() == [0, 1, 1, 0]


def test_pair_with_nulls(L):
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.kernels_labels import key_labels

    df = pd.DataFrame({"a": pd.array([None, 5, None, 5, 5, None], dtype="Int64"),
                       "b": pd.array([5, None, 5, None, 5, None], dtype="Int64")})
    label, D, first = key_labels(DeviceFrame.from_pandas(df), ["a", "b"])
    assert D == 4 and label.cpu().tolist() == [0, 1, 0, 1, 2, 3] and first.tolist() == [0, 1, 4, 5]


def test_collision_status(L, T):
    n = T + 9
    tags = np.full(n, 77, dtype=np.uint64)
    words = np.full((2, n), 5, dtype=np.uint64)
    nulls = np.zeros(n, np.uint8)
    assert run(L, tags, nulls, words, 2)[2].tolist() == [1, 0]
    bad = words.copy()
    bad[1, n - 1] = 6
    assert run(L, tags, nulls, bad, 2)[2].tolist() == [1, 2]
    bad_nulls = nulls.copy()
    bad_nulls[n // 2] = 1
    assert run(L, tags, bad_nulls, words, 2)[2].tolist() == [1, 2]
    assert R.key_labels(tags, nulls, bad, 2)[3] == 2 and R.key_labels(tags, bad_nulls, words, 2)[3] == 2


def test_two_runs_agree(L, T):
    rng = np.random.default_rng(17)
    n = 6 * T + 11
    tags = rng.integers(0, 3000, n).astype(np.uint64) << np.uint64(20)
    nulls = (rng.random(n) < 0.01).astype(np.uint8)
    a, b = run(L, tags, nulls), run(L, tags, nulls)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def _factorize(df):
    tuples = pd.Series(list(df.itertuples(index=False, name=None)), dtype=object)
    tuples = tuples.map(lambda t: tuple(None if pd.isna(v) else v for v in t))
    codes, uniques = pd.factorize(tuples, use_na_sentinel=False)
    first = pd.Series(np.arange(len(codes))).groupby(codes).min().to_numpy()
    return codes, first


def test_driver(L):
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.kernels_labels import key_labels, split_plan

    rng = np.random.default_rng(23)
    n = 100_000
    words = np.array(["a/b", "x=y", "p%q r", "é", "", "zz"], dtype=object)
    s = words[rng.integers(0, 6, n)]
    s[rng.random(n) < 0.1] = None
    df = pd.DataFrame({"i32": rng.integers(-50, 50, n).astype(np.int32),
                       "i64": pd.array(np.where(rng.random(n) < 0.1, None, rng.integers(0, 7, n) * 10 ** 12), dtype="Int64"),
                       "u8": rng.integers(0, 200, n).astype(np.uint8),
                       "s": s})
    frame = DeviceFrame.from_pandas(df)
    for keys in (["i32"], ["i64"], ["u8"], ["s"], ["i64", "s"]):
        label, D, first = key_labels(frame, keys)
        codes, want_first = _factorize(df[keys])
        assert D == len(want_first), keys
        np.testing.assert_array_equal(label.cpu().numpy(), codes)
        np.testing.assert_array_equal(first, want_first)
    perm, counts, first = split_plan(frame, ["i64", "s"])
    codes, _ = _factorize(df[["i64", "s"]])
    np.testing.assert_array_equal(perm.cpu().numpy(), np.argsort(codes, kind="stable"))
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(codes))
    with pytest.raises(ValueError, match="more than 4096"):
        key_labels(DeviceFrame.from_pandas(pd.DataFrame({"k": np.arange(5000)})), ["k"])
