"""nvt_partition_ids / nvt_partition_plan / nvt_partition_gather_many directly against the numpy
restatement (tests/partition_reference.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest

import partition_reference as R

pytestmark = pytest.mark.gpu


def _env():
    import torch

    from nvtabular_amd import _lib
    from nvtabular_amd import kernels as K

    return torch, _lib, _lib.load(), K


def _tags(columns, modes=None):
    """Key columns [(numpy values, bool validity or None)] -> uint64 tags read back from nvt_join_hash."""
    torch, L, lib, K = _env()
    from nvtabular_amd.device import DeviceColumn, pack_bitmap
    from nvtabular_amd.kernels_join import key_descs

    dev = torch.device("cuda")
    cols = []
    for vals, valid in columns:
        bitmap = torch.from_numpy(pack_bitmap(valid)).to(dev) if valid is not None else None
        cols.append(DeviceColumn(torch.from_numpy(vals).to(dev), bitmap))
    modes = modes or tuple(L.JOIN_FLOAT if v.dtype.kind == "f" else L.JOIN_INT for v, _ in columns)
    n, nk = len(columns[0][0]), len(columns)
    descs, alive = key_descs(cols, modes)
    tag = torch.empty(n, dtype=torch.int64, device=dev)
    nulls = torch.empty(n, dtype=torch.uint8, device=dev)
    words = torch.empty((nk, n), dtype=torch.int64, device=dev) if nk > 1 else None
    L.check(lib.nvt_join_hash(descs, nk, n, tag.data_ptr(), K.ptr(words), nulls.data_ptr(), K.stream_ptr()))
    return tag


def _ids(tag, P):
    torch, L, lib, K = _env()
    pid = torch.empty(tag.numel(), dtype=torch.int32, device=tag.device)
    L.check(lib.nvt_partition_ids(tag.data_ptr(), tag.numel(), P, pid.data_ptr(), K.stream_ptr()))
    return pid.cpu().numpy().view(np.uint32)


def _check_ids(columns, tuples, modes=None):
    tag = _tags(columns, modes)
    host = tag.cpu().numpy().view(np.uint64)
    for P in (1, 3, 8, 4096):
        pid = _ids(tag, P)
        np.testing.assert_array_equal(pid, R.partition_ids(host, P))
        first = {}
        for t, p in zip(tuples, pid.tolist()):   # equal key tuples, equal partition
            assert first.setdefault(t, p) == p, (t, P)


def test_ids_int_keys():
    rng = np.random.default_rng(0)
    for dt in (np.int32, np.int64):
        v = rng.integers(-50, 50, 1000).astype(dt)
        v[:4] = [np.iinfo(dt).min, np.iinfo(dt).max, 0, -1]
        _check_ids([(v, None)], v.tolist())


def test_ids_float_keys_zero_signs_and_nan():
    rng = np.random.default_rng(1)
    v = rng.integers(-20, 20, 600).astype(np.float32) / 4
    v[:6] = [0.0, -0.0, np.nan, -0.0, np.nan, 0.0]
    tuples = ["nan" if x != x else float(x) + 0.0 for x in v]   # (-0.0 + 0.0 == 0.0: one key)
    _check_ids([(v, None)], tuples)
    tag = _tags([(v, None)]).cpu().numpy()
    assert tag[0] == tag[1] == tag[3] == tag[5] and tag[2] == tag[4]


def test_ids_two_columns_with_nulls_in_either():
    rng = np.random.default_rng(2)
    n = 1500
    a = rng.integers(0, 6, n).astype(np.int64)
    b = rng.integers(0, 5, n).astype(np.int32)
    va, vb = rng.random(n) > 0.2, rng.random(n) > 0.2
    tuples = [(int(x) if p else None, int(y) if q else None) for x, y, p, q in zip(a, b, va, vb)]
    assert len(set(tuples)) > 30
    a = np.where(va, a, rng.integers(0, 99, n)).astype(np.int64)   # what lies under a null must not matter
    _check_ids([(a, va), (b, vb)], tuples)


# ---- plan ---------------------------------------------------------------------------------------

def _plan(pid_np, P):
    torch, L, lib, K = _env()
    dev = torch.device("cuda")
    n = len(pid_np)
    pid = torch.from_numpy(pid_np.view(np.int32)).to(dev)
    perm = torch.full((n,), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros(P, dtype=torch.int64, device=dev)
    need = C.c_uint64()
    L.check(lib.nvt_partition_plan_ws_bytes(n, P, C.byref(need)))
    ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 16
    ws[off: off + need.value] = 0xAB   # the entry may not rely on a cleared workspace
    L.check(lib.nvt_partition_plan(pid.data_ptr() if n else None, n, P, perm.data_ptr() if n else None,
                                   counts.data_ptr(), (ws.data_ptr() + off) if n else None, need.value,
                                   K.stream_ptr()))
    return perm.cpu().numpy(), counts.cpu().numpy().view(np.uint64)


def _plan_sizes():
    from nvtabular_amd import _lib

    tile = _lib.load().nvt_partition_tile_rows()
    return [0, 1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 1]


@pytest.mark.parametrize("P", [1, 2, 3, 64, 4096])
def test_plan_is_the_stable_sort(P):
    rng = np.random.default_rng(P)
    for n in _plan_sizes():
        pid = rng.integers(0, P, n).astype(np.uint32)
        perm, counts = _plan(pid, P)
        want_perm, want_counts = R.plan(pid, P)
        np.testing.assert_array_equal(perm, want_perm, err_msg=f"n={n}")
        np.testing.assert_array_equal(counts, want_counts, err_msg=f"n={n}")
        again = _plan(pid, P)
        np.testing.assert_array_equal(again[0], perm)
        np.testing.assert_array_equal(again[1], counts)


@pytest.mark.parametrize("P", [2, 3, 64, 4096])
def test_plan_one_partition_and_alternating(P):
    tile = _plan_sizes()[-3]
    n = 3 * tile + 1
    for pid in (np.zeros(n, np.uint32), np.full(n, P - 1, np.uint32),
                (np.arange(n) % 2 * (P - 1)).astype(np.uint32), (np.arange(n) % P).astype(np.uint32)):
        perm, counts = _plan(pid, P)
        want_perm, want_counts = R.plan(pid, P)
        np.testing.assert_array_equal(perm, want_perm)
        np.testing.assert_array_equal(counts, want_counts)


def test_plan_several_tiles_per_workgroup():
    """More tiles than workgroups (1024): every workgroup carries its cursors from tile to tile."""
    tile = _plan_sizes()[-3]
    n = 2 * 1024 * tile + tile + 1
    rng = np.random.default_rng(7)
    for P in (5, 1000):
        pid = rng.integers(0, P, n).astype(np.uint32)
        pid[rng.random(n) < 0.5] = 1   # one heavy partition: long same-id runs inside a wave
        perm, counts = _plan(pid, P)
        want_perm, want_counts = R.plan(pid, P)
        np.testing.assert_array_equal(counts, want_counts)
        np.testing.assert_array_equal(perm, want_perm)


# ---- gather -------------------------------------------------------------------------------------

_DTYPES = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


def _gather(columns, seg_rows, m):
    """columns: [(width, per segment (src values, bool validity or None))]; seg_rows: per segment
    the idx array.  Runs nvt_partition_gather_many in batches of 16 columns.
    -> [(values, bitmap or None)] read back."""
    torch, L, lib, K = _env()
    dev = torch.device("cuda")
    keep, words = [], []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr() if t.numel() else 0

    seg_at = len(words)
    start = 0
    for idx in seg_rows:
        words += [up(np.asarray(idx, dtype=np.int64)), start]
        start += len(idx)
    assert start == m
    jobs = []
    for width, per_seg in columns:
        with_valid = any(v is not None for _, v in per_seg)
        src_at = len(words)
        words += [up(s) for s, _ in per_seg]
        valid_at = None
        if with_valid:
            valid_at = len(words)
            words += [up(R.pack_bits(v)) if v is not None else 0 for _, v in per_seg]
        dst = torch.full((m,), 0x55, dtype=torch.from_numpy(np.zeros(1, _DTYPES[width])).dtype, device=dev)
        dst_valid = torch.full(((m + 63) // 64 * 8,), 0xFF, dtype=torch.uint8, device=dev) if with_valid else None
        jobs.append((width, src_at, valid_at, dst, dst_valid))
    table = torch.from_numpy(np.array(words or [0], dtype=np.uint64).view(np.int64)).to(dev)
    base = table.data_ptr()
    for j0 in range(0, len(jobs), L.PARTITION_MAX_COLS):
        batch = jobs[j0: j0 + L.PARTITION_MAX_COLS]
        descs = (L.PartitionCol * len(batch))()
        for d, (width, src_at, valid_at, dst, dst_valid) in zip(descs, batch):
            d.src = base + 8 * src_at
            d.src_valid = base + 8 * valid_at if valid_at is not None and m else None
            d.dst = dst.data_ptr() if m else None
            d.dst_valid = K.ptr(dst_valid) if m else None
            d.width = width
        L.check(lib.nvt_partition_gather_many(descs, len(batch), base + 8 * seg_at, len(seg_rows), m,
                                              K.stream_ptr()))
    torch.cuda.synchronize()
    return [(dst.cpu().numpy(), dst_valid.cpu().numpy() if dst_valid is not None else None)
            for _, _, _, dst, dst_valid in jobs]


def _split(m, boundaries):
    edges = [0] + [b for b in boundaries if 0 < b < m] + [m]
    return [edges[i + 1] - edges[i] for i in range(len(edges) - 1)]


def _case(m, seg_lens, ncols, valid_kind, seed):
    rng = np.random.default_rng(seed)
    src_rows = [int(rng.integers(1, 200)) for _ in seg_lens]
    seg_rows = [np.sort(rng.integers(0, r, k)) for r, k in zip(src_rows, seg_lens)]
    columns, want = [], []
    for c in range(ncols):
        width = (1, 4, 8, 2)[c % 4]
        per_seg = []
        for s, r in enumerate(src_rows):
            vals = rng.integers(0, 250, r).astype(_DTYPES[width])
            has = {"all": True, "none": False, "mixed": (s + c) % 2 == 0}[valid_kind]
            per_seg.append((vals, (rng.random(r) > 0.4) if has else None))
        columns.append((width, per_seg))
        with_valid = any(v is not None for _, v in per_seg)
        want.append(R.gather([(s, R.pack_bits(v) if v is not None else None, idx)
                              for (s, v), idx in zip(per_seg, seg_rows)], with_valid))
    got = _gather(columns, seg_rows, m)
    for c, ((gv, gb), (wv, wb)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(gv, wv.astype(gv.dtype), err_msg=f"column {c}")
        assert (gb is None) == (wb is None)
        if wb is not None:
            np.testing.assert_array_equal(gb, wb, err_msg=f"bitmap of column {c}")   # padding bits included


@pytest.mark.parametrize("valid_kind", ["all", "none", "mixed"])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 129])
def test_gather_one_and_three_segments(m, valid_kind):
    _case(m, [m], 3, valid_kind, seed=m)
    if m >= 3:
        _case(m, _split(m, [m // 3, 2 * m // 3]), 3, valid_kind, seed=m + 1000)
        _case(m, [m - 2, 0, 2], 3, valid_kind, seed=m + 2000)   # an empty segment in the middle


@pytest.mark.parametrize("boundary", [1, 32, 63, 64])
def test_gather_segment_boundary_inside_and_at_a_word(boundary):
    for valid_kind in ("all", "mixed"):
        _case(129, [boundary, 129 - boundary], 3, valid_kind, seed=boundary)
        _case(129, _split(129, [boundary, boundary + 1]), 3, valid_kind, seed=boundary + 50)


def test_gather_two_byte_values():
    for m, lens in ((129, [129]), (129, [63, 66]), (65, [1, 0, 64])):
        _case(m, lens, 4, "mixed", seed=m + len(lens))   # the fourth column is 2 bytes wide


def test_gather_seventeen_columns_take_two_batches():
    _case(129, [40, 25, 64], 17, "mixed", seed=17)
    _case(65, [65], 17, "all", seed=18)
