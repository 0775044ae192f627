"""nvt_batch_take_many / nvt_take_list_* against numpy: src[index] + astype, bit for bit (values,
offsets, bitmaps, NaN positions), with guard words around every destination."""
import ctypes as C

import numpy as np
import pytest
import torch

from nvtabular_amd import _lib

pytestmark = pytest.mark.gpu

N_SRC = 3000
SRC_DTYPES = [np.bool_, np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
CODE = {np.dtype(np.bool_): 4, np.dtype(np.uint8): 4, np.dtype(np.int8): 5, np.dtype(np.int16): 6,
        np.dtype(np.int32): 2, np.dtype(np.int64): 3, np.dtype(np.float32): 0, np.dtype(np.float64): 1}
GUARD = 16          # elements before and behind every destination
RNG = np.random.default_rng(7)


def dsts_of(src):
    src = np.dtype(src)
    out = [src, np.dtype(np.float32), np.dtype(np.float64)]
    if src.kind in "iub":
        out.append(np.dtype(np.int64))
    return list(dict.fromkeys(out))


def make_src(dt, n=N_SRC):
    dt = np.dtype(dt)
    if dt.kind == "b":
        return RNG.random(n) < 0.5
    if dt.kind == "f":
        v = (RNG.standard_normal(n) * 10.0 ** RNG.integers(-3, 12, n)).astype(dt)
        v[RNG.random(n) < 0.05] = np.nan
        return v
    info = np.iinfo(dt)
    v = RNG.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    v[:4] = [info.min, info.max, 0, info.max - 1]
    return v


def dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a).cuda()
    return t


def pack(bits):
    b = np.packbits(bits.astype(np.uint8), bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 8, np.uint8)])


def expect(src, valid, idx, n_src, dst_dt):
    inside = (idx >= 0) & (idx < n_src)
    safe = np.where(inside, idx, 0)
    ok = inside & (valid[safe] if valid is not None else True)
    with np.errstate(all="ignore"):
        vals = src[safe].astype(dst_dt)
    null = np.nan if np.dtype(dst_dt).kind == "f" else 0
    return np.where(ok, vals, np.array(null, dtype=dst_dt)).astype(dst_dt), ok


class Job:
    """One descriptor with guarded buffers."""

    def __init__(self, src, valid, dst_dt, m, with_bitmap=True, matrix=None, column=0):
        self.src, self.valid, self.dst_dt, self.m = src, valid, np.dtype(dst_dt), m
        self.tsrc = dev(src)
        self.tvalid = dev(pack(valid)) if valid is not None else None
        self.matrix, self.column = matrix, column
        if matrix is None:
            self.buf = torch.from_numpy(np.full(m + 2 * GUARD, 0x5A, np.uint8).repeat(self.dst_dt.itemsize)).cuda()
        self.bm_words = (m + 63) // 64
        self.bm = torch.full((self.bm_words + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda() if with_bitmap else None

    def fill(self, d):
        es = self.dst_dt.itemsize
        d.src = self.tsrc.data_ptr()
        d.src_valid = self.tvalid.data_ptr() if self.tvalid is not None else None
        if self.matrix is None:
            d.dst, d.dst_stride = self.buf.data_ptr() + GUARD * es, 1
        else:
            d.dst, d.dst_stride = self.matrix.data_ptr() + self.column * es, self.matrix.shape[1]
        d.dst_valid = self.bm.data_ptr() + 8 if self.bm is not None else None
        d.src_dtype, d.dst_dtype = CODE[np.dtype(self.src.dtype)], CODE[self.dst_dt]

    def check(self, idx, n_src, what=""):
        want, ok = expect(self.src, self.valid, idx, n_src, self.dst_dt)
        es = self.dst_dt.itemsize
        if self.matrix is None:
            raw = self.buf.cpu().numpy()
            assert (raw[: GUARD * es] == 0x5A).all() and (raw[(GUARD + self.m) * es:] == 0x5A).all(), what
            got = raw[GUARD * es: (GUARD + self.m) * es]
        else:
            got = np.ascontiguousarray(self.matrix.cpu().numpy()[:, self.column]).view(np.uint8)
        wb = want.view(np.uint8) if want.dtype != np.bool_ else want.astype(np.uint8)
        np.testing.assert_array_equal(got, wb.reshape(-1), err_msg=what)
        if self.bm is not None:
            words = self.bm.cpu().numpy()
            assert words[0] == 0x5A5A5A5A5A5A5A5A and words[-1] == 0x5A5A5A5A5A5A5A5A, what
            np.testing.assert_array_equal(words[1:-1].view(np.uint8), pack(ok), err_msg=what)


def run(jobs, idx, m, n_src):
    lib = _lib.load()
    descs = (_lib.TakeCol * len(jobs))()
    for d, j in zip(descs, jobs):
        j.fill(d)
    tidx = torch.from_numpy(idx).cuda() if idx is not None else None
    rc = lib.nvt_batch_take_many(tidx.data_ptr() if tidx is not None else None, m, n_src, descs, len(jobs),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.nvt_last_error()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def sources():
    out = {}
    for dt in SRC_DTYPES:
        out[np.dtype(dt)] = (make_src(dt), RNG.random(N_SRC) >= 0.05)
    return out


def all_jobs(sources, m, with_valid):
    jobs = []
    for dt, (src, valid) in sources.items():
        for dst in dsts_of(dt):
            jobs.append(Job(src, valid if with_valid else None, dst, m))
    return jobs


@pytest.mark.parametrize("m", [1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("kind", ["perm", "repeats"])
def test_take_every_dtype_pair(sources, m, kind):
    idx = RNG.permutation(N_SRC)[:m].astype(np.int64) if kind == "perm" else RNG.integers(0, 50, m).astype(np.int64)
    for with_valid in (True, False):
        jobs = all_jobs(sources, m, with_valid)
        run(jobs, idx, m, N_SRC)
        for j in jobs:
            j.check(idx, N_SRC, f"{j.src.dtype}->{j.dst_dt} m={m} valid={with_valid}")


@pytest.mark.parametrize("m", [65, 2049])
def test_take_identity_index(sources, m):
    jobs = all_jobs(sources, m, True)
    run(jobs, None, m, N_SRC)
    for j in jobs:
        j.check(np.arange(m), N_SRC, f"identity {j.src.dtype}->{j.dst_dt}")


@pytest.mark.parametrize("m", [65, 2049])
def test_take_out_of_range_index(sources, m):
    idx = RNG.permutation(N_SRC)[:m].astype(np.int64)
    for pos, bad in zip((0, 63, 64, m - 1), (-1, N_SRC, 1 << 40, -(1 << 62))):
        idx[pos] = bad
    jobs = all_jobs(sources, m, True) + all_jobs(sources, m, False)
    run(jobs, idx, m, N_SRC)
    for j in jobs:
        j.check(idx, N_SRC, f"out of range {j.src.dtype}->{j.dst_dt}")


def test_take_65_descriptors(sources):
    m = 300
    idx = RNG.permutation(N_SRC)[:m].astype(np.int64)
    src, valid = sources[np.dtype(np.int32)]
    jobs = [Job(src, valid if k % 2 else None, np.int64 if k % 3 else np.int32, m, with_bitmap=bool(k % 2))
            for k in range(65)]
    run(jobs, idx, m, N_SRC)
    for j in jobs:
        j.check(idx, N_SRC)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2049])
@pytest.mark.parametrize("ncols, dst", [(3, np.int64), (26, np.int64), (13, np.float32), (40, np.int64), (5, np.float64)])
def test_take_stacked(sources, m, ncols, dst):
    idx = RNG.permutation(N_SRC)[:m].astype(np.int64)
    idx[m // 2] = -1
    kinds = [k for k in sources if np.dtype(dst).kind == "f" or k.kind in "iub"]
    g = 4     # guard rows before and behind the matrix
    whole = torch.full((m + 2 * g, ncols), 77, dtype=torch.from_numpy(np.zeros(1, dst)).dtype).cuda()
    mat = whole[g: g + m]
    jobs = []
    for c in range(ncols):
        src, valid = sources[kinds[c % len(kinds)]]
        jobs.append(Job(src, valid if c % 2 else None, dst, m, with_bitmap=bool(c % 3 == 0), matrix=mat, column=c))
    lone = Job(*sources[np.dtype(np.float64)], np.float32, m)      # one contiguous descriptor in the same call
    order = list(RNG.permutation(ncols))
    run([jobs[c] for c in order[: ncols // 2]] + [lone] + [jobs[c] for c in order[ncols // 2:]], idx, m, N_SRC)
    lone.check(idx, N_SRC)
    for j in jobs:
        j.check(idx, N_SRC, f"stacked column {j.column}")
    want = np.stack([expect(j.src, j.valid, idx, N_SRC, dst)[0] for j in jobs], axis=1)
    host = whole.cpu().numpy()
    np.testing.assert_array_equal(host[g: g + m].view(np.uint8), want.view(np.uint8))
    assert (host[:g] == 77).all() and (host[g + m:] == 77).all()


def test_take_partial_matrix_is_not_clobbered(sources):
    """Descriptors that cover only some columns of a matrix leave the others alone."""
    m = 300
    idx = RNG.permutation(N_SRC)[:m].astype(np.int64)
    mat = torch.full((m, 4), 77, dtype=torch.int64).cuda()
    src, valid = sources[np.dtype(np.int16)]
    jobs = [Job(src, valid, np.int64, m, matrix=mat, column=c) for c in (1, 3)]
    run(jobs, idx, m, N_SRC)
    for j in jobs:
        j.check(idx, N_SRC)
    host = mat.cpu().numpy()
    assert (host[:, 0] == 77).all() and (host[:, 2] == 77).all()


# ---- lists ------------------------------------------------------------------------------------------
def list_source(off0=7):
    lens = RNG.choice([0, 1, 2, 70], 1000).astype(np.int64)
    lens[100] = 5000
    offsets = np.zeros(1001, np.int64)
    np.cumsum(lens, out=offsets[1:])
    return offsets + off0, int(offsets[-1])


def take_list(offsets, leaves, leaf_valid, dst_dts, idx, m, n_src):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    toff = torch.from_numpy(offsets).cuda()
    tidx = torch.from_numpy(idx).cuda() if idx is not None else None
    pidx = tidx.data_ptr() if tidx is not None else None
    need = C.c_uint64()
    assert lib.nvt_take_list_ws_bytes(m, C.byref(need)) == 0
    ws = torch.empty(need.value // 8, dtype=torch.int64).cuda()
    out_off = torch.full((m + 3,), 0x5A5A, dtype=torch.int64).cuda()
    out_off[1] = 0
    rc = lib.nvt_take_list_offsets(toff.data_ptr(), n_src, pidx, m, out_off.data_ptr() + 8, ws.data_ptr(),
                                   ws.numel() * 8, stream)
    assert rc == 0, lib.nvt_last_error()
    host_off = out_off.cpu().numpy()
    assert host_off[0] == 0x5A5A and host_off[-1] == 0x5A5A
    new_off = host_off[1:-1]
    ii = np.arange(m) if idx is None else idx
    inside = (ii >= 0) & (ii < n_src)
    safe = np.where(inside, ii, 0)
    lens = np.where(inside, offsets[safe + 1] - offsets[safe], 0)
    want_off = np.concatenate([[0], np.cumsum(lens)])
    np.testing.assert_array_equal(new_off, want_off)
    total = int(want_off[-1])
    leaf_idx = np.concatenate([np.arange(offsets[r] - offsets[0], offsets[r + 1] - offsets[0])
                               for r, k in zip(safe, inside) if k] + [np.zeros(0, np.int64)]).astype(np.int64)
    jobs = [Job(lv, leaf_valid, dt, total) for lv, dt in zip(leaves, dst_dts)]
    descs = (_lib.TakeCol * len(jobs))()
    for d, j in zip(descs, jobs):
        j.fill(d)
    rc = lib.nvt_take_list_many(descs, len(jobs), toff.data_ptr(), pidx, out_off.data_ptr() + 8, m, total, stream)
    assert rc == 0, lib.nvt_last_error()
    torch.cuda.synchronize()
    for j in jobs:
        j.check(leaf_idx, len(j.src), "leaves")
    return jobs, new_off, total


@pytest.mark.parametrize("m", [1, 64, 999])
def test_take_lists(m):
    offsets, nleaf = list_source()
    leaves = [RNG.integers(-2**62, 2**62, nleaf), RNG.integers(-2**31, 2**31, nleaf).astype(np.int32),
              RNG.standard_normal(nleaf).astype(np.float32)]
    valid = RNG.random(nleaf) >= 0.05
    for idx in (RNG.permutation(1000)[:m].astype(np.int64), None,
                np.concatenate([[100], RNG.integers(0, 1000, m - 1)]).astype(np.int64)):
        take_list(offsets, leaves, valid, [np.int64, np.int64, np.float32], idx, m, 1000)
    bad = RNG.permutation(1000)[:m].astype(np.int64)
    bad[0], bad[m - 1] = -1, 1 << 40           # an out-of-range index is an empty row
    take_list(offsets, leaves[:2], valid, [np.int64, np.int32], bad, m, 1000)


def test_take_lists_long_run_of_empty_rows():
    lens = np.concatenate([RNG.integers(1, 4, 500), np.zeros(2100, np.int64), RNG.integers(1, 4, 500)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    leaves = [np.arange(offsets[-1], dtype=np.int64)]
    take_list(offsets, leaves, None, [np.int64], None, 3100, 3100)
    idx = np.concatenate([np.arange(400, 2700), RNG.permutation(3100)[:200]]).astype(np.int64)
    take_list(offsets, leaves, None, [np.float64], idx, len(idx), 3100)


def test_take_lists_all_empty():
    offsets = np.full(51, 7, np.int64)
    _, new_off, total = take_list(offsets, [np.zeros(0, np.int64)], None, [np.int64], None, 50, 50)
    assert total == 0 and (new_off == 0).all()


@pytest.mark.parametrize("width", [1, 5])
def test_take_lists_padded_form(width):
    """sparse_as_dense: the gathered column through the padded mode of nvt_list_slice_many."""
    from nvtabular_amd import kernels_list as KL
    from nvtabular_amd import kernels_loader as KD
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    offsets, nleaf = list_source(off0=0)
    leaves = RNG.integers(1, 1000, nleaf)
    frame = DeviceFrame({"s": DeviceColumn(torch.from_numpy(leaves).cuda(), None, torch.from_numpy(offsets).cuda())})
    idx = RNG.permutation(1000)[:333].astype(np.int64)
    got, _ = KD.take_lists(frame, ["s"], torch.from_numpy(idx).cuda())
    values, new_off, _ = got["s"]
    cut = KL.slice_lists(DeviceFrame({"s": DeviceColumn(values, None, new_off)}), ["s"], 0, width, pad_width=width,
                         pad_value=0)["s"]
    want = np.zeros((333, width), np.int64)
    for r, i in enumerate(idx):
        row = leaves[offsets[i]: offsets[i + 1]][:width]
        want[r, : len(row)] = row
    np.testing.assert_array_equal(cut.data.cpu().numpy().reshape(333, width), want)
