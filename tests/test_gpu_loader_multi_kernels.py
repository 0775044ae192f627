"""nvt_batch_take_multi / nvt_take_list_*_multi against numpy: np.concatenate(sources)[index] +
astype, bit for bit (values, offsets, bitmaps, NaN positions), with guard words around every
destination.  Sizes come from the kernel's constants: tile = 256 rows, wave = 64, src_begin staged
in LDS up to 1024 sources."""
import numpy as np
import pytest
import torch

from nvtabular_amd import _lib
from nvtabular_amd import kernels_loader as KD
from nvtabular_amd.device import DeviceColumn, DeviceFrame

pytestmark = pytest.mark.gpu

SRC_DTYPES = [np.bool_, np.uint8, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
CODE = {np.dtype(np.bool_): 4, np.dtype(np.uint8): 4, np.dtype(np.int8): 5, np.dtype(np.int16): 6,
        np.dtype(np.int32): 2, np.dtype(np.int64): 3, np.dtype(np.float32): 0, np.dtype(np.float64): 1}
ORDERS = {"empty_inside": [1, 255, 256, 257, 0, 1000], "empty_first_and_last": [0, 1000, 257, 1, 256, 255, 0],
          "empty_run": [256, 0, 0, 1, 1000, 255, 257]}
GUARD = 16          # elements before and behind every destination
RNG = np.random.default_rng(11)


def dsts_of(src):
    src = np.dtype(src)
    out = [src, np.dtype(np.float32), np.dtype(np.float64)]
    if src.kind in "iub":
        out.append(np.dtype(np.int64))
    return list(dict.fromkeys(out))


def make_src(dt, n):
    dt = np.dtype(dt)
    if dt.kind == "b":
        return RNG.random(n) < 0.5
    if dt.kind == "f":
        v = (RNG.standard_normal(n) * 10.0 ** RNG.integers(-3, 12, n)).astype(dt)
        v[RNG.random(n) < 0.05] = np.nan
        return v
    info = np.iinfo(dt)
    v = RNG.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    v[:4] = [info.min, info.max, 0, info.max - 1][:n]
    return v


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a).cuda()


_ON_DEVICE = {}


def on_device(a, put):
    """The device copy of a source array, made once and never written (the array is kept alive)."""
    if id(a) not in _ON_DEVICE:
        _ON_DEVICE[id(a)] = (a, put(a))
    return _ON_DEVICE[id(a)][1]


def pack(bits):
    b = np.packbits(bits.astype(np.uint8), bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 8, np.uint8)])


def expect(sources, idx, dst_dt):
    """np.concatenate(sources)[index] with every source cast by astype; a source without a bitmap is
    all valid; a row outside the chunk is the null of the destination."""
    with np.errstate(all="ignore"):
        vals = np.concatenate([s.astype(dst_dt) for s, _ in sources] + [np.zeros(1, dst_dt)])
    valid = np.concatenate([v if v is not None else np.ones(len(s), bool) for s, v in sources] + [np.zeros(1, bool)])
    total = len(vals) - 1
    inside = (idx >= 0) & (idx < total)
    safe = np.where(inside, idx, total)
    ok = inside & valid[safe]
    null = np.nan if np.dtype(dst_dt).kind == "f" else 0
    return np.where(ok, vals[safe], np.array(null, dtype=dst_dt)).astype(dst_dt), ok


class Job:
    """One descriptor over several sources, with guarded buffers."""

    def __init__(self, sources, dst_dt, m, with_bitmap=True, matrix=None, column=0):
        self.sources, self.dst_dt, self.m = sources, np.dtype(dst_dt), m
        self.tsrc = [on_device(s, dev) for s, _ in sources]
        self.tvalid = [on_device(v, lambda b: dev(pack(b))) if v is not None else None for _, v in sources]
        self.matrix, self.column = matrix, column
        if matrix is None:
            self.buf = torch.from_numpy(np.full(m + 2 * GUARD, 0x5A, np.uint8).repeat(self.dst_dt.itemsize)).cuda()
        self.bm = torch.full(((m + 63) // 64 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64).cuda() if with_bitmap else None

    def records(self):
        out = []
        for (s, _), t, v in zip(self.sources, self.tsrc, self.tvalid):
            out += [t.data_ptr(), v.data_ptr() if v is not None else 0, CODE[np.dtype(s.dtype)]]
        return out

    def fill(self, d, table_row):
        es = self.dst_dt.itemsize
        d.src = table_row
        if self.matrix is None:
            d.dst, d.dst_stride = self.buf.data_ptr() + GUARD * es, 1
        else:
            d.dst, d.dst_stride = self.matrix.data_ptr() + self.column * es, self.matrix.stride(0)
        d.dst_valid = self.bm.data_ptr() + 8 if self.bm is not None else None
        d.dst_dtype = CODE[self.dst_dt]

    def check(self, idx, what=""):
        want, ok = expect(self.sources, idx, self.dst_dt)
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


def run(jobs, idx, m, sizes):
    lib = _lib.load()
    nsrc = len(sizes)
    begin = KD.src_begin(sizes)
    words = list(begin)
    for j in jobs:
        assert [len(s) for s, _ in j.sources] == list(sizes)
        words += j.records()
    table = torch.tensor(words, dtype=torch.int64).cuda()
    descs = (_lib.TakeCol * len(jobs))()
    for k, (d, j) in enumerate(zip(descs, jobs)):
        j.fill(d, table.data_ptr() + (nsrc + 1 + k * nsrc * 3) * 8)
    tidx = torch.from_numpy(idx).cuda() if idx is not None else None
    rc = lib.nvt_batch_take_multi(tidx.data_ptr() if tidx is not None else None, m, table.data_ptr(), nsrc, begin[-1],
                                  descs, len(jobs), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.nvt_last_error()
    torch.cuda.synchronize()


def chunk(dt, sizes, bitmaps):
    """Sources of one dtype; bitmaps: 'all', 'none' or 'some' (every second source)."""
    out = []
    for k, n in enumerate(sizes):
        has = bitmaps == "all" or (bitmaps == "some" and k % 2 == 0)
        out.append((make_src(dt, n), (RNG.random(n) >= 0.1) if has else None))
    return out


@pytest.fixture(scope="module")
def chunks():
    """Per order: per source dtype the chunk with bitmaps in some sources only, and without any; one
    column whose sources alternate between int32 and int64."""
    out = {}
    for key, sizes in ORDERS.items():
        per = {(np.dtype(dt), b): chunk(dt, sizes, b) for dt in SRC_DTYPES for b in ("some", "none")}
        mixed = [(make_src(np.int32 if k % 2 else np.int64, n), (RNG.random(n) >= 0.1) if k % 3 == 0 else None)
                 for k, n in enumerate(sizes)]
        out[key] = (sizes, per, mixed)
    return out


def all_jobs(per, mixed, m, bitmaps):
    jobs = [Job(per[(np.dtype(dt), bitmaps)], dst, m) for dt in SRC_DTYPES for dst in dsts_of(dt)]
    return jobs + [Job(mixed, np.int64, m), Job(mixed, np.float64, m)]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 256, 257, 700])
@pytest.mark.parametrize("order", list(ORDERS))
def test_multi_every_dtype_pair(chunks, order, m):
    sizes, per, mixed = chunks[order]
    total = sum(sizes)
    idx = RNG.permutation(total)[:m].astype(np.int64)
    idx[0] = RNG.choice(KD.src_begin(sizes)[:-1])             # the first row of some source
    for bitmaps in ("some", "none"):
        jobs = all_jobs(per, mixed, m, bitmaps)
        run(jobs, idx, m, sizes)
        for j in jobs:
            j.check(idx, f"{j.sources[0][0].dtype}->{j.dst_dt} m={m} bitmaps={bitmaps}")


@pytest.mark.parametrize("m", [65, 257, 1769])
def test_multi_identity_index(chunks, m):
    sizes, per, mixed = chunks["empty_first_and_last"]
    jobs = all_jobs(per, mixed, m, "some")
    run(jobs, None, m, sizes)
    for j in jobs:
        j.check(np.arange(m), f"identity {j.sources[0][0].dtype}->{j.dst_dt}")


@pytest.mark.parametrize("m", [65, 700])
def test_multi_out_of_range_index(chunks, m):
    sizes, per, mixed = chunks["empty_inside"]
    total = sum(sizes)
    idx = RNG.integers(0, total, m).astype(np.int64)
    for pos, bad in zip((0, 5, 63, 64, m - 2, m - 1), (-1, total, 1 << 40, -(1 << 62), total, -1)):
        idx[pos] = bad
    jobs = all_jobs(per, mixed, m, "some") + all_jobs(per, mixed, m, "none")
    run(jobs, idx, m, sizes)
    for j in jobs:
        j.check(idx, f"out of range {j.sources[0][0].dtype}->{j.dst_dt}")


def test_multi_65_descriptors(chunks):
    sizes, per, mixed = chunks["empty_run"]
    m = 300
    idx = RNG.permutation(sum(sizes))[:m].astype(np.int64)
    jobs = [Job(per[(np.dtype(np.int32), "some" if k % 2 else "none")], np.int64 if k % 3 else np.int32, m,
                with_bitmap=bool(k % 2)) for k in range(64)] + [Job(mixed, np.int64, m)]
    run(jobs, idx, m, sizes)
    for j in jobs:
        j.check(idx)


def stacked_jobs(per, mixed, mat, dst, m):
    kinds = [dt for dt in map(np.dtype, SRC_DTYPES) if np.dtype(dst).kind == "f" or dt.kind in "iub"]
    jobs = []
    for c in range(mat.shape[1]):
        src = mixed if c == 1 and np.dtype(dst) == np.int64 else per[(kinds[c % len(kinds)], "some" if c % 2 else "none")]
        jobs.append(Job(src, dst, m, with_bitmap=c % 3 == 0, matrix=mat, column=c))
    return jobs


def check_matrix(whole, g, m, jobs, idx, dst):
    for j in jobs:
        j.check(idx, f"stacked column {j.column}")
    want = np.stack([expect(j.sources, idx, dst)[0] for j in jobs], axis=1)
    host = whole.cpu().numpy()
    np.testing.assert_array_equal(np.ascontiguousarray(host[g: g + m]).view(np.uint8), want.view(np.uint8))
    assert (host[:g] == 77).all() and (host[g + m:] == 77).all()


@pytest.mark.parametrize("m", [1, 255, 256, 257, 700])
def test_multi_stacked_two_matrices_in_one_launch(chunks, m):
    """[m, 13] float32 and [m, 26] int64 in one launch, with one contiguous column between them."""
    sizes, per, mixed = chunks["empty_first_and_last"]
    idx = RNG.permutation(sum(sizes))[:m].astype(np.int64)
    idx[m // 2] = -1
    g = 4     # guard rows before and behind every matrix
    wf = torch.full((m + 2 * g, 13), 77, dtype=torch.float32).cuda()
    wi = torch.full((m + 2 * g, 26), 77, dtype=torch.int64).cuda()
    jf = stacked_jobs(per, mixed, wf[g: g + m], np.float32, m)
    ji = stacked_jobs(per, mixed, wi[g: g + m], np.int64, m)
    lone = Job(per[(np.dtype(np.float64), "some")], np.float32, m)
    order = list(RNG.permutation(26))
    run(jf[:6] + [ji[c] for c in order[:13]] + [lone] + jf[6:] + [ji[c] for c in order[13:]], idx, m, sizes)
    lone.check(idx)
    check_matrix(wf, g, m, jf, idx, np.float32)
    check_matrix(wi, g, m, ji, idx, np.int64)


@pytest.mark.parametrize("ncols, dst, g", [(13, np.float32, 3), (3, np.int64, 1), (25, np.int64, 1)])
def test_multi_stacked_at_an_unaligned_row_offset(chunks, ncols, dst, g):
    """The spill case: the matrix starts g rows into its buffer, not on a 16-byte boundary."""
    sizes, per, mixed = chunks["empty_inside"]
    m = 300
    assert (g * ncols * np.dtype(dst).itemsize) % 16
    idx = RNG.permutation(sum(sizes))[:m].astype(np.int64)
    whole = torch.full((m + 2 * g, ncols), 77, dtype=torch.from_numpy(np.zeros(1, dst)).dtype).cuda()
    jobs = stacked_jobs(per, mixed, whole[g: g + m], dst, m)
    run(jobs, idx, m, sizes)
    check_matrix(whole, g, m, jobs, idx, dst)


def test_multi_widest_rows_leave_no_room_to_stage_src_begin(chunks):
    """Rows of 256 bytes fill the 64 KiB of the tile image: src_begin is searched in memory."""
    sizes, per, mixed = chunks["empty_run"]
    m, g = 513, 2
    idx = RNG.permutation(sum(sizes))[:m].astype(np.int64)
    whole = torch.full((m + 2 * g, 32), 77, dtype=torch.int64).cuda()
    jobs = stacked_jobs(per, mixed, whole[g: g + m], np.int64, m)
    run(jobs, idx, m, sizes)
    check_matrix(whole, g, m, jobs, idx, np.int64)


@pytest.mark.parametrize("nsrc", [1024, 1025, 4096])
def test_multi_many_sources(nsrc):
    """1024 sources still fit the staged copy of src_begin (1025 entries); more are searched in memory."""
    sizes = RNG.integers(0, 4, nsrc).tolist()
    sizes[0], sizes[-1] = 0, 0
    total, m = sum(sizes), 700
    src = [(make_src(np.int32 if k % 2 else np.int64, n), (RNG.random(n) >= 0.2) if k % 5 == 0 else None)
           for k, n in enumerate(sizes)]
    idx = RNG.integers(0, total, m).astype(np.int64)
    idx[:3] = [total - 1, 0, total]
    mat = torch.full((m, 2), 77, dtype=torch.int64).cuda()
    jobs = [Job(src, np.int64, m), Job(src, np.float32, m, with_bitmap=False)] + \
        [Job(src, np.int64, m, matrix=mat, column=c) for c in (0, 1)]
    run(jobs, idx, m, sizes)
    for j in jobs:
        j.check(idx, f"nsrc={nsrc}")


def test_take_frames_driver(chunks):
    """kernels_loader.take_frames: plan, matrices and the source table built by the driver."""
    sizes, per, mixed = chunks["empty_inside"]
    names = {"a": per[(np.dtype(np.int16), "some")], "b": mixed, "x": per[(np.dtype(np.float64), "none")]}
    frames = []
    for s in range(len(sizes)):
        frames.append(DeviceFrame({n: DeviceColumn(dev(src[s][0]), dev(pack(src[s][1])) if src[s][1] is not None else None)
                                   for n, src in names.items()}))
    m = 500
    idx = RNG.permutation(sum(sizes))[:m].astype(np.int64)
    cats = torch.full((m + 3, 2), 77, dtype=torch.int64).cuda()
    x = torch.full((m,), 77, dtype=torch.float32).cuda()
    bm = torch.zeros(KD.bitmap_bytes(m), dtype=torch.uint8).cuda()
    KD.take_frames(frames, torch.from_numpy(idx).cuda(), [KD.Take("a", cats, column=0, row=3),
                                                          KD.Take("b", cats, column=1, row=3),
                                                          KD.Take("x", x, dst_valid=bm)])
    host = cats.cpu().numpy()
    assert (host[:3] == 77).all()
    np.testing.assert_array_equal(host[3:, 0], expect(names["a"], idx, np.int64)[0])
    np.testing.assert_array_equal(host[3:, 1], expect(names["b"], idx, np.int64)[0])
    want, ok = expect(names["x"], idx, np.float32)
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(bm.cpu().numpy(), pack(ok))


# ---- lists ------------------------------------------------------------------------------------------
def list_chunk(sizes, long_row=True, all_empty=False):
    """Per source: offsets that do not start at 0, two leaf columns that share them, leaf bitmaps in
    every second source only."""
    out = []
    for k, n in enumerate(sizes):
        lens = np.zeros(n, np.int64) if all_empty else RNG.choice([0, 0, 1, 2, 70], n).astype(np.int64)
        if long_row and n > 100:
            lens[100] = 5000                # one row longer than two leaf tiles
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        nleaf, off0 = int(off[-1]), 7 * k + 3
        pad = RNG.integers(-9, 9, off0)     # leaves in front of the source's first row
        ids = RNG.integers(-2**40, 2**40, nleaf) if k % 2 else RNG.integers(-2**31, 2**31, nleaf).astype(np.int32)
        w = RNG.standard_normal(nleaf).astype(np.float32)
        valid = (RNG.random(nleaf + off0) >= 0.1) if k % 2 == 0 else None
        out.append({"off": off + off0, "ids": np.concatenate([pad.astype(ids.dtype), ids]),
                    "w": np.concatenate([pad.astype(np.float32), w]), "valid": valid, "off0": off0})
    return out


def list_frames(srcs):
    frames = []
    for s in srcs:
        # (the bitmap and the leaves start at the column's leaf 0, which is offsets[0] leaves into the buffers
        #  the source was cut from: the views below start there)
        off0 = s["off0"]
        valid = dev(pack(s["valid"][off0:])) if s["valid"] is not None else None
        toff = dev(s["off"])
        frames.append(DeviceFrame({"ids": DeviceColumn(dev(s["ids"])[off0:], valid, toff),
                                   "w": DeviceColumn(dev(s["w"])[off0:], valid, toff)}))
    return frames


def list_expect(srcs, idx):
    sizes = [len(s["off"]) - 1 for s in srcs]
    begin = np.array(KD.src_begin(sizes))
    lens, ids, w, ok = [], [], [], []
    for i in idx:
        if not 0 <= i < begin[-1]:
            lens.append(0)
            continue
        k = int(np.searchsorted(begin[:-1], i, side="right") - 1)
        s, r = srcs[k], int(i - begin[k])
        a, b = s["off"][r], s["off"][r + 1]
        lens.append(b - a)
        ids.append(s["ids"][a:b].astype(np.int64))
        w.append(s["w"][a:b])
        ok.append(s["valid"][a:b] if s["valid"] is not None else np.ones(b - a, bool))
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)     # noqa: E731
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), cat(ids, np.int64), cat(w, np.float32), cat(ok, bool)


def check_lists(srcs, idx, m, cuts):
    frames = list_frames(srcs)
    tidx = torch.from_numpy(idx).cuda() if idx is not None else None
    want = torch.tensor(cuts, dtype=torch.int64).cuda()
    before = dict(KD.K.STATS)
    got, bounds = KD.take_lists_multi(frames, ["ids", "w"], tidx, m, want_offsets=want, dtypes={"ids": torch.int64})
    assert KD.K.STATS.get("loader_list_readback", 0) - before.get("loader_list_readback", 0) == (1 if m else 0)
    off, ids, w, ok = list_expect(srcs, np.arange(m) if idx is None else idx)
    assert got["ids"][1] is got["w"][1]                 # the columns still share their offsets
    np.testing.assert_array_equal(got["ids"][1].cpu().numpy(), off)
    np.testing.assert_array_equal(got["ids"][0].cpu().numpy(), np.where(ok, ids, 0))
    assert got["ids"][0].dtype == torch.int64 and got["w"][0].dtype == torch.float32
    gw = got["w"][0].cpu().numpy()
    np.testing.assert_array_equal(np.isnan(gw), ~ok)
    np.testing.assert_array_equal(gw[ok], w[ok])
    for name in ("ids", "w"):
        if any(s["valid"] is not None for s in srcs):       # a leaf bitmap comes out when any source has one
            np.testing.assert_array_equal(got[name][2].cpu().numpy(), pack(ok))
        else:
            assert got[name][2] is None
        np.testing.assert_array_equal(np.asarray(bounds[name]), off[cuts])
    return got


@pytest.mark.parametrize("m", [1, 64, 257, 1769])
@pytest.mark.parametrize("order", ["empty_inside", "empty_first_and_last"])
def test_multi_lists(order, m):
    sizes = ORDERS[order]
    srcs = list_chunk(sizes)
    total = sum(sizes)
    cuts = sorted({0, m // 3, m // 2, m})
    perm = RNG.permutation(total)[:m].astype(np.int64)
    check_lists(srcs, perm, m, cuts)
    check_lists(srcs, None, m, cuts)                                         # identity
    long_first = np.concatenate([[KD.src_begin(sizes)[sizes.index(1000)] + 100], RNG.integers(0, total, m - 1)])
    check_lists(srcs, long_first.astype(np.int64), m, cuts)
    bad = perm.copy()
    bad[0], bad[m - 1] = -1, total           # an out-of-range index is an empty row
    check_lists(srcs, bad, m, cuts)


def test_multi_lists_all_empty_chunk():
    srcs = list_chunk([5, 0, 300], long_row=False, all_empty=True)
    got = check_lists(srcs, RNG.permutation(305).astype(np.int64), 305, [0, 100, 305])
    assert got["ids"][0].numel() == 0 and int(got["ids"][1].abs().sum()) == 0


def test_multi_lists_long_run_of_empty_rows():
    """More rows than one leaf tile's staged offsets between two leaves: the unstaged row search."""
    lens = [np.concatenate([RNG.integers(1, 4, 300), np.zeros(1500, np.int64)]), np.zeros(900, np.int64),
            np.concatenate([np.zeros(100, np.int64), RNG.integers(1, 4, 300)])]
    srcs = []
    for k, ln in enumerate(lens):
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        n = int(off[-1])
        srcs.append({"off": off, "ids": np.arange(n, dtype=np.int64) + 1000 * k, "w": np.arange(n, dtype=np.float32),
                     "valid": None, "off0": 0})
    check_lists(srcs, None, 3100, [0, 1800, 3100])


def test_multi_lists_more_sources_than_the_staged_table():
    sizes = [2] * 1100
    srcs = list_chunk(sizes, long_row=False)
    check_lists(srcs, RNG.permutation(2200)[:700].astype(np.int64), 700, [0, 333, 700])
