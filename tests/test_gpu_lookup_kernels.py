"""Kernel-level matrix for the KEY and RECORD side of the JoinGroupby / TargetEncoding transform: the
flat index, the key directory and the two kernels that read the packed per-group records ("lookup
images").  Every entry point is called through ``_lib.load()`` on plain torch tensors and every
output is compared with the numpy references of lookup_reference.py, which test_lookup_reference.py
pins to a dict lookup and to records written by hand on the CPU.  Nothing is compared kernel to
kernel.  Output buffers are pre-filled with a poison byte (0xA5), so an element a kernel did not
write shows; every device tensor a launch reads is held in a variable until its output is back.

    helper           entry point                  kernels reached
    Index (flat)     nvt_flat_index_tmp_bytes,    flat_params_kernel, flat_build_kernel (+ the table
                     nvt_flat_index_build         clear)
    Index (keydir)   nvt_keydir_build             keydir_first_kernel, keydir_keys_kernel
    flat_lookup      nvt_flat_lookup              flat_lookup_kernel<int32 / int64>
    image_lookup     nvt_flat_lookup_image,       flat_lookup_image_kernel<K, 2 / 4 / 8 / 16 / 24>,
                     nvt_keydir_lookup_image      keydir_lookup_image_kernel<K, 2 / 4 / 8 / 16 / 24>

Sizes, from the constants of the sources (kBlock = 256, stream_grid(n, 512, 8) capped at 2048
workgroups): every thread takes a second row from n = 257 on, a second workgroup exists from
n = 513, a third trip of the grid-stride loop only beyond 2048 * 512 rows -- 0, 1, 63, 64, 65, 255,
256, 257, 511, 512, 513, 1 048 576 and 1 048 576 + 513 rows.  The two large cases are the only ones
over a few thousand rows: the extra trip does not exist below them.

Everything here moves bytes: positions, group ids and record reads are compared bit for bit.

One thing cannot be built: more shared 16-byte windows than MAXC / 2.  A window needs two members
and MAXC >= ncols, so an output never falls back to its own load because the windows ran out; the
densest case (ncols = MAXC, every window a pair) is in test_record_layouts.

Argument checks: the seven rejections of the entry points of this family (NVT_EINVAL with a
message, nothing launched) have one assertion each in test_argument_checks.

Left out, by name: the four record BUILDERS (nvt_image_pack, nvt_jg_image, nvt_te_image,
nvt_image_build) and the per-row kernels (nvt_flat_lookup_gather, nvt_flat_lookup_te, nvt_te_apply,
nvt_te_apply_folds, nvt_gather_f64) -- their references (jg_stats, te_values, te_values_exact,
build_image) are in lookup_reference.py and pinned on the CPU, the device side is still compared
with itself in test_gpu_lookup_image.py / test_gpu_keydir.py and, for te_apply / gather, with
cont_reference.py in test_gpu_cont_kernels.py; fold ids >= kfold (the caller's contract); string
keys and multi-rank merges; the retry and demotion logic of ops/_groupby.py; timing.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import lookup_reference as R

pytestmark = pytest.mark.gpu

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
TRIP = 2048 * 512
ROWS_SMALL = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513]
ROWS_LARGE = [TRIP, TRIP + 513]
PATHS = ["flat", "keydir"]
POISON = 0xA5
CODE = {"float32": 0, "float64": 1, "int32": 2, "int64": 3}       # include/nvt_hip.h NVT_F32 ..
NP = {"int32": np.int32, "int64": np.int64}


class Lib:
    def __init__(self):
        from nvtabular_amd import _lib
        from nvtabular_amd import kernels as K

        self.m, self.lib, self.K = _lib, _lib.load(), K
        assert [_lib.NVT_F32, _lib.NVT_F64, _lib.NVT_I32, _lib.NVT_I64] == list(CODE.values())
        self.AUX_WORDS, self.MAXDISP = K.FlatIndex.FLAT_AUX_WORDS, K.FlatIndex.FLAT_AUX_MAXDISP
        self.NULLGROUP = self.MAXDISP + 2                            # NVT_FLAT_AUX_NULLGROUP

    def call(self, name, *args):
        self.m.check(getattr(self.lib, name)(*args, self.K.stream_ptr()), name)

    def refused(self, name, *args):
        """The call returns NVT_EINVAL and leaves a message that names it."""
        assert getattr(self.lib, name)(*args, self.K.stream_ptr()) == -1, name         # NVT_EINVAL
        msg = self.lib.nvt_last_error()
        assert msg and name.encode() in msg, msg
        return msg.decode()


@pytest.fixture(scope="module")
def L():
    return Lib()


@pytest.fixture(scope="module", autouse=True)
def _free():
    _CACHE.clear()
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


_CACHE = {}


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.cpu().numpy()


def poison(n, dtype):
    return torch.full((max(n, 1) * np.dtype(dtype).itemsize,), POISON, dtype=torch.uint8, device="cuda")


def as_np(t, n, dtype):
    return host(t).view(dtype)[:n]


def ok(msg):
    assert msg is None, msg


def u32s(v):
    return (C.c_uint32 * max(len(v), 1))(*[int(x) for x in v])


def u64s(v):
    return (C.c_uint64 * max(len(v), 1))(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in v])


def ptrs(L, ts):
    return L.m.ptr_array([None if t is None else t.data_ptr() for t in ts])


def p_(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------
# helpers: one per entry point
# ---------------------------------------------------------------------------------------------
class Index:
    """Both indexes of one ascending int32 key list: the flat table (nvt_flat_index_build) with
    ``slots`` home slots and the key directory (nvt_keydir_build) with ``B`` buckets, the latter
    read back and held against its definition."""

    def __init__(self, L, ids, load=1.0, slots=None):
        ids = np.ascontiguousarray(ids, np.int32)
        self.L, self.ids, self.n = L, ids, ids.size
        n = ids.size
        self.keys = dev(ids)
        self.slots = int(slots or max(64, int(n / min(load, 8.0) * 2) + 1))
        self.capacity = self.slots + n + 64
        self.table = torch.full((self.capacity,), 0x0505050505050505, dtype=torch.int64, device="cuda")
        self.aux = torch.zeros(L.AUX_WORDS, dtype=torch.int32, device="cuda")
        need = C.c_uint64()
        L.m.check(L.lib.nvt_flat_index_tmp_bytes(n, C.byref(need)), "nvt_flat_index_tmp_bytes")
        tmp = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device="cuda")
        L.call("nvt_flat_index_build", self.keys.data_ptr(), n, self.slots, self.aux.data_ptr(),
               self.table.data_ptr(), self.capacity, tmp.data_ptr())
        self.B = max(1, int(n / load))
        self.dir = torch.full((4 * (self.B + 1),), 0x25252525, dtype=torch.int32, device="cuda")
        L.call("nvt_keydir_build", self.keys.data_ptr(), n, self.B, self.dir.data_ptr())
        self.dir_host = host(self.dir)
        R.check_keydir(self.dir_host, ids, self.B)
        self.bucket_sizes = np.diff(self.dir_host.view(np.uint32).reshape(-1, 4)[:, 0].astype(np.int64))

    def set_null_group(self, g):
        self.aux[self.L.NULLGROUP] = int(g) + 1

    def maxdisp(self):
        return int(self.aux[self.L.MAXDISP].item()) & 0xFFFFFFFF


def flat_lookup(L, ix, rows, valid=None, key_offset=0):
    n = rows.size
    out = poison(n, np.int64)
    vb = None if valid is None else dev(R.pack_bits(valid))
    keys = dev(rows)
    L.call("nvt_flat_lookup", p_(keys), CODE[rows.dtype.name], p_(vb), n, ix.aux.data_ptr(),
           ix.table.data_ptr(), ix.capacity, key_offset, out.data_ptr())
    return as_np(out, n, np.int64)


def image_lookup(L, path, ix, rows, image, stride, cols, valid=None, key_offset=0, null_group=-1,
                 gid_in=None, want_gid=False):
    """cols: [(byte offset, size, fold ids uint8 or None, miss bits)] -> ([uint32 / uint64 per
    column], *unseen, gid_out or None) through nvt_flat_lookup_image / nvt_keydir_lookup_image."""
    n, nc = rows.size, len(cols)
    outs = [poison(n, np.uint32 if c[1] == 4 else np.uint64) for c in cols]
    folds = [None if c[2] is None else dev(np.asarray(c[2], np.uint8)) for c in cols]
    flag = torch.zeros(1, dtype=torch.int64, device="cuda")
    vb = None if valid is None else dev(R.pack_bits(valid))
    keys = dev(rows)
    tail = (image.data_ptr(), stride, nc, ptrs(L, outs), ptrs(L, folds), u32s([c[0] for c in cols]),
            u32s([c[1] for c in cols]), u64s([c[3] for c in cols]), flag.data_ptr())
    gid = None
    if path == "flat":
        ix.set_null_group(null_group)
        gin = None if gid_in is None else dev(np.asarray(gid_in, np.int32))
        gid = poison(n, np.int32) if want_gid else None
        L.call("nvt_flat_lookup_image", p_(keys), CODE[rows.dtype.name], p_(vb), n, ix.aux.data_ptr(),
               ix.table.data_ptr(), ix.capacity, key_offset, p_(gin), p_(gid), *tail)
        gid = as_np(gid, n, np.int32) if want_gid else None
    else:
        L.call("nvt_keydir_lookup_image", p_(keys), CODE[rows.dtype.name], p_(vb), n, ix.dir.data_ptr(), ix.B,
               ix.keys.data_ptr(), ix.n, key_offset, null_group, *tail)
    got = [as_np(o, n, np.uint32 if c[1] == 4 else np.uint64) for o, c in zip(outs, cols)]
    return got, int(flag.item()), gid


def check_positions(L, path, ix, rows, valid=None, key_offset=0, null_group=-1, what="", exp=None):
    """Group id per row against R.position: nvt_flat_lookup and nvt_flat_lookup_image (gid_out,
    record g = the int64 g), or nvt_keydir_lookup_image; *unseen is 1 exactly when a row misses."""
    if exp is None:
        exp = R.position(ix.ids, rows, valid, key_offset, null_group)
    recs = ix.n + 1
    image = torch.arange(recs, dtype=torch.int64, device="cuda")
    got, flag, gid = image_lookup(L, path, ix, rows, image, 8, [(0, 8, None, -1)], valid, key_offset, null_group,
                                  want_gid=True)
    ok(R.bits_mismatch(got[0].view(np.int64), exp, what=f"{what} {path} image record"))
    assert flag == int((exp < 0).any()), f"{what} {path}: *unseen {flag}"
    if path == "flat":
        ok(R.bits_mismatch(gid, exp.astype(np.int32), what=f"{what} gid_out"))
        ok(R.bits_mismatch(flat_lookup(L, ix, rows, valid, key_offset), exp, what=f"{what} nvt_flat_lookup"))
    return exp


def probe_rows(rng, ids, n, dtype, key_offset=0):
    """n rows: three quarters keys of the list, the rest their neighbours and values of the whole
    int32 window (all moved by key_offset)."""
    k = ids.astype(np.int64)[rng.integers(0, ids.size, n)]
    r = rng.random(n)
    k = np.where(r < 0.1, np.minimum(k + 1, I32.max), k)
    k = np.where((r >= 0.1) & (r < 0.2), np.maximum(k - 1, I32.min), k)
    k = np.where(r >= 0.9, rng.integers(I32.min, I32.max, n, endpoint=True), k)
    return (k + key_offset).astype(dtype)


def some_ids(rng, n):
    return np.unique(rng.integers(I32.min, I32.max, n, endpoint=True)).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# key lookup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("path", PATHS)
def test_lookup_row_counts(L, path, dtype):
    rng = np.random.default_rng(seed_of("rows", path, dtype))
    ids = some_ids(rng, 300)
    ix = Index(L, ids)
    for n in ROWS_SMALL:
        rows = probe_rows(rng, ids, n, NP[dtype])
        valid = rng.random(n) > 0.1 if n % 2 else None
        exp = check_positions(L, path, ix, rows, valid, what=f"n={n}")
        assert n < 63 or ((exp >= 0).any() and (exp < 0).any())
    hits = ids[rng.integers(0, ids.size, 513)].astype(NP[dtype])              # a case without a miss: flag 0
    assert (check_positions(L, path, ix, hits, what="all hits") >= 0).all()


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("path", PATHS)
def test_lookup_third_trip(L, path, dtype):
    """Beyond 2048 * 512 rows the grid-stride loop makes a third trip."""
    key = ("large", dtype)
    if key not in _CACHE:
        rng = np.random.default_rng(seed_of(*key))
        ids = some_ids(rng, 5000)
        off = 0 if dtype == "int32" else 3_000_000_000_000
        rows = probe_rows(rng, ids, ROWS_LARGE[-1], NP[dtype], off)
        _CACHE[key] = ids, off, rows, R.position(ids, rows, None, off)
    ids, off, rows, exp = _CACHE[key]
    ix = Index(L, ids)
    for n in ROWS_LARGE:
        check_positions(L, path, ix, rows[:n], None, off, what=f"n={n}", exp=exp[:n])


def _edge_rows(ids):
    near = ids.astype(np.int64)[:, None] + np.array([-1, 0, 1])[None, :]
    fixed = [I32.min, I32.min + 1, -1, 0, 1, I32.max - 1, I32.max]
    return np.unique(np.clip(np.concatenate([near.reshape(-1), fixed]), I32.min, I32.max)).astype(np.int32)


@pytest.mark.parametrize("path", PATHS)
def test_key_lists_and_loads(L, path):
    """Lists of 1, 2, 3, 4 and 64 keys, INT32_MIN / INT32_MAX in the list (has_min of the flat
    table, m == 0 of range_map_params), dense keys under many more buckets than keys (sh > 0), at
    directory loads 0.25, 1, 3 and 64: every key, its neighbours and the ends of the window."""
    lists = [[7], [I32.min], [I32.max], [-3, 9], [I32.min, I32.max], [I32.min, I32.min + 1], [1, 2, 3],
             [I32.min, 0, I32.max], [-5, 0, 5, 6], [I32.min, -3, 0, 5, I32.max], list(range(100, 164)),
             list(range(I32.max - 63, I32.max + 1)), list(range(I32.min, I32.min + 64)),
             list(range(-(2**30), 2**30, 2**25))]
    for ids in lists:
        ids = np.array(ids, np.int32)
        rows = _edge_rows(ids)
        for load in (0.25, 1.0, 3.0, 64.0):
            ix = Index(L, ids, load=load)
            check_positions(L, path, ix, rows, what=f"{ids[:3]}.. x{ids.size} load {load}")
    rng = np.random.default_rng(seed_of("loads"))
    ids = some_ids(rng, 3000)
    rows = probe_rows(rng, ids, 4000, np.int32)
    for load in (0.25, 1.0, 3.0, 64.0):
        check_positions(L, path, Index(L, ids, load=load), rows, what=f"3000 keys load {load}")
    # a dense list under 2^20 buckets / slots: the integer-factor map
    ids = np.arange(1000, 1200, dtype=np.int32)
    ix = Index(L, ids, load=200 / 2**20, slots=2**20)
    check_positions(L, path, ix, _edge_rows(ids), what="dense, 2^20 buckets")


@pytest.mark.parametrize("path", PATHS)
def test_buckets_of_1_2_3_4_7_8_and_9_keys(L, path):
    """keydir_find: three keys inside the directory entry, kDirSteps = 4 walked from first + 3,
    then bisection.  Clusters of c keys two apart, the clusters 2^20 apart, one key per bucket on
    average: a cluster shares a bucket.  Every key is probed, and every gap."""
    sizes = [1, 2, 3, 4, 7, 8, 9, 5, 12, 16] * 6
    rng = np.random.default_rng(seed_of("buckets"))
    rng.shuffle(sizes)
    ids = np.concatenate([-(2**29) + j * 2**20 + 2 * np.arange(c) for j, c in enumerate(sizes)]).astype(np.int32)
    ix = Index(L, ids, load=1.0)
    assert {1, 2, 3, 4, 7, 8, 9} <= set(ix.bucket_sizes.tolist()), sorted(set(ix.bucket_sizes.tolist()))
    rows = _edge_rows(ids)
    exp = check_positions(L, path, ix, rows, what="clusters")
    assert (exp >= 0).sum() == ids.size
    check_positions(L, path, ix, rows.astype(np.int64) + 77, None, 77, what="clusters int64")


def test_flat_runs_longer_than_the_linear_probe(L, monkeypatch):
    """K consecutive keys and one key 2^30 away: the monotone map sends a key offset d to home slot
    floor(d * factor) with factor <= slots / (span + 1), so every d < (span + 1) / slots has home
    slot 0 and the layout rule p_i = max(h_i, p_(i-1) + 1) puts key i at slot i: the reported
    displacement is K - 1, and a lookup of the later keys leaves the 8 linear steps (galloping)."""
    from nvtabular_amd import kernels as K

    monkeypatch.setattr(K, "KEYED_IMAGES", False)                # (the driver lays the table out at once)
    for count, fine in ((40, True), (5000, False)):
        ids = np.concatenate([np.arange(count), [2**30]]).astype(np.int32)
        slots = max(64, int(ids.size / 0.5) + 1)
        assert count < (2**30 + 1) // slots
        home = np.zeros(count, np.int64)
        disp = int((R.flat_positions(home) - home).max())
        assert disp == count - 1
        ix = Index(L, ids, slots=slots)
        assert ix.maxdisp() == disp
        rows = np.concatenate([np.arange(-3, count + 3), [2**30 - 1, 2**30, 2**30 + 1]]).astype(np.int32)
        check_positions(L, "flat", ix, rows, what=f"run of {count}")
        index = K.FlatIndex(dev(ids))
        assert index.slots == slots and index.ok() == (disp <= K.FlatIndex.MAX_DISPLACEMENT) == fine


@pytest.mark.parametrize("path", PATHS)
def test_int64_offsets_overflow_window_and_nulls(L, path):
    rng = np.random.default_rng(seed_of("int64", path))
    ids = np.unique(np.concatenate([some_ids(rng, 400), [I32.min, I32.max]])).astype(np.int32)
    ix = Index(L, ids)
    for off in (-7_000_000_000_000, 5_000_000_000, 2**31, -(2**31), I64.max - 5, I64.min + 5, 1, -1):
        lo, hi = max(I64.min, off + I32.min), min(I64.max, off + I32.max)
        inside = np.array([k for k in (ids.astype(object) + off) if lo <= k <= hi], np.int64)
        edge = [I64.min, I64.min + 1, I64.max - 1, I64.max, 0, lo, hi]
        edge += [lo - 1] if lo > I64.min else []                 # one below / above the int32 window
        edge += [hi + 1] if hi < I64.max else []
        rows = np.concatenate([inside[rng.integers(0, inside.size, 600)], np.array(edge, np.int64),
                               rng.integers(lo, hi, 100, endpoint=True)])
        valid = rng.random(rows.size) > 0.15
        exp = check_positions(L, path, ix, rows, None, off, what=f"offset {off}")
        assert (exp >= 0).sum() >= 600
        check_positions(L, path, ix, rows, valid, off, -1, what=f"offset {off} nulls miss")
        check_positions(L, path, ix, rows, valid, off, ix.n, what=f"offset {off} null group")
    # int32 columns with a validity bitmap whose bytes under a null are keys of the list
    rows = ids[rng.integers(0, ids.size, 700)]
    valid = rng.random(700) > 0.5
    check_positions(L, path, ix, rows, valid, 0, -1, what="int32 nulls miss")
    exp = check_positions(L, path, ix, rows, valid, 0, ix.n, what="int32 null group")
    assert (exp >= 0).all()                                      # (flag 0: the null group is a group)


# ---------------------------------------------------------------------------------------------
# record layouts
# ---------------------------------------------------------------------------------------------
def _layout(rng, ncols, stride, kfold, dense=False):
    """[(offset, size, per_fold)]: 4- and 8-byte values, fold-indexed and fixed; outputs 0 and 1
    share a 16-byte window with an 8-byte value at window offset 8; output 2 asks for the offset
    of output 0 again; with 8 or more outputs every second one pairs up with its predecessor's
    window.  dense: ncols / 2 windows of two fixed outputs each, as many as the kernel holds (one
    pair asks for the same 8 bytes twice)."""
    if dense:
        wins = 16 * rng.permutation(stride // 16)[:ncols // 2]
        cols = []
        for w in wins:
            cols += [(int(w) + 4 * int(rng.integers(0, 4)), 4, False), (int(w) + 8 * int(rng.integers(0, 2)), 8, False)]
        if ncols >= 4:
            cols[2] = cols[3]
        return cols
    cols = []
    for c in range(ncols):
        size = int(rng.choice([4, 8]))
        per_fold = bool(kfold > 0 and rng.random() < 0.3)
        span = size * (kfold + 1 if per_fold else 1)
        off = int(rng.integers(0, (stride - span) // size + 1)) * size
        cols.append((off, size, per_fold))
    if kfold == 256:                                             # slot 256 ends with the record
        cols[3], cols[4] = (stride - 8 * 257, 8, True), (8, 4, True)
    win = 16 * int(rng.integers(0, stride // 16)) if stride % 16 == 0 else 0
    if stride >= 16:
        cols[0] = (win + int(rng.choice([0, 4])), 4, False)
        if ncols >= 2:
            cols[1] = (win + 8, 8, False)
        if ncols >= 3:
            cols[2] = cols[0]
    if ncols >= 8 and stride % 16 == 0:                          # as many windows as the kernel holds
        for c in range(4, ncols, 2):
            w = 16 * int(rng.integers(0, stride // 16))
            cols[c - 1] = (w + 4 * int(rng.integers(0, 4)), 4, False)
            cols[c] = (w + 8 * int(rng.integers(0, 2)), 8, False)
    if kfold and (ncols == 1 or ncols >= 4) and not any(pf for _, _, pf in cols):
        size = int(rng.choice([4, 8]))                           # at least one fold-indexed output
        cols[-1] = (int(rng.integers(0, (stride - size * (kfold + 1)) // size + 1)) * size, size, True)
    return cols


def _check_layout(L, path, dtype, ncols, stride, kfold, groups=37, n=700, misalign=False, tag="", dense=False):
    rng = np.random.default_rng(seed_of("layout", dtype, ncols, stride, kfold, tag, dense))
    ids = some_ids(rng, groups)
    ix = Index(L, ids)
    recs = ix.n + 1
    img = rng.integers(0, 256, recs * stride, dtype=np.uint8)   # every byte distinguishable
    buf = dev(np.concatenate([np.zeros(8, np.uint8), img]) if misalign else img)
    image = buf[8:] if misalign else buf
    assert image.data_ptr() % 16 == (8 if misalign else 0)
    off = 0 if dtype == "int32" else -44_000_000_000
    rows = probe_rows(rng, ids, n, NP[dtype], off)
    valid = rng.random(n) > 0.1
    lay = _layout(rng, ncols, stride, kfold, dense)
    # what the case is about is in the layout, whatever the seed: a fold-indexed output (one
    # output alone, or four and more, with folds) and two fixed outputs in one 16-byte window
    fixed = [o // 16 for o, _, pf in lay if not pf]
    assert not (kfold and (ncols == 1 or ncols >= 4)) or any(pf for _, _, pf in lay), lay
    assert ncols < 2 or stride < 16 or max(fixed.count(w) for w in fixed) >= 2, lay
    folds = [rng.integers(0, kfold, n).astype(np.uint8) if pf else None for _, _, pf in lay]
    if kfold == 256:
        for f in folds:
            if f is not None:
                f[::7] = 255
    miss = [int(rng.integers(0, 2**63)) for _ in lay]
    cols = [(o, s, f, m) for (o, s, _), f, m in zip(lay, folds, miss)]
    g = R.position(ids, rows, valid, off, ix.n)
    got, flag, gid = image_lookup(L, path, ix, rows, image, stride, cols, valid, off, ix.n, want_gid=True)
    assert flag == int((g < 0).any())
    for c, (o, s, f, m) in enumerate(cols):
        ok(R.bits_mismatch(got[c], R.read_image(img, stride, g, o, s, f, m),
                           what=f"{path} {dtype} ncols {ncols} stride {stride} column {c} {lay[c]}"))
    if path == "flat":                                           # gid_out feeds gid_in: no probe, same columns
        ok(R.bits_mismatch(gid, g.astype(np.int32), what="gid_out"))
        again, flag, _ = image_lookup(L, path, ix, rows[::-1].copy(), image, stride, cols, None, off, -1, gid_in=gid)
        assert flag == int((g < 0).any())
        for c in range(ncols):
            ok(R.bits_mismatch(again[c], got[c], what=f"gid_in column {c}"))


@pytest.mark.parametrize("ncols", [1, 2, 3, 4, 5, 8, 9, 16, 17, 24])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("path", PATHS)
def test_record_layouts(L, path, dtype, ncols):
    """Each MAXC instantiation (2, 4, 8, 16, 24) at its edge and one past it; at the edge also with
    MAXC / 2 shared windows."""
    _check_layout(L, path, dtype, ncols, 64 if ncols <= 8 else 192, 3)
    if ncols in (2, 4, 8, 16, 24):
        _check_layout(L, path, dtype, ncols, 64 if ncols <= 8 else 192, 0, dense=True)


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("path", PATHS)
def test_record_layouts_without_windows_and_with_255_folds(L, path, dtype):
    _check_layout(L, path, dtype, 6, 24, 1, tag="stride 24")               # not a multiple of 16: no windows
    _check_layout(L, path, dtype, 8, 64, 3, misalign=True, tag="8 mod 16")  # the image is not 16-byte aligned
    _check_layout(L, path, dtype, 5, 2112, 256, groups=9, tag="kfold 256")  # fold id 255: slot 256 of 257
    _check_layout(L, path, dtype, 1, 8, 0, tag="stride 8")
    for n in (1, 257, 513):
        _check_layout(L, path, dtype, 4, 32, 2, n=n, tag=f"n {n}")


# ---------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------
def test_argument_checks(L):
    """NVT_EINVAL with a message before any launch: outputs, images and *unseen keep what they
    held.  One assertion per rejection."""
    ids = np.arange(10, dtype=np.int32)
    ix = Index(L, ids)
    rows = dev(ids)
    image = torch.full((11 * 64,), POISON, dtype=torch.uint8, device="cuda")
    outs = [poison(10, np.uint64) for _ in range(25)]
    flag = torch.zeros(1, dtype=torch.int64, device="cuda")

    def lookup(name, ncols, offs, sizes):
        mid = ((ix.aux.data_ptr(), ix.table.data_ptr(), ix.capacity, 0, None, None) if name == "nvt_flat_lookup_image"
               else (ix.dir.data_ptr(), ix.B, ix.keys.data_ptr(), ix.n, 0, -1))
        return L.refused(name, rows.data_ptr(), CODE["int32"], None, 10, *mid, image.data_ptr(), 64, ncols,
                         ptrs(L, outs[:ncols]), ptrs(L, [None] * ncols), u32s(offs), u32s(sizes), u64s([0] * ncols),
                         flag.data_ptr())

    for name in ("nvt_flat_lookup_image", "nvt_keydir_lookup_image"):
        assert "1..24 outputs" in lookup(name, 25, [0] * 25, [8] * 25)                # ncols = 25
        assert "outside the record" in lookup(name, 2, [0, 64], [8, 8])               # a value outside the record
        assert "aligned to the value size" in lookup(name, 2, [0, 12], [8, 8])        # a misaligned offset
    # nvt_image_build: a stride of 200; a part with more groups than records
    tc, ts = dev(np.full(10, 3, np.int64)), dev(np.ones(10))
    fc, fs = dev(np.ones(20, np.int64)), dev(np.ones(20))
    part = (L.m.ImagePart * 1)(L.m.ImagePart(
        kind=L.m.IMAGE_PART_TE, kfold=2, out_dtype=CODE["float32"], offset=0, groups=10, tot_count=tc.data_ptr(),
        tot_sum=ts.data_ptr(), fold_count=fc.data_ptr(), fold_sum=fs.data_ptr(), p_smooth=0.5, y_mean=0.25,
        moments=None))
    big = torch.full((11 * 200,), POISON, dtype=torch.uint8, device="cuda")
    assert "<= 192" in L.refused("nvt_image_build", part, 1, 11, big.data_ptr(), 200)
    assert "more groups than records" in L.refused("nvt_image_build", part, 1, 9, big.data_ptr(), 64)
    # kfold = 257; a fold pointer with kfold = 1
    out = poison(10, np.float32)
    rec = dev(np.ones((10, 2 * 258)))
    fold = dev(np.zeros(10, np.uint8))
    te = (rows.data_ptr(), CODE["int32"], None, 10, ix.aux.data_ptr(), ix.table.data_ptr(), ix.capacity, 0)
    assert "256" in L.refused("nvt_te_image", tc.data_ptr(), ts.data_ptr(), fc.data_ptr(), fs.data_ptr(), 257, 10,
                              0.5, 0.25, CODE["float32"], big.data_ptr(), 2200, 0)
    assert "fold ids come with kfold > 1" in L.refused("nvt_flat_lookup_te", *te, fold.data_ptr(), 1, rec.data_ptr(),
                                                      1.0, 0.5, out.data_ptr(), CODE["float32"])
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    for t in outs + [out, image, big]:
        assert bool((t == POISON).all())
