"""Kernel-level matrix for the hash join against an external table (nvtabular_amd/csrc/nvt_join.hip
with the shared scan of nvt_scan.hpp): the nine ``nvt_join_*`` entry points called through
``_lib.load()`` with ``_lib.JoinKey`` / ``_lib.JoinIndex`` / ``_lib.JoinCol`` on plain torch tensors,
every output tensor compared with the numpy references of join_reference.py (which
test_join_reference.py pins to ``pandas.merge`` on the CPU).  Nothing is approximate here: every
comparison is exact.  Output buffers are pre-filled with a poison byte (0xA5; validity words with
0xFF), so an element a kernel did not write shows.

What the operator (test_gpu_join_external.py) cannot reach and this file does:

    slot tables    hand-made tags at capacities 2, 4 and 64, read back and checked with
                   ``check_slots``: exact load 0.5, 32 tags of ONE wave that share home slot
                   capacity - 2 (the chain wraps to slot 0 and every lane contends for one slot),
                   the tags 0 and 2^64 - 1, 100 000 random groups
    probing        present keys at the far end of the wrapped chain, absent keys that walk all of it
                   to the first empty slot, a left key equal to ``empty``, the null group with
                   null_count 0 and > 0 (nulls by bitmap and by NaN), inner / left counts, out_keep,
                   out_total and unmatched seeded with a non-zero value and accumulated over two
                   calls, every optional output NULL in turn
    verification   2 to 4 components: tags from nvt_join_hash inserted against FORGED external words
                   and null bits, so that the comparison behind a tag hit decides the result
    scan           scan_small_kernel at 1, 2, 3 and 16 rounds of 8192 elements, the three-launch
                   scan at large sizes and (through a buffer that is not 16-byte aligned) at small
                   ones, with running sums beyond 2^31
    keys           every dtype and mode, NaN with sign and payload, infinities, denormals, -0.0,
                   float32 widened, int64 beyond 2^53 as doubles, uint8 >= 128, garbage under
                   cleared validity bits; nvt_join_hash's words and null bits

Sizes.  The per-row kernels (hash, insert, probe, expand) launch stream_grid(n, 256): at most 2048
workgroups of 256 rows, so TRIP = 524 288 rows are one full grid; the one-wave-per-64-rows kernels
(probe_gather, gather) launch stream_grid(ceil(n / 64), 4), the same figure.  Row counts are
1, 63, 64, 65, 127, 129, 255, 257 (around one wave, two waves, one workgroup) and TRIP + 65: a
second grid-stride trip that ends in a ragged wave.

Edits of the kernels that this file was run against, and the tests that then fail (every other
test of the file still passes): the probe loop bounded to 8 steps -- test_probe_hand_made_tables
[cap64-one-chain, 100k], test_probe_walks_the_whole_wrapped_chain, test_probe_gather[mixed, all-hits];
no comparison of ix.nulls, or of component 0 of ix.words only -- test_forged_verification[2, 3, 4];
no -0.0 fold -- test_hash_one_component[float32, float64], test_hash_mixed_components,
test_probe_float_mode_and_nan_nulls[float32, float64]; cnt for max(cnt, 1) -- every [left] case of
test_probe_hand_made_tables, the chain, float-mode and forged tests, test_composed_pipeline[3-left];
*out_total stored, not added -- test_probe_hand_made_tables, test_probe_float_mode_and_nan_nulls,
test_composed_pipeline; the validity ballot from `hit` alone -- test_probe_gather[mixed, all-hits],
test_gather, test_composed_pipeline; carry = all in scan_small_kernel -- test_offsets[16385, 131071,
131072; big] (with EVERY file that includes nvt_scan.hpp rebuilt: the library holds one copy of the
header's static kernels per file and the runtime resolves them by name, so nvt_join.hip rebuilt
alone still ran an unedited copy); the null bits XOR-ed unmixed into tuple_tag's seed, as they were
before this file existed -- test_hash_tuples_equal_and_distinct, test_null_bits_do_not_cancel_against_
the_first_word, test_operator_takes_keys_that_used_to_share_a_tag.

Left out, by name: the string-key surrogate path (test_gpu_strings.py); list columns carried
through the join; workflows and threading (test_gpu_join_external.py); more than 2^32 output rows;
argument rejection (test_join_external_host.py); the session-operator kernels of nvt_list.hip,
whose operator tests are already a direct matrix.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import join_reference as R

pytestmark = pytest.mark.gpu

INT, FLT = R.JOIN_INT, R.JOIN_FLOAT
TRIP = 2048 * 256
ROWS = [1, 63, 64, 65, 127, 129, 255, 257, TRIP + 65]
EMPTY = 1 << 63                     # INT64_MIN as a tag: what the host driver picks first
POISON = 0xA5
POISON64 = 0xA5A5A5A5A5A5A5A5
CODE = {"float32": 0, "float64": 1, "int32": 2, "int64": 3, "uint8": 4}   # include/nvt_hip.h NVT_F32 ..
WIDTH_DTYPE = {1: np.uint8, 4: np.int32, 8: np.int64}


class Lib:
    def __init__(self):
        from nvtabular_amd import _lib
        from nvtabular_amd import kernels as K

        self.m, self.lib, self.K = _lib, _lib.load(), K
        assert [_lib.NVT_F32, _lib.NVT_F64, _lib.NVT_I32, _lib.NVT_I64, _lib.NVT_U8] == list(CODE.values())
        assert (_lib.JOIN_INT, _lib.JOIN_FLOAT) == (INT, FLT)

    def call(self, name, *args):
        self.m.check(getattr(self.lib, name)(*args, self.K.stream_ptr()), name)


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
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def poisoned(n, dtype, byte=POISON):
    """max(n, 1) elements of `dtype` (numpy) with every byte = `byte`."""
    size = max(int(n), 1) * np.dtype(dtype).itemsize
    return torch.full((size,), byte, dtype=torch.uint8, device="cuda")


def read(t, dtype, n):
    return host(t).view(dtype)[:n]


def still_poison(t, byte=POISON):
    return bool((host(t) == byte).all())


# ---------------------------------------------------------------------------------------------
# wrappers of the entry points; each checks its buffer sizes before it launches
# ---------------------------------------------------------------------------------------------
def key_descs(L, cols, n):
    """cols: (numpy values, validity as bool or None, mode) per component."""
    descs = (L.m.JoinKey * len(cols))()
    alive = []
    for d, (x, valid, mode) in zip(descs, cols):
        assert x.size == n and (valid is None or valid.size == n)
        t = dev(x)
        v = None if valid is None else dev(R.pack_bits(valid))
        assert v is None or v.numel() * 8 >= n
        alive += [t, v]
        d.x = t.data_ptr() if n else None
        d.valid = v.data_ptr() if v is not None and n else None
        d.dtype = CODE[x.dtype.name]
        d.mode = mode
    return descs, alive


def run_hash(L, cols, n):
    """-> (tags uint64 [n], words uint64 [nkeys][n], nulls uint8 [n], words buffer)."""
    nk = len(cols)
    descs, alive = key_descs(L, cols, n)
    tag, nulls, words = poisoned(n, np.uint64), poisoned(n, np.uint8), poisoned(nk * n, np.uint64)
    L.call("nvt_join_hash", descs, nk, n, tag.data_ptr(), words.data_ptr(), nulls.data_ptr())
    return read(tag, np.uint64, n), read(words, np.uint64, nk * n).reshape(nk, n), read(nulls, np.uint8, n), words


def make_table(L, capacity, tags, first, count, empty=EMPTY):
    """Slots {empty, 0, 0}, then nvt_join_insert.  -> the slots tensor (capacity x 2 int64)."""
    tags = np.asarray(tags, np.uint64)
    first, count = np.asarray(first, np.uint32), np.asarray(count, np.uint32)
    ng = tags.size
    assert first.size == ng and count.size == ng and ng <= capacity // 2 and capacity & (capacity - 1) == 0
    slots = torch.zeros((capacity, 2), dtype=torch.int64, device="cuda")
    slots[:, 0] = empty - (1 << 64) if empty >= 1 << 63 else empty
    t, f, c = dev(tags), dev(first), dev(count)
    L.call("nvt_join_insert", slots.data_ptr(), capacity, empty, t.data_ptr(), f.data_ptr(), c.data_ptr(), ng)
    torch.cuda.synchronize()
    return slots


def index_of(L, slots, nkeys, n_ext, empty=EMPTY, words=None, nulls=None, null_group=(0, 0)):
    """-> (nvt_join_index, tensors to keep alive).  words: uint64 [nkeys][n_ext], nulls: uint8 [n_ext]."""
    s = L.m.JoinIndex()
    alive = [slots]
    s.slots, s.capacity, s.empty = slots.data_ptr(), slots.shape[0], empty
    if words is not None:
        assert words.shape == (nkeys, n_ext) and nulls.shape == (n_ext,)
        w, nl = dev(words), dev(nulls)
        alive += [w, nl]
        s.words, s.nulls = w.data_ptr(), nl.data_ptr()
    assert null_group[1] == 0 or null_group[0] + null_group[1] <= n_ext
    s.n_ext, s.null_first, s.null_count, s.nkeys = n_ext, null_group[0], null_group[1], nkeys
    return s, alive


def run_probe(L, ix, cols, n, inner, skip=(), total=None):
    """-> {first, count, keep} as numpy (None where the output was passed as NULL)."""
    descs, alive = key_descs(L, cols, n)
    first = poisoned(n, np.int64)
    count = None if "count" in skip else poisoned(n, np.uint32)
    keep = None if "keep" in skip else poisoned(n, np.uint8)
    assert total is None or (total.dtype == torch.int64 and total.numel() == 1)
    L.call("nvt_join_probe", C.byref(ix[0]), descs, len(cols), n, int(inner), first.data_ptr(), L.K.ptr(count),
           L.K.ptr(keep), L.K.ptr(total))
    return {"first": read(first, np.int64, n), "count": None if count is None else read(count, np.uint32, n),
            "keep": None if keep is None else read(keep, np.uint8, n),
            "raw": (first, count, keep)}


def col_descs(L, jobs):
    """jobs: (src tensor, src_valid tensor or None, dst tensor, dst_valid tensor or None, width)."""
    descs = (L.m.JoinCol * len(jobs))()
    for d, (src, sv, dst, dv, width) in zip(descs, jobs):
        d.src, d.src_valid, d.dst, d.dst_valid = src.data_ptr(), L.K.ptr(sv), dst.data_ptr(), L.K.ptr(dv)
        d.width = width
    return descs


def payload(n_src, widths, with_valid, rng):
    """[(values numpy, valid bool or None, width)]: one source column per entry of `widths`."""
    out = []
    for j, w in enumerate(widths):
        dt = WIDTH_DTYPE[w]
        i = np.iinfo(dt)
        vals = rng.integers(i.min, i.max, max(n_src, 1), dtype=dt, endpoint=True)
        vals[vals == 0] = 1                                   # 0 is what a miss writes
        valid = (rng.random(max(n_src, 1)) >= 0.3) if with_valid[j % len(with_valid)] else None
        out.append((vals, valid, w))
    return out


def gather_jobs(srcs, m, dst_valid):
    """Device buffers of one launch: sources as they are, poisoned destinations of m rows."""
    jobs = []
    for j, (vals, valid, w) in enumerate(srcs):
        sv = None if valid is None else dev(R.pack_bits(valid))
        dv = poisoned((m + 63) // 64, np.uint64, 0xFF) if dst_valid[j % len(dst_valid)] else None
        jobs.append((dev(vals), sv, poisoned(m, WIDTH_DTYPE[w]), dv, w))
    return jobs


def check_gathered(jobs, srcs, idx, m, what):
    """Every destination of a launch against R.gather; validity words whole, bits past m = 0."""
    for j, ((_, _, dst, dv, w), (vals, valid, _)) in enumerate(zip(jobs, srcs)):
        exp, exp_valid = R.gather(idx, vals, valid)
        R.first_mismatch(read(dst, WIDTH_DTYPE[w], m), exp, f"{what}, column {j} (width {w}): values")
        if dv is not None:
            R.first_mismatch(host(dv)[:(m + 63) // 64 * 8], R.pack_words(exp_valid),
                             f"{what}, column {j} (width {w}): validity words")


# ---------------------------------------------------------------------------------------------
# nvt_join_hash
# ---------------------------------------------------------------------------------------------
def bits64(*patterns):
    return np.array(patterns, np.uint64).view(np.float64)


def bits32(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


EDGES = {
    "float64": np.concatenate([
        [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.225073858507201e-308, 1.1, float(np.float32(1.1)), 2.0**53,
         2.0**53 + 2, -1.0, 1.0],
        bits64(0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF00000DEADBEEF, 0xFFFFFFFFFFFFFFFF)]),
    "float32": np.concatenate([
        np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, 1.1, 16777216.0, -1.0], np.float32),
        bits32(0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF80BEEF, 0xFFFFFFFF)]),
    "int64": np.array([0, -1, 1, 2**53, 2**53 + 1, 2**53 + 2, 2**53 + 3, -2**53 - 1, -2**63, 2**63 - 1, 2**63 - 513,
                       2**63 - 512, 2**62 + 1, -2**63 + 1], np.int64),
    "int32": np.array([0, -1, 1, -2**31, 2**31 - 1, 2**24 + 1], np.int32),
    "uint8": np.array([0, 1, 127, 128, 200, 255], np.uint8),
}


def key_values(dtype, n, rng):
    """Random bit patterns of the type (for floats: NaNs, infinities and denormals among them) with
    the edge values at the start, and at the end where there is room (the second grid trip)."""
    dt = np.dtype(dtype)
    raw = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt).copy()
    if dt.kind == "f":                               # half of the rows: small whole numbers, so keys repeat
        small = rng.random(n) < 0.5
        raw[small] = rng.integers(-3, 4, int(small.sum())).astype(dt)
    e = EDGES[dt.name]
    k = min(n, e.size)
    raw[:k] = e[:k]
    if n >= 2 * e.size:
        raw[n - e.size:] = e
    return raw


def validity(n, rng, kind):
    if kind == "none":
        return None
    v = rng.random(n) >= 0.2
    if kind == "edges-valid":                        # the edge values at both ends stay valid rows
        v[:32] = True
        v[-32:] = True
    return v


HASH_CASES = [(d, m) for d in CODE for m in (INT, FLT) if not (d.startswith("float") and m == INT)]


@pytest.mark.parametrize("bitmap", ["none", "edges-valid", "random"])
@pytest.mark.parametrize("dtype,mode", HASH_CASES, ids=[f"{d}-{'int' if m == INT else 'float'}" for d, m in HASH_CASES])
def test_hash_one_component(L, dtype, mode, bitmap):
    """tag == word == canon(value), nulls == the null bit; the words buffer of a one-component key is
    not written; a row's result does not depend on its position."""
    rng = np.random.default_rng(seed_of("hash1", dtype, mode, bitmap))
    for n in ROWS + [len(EDGES[dtype]), 1000]:
        x = key_values(dtype, n, rng)
        valid = validity(n, rng, bitmap)
        what = f"nvt_join_hash {dtype} mode={mode} bitmap={bitmap} rows={n}"
        exp_w, exp_null = R.canon(x, dtype, mode, valid)
        tag, _, nulls, words_buf = run_hash(L, [(x, valid, mode)], n)
        R.first_mismatch(nulls, exp_null.astype(np.uint8), what + ": nulls")
        R.first_mismatch(tag, exp_w, what + ": tag")
        assert still_poison(words_buf), what + ": out_words written for a one-component key"
        if n in (257, TRIP + 65):
            s = 77 % n
            tag2, _, nulls2, _ = run_hash(L, [(np.roll(x, s), None if valid is None else np.roll(valid, s), mode)], n)
            R.first_mismatch(np.roll(tag2, -s), tag, what + ": tag of the rows moved by 77")
            R.first_mismatch(np.roll(nulls2, -s), nulls, what + ": nulls of the rows moved by 77")
    if dtype == "float64" and bitmap != "random":      # the named edges, spelled out
        x = EDGES[dtype]
        tag, _, nulls, _ = run_hash(L, [(x, None, FLT)], x.size)
        assert tag[0] == tag[1] == 0 and not nulls[:13].any() and nulls[13:].all() and not tag[13:].any()
        assert tag[2] == 0x7FF0000000000000 and tag[3] == 0xFFF0000000000000 and tag[4] == 1
    if dtype == "int64" and mode == FLT and bitmap == "none":
        tag, _, _, _ = run_hash(L, [(EDGES[dtype], None, FLT)], EDGES[dtype].size)
        # ties round to even: 2^53 + 1 -> 2^53, 2^53 + 3 -> 2^53 + 4
        assert tag[3] == tag[4] != tag[5] != tag[6] == bits64(0x4340000000000002).view(np.uint64)[0]


ALPHABET = {2: 64, 3: 16, 4: 8}       # values per component (one of them null): 4096 distinct tuples


@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_hash_tuples_equal_and_distinct(L, nkeys):
    """The whole product of a small alphabet (value 0 .. a - 2 or null) in every component: tuples
    that are permutations of one another, tuples that differ only in WHICH component is null (a
    null's word is 0, and 0 is a value).  words and nulls exactly; equal tuples <-> equal tags."""
    a = ALPHABET[nkeys]
    rng = np.random.default_rng(seed_of("tuples", nkeys))
    ids = np.arange(a ** nkeys)
    ids = rng.permutation(np.concatenate([ids, rng.integers(0, ids.size, 2000)]))
    n = ids.size
    dtypes = [np.int64, np.int32, np.uint8, np.int64][:nkeys]
    cols = []
    for k in range(nkeys):
        digit = (ids // a ** k) % a
        valid = digit != a - 1
        x = np.where(valid, digit, rng.integers(0, a, n)).astype(dtypes[k])       # garbage under the nulls
        cols.append((x, valid, INT))
    exp_w, exp_null = R.canon_many([c[0] for c in cols], [c[1] for c in cols], [INT] * nkeys)
    assert np.unique(np.vstack([exp_w, exp_null[None, :].astype(np.uint64)]), axis=1).shape[1] == a ** nkeys
    tag, words, nulls, _ = run_hash(L, cols, n)
    what = f"nvt_join_hash, {nkeys} components, {a ** nkeys} tuples"
    R.first_mismatch(nulls, exp_null, what + ": nulls")
    R.first_mismatch(words, exp_w, what + ": words")
    by_tuple = np.full(a ** nkeys, 0, np.uint64)
    by_tuple[ids] = tag
    R.first_mismatch(tag, by_tuple[ids], what + ": equal tuples, equal tags")
    assert np.unique(by_tuple).size == a ** nkeys, what + ": two distinct tuples share a tag"
    s = 1234
    moved = [(np.roll(x, s), np.roll(v, s), m) for x, v, m in cols]
    tag2, words2, nulls2, _ = run_hash(L, moved, n)
    R.first_mismatch(np.roll(tag2, -s), tag, what + ": tags of the rows moved")
    R.first_mismatch(np.roll(words2, -s, axis=1), words, what + ": words of the rows moved")


def test_null_bits_do_not_cancel_against_the_first_word(L):
    """(0, null) and (2, 0), (null, 5) and (-1, 5): pairs whose null bits and first word differ in
    the same bit of (word + constant).  The fingerprint used to XOR the two unmixed, the pair shared a
    tag, and ExternalIndex refused an external table that held both keys."""
    a = np.array([0, 2, 77, -1, 0, 4], np.int64)
    av = np.array([True, True, False, True, True, True])
    b = np.array([9, 0, 5, 5, 0, 9], np.int32)
    bv = np.array([False, True, True, True, True, False])
    tag, words, nulls, _ = run_hash(L, [(a, av, INT), (b, bv, INT)], 6)
    R.first_mismatch(words, np.array([[0, 2, 0, 2**64 - 1, 0, 4], [0, 0, 5, 5, 0, 0]], np.uint64), "words")
    R.first_mismatch(nulls, np.array([2, 0, 1, 0, 0, 2], np.uint8), "nulls")
    assert np.unique(tag).size == 6, [hex(int(t)) for t in tag]


@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_hash_mixed_components(L, nkeys):
    """float32 widened / float64 / int64 as double / uint8 by value, garbage under the nulls, at every
    row count: words [nkeys][n] and nulls exactly; rows with equal canonical keys have equal tags."""
    spec = [("float32", FLT, "random"), ("int64", FLT, "none"), ("uint8", INT, "random"), ("float64", FLT, "random")]
    rng = np.random.default_rng(seed_of("mixed", nkeys))
    for n in ROWS:
        cols = []
        for dtype, mode, bitmap in spec[:nkeys]:
            x = key_values(dtype, n, rng)
            if dtype != "uint8":
                x[n // 2:] = rng.integers(0, 3, n - n // 2).astype(x.dtype)       # repeats: equal tuples exist
            cols.append((x, validity(n, rng, bitmap), mode))
        exp_w, exp_null = R.canon_many([c[0] for c in cols], [c[1] for c in cols], [c[2] for c in cols])
        tag, words, nulls, _ = run_hash(L, cols, n)
        what = f"nvt_join_hash, {nkeys} mixed components, rows={n}"
        R.first_mismatch(nulls, exp_null, what + ": nulls")
        R.first_mismatch(words, exp_w, what + ": words")
        _, first_of, inv = np.unique(np.vstack([exp_w, exp_null[None, :].astype(np.uint64)]), axis=1,
                                     return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        R.first_mismatch(tag, tag[first_of][inv], what + ": equal tuples, equal tags")
        assert np.unique(tag).size == first_of.size, what + ": two distinct tuples share a tag"


# ---------------------------------------------------------------------------------------------
# nvt_join_insert, the table read back; nvt_join_probe on those tables
# ---------------------------------------------------------------------------------------------
def tags_with_home(home, capacity, k, skip=0):
    """The first k integers >= 1 (after `skip` of them) whose home slot in a table of `capacity` is `home`."""
    cand = np.arange(1, 64 * capacity * (k + skip + 8), dtype=np.uint64)
    hit = cand[R.home_slot(cand, capacity) == np.uint64(home)]
    assert hit.size >= k + skip
    return hit[skip: skip + k]


def table_case(name):
    """-> (capacity, tags, first, count)."""
    rng = np.random.default_rng(seed_of("table", name))
    if name == "cap2":
        tags = np.array([5], np.uint64)
    elif name == "cap4":
        tags = np.array([5, 6], np.uint64)
    elif name == "cap4-extreme-tags":
        tags = np.array([0, 2**64 - 1], np.uint64)
    elif name == "cap64-load-half":
        tags = np.unique(rng.integers(0, 2**63, 64).astype(np.uint64))[:32] * np.uint64(2) + np.uint64(1)
        tags = rng.permutation(tags)
    elif name == "cap64-one-chain":
        tags = tags_with_home(62, 64, 32)
    elif name == "100k":
        tags = np.unique(rng.integers(-2**63 + 64, 2**63 - 1, 101_000).view(np.uint64))
        tags = rng.permutation(tags)[:100_000]
    else:
        raise AssertionError(name)
    capacity = {"cap2": 2, "cap4": 4, "cap4-extreme-tags": 4, "100k": 262_144}.get(name, 64)
    ng = tags.size
    assert np.unique(tags).size == ng and not (tags == np.uint64(EMPTY)).any()
    count = (1 + rng.integers(0, 5, ng)).astype(np.uint32)
    count[0] = 1
    first = rng.permutation(ng).astype(np.uint32) * np.uint32(5)     # [first, first + count) within 5 * ng rows
    return capacity, tags, first, count


TABLES = ["cap2", "cap4", "cap4-extreme-tags", "cap64-load-half", "cap64-one-chain", "100k"]


def table(L, name):
    if ("table", name) not in _CACHE:
        capacity, tags, first, count = table_case(name)
        _CACHE["table", name] = (capacity, tags, first, count, make_table(L, capacity, tags, first, count))
    return _CACHE["table", name]


@pytest.mark.parametrize("name", TABLES)
def test_insert_and_read_back(L, name):
    capacity, tags, first, count, slots = table(L, name)
    if name == "100k":
        cap, nbytes = C.c_uint64(), C.c_uint64()
        L.m.check(L.lib.nvt_join_table_bytes(tags.size, C.byref(cap), C.byref(nbytes)), "nvt_join_table_bytes")
        assert (cap.value, nbytes.value) == (capacity, capacity * 16)
    got = host(slots).view(np.uint64)
    R.check_slots(got, capacity, EMPTY, tags, first, count)
    occupied = np.flatnonzero(got[:, 0] != np.uint64(EMPTY))
    if name == "cap64-one-chain":      # 32 entries from slot 62 on: the chain wraps to slot 0
        assert (R.home_slot(tags, 64) == 62).all()
        assert sorted(occupied.tolist()) == sorted((62 + np.arange(32)) % 64)
    if name == "cap64-load-half":
        assert occupied.size == 32 == capacity // 2
    # a table that holds nothing: the launch is skipped, every slot stays {empty, 0, 0}
    none = make_table(L, 2, [], [], [])
    R.check_slots(host(none), 2, EMPTY, [], [], [])


def left_keys_for(name, tags, n, rng):
    """int64 keys: present tags (every one of them where n allows), absent keys, `empty` itself."""
    capacity = {"cap2": 2, "cap4": 4, "cap4-extreme-tags": 4, "100k": 262_144}.get(name, 64)
    keys = tags[rng.integers(0, tags.size, n)].copy()
    k = min(n, tags.size)
    keys[:k] = tags[:k]
    absent = rng.random(n) < 0.3
    if n > 2 * tags.size or n < 4:
        absent[:k] = False
    if name == "cap64-one-chain":      # absent keys that start at the head of the chain and walk all of it
        pool = tags_with_home(62, 64, 8, skip=32)
    else:
        pool = np.setdiff1d(rng.integers(0, 2**63, 64).astype(np.uint64) | np.uint64(1), tags)
        pool = np.setdiff1d(np.append(pool, np.array([1, 2**63 - 1, 2**63 + 1], np.uint64)), tags)
    assert not np.isin(pool, tags).any() and pool.size
    keys[absent] = pool[rng.integers(0, pool.size, int(absent.sum()))]
    if n >= 8:
        keys[rng.integers(0, n, max(1, n // 50))] = np.uint64(EMPTY)
    return keys, capacity


@pytest.mark.parametrize("inner", [0, 1], ids=["left", "inner"])
@pytest.mark.parametrize("name", TABLES)
def test_probe_hand_made_tables(L, name, inner):
    """One component, int64 keys by value (tag == key).  The null group: absent (null_count = 0) and
    present; left nulls by bitmap.  out_total is seeded with 1000 and accumulated over two calls."""
    capacity, tags, first, count, slots = table(L, name)
    n_ext = 5 * tags.size + 10
    model = {((int(t),), 0): (int(f), int(c)) for t, f, c in zip(tags, first, count)}
    sizes = ROWS if name in ("100k", "cap64-one-chain") else [1, 65, 257]
    for null_group in [(0, 0), (5 * tags.size + 3, 7)]:
        ix = index_of(L, slots, 1, n_ext, null_group=null_group)
        m = dict(model)
        if null_group[1]:
            m[(0,), 1] = null_group
        for n in sizes:
            rng = np.random.default_rng(seed_of("probe", name, inner, null_group, n))
            keys, _ = left_keys_for(name, tags, n, rng)
            valid = rng.random(n) >= 0.15
            if n == 1:
                valid[:] = null_group[1] == 0
            x = keys.view(np.int64).copy()
            x[~valid] = rng.permutation(x)[~valid]                  # a null row holds some other row's key
            w, nl = R.canon(x, np.int64, INT, valid)
            exp_first, exp_count, exp_keep, exp_total = R.probe(m, w, nl.astype(np.uint8), inner)
            what = f"nvt_join_probe table={name} inner={inner} null_group={null_group} rows={n}"
            if n >= 65:
                assert (exp_first >= 0).any() and (exp_first < 0).any(), what + ": the case has no hit or no miss"
                assert (keys[valid] == np.uint64(EMPTY)).any() or n < 257, what + ": no key equal to `empty`"
            total = torch.full((1,), 1000, dtype=torch.int64, device="cuda")
            got = run_probe(L, ix, [(x, valid, INT)], n, inner, total=total)
            R.first_mismatch(got["first"], exp_first, what + ": out_first")
            R.first_mismatch(got["count"], exp_count, what + ": out_count")
            R.first_mismatch(got["keep"], exp_keep, what + ": out_keep")
            assert int(host(total)[0]) == 1000 + exp_total, what + ": out_total after one call"
            again = run_probe(L, ix, [(x, valid, INT)], n, inner, total=total)
            R.first_mismatch(again["first"], exp_first, what + ": out_first, second call")
            assert int(host(total)[0]) == 1000 + 2 * exp_total, what + ": out_total after two calls"
            if n in (65, TRIP + 65):                                 # each optional output NULL in turn
                for skip in ("count", "keep", "total"):
                    t = None if skip == "total" else torch.full((1,), 5, dtype=torch.int64, device="cuda")
                    got = run_probe(L, ix, [(x, valid, INT)], n, inner, skip=(skip,), total=t)
                    R.first_mismatch(got["first"], exp_first, what + f": out_first without {skip}")
                    if skip != "count":
                        R.first_mismatch(got["count"], exp_count, what + f": out_count without {skip}")
                    if skip != "keep":
                        R.first_mismatch(got["keep"], exp_keep, what + f": out_keep without {skip}")
                    if t is not None:
                        assert int(host(t)[0]) == 5 + exp_total, what + f": out_total without {skip}"
    # n = 0 is a no-op
    total = torch.full((1,), 1000, dtype=torch.int64, device="cuda")
    got = run_probe(L, ix, [(np.empty(0, np.int64), None, INT)], 0, inner, total=total)
    assert all(still_poison(t) for t in got["raw"]) and int(host(total)[0]) == 1000


def test_probe_walks_the_whole_wrapped_chain(L):
    """The 32 tags of home slot 62: each present key is found wherever its lane's CAS put it (up to
    31 steps from home, across the wrap), each absent key of the same home slot walks 32 occupied
    slots to the first empty one."""
    capacity, tags, first, count, slots = table(L, "cap64-one-chain")
    got_slots = host(slots).view(np.uint64)
    pos = {int(t): p for p, t in enumerate(got_slots[:, 0].tolist())}
    steps = np.array([(pos[int(t)] - 62) % 64 for t in tags])
    assert sorted(steps.tolist()) == list(range(32))
    absent = tags_with_home(62, 64, 8, skip=32)
    keys = np.concatenate([tags, absent]).view(np.int64)
    ix = index_of(L, slots, 1, 5 * tags.size)
    for inner in (0, 1):
        got = run_probe(L, ix, [(keys, None, INT)], keys.size, inner)
        R.first_mismatch(got["first"], np.concatenate([first.astype(np.int64), np.full(8, -1, np.int64)]),
                         f"chain, inner={inner}: out_first")
        k = np.concatenate([count, np.zeros(8, np.uint32)])
        R.first_mismatch(got["count"], k if inner else np.maximum(k, 1).astype(np.uint32),
                         f"chain, inner={inner}: out_count")


@pytest.mark.parametrize("dtype", ["float64", "float32", "int64"])
def test_probe_float_mode_and_nan_nulls(L, dtype):
    """NVT_JOIN_FLOAT on the left side against a table of double bit patterns: -0.0 finds 0.0, float32
    is widened, an integer column is converted; a NaN (any sign, any payload) is a null whatever its
    validity bit says and finds the null group."""
    ext = np.array([0.0, 1.0, -1.0, 2.5, np.inf, -np.inf, 16777216.0, float(np.float32(1.1)), 2.0**53, 1e300])
    tags = ext.view(np.uint64).copy()
    ng = tags.size
    first = (np.arange(ng) * 3).astype(np.uint32)
    count = (1 + np.arange(ng) % 3).astype(np.uint32)
    slots = make_table(L, 64, tags, first, count)
    R.check_slots(host(slots), 64, EMPTY, tags, first, count)
    model = {((int(t),), 0): (int(f), int(c)) for t, f, c in zip(tags, first, count)}
    rng = np.random.default_rng(seed_of("float probe", dtype))
    for null_group in [(0, 0), (40, 2)]:
        m = dict(model)
        if null_group[1]:
            m[(0,), 1] = null_group
        ix = index_of(L, slots, 1, 64, null_group=null_group)
        for n in (1, 65, 257, 4097):
            if dtype == "int64":
                x = rng.integers(-3, 4, n).astype(np.int64)
                x[::7] = 2**53 + 1                                   # == 2^53 as a double
                x[1::7] = 16777216
            else:
                x = np.concatenate([ext, [-0.0, 1.1, 3.0, 5e-324], EDGES["float64"][13:]])[rng.integers(0, 19, n)]
                with np.errstate(all="ignore"):                      # (1e300 is inf as a float32)
                    x = x.astype(dtype)
                if dtype == "float32":                               # NaN payloads of the narrow type
                    x[::11] = bits32(0xFFC00001)[0]
            valid = None if n == 257 else rng.random(n) >= 0.1
            w, nl = R.canon(x, dtype, FLT, valid)
            for inner in (0, 1):
                exp_first, exp_count, exp_keep, exp_total = R.probe(m, w, nl.astype(np.uint8), inner)
                total = torch.zeros(1, dtype=torch.int64, device="cuda")
                got = run_probe(L, ix, [(x, valid, FLT)], n, inner, total=total)
                what = f"nvt_join_probe {dtype} float mode null_group={null_group} rows={n} inner={inner}"
                R.first_mismatch(got["first"], exp_first, what + ": out_first")
                R.first_mismatch(got["count"], exp_count, what + ": out_count")
                R.first_mismatch(got["keep"], exp_keep, what + ": out_keep")
                assert int(host(total)[0]) == exp_total, what + ": out_total"
                if n == 4097 and dtype != "int64":
                    nan_rows = np.isnan(x.astype(np.float64)) & (True if valid is None else valid)
                    assert nan_rows.any() and (exp_first[nan_rows] >= 0).all() == (null_group[1] > 0)


# ---------------------------------------------------------------------------------------------
# 2 to 4 components: what is compared behind a tag hit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_forged_verification(L, nkeys):
    """The left rows' own tags (nvt_join_hash) are inserted, `first` pointing at external rows whose
    words and null bits the test supplies.  Equal words and nulls: a hit with that first / count.
    One component changed, or only the null bits changed: a miss, although the tag matches."""
    rng = np.random.default_rng(seed_of("forged", nkeys))
    n = 600
    flat = rng.permutation(40 ** 2)[:n]                              # component 0: distinct, never null
    cols = []
    for k in range(nkeys):
        x = flat if k == 0 else (flat // 40 ** (k % 2)) % 40 + 1000 * k
        x = x.astype([np.int64, np.int32, np.int64, np.int32][k])
        valid = rng.random(n) >= 0.2 if k >= 1 else None
        cols.append((x, valid, INT))
    tag, words, nulls, _ = run_hash(L, cols, n)
    exp_w, exp_null = R.canon_many([c[0] for c in cols], [c[1] for c in cols], [INT] * nkeys)
    R.first_mismatch(words, exp_w, "forged: words of the left rows")
    R.first_mismatch(nulls, exp_null, "forged: nulls of the left rows")
    assert np.unique(tag).size == n and not (tag == np.uint64(EMPTY)).any()
    at = rng.permutation(n)                                          # external row of left row i
    first = at.astype(np.uint32)
    count = (1 + rng.integers(0, 4, n)).astype(np.uint32)
    slots = make_table(L, 2048, tag, first, count)
    R.check_slots(host(slots), 2048, EMPTY, tag, first, count)
    changed = rng.random(n) < 0.5
    assert changed.any() and not changed.all()

    forgeries = [("nothing changed", None, 0)]
    forgeries += [(f"component {j} changed", j, 0) for j in range(nkeys)]
    forgeries += [(f"null bit {j} flipped", None, 1 << j) for j in range(nkeys)]
    for what, comp, null_xor in forgeries:
        ew = np.zeros((nkeys, n), np.uint64)
        en = np.zeros(n, np.uint8)
        ew[:, at] = words
        en[at] = nulls
        miss = changed if (comp is not None or null_xor) else np.zeros(n, bool)
        if comp is not None:
            ew[comp, at[miss]] += np.uint64(1)
        en[at[miss]] ^= np.uint8(null_xor)
        ix = index_of(L, slots, nkeys, n, words=ew, nulls=en)
        for inner in (0, 1):
            got = run_probe(L, ix, cols, n, inner)
            msg = f"forged verification, {nkeys} components, {what}, inner={inner}"
            R.first_mismatch(got["first"], np.where(miss, -1, at).astype(np.int64), msg + ": out_first")
            k = np.where(miss, 0, count).astype(np.uint32)
            R.first_mismatch(got["count"], k if inner else np.maximum(k, 1).astype(np.uint32), msg + ": out_count")
            R.first_mismatch(got["keep"], (~miss).astype(np.uint8), msg + ": out_keep")


# ---------------------------------------------------------------------------------------------
# nvt_join_probe_gather
# ---------------------------------------------------------------------------------------------
def unique_table(L):
    """1000 unique int64 keys (count 1, first = a permutation of the external rows)."""
    if "unique" not in _CACHE:
        rng = np.random.default_rng(seed_of("unique table"))
        keys = rng.permutation(np.arange(-500, 1500, 2, dtype=np.int64))
        first = rng.permutation(keys.size).astype(np.uint32)
        count = np.ones(keys.size, np.uint32)
        slots = make_table(L, 2048, keys.view(np.uint64), first, count)
        R.check_slots(host(slots), 2048, EMPTY, keys.view(np.uint64), first, count)
        _CACHE["unique"] = (keys, first, slots)
    return _CACHE["unique"]


@pytest.mark.parametrize("ncols", [1, 16])
@pytest.mark.parametrize("hits", ["mixed", "all-hits", "all-misses"])
def test_probe_gather(L, ncols, hits):
    """Left join on unique keys in one launch: widths 1, 4 and 8, src_valid NULL (bit 1 on a hit) and a
    bitmap (copied on a hit), value 0 and bit 0 on a miss, whole validity words with bits past n = 0
    over a 0xFF poison, *unmatched seeded with 7 and accumulated over two calls."""
    keys, first, slots = unique_table(L)
    n_ext = keys.size
    ix = index_of(L, slots, 1, n_ext)
    model = {((int(k),), 0): (int(f), 1) for k, f in zip(keys.view(np.uint64), first)}
    widths = [8, 4, 1, 4, 8, 1, 1, 8, 4, 4, 1, 8, 8, 8, 4, 1][:ncols] if ncols > 1 else None
    for n in ROWS:
        for w1 in ([8, 4, 1] if ncols == 1 and n in (65, 257) else [8] if ncols == 1 else [None]):
            rng = np.random.default_rng(seed_of("probe_gather", ncols, hits, n, w1))
            x = {"mixed": rng.integers(-520, 1520, n), "all-hits": keys[rng.integers(0, n_ext, n)],
                 "all-misses": rng.integers(-520, 1520, n) | 1}[hits].astype(np.int32)
            valid = rng.random(n) >= 0.1 if hits == "mixed" else None     # (a null finds no null group here)
            srcs = payload(n_ext, widths or [w1], [True, False] if ncols > 1 else [n % 2 == 1], rng)
            w, nl = R.canon(x, np.int32, INT, valid)
            idx, _, keep, _ = R.probe(model, w, nl.astype(np.uint8), 0)
            misses = int(n - keep.sum())
            what = f"nvt_join_probe_gather {hits} ncols={ncols} rows={n} width={w1}"
            assert {"mixed": 0 < misses < n or n < 63, "all-hits": misses == 0, "all-misses": misses == n}[hits], what
            jobs = gather_jobs(srcs, n, [True])
            descs, alive = key_descs(L, [(x, valid, INT)], n)
            unmatched = torch.full((1,), 7, dtype=torch.int64, device="cuda")
            for call in (1, 2):
                L.call("nvt_join_probe_gather", C.byref(ix[0]), descs, 1, n, col_descs(L, jobs), len(jobs),
                       unmatched.data_ptr())
                check_gathered(jobs, srcs, idx, n, f"{what}, call {call}")
                assert int(host(unmatched)[0]) == 7 + call * misses, f"{what}: *unmatched after call {call}"
            L.call("nvt_join_probe_gather", C.byref(ix[0]), descs, 1, n, col_descs(L, jobs), len(jobs), None)
            check_gathered(jobs, srcs, idx, n, what + ", unmatched = NULL")
    # n = 0: a no-op that leaves the outputs untouched
    rng = np.random.default_rng(0)
    srcs = payload(n_ext, widths or [8], [True], rng)
    jobs = gather_jobs(srcs, 0, [True])
    descs, alive = key_descs(L, [(np.empty(0, np.int32), None, INT)], 0)
    unmatched = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    L.call("nvt_join_probe_gather", C.byref(ix[0]), descs, 1, 0, col_descs(L, jobs), len(jobs), unmatched.data_ptr())
    assert all(still_poison(j[2]) and still_poison(j[3], 0xFF) for j in jobs) and int(host(unmatched)[0]) == 7


# ---------------------------------------------------------------------------------------------
# nvt_join_offsets: both scan paths
# ---------------------------------------------------------------------------------------------
ALIGNED_LENS = [1, 2, 9, 8191, 8192, 8193, 16384, 16385, 131071, 131072, 131073, 300_001]
OFFSET_LENS = [1, 2047, 2048, 2049, 4097]
GUARD = 8


def scan_counts(length, data, rng):
    """counts[0 .. length): counts[length - 1] = 0 (the entry behind the last row).  "big": 0 .. 5
    and two entries near 2^31 (one in the first 8192-element round where there is one, one in the
    last quarter), the total in [2^32 - 4096, 2^32 - 1]; a single count: 2^32 - 1000."""
    c = np.zeros(length, np.uint32)
    n = length - 1
    if data == "zeros" or n == 0:
        return c
    if n == 1:
        c[0] = 2**32 - 1000
        return c
    c[:n] = rng.integers(0, 6, n)
    a, b = min(n // 3, 5000), n - 1 - n // 8
    assert a != b
    c[a] = c[b] = 0
    target = 2**32 - 1 - int(rng.integers(0, 4096))
    c[a] = 2**31 - 17
    c[b] = target - int(c.astype(np.uint64).sum())
    return c


@pytest.mark.parametrize("data", ["big", "zeros"])
@pytest.mark.parametrize("length,shift", [(n, 0) for n in ALIGNED_LENS] + [(n, 1) for n in OFFSET_LENS],
                         ids=lambda v: str(v))
def test_offsets(L, length, shift, data):
    """len = n + 1 entries scanned in place.  On a 16-byte aligned buffer len <= 131072 is the
    one-workgroup scan (1, 2, 3 and 16 rounds of 8192), beyond it the three-launch scan; a buffer
    one element off alignment takes the three-launch scan at any size.  Guard elements on both
    sides of the array stay as they were."""
    rng = np.random.default_rng(seed_of("offsets", length, shift, data))
    n = length - 1
    counts = scan_counts(length, data, rng)
    exp = R.exclusive_offsets(counts)
    total = int(exp[-1]) + int(counts[-1])
    if data == "big" and length >= 2:
        assert 2**32 - 4096 <= total <= 2**32 - 1, total
    assert int(exp.max()) < 2**32
    buf = torch.full((GUARD + shift + length + GUARD,), -1515870811, dtype=torch.int32, device="cuda")   # 0xA5A5A5A5
    view = buf[GUARD + shift: GUARD + shift + length]
    view.copy_(dev(counts))
    assert view.data_ptr() % 16 == 4 * shift and view.numel() == length
    need = C.c_uint64()
    L.m.check(L.lib.nvt_join_scan_ws_bytes(n, C.byref(need)), "nvt_join_scan_ws_bytes")
    assert need.value == (length + 2047) // 2048 * 8
    ws = poisoned(need.value // 8 + GUARD, np.uint64)
    L.call("nvt_join_offsets", view.data_ptr(), n, ws.data_ptr(), need.value)
    got = host(buf).view(np.uint32)
    what = f"nvt_join_offsets len={length} shift={shift} {data}"
    R.first_mismatch(got[GUARD + shift: GUARD + shift + length], exp.astype(np.uint32), what)
    assert (got[:GUARD + shift] == 0xA5A5A5A5).all() and (got[GUARD + shift + length:] == 0xA5A5A5A5).all(), \
        what + ": written outside the array"
    assert (host(ws).view(np.uint64)[need.value // 8:] == POISON64).all(), what + ": written behind the workspace"


# ---------------------------------------------------------------------------------------------
# nvt_join_expand
# ---------------------------------------------------------------------------------------------
def expand_case(n, m, rng, huge=None):
    """counts of n left rows that sum to m: zero-count runs at the start, in the middle and at the
    end, rows without a match (first = -1, count 1), optionally one row with `huge` outputs."""
    z = max(1, n // 10)
    allowed = np.ones(n, bool)
    allowed[:z] = allowed[n // 2: n // 2 + z] = allowed[n - z:] = False
    allowed &= rng.random(n) < 0.7
    rows = np.flatnonzero(allowed)
    assert rows.size >= 2
    counts = np.zeros(n, np.int64)
    first = rng.integers(0, 1_000_000, n).astype(np.int64)
    rest = m
    if huge:
        counts[rows[rows.size // 2]] = huge
        rest -= huge
    k = min(rest // 3, rows.size // 5)
    missing = rng.choice(rows, k, replace=False)
    counts[missing] += 1
    first[missing] = -1
    hit_rows = np.setdiff1d(rows, missing)
    counts[hit_rows] += rng.multinomial(rest - k, np.full(hit_rows.size, 1.0 / hit_rows.size))
    first[~allowed] = np.where(rng.random(int((~allowed).sum())) < 0.5, -1, 7)    # zero-count rows of both kinds
    assert counts.sum() == m and not counts[~allowed].any()
    return counts.astype(np.uint32), first


@pytest.mark.parametrize("n,m,huge", [(10, 1, None), (300, 64, None), (300, 65, None), (1000, 101_500, 100_000),
                                      (100_000, TRIP + 65, None), (2, 5, None)])
def test_expand(L, n, m, huge):
    rng = np.random.default_rng(seed_of("expand", n, m))
    if n == 2:
        counts, first = np.array([5, 0], np.uint32), np.array([-1, 3], np.int64)
    else:
        counts, first = expand_case(n, m, rng, huge)
    off = R.exclusive_offsets(np.append(counts, np.uint32(0)))
    assert int(off[-1]) == m
    exp_left, exp_ext = R.expand(off, first, m)
    if n > 2:
        assert counts[0] == 0 and counts[-1] == 0 and (m < 3 or (exp_ext < 0).any())
    d_off, d_first = dev(off.astype(np.uint32)), dev(first)
    left, ext = poisoned(m, np.int64), poisoned(m, np.int64)
    L.call("nvt_join_expand", d_off.data_ptr(), d_first.data_ptr(), n, m, left.data_ptr(), ext.data_ptr())
    what = f"nvt_join_expand n={n} m={m}"
    R.first_mismatch(read(left, np.int64, m), exp_left, what + ": left rows")
    R.first_mismatch(read(ext, np.int64, m), exp_ext, what + ": external positions")
    # m = 0 is a no-op
    left, ext = poisoned(4, np.int64), poisoned(4, np.int64)
    L.call("nvt_join_expand", d_off.data_ptr(), d_first.data_ptr(), n, 0, left.data_ptr(), ext.data_ptr())
    L.call("nvt_join_expand", None, None, 0, 0, None, None)
    assert still_poison(left) and still_poison(ext)


# ---------------------------------------------------------------------------------------------
# nvt_join_gather
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
def test_gather(L, m):
    """idx with -1, repeats and the last source row; widths 1, 4 and 8 with src_valid NULL and a
    bitmap in one launch; dst_valid non-NULL for every column, NULL for every column, and mixed."""
    rng = np.random.default_rng(seed_of("gather", m))
    n_src = 1003
    idx = rng.integers(0, n_src, m).astype(np.int64)
    idx[rng.random(m) < 0.2] = -1
    idx[rng.integers(0, m, max(1, m // 9))] = n_src - 1
    if m >= 63:
        idx[5:9] = idx[4]
        assert (idx == -1).any() and (idx == n_src - 1).any()
    srcs = payload(n_src, [1, 4, 8, 1, 4, 8], [True, True, True, False, False, False], rng)
    d_idx = dev(idx)
    for dst_valid in ([True], [False], [True, False]):
        jobs = gather_jobs(srcs, m, dst_valid)
        L.call("nvt_join_gather", d_idx.data_ptr(), m, col_descs(L, jobs), len(jobs))
        check_gathered(jobs, srcs, idx, m, f"nvt_join_gather rows={m} dst_valid={dst_valid}")
    if m == 1:                                        # m = 0 is a no-op
        jobs = gather_jobs(srcs, 0, [True])
        L.call("nvt_join_gather", None, 0, col_descs(L, jobs), len(jobs))
        assert all(still_poison(j[2]) and still_poison(j[3], 0xFF) for j in jobs)


# ---------------------------------------------------------------------------------------------
# the composed pipeline
# ---------------------------------------------------------------------------------------------
def group_on_device(tag, nulls, nk):
    """The grouping of kernels_join.ExternalIndex, in torch: stable sorts, the null group last."""
    n = tag.numel()
    order = torch.sort(tag, stable=True)[1]
    if nk == 1:
        order = order[torch.sort(nulls[order], stable=True)[1]]
    st, sn = tag[order], nulls[order]
    new = torch.ones(n, dtype=torch.bool, device=tag.device)
    new[1:] = (st[1:] != st[:-1]) | (sn[1:] != sn[:-1])
    starts = torch.nonzero(new).flatten()
    counts = torch.diff(torch.cat([starts, torch.tensor([n], device=tag.device)]))
    return order, st[starts], sn[starts], starts, counts


@pytest.mark.parametrize("how", ["left", "inner"])
@pytest.mark.parametrize("nkeys", [1, 3])
def test_composed_pipeline(L, nkeys, how):
    """hash -> group (torch, as ExternalIndex does) -> insert -> probe -> offsets -> expand -> gather
    at 2049 left rows against 700 external rows with duplicate keys and nulls on both sides, equal
    to the reference pipeline row for row."""
    rng = np.random.default_rng(seed_of("composed", nkeys))
    n, ne = 2049, 700
    inner = how == "inner"

    def side(rows):
        a = rng.integers(0, 60 if nkeys == 1 else 6, rows).astype(np.float64)
        a[rng.random(rows) < 0.1] = np.nan
        b = rng.integers(0, 5, rows).astype(np.int32)
        bv = rng.random(rows) >= 0.15
        b[~bv] = rng.integers(-99, 99, int((~bv).sum()))
        c = rng.integers(0, 4, rows).astype(np.uint8) + np.uint8(126)
        return [(a, None), (b, bv), (c, None)][:nkeys]

    modes = (FLT, INT, INT)[:nkeys]
    left, ext = side(n), side(ne)
    v = np.arange(ne, dtype=np.int64) + 1
    w = rng.integers(1, 2**31 - 1, ne).astype(np.int32)
    w_valid = rng.random(ne) >= 0.3
    lx = rng.integers(1, 255, n).astype(np.uint8)
    exp_left, exp_ext, exp_order, exp_cols = R.join_ref(left, ext, modes, inner, [(v, None), (w, w_valid)])
    m = exp_left.size
    assert m > n or inner

    # build
    etag, ewords, enulls, _ = run_hash(L, [(x, vb, md) for (x, vb), md in zip(ext, modes)], ne)
    order, gtag, gnull, starts, counts = group_on_device(dev(etag), dev(enulls), nkeys)
    null_group = (0, 0)
    if nkeys == 1 and bool(gnull[-1] != 0):
        null_group = (int(starts[-1]), int(counts[-1]))
        gtag, starts, counts = gtag[:-1], starts[:-1], counts[:-1]
    assert (null_group[1] > 0) == (nkeys == 1)
    ng = int(gtag.numel())
    assert int(counts.max()) > 1 and not bool((gtag == -(1 << 63)).any())
    horder = host(order)
    slots = make_table(L, 2048, host(gtag).view(np.uint64), host(starts).astype(np.uint32),
                       host(counts).astype(np.uint32))
    R.check_slots(host(slots), 2048, EMPTY, host(gtag).view(np.uint64), host(starts), host(counts))
    ix = index_of(L, slots, nkeys, ne, words=ewords[:, horder] if nkeys > 1 else None,
                  nulls=enulls[horder] if nkeys > 1 else None, null_group=null_group)
    # probe, offsets, expand
    lcols = [(x, vb, md) for (x, vb), md in zip(left, modes)]
    descs, alive = key_descs(L, lcols, n)
    first = poisoned(n, np.int64)
    cnt = poisoned(n + 1, np.uint32).view(torch.int32)
    cnt[n:].zero_()
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    L.call("nvt_join_probe", C.byref(ix[0]), descs, nkeys, n, int(inner), first.data_ptr(), cnt.data_ptr(), None,
           total.data_ptr())
    what = f"composed pipeline, {nkeys} components, {how}"
    assert int(host(total)[0]) == m, what + ": total"
    need = C.c_uint64()
    L.m.check(L.lib.nvt_join_scan_ws_bytes(n, C.byref(need)), "nvt_join_scan_ws_bytes")
    ws = poisoned(need.value // 8, np.uint64)
    L.call("nvt_join_offsets", cnt.data_ptr(), n, ws.data_ptr(), need.value)
    assert int(host(cnt).view(np.uint32)[n]) == m, what + ": offsets[n]"
    left_row, ext_row = poisoned(m, np.int64), poisoned(m, np.int64)
    L.call("nvt_join_expand", cnt.data_ptr(), first.data_ptr(), n, m, left_row.data_ptr(), ext_row.data_ptr())
    got_left, got_ext = read(left_row, np.int64, m), read(ext_row, np.int64, m)
    R.first_mismatch(got_left, exp_left, what + ": left rows")
    R.first_mismatch(got_ext >= 0, exp_ext >= 0, what + ": matched")
    hit = exp_ext >= 0
    R.first_mismatch(horder[got_ext[hit]], exp_order[exp_ext[hit]], what + ": external rows")
    # gather: the left column by left row, the payload (grouped order) by external position
    lsrc = [(lx, None, 1)]
    jobs = gather_jobs(lsrc, m, [False])
    L.call("nvt_join_gather", left_row.view(torch.int64).data_ptr(), m, col_descs(L, jobs), 1)
    check_gathered(jobs, lsrc, exp_left, m, what + ": left column")
    psrc = [(v[horder], None, 8), (w[horder], w_valid[horder], 4)]
    jobs = gather_jobs(psrc, m, [True])
    L.call("nvt_join_gather", ext_row.view(torch.int64).data_ptr(), m, col_descs(L, jobs), 2)
    for (_, _, dst, dv, width), (exp_vals, exp_valid) in zip(jobs, exp_cols):
        R.first_mismatch(read(dst, WIDTH_DTYPE[width], m), exp_vals, what + f": payload values (width {width})")
        R.first_mismatch(host(dv)[:(m + 63) // 64 * 8], R.pack_words(exp_valid), what + ": payload validity words")


@pytest.mark.parametrize("how", ["left", "inner"])
def test_operator_takes_keys_that_used_to_share_a_tag(how):
    """The pairs of test_null_bits_do_not_cancel_against_the_first_word as an external table of
    ops.JoinExternal: building its index raised "two different external keys share a 64-bit
    fingerprint"."""
    import pandas as pd

    from nvtabular_amd import ops
    from nvtabular_amd.device import DeviceFrame
    from nvtabular_amd.selector import ColumnSelector

    # `a` is an integer column on both sides (compared by value), `b` a float column with a null
    ext = pd.DataFrame({"a": np.array([0, 2, 4], np.int64), "b": np.array([np.nan, 0.0, 1.0]),
                        "v": np.array([10, 20, 30], np.int64)})
    left = pd.DataFrame({"a": np.array([2, 0, 0, 4, 7], np.int64), "b": np.array([0.0, np.nan, 0.0, 1.0, np.nan])})
    frame = DeviceFrame.from_pandas(left)
    op = ops.JoinExternal(ext, on=["a", "b"], how=how)
    got = op.transform(ColumnSelector(list(frame.columns)), frame).to_pandas()
    exp = left.merge(ext, on=["a", "b"], how=how)
    assert exp["v"].fillna(-1).tolist() == ([20, 10, -1, 30, -1] if how == "left" else [20, 10, 30])
    assert list(got.columns) == list(exp.columns) and len(got) == len(exp)
    for c in exp.columns:
        R.first_mismatch(got[c].isna().to_numpy(), exp[c].isna().to_numpy(), f"{how}: nulls of {c}")
        R.first_mismatch(got[c].fillna(-9).to_numpy().astype(np.float64),
                         exp[c].fillna(-9).to_numpy().astype(np.float64), f"{how}: values of {c}")
