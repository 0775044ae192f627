"""Kernel-level matrix for csrc/nvt_groupby.hip, nvt_order_rows.hip and nvt_segreduce.hip:
``K.GroupbyTable`` (the hash-table groupby of JoinGroupby / TargetEncoding / Groupby),
``K.order_rows`` and ``K.seg_aggregate`` (the Groupby operator) called directly on torch tensors
and compared with the numpy references of
groupby_reference.py, which test_groupby_reference.py pins to pandas on the CPU.  Every comparison
is exact, except the two general-value cases at the end of the table and the segmented-reduce
sections: those use the summation bound (m - 1) * 2^-53 * sum(|v|) and nothing else.

Helper -> kernels reached:

    table(...)          nvt_gb_clear: gb_clear_kernel.  nvt_gb_update, n < 2^15 ("rows"):
                        gb_update_kernel (find_slot, per-row atomicAdd, atomic_min_f64 /
                        atomic_max_f64).  n >= 2^15 ("sort"): gb_assign_kernel -> sort_words_bits
                        on the slot bits -> gb_segreduce_kernel<EXCL = false, SQ, MM>, one
                        instantiation per (sumsq, minmax) pair.  Every part of a table names the
                        path it means and the helper asserts it from n against SWITCH = 1 << 15.
                        nvt_gb_compact: gb_compact_kernel.  nvt_gb_lookup on the compacted table:
                        gb_lookup_kernel (find_slot without insert, head.index)
    own block           nvt_gb_create (one block for the arrays) and the table-owned scratch of
                        nvt_gb_update, grown on demand: test_table_with_its_own_block_and_scratch
    merged(...)         nvt_gb_merge: gb_merge_kernel
    index + lookup      nvt_gb_index_build: gb_clear_kernel + gb_index_build_kernel; gb_lookup_kernel
    dev_order(...)      nvt_sort_key_u64: sort_key_kernel<float | double | int32 | int64 | uint8>
                        (bool through the uint8 view); nvt_order_rows: pack_words_kernel +
                        sort_words_bits, two rounds of 32 bits per sort column, one of hi_bits per
                        gid refinement
    dev_seg(...)        nvt_seg_aggregate: gb_segreduce_kernel<false, SQ, MM> with a per-column
                        value count (GbView::vcount) and no table behind it

Sizes, from the constants of the .hip files.  nvt_gb_update switches paths at n == 1 << 15: 32 767
is the last per-row size, 32 768 the first sorted one.  gb_segreduce_kernel: the launch is
stream_grid(n, kBlock * 4 = 1024, 8), at most 256 CUs * 8 = 2048 workgroups of 4 waves, and each
wave walks roundup64(ceil(n / nwaves)) words in rows of kWave = 64, U = 4 rows (256 words) per
trip.  So 63 / 64 / 65 are one row, short, full and one word more; 255 / 256 / 257 and 1023 / 1025
the same around one trip of one wave and around one workgroup; 32 768 gives 128 waves exactly one
trip each; from 1024 * 2048 = 2 097 152 rows on the wave count stays 8192 and the chunks grow past
one trip: 2 200 003 rows are chunks of 320 words (a full trip and one row of a second),
3 * 2^21 + 5 rows chunks of 832 (three trips and one row).  Only there does the run a wave carries
cross a trip.  nvt_order_rows: the radix range of a gid refinement is hi_bits = bits of ngroups
(ids 0 .. ngroups, the last one the null marker), 8 bits per radix pass: a second pass from
ngroups = 256 on, a third from 65 536; the passes work in tiles of kS2Tile = 4096 words.  gb_compact_kernel: tiles of kBlock *
kGbCompactItems = 2048 slots, one workgroup per tile: capacity 64 (a fraction of a tile), 2048,
4096 and 65 536 (32 tiles).

Exact sums: values are multiples of 2^-4 with |v| <= 2^10 and no group has more than 2^23 rows, so
every partial sum is a multiple of 2^-4 below 2^33 (37 bits) and every partial sum of squares a
multiple of 2^-8 below 2^43 (51 bits): any order of summation gives the same float64.
``assert_exact`` checks that on the generated data.

Left out, by name: the nvt_sgb_* sort path and merge_sorted_comps, the exchange kernels
(test_gpu_sorted_groupby.py and the operator tests), the flat index, the key directory and the
record reads (test_gpu_lookup_kernels.py against lookup_reference.py), te_apply* and gather
(test_gpu_cont_kernels.py), the retry and demotion logic of ops/_groupby.py, string keys,
multi-rank merges.
"""
import math
import zlib

import numpy as np
import pytest
import torch

import groupby_reference as R

pytestmark = pytest.mark.gpu

SWITCH = 1 << 15                      # nvt_gb_update: per-row atomics below, sort path from here on
TRIP = 256                            # gb_segreduce_kernel: kWave * U words per trip
LARGE = [2_200_003, 3 * 2**21 + 5]    # chunks of 320 and of 832 words
I64 = np.iinfo(np.int64)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
VAL_DTYPES = ["float64", "float32", "int32", "int64", "uint8", "bool", "float64", "float32"]


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bitmap(valid):
    return None if valid is None else dev(R.pack_bits(valid))


def host(t):
    return t.cpu().numpy()


def chunk_words(n):
    """Words per wave of gb_segreduce_kernel at n words."""
    nwaves = min(-(-n // 1024), 2048) * 4
    return -(-(-(-n // nwaves)) // 64) * 64


# ---------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------
def key_columns(rng, n, nkeys, shape, nulls=True):
    """(keys, validity) of nkeys int64 columns.  single: one group; distinct: every row its own
    key; skewed: few hot keys, a long tail; extremes: INT64_MIN / INT64_MAX / 0 and neighbours;
    masks: components are 0 or null (and 0, or anything, under the null), so tuples differ only
    in their null mask.  nulls: ~10 % per component (the last column keeps no bitmap at all when
    there are several)."""
    keys = []
    for k in range(nkeys):
        if shape == "single":
            col = np.full(n, [5, I64.min, -3][k], np.int64)
        elif shape == "distinct" and k == 0:
            with np.errstate(over="ignore"):      # x -> a x mod 2^64 is a bijection (a odd)
                col = ((rng.permutation(n).astype(np.uint64) + np.uint64(1))
                       * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        elif shape == "extremes":
            col = np.array([I64.min, I64.max, 0, -1, 1, I64.min + 1, I64.max - 1], np.int64)[rng.integers(0, 7, n)]
        elif shape == "masks":
            col = np.zeros(n, np.int64)
        else:                                     # skewed (and the further columns of distinct)
            card = max(1, min(n // 3, 30_000)) if k == 0 else 3
            ids = rng.integers(I64.min, I64.max, card, dtype=np.int64) if k == 0 else np.arange(card) - 1
            col = ids[(rng.random(n) ** 3 * card).astype(np.int64)]
        keys.append(col)
    valid = [None] * nkeys
    if shape == "masks":
        valid = [rng.random(n) >= 0.4 for _ in range(nkeys)]
        for k in range(nkeys):                    # under a null: 0 mostly, sometimes anything
            valid[k][:1] = True
            bad = np.flatnonzero(~valid[k])
            keys[k][bad[::3]] = rng.integers(I64.min, I64.max, bad[::3].size, dtype=np.int64)
    elif nulls:
        for k in range(nkeys if nkeys == 1 else nkeys - 1):
            valid[k] = rng.random(n) >= 0.1
            valid[k][:1] = True                   # (value_columns empties column 1 for row 0's key)
            bad = np.flatnonzero(~valid[k])
            keys[k][bad[::2]] = 0                 # a null over the bytes of key 0 is not key 0
    return keys, valid


def value_columns(rng, n, nvals, keys=None):
    """nvals columns of VAL_DTYPES: floats are multiples of 2^-4 within +-2^10 with ~10 % NaN,
    integers lie within +-2^10.  Column j has no bitmap when j % 3 == 0, else ~20 % nulls in a
    bitmap (n is rarely a multiple of 8: the last byte is partial); all rows of the first row's
    key are null in column 1, so that group has no value there."""
    vals, valid = [], []
    for j in range(nvals):
        dt = VAL_DTYPES[j]
        if dt.startswith("float"):
            v = (rng.integers(-2**14, 2**14 + 1, n) / 16.0).astype(dt)
            v[rng.random(n) < 0.1] = np.nan
        elif dt == "bool":
            v = rng.random(n) < 0.4
        elif dt == "uint8":
            v = rng.integers(0, 256, n).astype(np.uint8)
        else:
            v = rng.integers(-2**10, 2**10 + 1, n).astype(dt)
        ok = None if j % 3 == 0 else rng.random(n) >= 0.2
        if j == 1 and keys is not None and n:
            ok &= keys[0] != keys[0][0]
        vals.append(v)
        valid.append(ok)
    return vals, valid


def assert_exact(vals, largest_group):
    """The generated values keep every sum and sum of squares order-independent (see above)."""
    assert largest_group <= 2**23, largest_group
    for v in vals:
        x = np.asarray(v).astype(np.float64)
        x = x[~np.isnan(x)]
        assert (np.abs(x) <= 2**10).all() and (x * 16 == np.rint(x * 16)).all()


def sum_bound_check(got, vals_by_group, what):
    """|got - fsum| <= (m - 1) * 2^-53 * sum(|v|): the bound of ANY order of m float64 additions."""
    for g, v in enumerate(vals_by_group):
        exact = math.fsum(v.tolist())
        bound = max(len(v) - 1, 0) * 2.0**-53 * math.fsum(np.abs(v).tolist())
        err = abs(float(got[g]) - exact)
        assert err <= bound, f"{what}: group {g} of {len(v)} values: error {err:.3e} > bound {bound:.3e}"


# ---------------------------------------------------------------------------------------------
# hash table
# ---------------------------------------------------------------------------------------------
def host_comp(comp):
    f = lambda lst: [host(t) for t in lst]  # noqa: E731
    return dict(keys=f(comp["keys"]), null_mask=host(comp["null_mask"]), size=host(comp["size"]),
                count=host(comp["count"]), sum=f(comp["sum"]), sumsq=f(comp["sumsq"]),
                min=f(comp["min"]), max=f(comp["max"]), n=comp["n"])


def capacity_for(groups):
    return max(64, -(-groups * 4 // 3) + 1)       # the driver keeps a table at most 3 / 4 full


def update(K, t, part):
    keys, kvalid, vals, vvalid, path = part
    n = keys[0].size
    assert path in ("rows", "sort") and (n < SWITCH) == (path == "rows"), (n, path)
    t.update([dev(k) for k in keys], [bitmap(v) for v in kvalid],
             [dev(v) for v in vals[:t.nvals]], [bitmap(v) for v in vvalid[:t.nvals]])


def table(K, parts, nvals, sumsq, minmax, capacity, what, groups=None, overflow=False):
    """One table over the parts (keys, key validity, values, value validity, path): (table,
    compacted groups on the device, the same on the host in the reference's order)."""
    nkeys = len(parts[0][0])
    t = K.GroupbyTable(nkeys, nvals, capacity, sumsq=sumsq, minmax=minmax)
    for part in parts:
        update(K, t, part)
    return (t,) + compacted(K, t, what, sum(p[0][0].size for p in parts), groups, overflow)


def compacted(K, t, what, rows=None, groups=None, overflow=False):
    from nvtabular_amd import _lib

    st = t.state()
    assert bool(st[_lib.ST_OVERFLOW]) == overflow, f"{what}: overflow flag {st[_lib.ST_OVERFLOW]}"
    if rows is not None:
        assert st[_lib.ST_ROWS] == rows, f"{what}: ST_ROWS {st[_lib.ST_ROWS]}, expected {rows}"
    if groups is not None:
        assert st[_lib.ST_OCCUPIED] == groups, f"{what}: {st[_lib.ST_OCCUPIED]} slots, expected {groups}"
    comp = t.compact()
    return comp, R.sort_groups(host_comp(comp))


def rows_find_their_group(K, t, comp, keys, kvalid, what):
    """compact()'s promise about its own index: lookup on the compacted table returns g with
    keys[g], null_mask[g] = the row's tuple."""
    g = host(t.lookup([dev(k) for k in keys], [bitmap(v) for v in kvalid]))
    assert g.dtype == np.int64 and g.shape == keys[0].shape
    assert ((g >= 0) & (g < comp["n"])).all(), f"{what}: {int((g < 0).sum())} rows without a group"
    nm = np.zeros(g.size, np.int64)
    for k in range(len(keys)):
        ok = np.ones(g.size, bool) if kvalid[k] is None else kvalid[k]
        nm |= (~ok).astype(np.int64) << k
        R.first_mismatch(host(comp["keys"][k])[g], np.where(ok, keys[k], 0), f"{what}: lookup, key {k}")
    R.first_mismatch(host(comp["null_mask"])[g].astype(np.int64), nm, f"{what}: lookup, null mask")


def check_matrix(K, keys, kvalid, path, what, nvals_list=(0, 1, 8), flags=FLAGS, lookup=True):
    """One reference over all eight value columns with both flags, then a table per (nvals, sumsq,
    minmax): a table of fewer columns holds the first ones."""
    n = keys[0].size
    rng = np.random.default_rng(seed_of(what, "values"))
    vals, vvalid = value_columns(rng, n, 8, keys)
    exp = R.table_groups(keys, kvalid, vals, vvalid, sumsq=True, minmax=True)
    assert_exact(vals, int(exp["size"].max()) if n else 0)
    if n > 8:
        assert np.isnan(exp["min"][1]).any(), "a group without a value in column 1"
    for nvals in nvals_list:
        for sumsq, minmax in (flags if nvals else FLAGS[:1]):
            w = f"{what} nvals={nvals} sumsq={sumsq} minmax={minmax}"
            t, comp, got = table(K, [(keys, kvalid, vals, vvalid, path)], nvals, sumsq, minmax,
                                 capacity_for(exp["n"]), w, groups=exp["n"])
            R.assert_same_groups(got, exp, w, sumsq and nvals > 0, minmax and nvals > 0)
            if lookup and nvals == nvals_list[-1] and (sumsq, minmax) == flags[-1] and n:
                rows_find_their_group(K, t, comp, keys, kvalid, w)
    return exp


@pytest.mark.parametrize("nkeys", [1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 32767])
def test_update_per_row_path(K, n, nkeys):
    rng = np.random.default_rng(seed_of("rows", n, nkeys))
    keys, kvalid = key_columns(rng, n, nkeys, "skewed")
    check_matrix(K, keys, kvalid, "rows", f"rows n={n} nkeys={nkeys}")


@pytest.mark.parametrize("nkeys", [1, 2, 3])
@pytest.mark.parametrize("n", [32768, 32769, 100_003])
def test_update_sort_path(K, n, nkeys):
    rng = np.random.default_rng(seed_of("sort", n, nkeys))
    keys, kvalid = key_columns(rng, n, nkeys, "skewed")
    assert chunk_words(n) <= TRIP
    check_matrix(K, keys, kvalid, "sort", f"sort n={n} nkeys={nkeys}")


@pytest.mark.parametrize("n", LARGE)
def test_update_sort_path_chunks_of_several_trips(K, n):
    """Chunks of 320 / 832 words: the carried run crosses trips, the last trip is partial.  A hot
    key owns a third of the rows (a run over thousands of whole chunks), the rest is skewed."""
    assert chunk_words(n) == {LARGE[0]: 320, LARGE[1]: 832}[n]
    rng = np.random.default_rng(seed_of("large", n))
    keys, _ = key_columns(rng, n, 1, "skewed", nulls=False)
    keys[0][rng.random(n) < 0.33] = 42
    v = (rng.integers(-2**14, 2**14 + 1, n) / 16.0)
    v[rng.random(n) < 0.05] = np.nan
    exp = R.table_groups(keys, [None], [v], [None], sumsq=True, minmax=True)
    assert_exact([v], int(exp["size"].max()))
    assert exp["size"].max() > 100 * chunk_words(n)
    _, _, got = table(K, [(keys, [None], [v], [None], "sort")], 1, True, True,
                      capacity_for(exp["n"]), f"large {n}", groups=exp["n"])
    R.assert_same_groups(got, exp, f"large {n}")


@pytest.mark.parametrize("path,n", [("rows", 1023), ("sort", 40_001)])
@pytest.mark.parametrize("shape", ["single", "distinct", "skewed", "extremes", "masks"])
def test_key_shapes(K, shape, path, n):
    for nkeys in (1, 2, 3):
        rng = np.random.default_rng(seed_of("shape", shape, n, nkeys))
        keys, kvalid = key_columns(rng, n, nkeys, shape, nulls=shape != "single")
        exp = check_matrix(K, keys, kvalid, path, f"{shape} {path} nkeys={nkeys}", nvals_list=(2,),
                           flags=FLAGS[3:])
        if shape == "single":
            assert exp["n"] == 1
        elif shape == "distinct":
            assert exp["n"] >= n * 0.85
        elif shape == "masks":
            # all stored keys are 0: the groups ARE the null masks -- (0,) against (null,);
            # (0, null) against (null, 0)
            assert exp["n"] == 2**nkeys and all((k == 0).all() for k in exp["keys"])
            assert exp["null_mask"].tolist() == list(range(2**nkeys))
        elif shape == "extremes":
            assert {I64.min, I64.max, 0} <= set(exp["keys"][0].tolist())


@pytest.mark.parametrize("path,n", [("rows", 4001), ("sort", 36_007)])
def test_int64_values_of_two_to_the_53_and_bool_columns(K, path, n):
    """Values are reduced as float64 (include/nvt_hip.h): +-2^53 is exact, in min / max and -- as
    multiples of 2^53 -- in the sums; bool columns go through the uint8 view."""
    rng = np.random.default_rng(seed_of("2^53", n))
    keys, kvalid = key_columns(rng, n, 1, "skewed")
    big = np.array([2**53, -(2**53), 0], np.int64)[rng.integers(0, 3, n)]
    flag = rng.random(n) < 0.5
    ok = rng.random(n) >= 0.3
    exp = R.table_groups(keys, kvalid, [big, flag], [ok, None], sumsq=True, minmax=True)
    assert 2.0**53 in exp["max"][0] and -(2.0**53) in exp["min"][0] and 1.0 in exp["max"][1]
    _, _, got = table(K, [(keys, kvalid, [big, flag], [ok, None], path)], 2, True, True,
                      capacity_for(exp["n"]), f"2^53 {path}", groups=exp["n"])
    R.assert_same_groups(got, exp, f"2^53 {path}")


@pytest.mark.parametrize("order", ["small_then_large", "large_then_small"])
def test_updates_of_both_paths_accumulate_in_one_table(K, order):
    rng = np.random.default_rng(seed_of("accumulate"))
    sizes = [1000, 40_000] if order == "small_then_large" else [40_000, 1000]
    n = sum(sizes)
    keys, kvalid = key_columns(rng, n, 2, "skewed")
    vals, vvalid = value_columns(rng, n, 3, keys)
    cut = sizes[0]
    parts = []
    for s in (slice(0, cut), slice(cut, n)):
        take = lambda lst: [None if x is None else x[s] for x in lst]  # noqa: E731
        parts.append((take(keys), take(kvalid), take(vals), take(vvalid),
                      "rows" if (s.stop - s.start) < SWITCH else "sort"))
    assert {p[4] for p in parts} == {"rows", "sort"}
    exp = R.table_groups(keys, kvalid, vals, vvalid, sumsq=True, minmax=True)
    assert_exact(vals, int(exp["size"].max()))
    cap = capacity_for(exp["n"])
    t, comp, got = table(K, parts, 3, True, True, cap, order, groups=exp["n"])
    R.assert_same_groups(got, exp, order)
    rows_find_their_group(K, t, comp, keys, kvalid, order)
    # clear(), then one part again: a fresh table of that part
    t.clear()
    update(K, t, parts[1])
    one = R.table_groups(*parts[1][:4], sumsq=True, minmax=True)
    _, got = compacted(K, t, f"{order} after clear", rows=parts[1][0][0].size, groups=one["n"])
    R.assert_same_groups(got, one, f"{order} after clear")


def test_table_with_its_own_block_and_scratch(K):
    """nvt_gb_create and no nvt_gb_set_workspace: the table allocates its arrays as one block and
    the sort path's scratch itself (K.GroupbyTable never does: nvt_gb_create_in and a torch
    workspace).  nkeys 2, nvals 1, sumsq and min / max, capacity 65 536; keys from about 3000
    tuples.  Updates of 32 768 rows (the smallest sort-path n: the scratch is allocated, a quarter
    over what this n needs), of 100 003 rows and of 150 001 rows, then compact and destroy.  The
    100 003 rows fit into the first buffer (11.0 MB needed, 11.6 MB there); the 150 001 need
    12.3 MB, so that update frees the buffer and grows a new one.  The sizes are asserted below
    from nvt_gb_update_ws_bytes, which is what nvt_gb_update needs (the unsplit unit needed 256
    bytes less of each)."""
    import ctypes as C

    from nvtabular_amd import _lib

    sizes = [SWITCH, 100_003, 150_001]
    lib = _lib.load()
    ws = C.c_uint64()
    need = []
    for m in sizes:
        assert lib.nvt_gb_update_ws_bytes(m, C.byref(ws)) == 0
        need.append(ws.value)
    grown = need[0] + need[0] // 4
    assert need[1] + 4096 < grown < need[2] - 4096, (need, grown)
    n = sum(sizes)
    rng = np.random.default_rng(seed_of("own block"))
    ids = rng.integers(I64.min, I64.max, 1000, dtype=np.int64)
    keys = [ids[(rng.random(n) ** 3 * 1000).astype(np.int64)], rng.integers(-1, 2, n)]
    kvalid = [rng.random(n) >= 0.1, None]
    vals, vvalid = value_columns(rng, n, 1, keys)
    exp = R.table_groups(keys, kvalid, vals, vvalid, sumsq=True, minmax=True)
    assert_exact(vals, int(exp["size"].max()))
    assert 2000 < exp["n"] < 6000, exp["n"]
    # a GroupbyTable around the handle of nvt_gb_create: state(), compact() and lookup() as usual
    t = K.GroupbyTable.__new__(K.GroupbyTable)
    t.lib, t.nkeys, t.nvals, t.capacity, t._mem, t._ws = lib, 2, 1, 65536, None, None
    t.flags = _lib.NVT_GB_SUMSQ | _lib.NVT_GB_MINMAX
    t.device = torch.device("cuda", torch.cuda.current_device())
    t.handle = C.c_void_p()
    _lib.check(lib.nvt_gb_create(2, 1, t.flags, t.capacity, C.byref(t.handle)), "nvt_gb_create")
    t.clear()
    lo = 0
    for m in sizes:
        s = slice(lo, lo + m)
        k = [dev(c[s]) for c in keys]
        kv, v = bitmap(kvalid[0][s]), dev(vals[0][s])
        _lib.check(lib.nvt_gb_update(t.handle, _lib.ptr_array([c.data_ptr() for c in k]),
                                     _lib.ptr_array([kv.data_ptr(), None]), _lib.ptr_array([v.data_ptr()]),
                                     (C.c_int * 1)(K.dtype_code(v.dtype)), _lib.ptr_array([None]), m,
                                     K.stream_ptr()), "nvt_gb_update")
        torch.cuda.current_stream().synchronize()     # the columns of this part go away
        lo += m
    comp, got = compacted(K, t, "own block", rows=n, groups=exp["n"])
    R.assert_same_groups(got, exp, "own block")
    rows_find_their_group(K, t, comp, keys, kvalid, "own block")
    torch.cuda.current_stream().synchronize()
    lib.nvt_gb_destroy(t.handle)
    t.handle = None


def merged(K, comps, nkeys, nvals, sumsq, minmax, capacity, what, drop=()):
    """A fresh table that merges the compacted tables one after the other; ``drop``: per call,
    the optional lists to leave out although the table carries them."""
    t = K.GroupbyTable(nkeys, nvals, capacity, sumsq=sumsq, minmax=minmax)
    for i, c in enumerate(comps):
        gone = drop[i] if i < len(drop) else ()
        t.merge(c["keys"], c["null_mask"], c["size"], c["count"], c["sum"],
                [] if "sumsq" in gone else c["sumsq"], [] if "minmax" in gone else c["min"],
                [] if "minmax" in gone else c["max"])
    return (t,) + compacted(K, t, what, rows=0)


@pytest.mark.parametrize("nkeys", [1, 3])
def test_merge(K, nkeys):
    rng = np.random.default_rng(seed_of("merge", nkeys))
    n = 6000
    keys, kvalid = key_columns(rng, n, nkeys, "skewed")
    vals, vvalid = value_columns(rng, n, 2, keys)
    vvalid[0] = rng.random(n) >= 0.2
    vvalid[0][:n // 2] &= keys[0][:n // 2] != keys[0][0]         # a group with NaN min in part a only
    assert (keys[0][n // 2:] == keys[0][0]).any()

    def part(s):
        take = lambda lst: [None if x is None else x[s] for x in lst]  # noqa: E731
        p = (take(keys), take(kvalid), take(vals), take(vvalid), "rows")
        return p, R.table_groups(*p[:4], sumsq=True, minmax=True)

    (pa, ea), (pb, eb) = part(slice(0, n // 2)), part(slice(n // 2, n))
    assert_exact(vals, n)
    both = R.merge_groups(ea, eb)
    shared = both["n"] < ea["n"] + eb["n"]
    assert shared and both["n"] > max(ea["n"], eb["n"])               # overlapping, neither contains the other
    nan_a = np.isnan(ea["min"][0])
    assert nan_a.any() and not np.isnan(both["min"][0]).all()
    cap = capacity_for(both["n"])
    _, ca, ga = table(K, [pa], 2, True, True, cap, "part a", groups=ea["n"])
    _, cb, gb = table(K, [pb], 2, True, True, cap, "part b", groups=eb["n"])
    R.assert_same_groups(ga, ea, "part a")
    # a compacted table merged into an empty one reproduces itself (NaN min / max are skipped and
    # the untouched +-inf come out as NaN again)
    _, _, got = merged(K, [ca], nkeys, 2, True, True, cap, "a alone")
    R.assert_same_groups(got, ea, "merge: a into an empty table")
    # overlapping tables, in both orders
    for name, comps in (("a + b", [ca, cb]), ("b + a", [cb, ca])):
        t, comp, got = merged(K, comps, nkeys, 2, True, True, cap, name)
        R.assert_same_groups(got, both, f"merge: {name}")
        rows_find_their_group(K, t, comp, keys, kvalid, f"merge: {name}")
    # disjoint tables: the rows of b whose tuple a does not have
    fresh = R.lookup(ea["keys"], ea["null_mask"], pb[0], pb[1]) == -1
    assert fresh.any() and not fresh.all()
    pc = tuple([None if x is None else x[fresh] for x in lst] for lst in pb[:4]) + ("rows",)
    ec = R.table_groups(*pc[:4], sumsq=True, minmax=True)
    _, cc, _ = table(K, [pc], 2, True, True, cap, "part c", groups=ec["n"])
    _, _, got = merged(K, [ca, cc], nkeys, 2, True, True, cap, "a + c")
    apart = R.merge_groups(ea, ec)
    assert apart["n"] == ea["n"] + ec["n"]
    R.assert_same_groups(got, apart, "merge: disjoint")
    # lists absent in the second call while the table carries them: sizes, counts and sums add,
    # sumsq / min / max are those of the first call alone
    zeros = [np.zeros(eb["n"]) for _ in range(2)]
    nans = [np.full(eb["n"], np.nan) for _ in range(2)]
    _, _, got = merged(K, [ca, cb], nkeys, 2, True, True, cap, "b without lists",
                       drop=[(), ("sumsq", "minmax")])
    exp = R.merge_groups(ea, dict(eb, sumsq=zeros, min=nans, max=nans))
    R.assert_same_groups(got, exp, "merge: b without sumsq / min / max")
    _, _, got = merged(K, [ca, cb], nkeys, 2, True, True, cap, "b without sumsq", drop=[(), ("sumsq",)])
    R.assert_same_groups(got, R.merge_groups(ea, dict(eb, sumsq=zeros)), "merge: b without sumsq")


@pytest.mark.parametrize("fill", ["one", "half", "three_quarters"])
@pytest.mark.parametrize("capacity", [64, 2048, 4096, 65536])
def test_compact_tiles(K, capacity, fill):
    groups = {"one": 1, "half": capacity // 2, "three_quarters": capacity * 3 // 4}[fill]
    rng = np.random.default_rng(seed_of("compact", capacity, fill))
    k0 = rng.integers(I64.min, I64.max, groups, dtype=np.int64)
    assert np.unique(k0).size == groups
    keys = [rng.permutation(np.concatenate([k0, k0, k0[:3]])), None]
    keys[1] = keys[0] % 5
    n = keys[0].size
    kvalid = [None, None]
    vals, vvalid = value_columns(rng, n, 2, keys)
    path = "rows" if n < SWITCH else "sort"
    exp = R.table_groups(keys, kvalid, vals, vvalid, minmax=True)
    assert exp["n"] == groups
    what = f"compact capacity={capacity} groups={groups}"
    t, comp, got = table(K, [(keys, kvalid, vals, vvalid, path)], 2, False, True, capacity, what,
                         groups=groups)
    assert t.capacity == capacity
    R.assert_same_groups(got, exp, what, sumsq=False)
    rows_find_their_group(K, t, comp, keys, kvalid, what)
    g = host(t.lookup([dev(keys[0][:50] ^ 1), dev(keys[1][:50])], [None, None]))
    assert (g == -1).all(), f"{what}: keys that are not in the table"


@pytest.mark.parametrize("nkeys", [1, 2, 3])
def test_index_build_and_lookup(K, nkeys):
    rng = np.random.default_rng(seed_of("index", nkeys))
    keys, kvalid = key_columns(rng, 5000, nkeys, "skewed")
    kvalid = [rng.random(5000) >= 0.1 for _ in range(nkeys)]
    g = R.table_groups(keys, kvalid, [], None)
    rows, rvalid = key_columns(rng, 3000, nkeys, "skewed")
    rows = [np.concatenate([r, k[:2000]]) for r, k in zip(rows, keys)]      # absent and present keys
    rvalid = [np.concatenate([np.ones(3000, bool) if v is None else v, w[:2000]])
              for v, w in zip(rvalid, kvalid)]
    some_null = ~np.logical_and.reduce(rvalid)
    for name, pick in (("with null groups", np.ones(g["n"], bool)), ("without null groups", g["null_mask"] == 0)):
        gk = [k[pick] for k in g["keys"]]
        gm = g["null_mask"][pick]
        t = K.GroupbyTable(nkeys, 0, capacity_for(gm.size))
        t.index_build([dev(k) for k in gk], dev(gm))
        exp = R.lookup(gk, gm, rows, rvalid)
        got = host(t.lookup([dev(r) for r in rows], [bitmap(v) for v in rvalid]))
        R.first_mismatch(got, exp, f"index {name} nkeys={nkeys}")
        assert (exp == -1).any() and (exp >= 0).any()
        if name == "without null groups":
            assert (got[some_null] == -1).all()
        else:
            assert (got[some_null] >= 0).any()
    # a table built from no groups at all
    t = K.GroupbyTable(nkeys, 0, 64)
    t.index_build([dev(k[:0]) for k in g["keys"]], dev(g["null_mask"][:0]))
    assert (host(t.lookup([dev(r) for r in rows], [bitmap(v) for v in rvalid])) == -1).all()


@pytest.mark.parametrize("path,n", [("rows", 3000), ("sort", 33_000)])
def test_overflow_is_reported_and_the_groups_with_a_slot_stay_exact(K, path, n):
    """200 distinct keys into 64 slots: find_slot gives up after kGbMaxProbe probes and returns
    normally, ST_OVERFLOW is set, and a key that did get a slot has all its rows."""
    from nvtabular_amd import _lib

    rng = np.random.default_rng(seed_of("overflow", n))
    k0 = rng.integers(I64.min, I64.max, 200, dtype=np.int64)
    keys = [k0[rng.integers(0, 200, n)]]
    vals, vvalid = value_columns(rng, n, 2)
    exp = R.table_groups(keys, [None], vals, vvalid, sumsq=True, minmax=True)
    assert exp["n"] == 200
    assert_exact(vals, n)
    t, comp, got = table(K, [(keys, [None], vals, vvalid, path)], 2, True, True, 64,
                         f"overflow {path}", overflow=True)
    assert t.capacity == 64 and got["n"] == 64 == t.state()[_lib.ST_OCCUPIED]
    at = np.searchsorted(exp["keys"][0], got["keys"][0])
    pick = lambda lst: [x[at] for x in lst]  # noqa: E731
    sub = dict(keys=pick(exp["keys"]), null_mask=exp["null_mask"][at], size=exp["size"][at],
               count=exp["count"][at], sum=pick(exp["sum"]), sumsq=pick(exp["sumsq"]),
               min=pick(exp["min"]), max=pick(exp["max"]), n=64)
    R.assert_same_groups(got, sub, f"overflow {path}")


def test_compact_reports_a_group_of_infinities_as_no_value_seg_aggregate_does_not(K):
    """include/nvt_hip.h, nvt_gb_compact: the table has no per-column value count, +inf in min
    (-inf in max) IS "no value seen".  A group whose values are all +inf therefore reports min NaN
    (its max is +inf), all -inf max NaN.  nvt_seg_aggregate counts per column: its caller sees the
    true infinity next to a count > 0."""
    inf = np.inf
    keys = [np.array([1, 1, 2, 2, 3, 3, 4], np.int64)]
    v = np.array([inf, inf, -inf, -inf, 1.0, inf, np.nan])
    for path, reps in (("rows", 1), ("sort", 5000)):
        kk, vv = [np.tile(keys[0], reps)], np.tile(v, reps)
        _, _, got = table(K, [(kk, [None], [vv], [None], path)], 1, False, True, 64, f"inf {path}", groups=4)
        assert got["keys"][0].tolist() == [1, 2, 3, 4]
        np.testing.assert_array_equal(got["min"][0], [np.nan, -inf, 1.0, np.nan])
        np.testing.assert_array_equal(got["max"][0], [inf, np.nan, inf, np.nan])
        np.testing.assert_array_equal(got["sum"][0], [inf, -inf, inf, 0.0])
        ref = R.table_groups(kk, [None], [vv], [None], minmax=True)      # the true values
        np.testing.assert_array_equal(ref["min"][0], [inf, -inf, 1.0, np.nan])
        np.testing.assert_array_equal(ref["max"][0], [inf, -inf, inf, np.nan])
        gid = kk[0] - 1
        words = R.order_rows(gid.size, (), True, gid, 4)
        size, count, _, _, mn, mx = dev_seg(K, words, 4, [vv], [None], False, True)
        R.first_mismatch(count[0], np.array([2, 2, 2, 0]) * reps, "count")
        np.testing.assert_array_equal(np.where(count[0] > 0, mn[0], np.nan), ref["min"][0])
        np.testing.assert_array_equal(np.where(count[0] > 0, mx[0], np.nan), ref["max"][0])
        assert mn[0][3] == inf and mx[0][3] == -inf                       # untouched initial values


@pytest.mark.parametrize("path,n", [("rows", 20_000), ("sort", 40_000)])
def test_table_general_values_within_the_summation_bound(K, path, n):
    rng = np.random.default_rng(seed_of("general", n))
    keys, kvalid = key_columns(rng, n, 1, "skewed")
    vals = [rng.normal(0, 1e3, n), rng.normal(0, 1e3, n).astype(np.float32)]
    vals[0][rng.random(n) < 0.1] = np.nan
    vvalid = [None, rng.random(n) >= 0.2]
    exp = R.table_groups(keys, kvalid, vals, vvalid, sumsq=True, minmax=True)
    _, _, got = table(K, [(keys, kvalid, vals, vvalid, path)], 2, True, True, capacity_for(exp["n"]),
                      f"general {path}", groups=exp["n"])
    R.assert_same_groups(dict(got, sum=[], sumsq=[], min=[], max=[]),
                         dict(exp, sum=[], sumsq=[], min=[], max=[]), f"general {path}")
    for j in range(2):
        by_group = R.split_by_group(vals[j], vvalid[j], exp["row_group"], exp["n"])
        sum_bound_check(got["sum"][j], by_group, f"general {path} sum[{j}]")
        sum_bound_check(got["sumsq"][j], [v * v for v in by_group], f"general {path} sumsq[{j}]")
        np.testing.assert_array_equal(got["min"][j], exp["min"][j])
        np.testing.assert_array_equal(got["max"][j], exp["max"][j])


# ---------------------------------------------------------------------------------------------
# row order
# ---------------------------------------------------------------------------------------------
SORT_DTYPES = ["float32", "float64", "int32", "int64", "uint8", "bool"]


def dev_order(K, n, cols=(), ascending=True, gid=None, ngroups=0):
    """K.order_rows over host columns [(values, validity bools or None), ...]."""
    asc = [ascending] * len(cols) if isinstance(ascending, bool) else list(ascending)
    sk = [(dev(v), bitmap(ok), a) for (v, ok), a in zip(cols, asc)]
    w = K.order_rows(n, torch.device("cuda", torch.cuda.current_device()), sk, dev(gid), ngroups)
    assert w.dtype == torch.int64 and w.numel() == n
    return host(w)


def rows_of(words):
    return words & 0xFFFFFFFF


def sort_column(rng, n, dtype, nulls):
    """Many duplicates (a pool of edge values) mixed with values whose 64-bit images differ in
    both 32-bit halves; NaN among the floats; optional validity."""
    if dtype.startswith("float"):
        tiny = np.finfo(dtype).smallest_subnormal
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 4 * tiny, 1.5, -1.5,
                         np.finfo(dtype).max, np.finfo(dtype).min, np.finfo(dtype).tiny], dtype)
        wide = rng.normal(0, 1e6, n).astype(dtype)
    elif dtype == "bool":
        return rng.random(n) < 0.5, (rng.random(n) >= 0.2 if nulls else None)
    elif dtype == "uint8":
        pool = np.array([0, 1, 127, 128, 254, 255], np.uint8)
        wide = rng.integers(0, 256, n).astype(np.uint8)
    else:
        i = np.iinfo(dtype)
        pool = np.array([i.min, i.min + 1, i.max - 1, i.max, 0, -1, 1, 77], dtype)
        wide = rng.integers(i.min, i.max, n, dtype=dtype)
    v = np.where(rng.random(n) < 0.6, pool[rng.integers(0, pool.size, n)], wide).astype(pool.dtype)
    return v, (rng.random(n) >= 0.2 if nulls else None)


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", SORT_DTYPES)
def test_one_sort_column(K, dtype, ascending):
    for n in (0, 1, 2, 4095, 4096, 4097, 100_003):
        for nulls in (False, True):
            rng = np.random.default_rng(seed_of("sort column", dtype, n, nulls))
            v, ok = sort_column(rng, n, dtype, nulls)
            exp = R.sort_key_order([(v, ok)], ascending)
            got = rows_of(dev_order(K, n, [(v, ok)], ascending))
            R.first_mismatch(got, exp, f"{dtype} asc={ascending} n={n} nulls={nulls}")


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_signed_zeros_tie_and_keep_row_order(K, dtype, ascending):
    for zeros in ([0.0, -0.0], [-0.0, 0.0], [0.0, -0.0, 0.0, -0.0, -0.0, 0.0]):
        v = np.array(zeros + [1.0, -1.0], dtype)
        m = len(zeros)
        exp = [m + 1] + list(range(m)) + [m] if ascending else [m] + list(range(m)) + [m + 1]
        assert R.sort_key_order([(v, None)], ascending).tolist() == exp
        got = rows_of(dev_order(K, v.size, [(v, None)], ascending))
        assert got.tolist() == exp, f"{dtype} {zeros} asc={ascending}: {got.tolist()}"


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
def test_the_reserved_null_image_ties_the_two_int64_values_at_the_far_end(K, ascending):
    """include/nvt_hip.h, nvt_sort_key_u64: the largest 64-bit image belongs to the nulls, the
    value that would map to it shares the image below -- INT64_MAX with INT64_MAX - 1 ascending,
    INT64_MIN with INT64_MIN + 1 descending: the pair stays in ROW order, in front of the nulls.
    The pair at the other end, int32 and uint8 columns (widened first) and floats (the images of
    that end are NaN bit patterns: -inf and -DBL_MAX descending are apart) order exactly."""
    a, b = (I64.max, I64.max - 1) if ascending else (I64.min, I64.min + 1)
    for pair in ([a, b], [b, a]):
        v = np.array(pair + [0, 0], np.int64)
        ok = np.array([1, 1, 1, 0], bool)
        got = rows_of(dev_order(K, 4, [(v, ok)], ascending)).tolist()
        assert got == [2, 0, 1, 3] == R.sort_key_order([(v, ok)], ascending).tolist(), (pair, got)
    c, d = (I64.min, I64.min + 1) if ascending else (I64.max, I64.max - 1)    # the near end: exact
    for pair, exp in (([c, d], [0, 1, 2]), ([d, c], [1, 0, 2])):
        v = np.array(pair + [0], np.int64)
        assert rows_of(dev_order(K, 3, [(v, None)], ascending)).tolist() == exp, pair
    for dtype in (np.int32, np.uint8):
        i = np.iinfo(dtype)
        for pair in ([i.max, i.max - 1], [i.max - 1, i.max], [i.min, i.min + 1], [i.min + 1, i.min]):
            v = np.array(pair, dtype)
            exp = [0, 1] if (pair[0] < pair[1]) == ascending else [1, 0]
            assert rows_of(dev_order(K, 2, [(v, None)], ascending)).tolist() == exp, (dtype, pair)
    for dtype in (np.float32, np.float64):
        f = np.finfo(dtype)
        v = np.array([f.min, -np.inf, -np.inf, f.min, np.inf, f.max, np.nan], dtype)
        exp = [1, 2, 0, 3, 5, 4, 6] if ascending else [4, 5, 0, 3, 1, 2, 6]
        assert rows_of(dev_order(K, 7, [(v, None)], ascending)).tolist() == exp, dtype
        assert R.sort_key_order([(v, None)], ascending).tolist() == exp


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
def test_several_sort_columns(K, ascending):
    """The less significant columns decide only inside the ties of the more significant ones."""
    for n in (4097, 50_021):
        rng = np.random.default_rng(seed_of("columns", n))
        cols = [(rng.integers(0, 5, n).astype(np.uint8), rng.random(n) >= 0.1),
                (np.round(rng.normal(0, 3, n)).astype(np.float32), None),
                sort_column(rng, n, "int64", True)]
        for m in (2, 3):
            R.first_mismatch(rows_of(dev_order(K, n, cols[:m], ascending)),
                             R.sort_key_order(cols[:m], ascending), f"{m} columns n={n}")
        asc = [ascending, not ascending, ascending]
        R.first_mismatch(rows_of(dev_order(K, n, cols, asc)), R.sort_key_order(cols, asc),
                         f"a direction per column n={n}")


@pytest.mark.parametrize("ngroups", [0, 1, 255, 256, 257, 65_535, 65_536])
def test_group_refinement(K, ngroups):
    n = 70_001
    rng = np.random.default_rng(seed_of("gid", ngroups))
    gid = rng.integers(0, ngroups, n) if ngroups else np.full(n, -1, np.int64)
    gid[rng.random(n) < 0.05] = -1
    if ngroups:
        gid[[7, n - 1]] = ngroups - 1                 # the largest id and the null marker above it
        gid[[0, n - 2]] = 0
    gid[3] = -1
    ts = rng.integers(0, 50, n).astype(np.int32)
    for cols in ((), [(ts, None)]):
        what = f"ngroups={ngroups} sort columns={len(cols)}"
        got = dev_order(K, n, cols, True, gid, ngroups)
        R.first_mismatch(got, R.order_rows(n, cols, True, gid, ngroups), what)
        rows = rows_of(got)
        assert np.array_equal(np.sort(rows), np.arange(n)), f"{what}: not a permutation"
        R.first_mismatch(got >> 32, np.where(gid[rows] < 0, ngroups, gid[rows]), f"{what}: high half")
        nulls = rows[(got >> 32) == ngroups]
        assert nulls.size == (gid == -1).sum() and (got[n - nulls.size:] >> 32 == ngroups).all()
        if not cols:
            assert (np.diff(nulls) > 0).all(), f"{what}: null rows out of their prior order"


@pytest.mark.parametrize("ascending", [True, False], ids=["asc", "desc"])
def test_groupby_contract_sort_columns_then_groups(K, ascending):
    for n in (0, 1, 4097, 100_003):
        rng = np.random.default_rng(seed_of("contract", n))
        G = 300
        gid = rng.integers(-1, G, n)
        cols = [sort_column(rng, n, "float64", True), (rng.integers(0, 9, n).astype(np.int32), None)]
        got = dev_order(K, n, cols, ascending, gid, G)
        R.first_mismatch(got, R.order_rows(n, cols, ascending, gid, G), f"contract n={n}")
        R.first_mismatch(dev_order(K, n), np.arange(n, dtype=np.int64), f"identity n={n}")


# ---------------------------------------------------------------------------------------------
# segmented reduce
# ---------------------------------------------------------------------------------------------
def dev_seg(K, words, ngroups, vals, vvalid, sumsq, minmax):
    """K.seg_aggregate on host columns -> host arrays (count cut to [V, G])."""
    out = K.seg_aggregate(dev(words), ngroups, [dev(v) for v in vals], [bitmap(v) for v in vvalid],
                          sumsq=sumsq, minmax=minmax)
    size, count, sm, sq, mn, mx = (None if t is None else host(t) for t in out)
    nv = len(vals)
    assert (sq is None) == (not (sumsq and nv)) and (mn is None) == (mx is None) == (not (minmax and nv))
    return size, count[:nv], sm[:nv], sq, mn, mx


def run_lengths(rng, n, shape):
    """Lengths of consecutive runs that add up to n."""
    if shape == "one":
        return np.array([n])
    if shape == "ones":
        return np.ones(n, np.int64)
    if shape in ("r63", "r64", "r65"):
        pat = [int(shape[1:])]
    elif shape == "lane63":                       # every second run ends at lane 63, another group follows
        pat = [1, 63, 64, 5, 59, 128, 30, 34]
    elif shape == "span":                         # short runs, then one run over several whole chunks
        c = chunk_words(n)
        pat = rng.integers(1, 40, 5).tolist() + [min(5 * c + 17, max(n - 200, 1))] + rng.integers(1, 300, 400).tolist()
    else:                                         # mixed
        pat = np.minimum(rng.geometric(0.02, 4000), 700).tolist()
    lens = np.resize(np.array(pat, np.int64), n)  # (more than enough of them)
    ends = np.cumsum(lens)
    m = int(np.searchsorted(ends, n)) + 1
    lens = lens[:m].copy()
    lens[-1] -= ends[m - 1] - n
    assert lens.sum() == n and (lens > 0).all()
    return lens


def seg_case(rng, n, shape, gaps=False, null_tail=False):
    """(gid per row, ngroups): the runs of ``shape`` laid over a random permutation of the rows
    (values are gathered by row); gaps: only every third id is used and five ids at the end stay
    empty; null_tail: the last run(s), ~10 % of the rows, are rows of null keys (gid -1)."""
    lens = run_lengths(rng, n, shape)
    ids = np.arange(lens.size, dtype=np.int64)
    if gaps:
        ids = ids * 3 + 1
    G = int(ids[-1]) + 1 + (5 if gaps else 0)
    sorted_gid = np.repeat(ids, lens)
    if null_tail:
        cut = n - max(n // 10, 1)
        G = int(sorted_gid[cut - 1]) + 1 + (5 if gaps else 0) if cut > 0 else 1
        sorted_gid[cut:] = -1
    gid = np.empty(n, np.int64)
    gid[rng.permutation(n)] = sorted_gid
    return gid, G


def check_seg(K, gid, G, vals, vvalid, sumsq, minmax, what, words=None):
    n = gid.size
    words = R.order_rows(n, (), True, gid, G) if words is None else words
    exp = R.seg_aggregate(words, G, vals, vvalid, sumsq, minmax)
    got = dev_seg(K, words, G, vals, vvalid, sumsq, minmax)
    names = ("size", "count", "sum", "sumsq", "min", "max")
    for name, g, e in zip(names, got, exp):
        assert (g is None) == (e is None), f"{what}: {name}"
        if g is None:
            continue
        assert g.shape == e.shape, f"{what}: {name} shape {g.shape}, expected {e.shape}"
        if name in ("size", "count"):
            R.first_mismatch(g.reshape(-1), e.reshape(-1), f"{what}: {name}")
        else:
            np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")
    return exp


def seg_values(rng, n, nvals):
    """value_columns in another dtype order (mixed dtypes from three columns on), NaN and
    bitmaps as there: the counts differ between the columns."""
    vals, vvalid = value_columns(rng, n, 8)
    pick = [0, 2, 1, 3, 4, 5, 6, 7][:nvals]
    return [vals[j] for j in pick], [vvalid[j] for j in pick]


SEG_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 32_768, 100_003]
SEG_SHAPES = ["one", "ones", "r64", "r63", "r65", "lane63", "span", "mixed"]


@pytest.mark.parametrize("n", SEG_SIZES)
def test_seg_aggregate_run_shapes(K, n):
    rng = np.random.default_rng(seed_of("seg", n))
    vals, vvalid = seg_values(rng, n, 2)
    assert_exact(vals, n)
    for shape in SEG_SHAPES:
        for gaps, null_tail in ((False, False), (True, True)):
            gid, G = seg_case(rng, n, shape, gaps, null_tail)
            what = f"seg n={n} {shape} gaps={gaps} null_tail={null_tail}"
            size = check_seg(K, gid, G, vals, vvalid, True, True, what)[0]
            if gaps:
                assert size[-1] == 0 and (G < 3 or size[2] == 0) and (gid == -1).any(), what
            if shape == "span" and n > 2000 and not null_tail:
                assert size.max() > 5 * chunk_words(n), what


@pytest.mark.parametrize("n", LARGE)
def test_seg_aggregate_chunks_of_several_trips(K, n):
    """Chunks of 320 / 832 words: runs of every length cross rows, trips and chunks; one run spans
    several whole chunks; empty groups and a tail of null-key words."""
    assert chunk_words(n) > TRIP
    rng = np.random.default_rng(seed_of("seg large", n))
    v = (rng.integers(-2**14, 2**14 + 1, n) / 16.0)
    v[rng.random(n) < 0.1] = np.nan
    assert_exact([v], n)
    gid, G = seg_case(rng, n, "span", gaps=True, null_tail=True)
    size = check_seg(K, gid, G, [v], [None], True, True, f"seg large n={n}")[0]
    assert size.max() > 5 * chunk_words(n) and size[-1] == 0


@pytest.mark.parametrize("n", [1025, 100_003])
@pytest.mark.parametrize("nvals", [0, 1, 3, 8])
def test_seg_aggregate_value_columns_and_flags(K, nvals, n):
    rng = np.random.default_rng(seed_of("seg values", n, nvals))
    vals, vvalid = seg_values(rng, n, nvals)
    assert_exact(vals, n)
    gid, G = seg_case(rng, n, "mixed", gaps=True, null_tail=True)
    if nvals > 1:
        vvalid[1] = (rng.random(n) >= 0.2) & (gid != gid[0])        # a group without a value in column 1
    for sumsq, minmax in FLAGS:
        what = f"seg values n={n} nvals={nvals} sumsq={sumsq} minmax={minmax}"
        size, count, sm, sq, mn, mx = check_seg(K, gid, G, vals, vvalid, sumsq, minmax, what)
        if nvals > 1 and gid[0] >= 0:
            g = gid[0]
            assert size[g] > 0 and count[1][g] == 0 and sm[1][g] == 0
            assert mn is None or (mn[1][g] == np.inf and mx[1][g] == -np.inf)
            assert (count[0] != count[1]).any()


def test_seg_aggregate_groups_of_infinities(K):
    n = 3000
    rng = np.random.default_rng(seed_of("seg inf"))
    gid, G = seg_case(rng, n, "r65")
    v = (rng.integers(-2**14, 2**14, n) / 16.0)
    v[gid % 3 == 0] = np.inf
    v[gid % 3 == 1] = -np.inf
    w = v.astype(np.float32)
    ok = rng.random(n) >= 0.3
    _, count, sm, sq, mn, mx = check_seg(K, gid, G, [v, w], [None, ok], True, True, "seg inf")
    assert (mn[0][0::3] == np.inf).all() and (mx[0][1::3] == -np.inf).all() and (count[0] > 0).all()
    assert (sm[0][0::3] == np.inf).all() and (sq[1][1::3][count[1][1::3] > 0] == np.inf).all()


@pytest.mark.parametrize("n", [40_000])
def test_seg_aggregate_general_values_within_the_summation_bound(K, n):
    rng = np.random.default_rng(seed_of("seg general"))
    gid, G = seg_case(rng, n, "mixed", gaps=True, null_tail=True)
    vals = [rng.normal(0, 1e3, n), rng.normal(0, 1e3, n).astype(np.float32)]
    vals[0][rng.random(n) < 0.1] = np.nan
    vvalid = [None, rng.random(n) >= 0.2]
    words = R.order_rows(n, (), True, gid, G)
    exp = R.seg_aggregate(words, G, vals, vvalid, True, True)
    got = dev_seg(K, words, G, vals, vvalid, True, True)
    R.first_mismatch(got[0], exp[0], "size")
    R.first_mismatch(got[1].reshape(-1), exp[1].reshape(-1), "count")
    np.testing.assert_array_equal(got[4], exp[4])
    np.testing.assert_array_equal(got[5], exp[5])
    for j in range(2):
        by_group = R.split_by_group(vals[j], vvalid[j], gid, G)
        sum_bound_check(got[2][j], by_group, f"seg general sum[{j}]")
        sum_bound_check(got[3][j], [v * v for v in by_group], f"seg general sumsq[{j}]")


def test_order_rows_into_seg_aggregate_on_the_device(K):
    """The two device calls chained, as ops/groupby.py does: the words never leave the GPU."""
    n, G = 100_003, 5000
    rng = np.random.default_rng(seed_of("chain"))
    gid = (rng.random(n) ** 2 * G).astype(np.int64)
    gid[rng.random(n) < 0.05] = -1
    ts = rng.integers(0, 1000, n).astype(np.int32)
    vals, vvalid = seg_values(rng, n, 3)
    assert_exact(vals, n)
    words = K.order_rows(n, torch.device("cuda", torch.cuda.current_device()), [(dev(ts), None, False)],
                         dev(gid), G)
    out = K.seg_aggregate(words, G, [dev(v) for v in vals], [bitmap(v) for v in vvalid], sumsq=True,
                          minmax=True)
    ref_words = R.order_rows(n, [(ts, None)], False, gid, G)
    R.first_mismatch(host(words), ref_words, "chain: words")
    exp = R.seg_aggregate(ref_words, G, vals, vvalid, True, True)
    R.first_mismatch(host(out[0]), exp[0], "chain: size")
    R.first_mismatch(host(out[1]).reshape(-1), exp[1].reshape(-1), "chain: count")
    for name, g, e in zip(("sum", "sumsq", "min", "max"), out[2:], exp[2:]):
        np.testing.assert_array_equal(host(g), e, err_msg=f"chain: {name}")
