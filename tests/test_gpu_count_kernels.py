"""Kernel-level matrix for Categorify's counting step: ``K.DenseCountJob`` / ``K.dense_count_many``,
``K.CountTable`` / ``K.count_into_new_table``, ``K.merge_dense`` / ``K.merge_dense_many`` and
``K.range_splitters`` called directly on torch tensors, every (key, count) list compared with the
numpy references of count_reference.py (which test_count_reference.py pins to the pandas oracle on
the CPU).  Nothing is approximate here: every comparison is exact.

Path id -> kernels (csrc/; nvt_dense_count.hip is the driver that decodes the path and checks the
arguments):

    6 / 0 / 7   LDS-resident, nvt_count_lds.hip: lds_stage_kernel<K, u32 | u64, 16384 | 8192> (one /
                one / two key classes per row slab; 6 replicates hot keys per 8-lane group) +
                range_merge_kernel
    1 / 2 / 3   partitioned, nvt_count_part.hip: part_hist_kernel -> scan -> part_scatter_kernel<LEVEL
                1 (, 2)> -> part_count_kernel -> part_offsets / part_copy / part_merge_kernel
                (256 / 64 x 64 / 64 x 256 buckets)
    1|16 ..     the same behind the hot-key filter (int32 keys, no weights): hot_sample_kernel
                (nvt_hot_sample.hip), part_hist_hot_kernel (cold bitmap) ... hot_reduce_kernel
    9           range path, nvt_range_count.hip: hot_sample_kernel (range map, nvt_hot_sample.hip),
                rp_partition_kernel,
                hot_totals_kernel, rp_count_kernel; key-ordered list, class histogram, dumped table
    10          sort path, nvt_sort_count.hip: sc_pack, s32_hist / s32_base / s32_scatter (radix
                passes), sc_rle_kernel, sc_counts_kernel; key-ordered list, class histogram
    -1          nvt_count.hip: one open-addressing table in HBM (CountTable), nvt_count_merge_* with
                weights

One helper per way of reaching a family (``lds``, ``part``, ``rng_path``, ``sort_path``,
``fallback``), and every helper asserts the path the column ENDED on and that nothing was
relaunched; the cases that are designed to escalate assert where they end and that
``K.STATS["count_relaunches"]`` moved.  No case accepts "either path".

Sizes, from the constants of the .hip files.  lds_stage_kernel, unweighted: the column is
nvec = n / VEC 16-byte vectors (VEC = 4 int32 / 2 int64 keys) cut into kSlabs = 256 contiguous
slabs of ceil(nvec / 256); the 16 waves of a workgroup draw batches of NVT_STAGE_U * 64 = 128
vectors from an LDS counter; the rows behind the last vector go through a scalar loop; the validity
byte of a vector is shifted by (v * VEC) & 7.  So: 0..9, 63, 65 (nothing but tail / a vector or
two), 255 / 256 / 257 (fewer rows, then fewer vectors, than slabs), 1023 / 1025, B = 256 * 128 *
VEC (every slab exactly one batch), B - 1 (last slab short + tail), B + 1 (tail), B + VEC + 1 (slabs
of 129 vectors: a second, partial batch), 16 * B + 3 (16 batches per slab: every wave draws one).
Weighted: rows i0 = slab * 1024 + thread, stride 256 * 1024 = 262 144, four in flight per trip:
262 143 / 262 145 (second row of a trip), 1 048 576 + 5 (second trip).  Partitioned paths: kTile =
8192 rows per scatter tile, kChunk = 65 536 rows per count workgroup (path 1: max(65 536, n / 256 *
8 / 7 + 1)), and the hot sample reads 64 blocks of 1024 rows, the whole column up to 65 536 rows;
part_hist_hot_kernel walks the tiles with kHotBlocks = 256 workgroups, each with hot counters of its
own that hot_reduce_kernel adds up: 257 * 8192 + 5 rows give every workgroup a tile and one two.
The per-tile histogram (256 counters per tile on path 1) is scanned by one scan_small_kernel launch
up to kScanSmallMax = 131 072 counters and by scan_chunk_kernel + scan_totals_kernel beyond: 513 *
8192 + 3 rows are 514 tiles.
Range path: one round of a partition workgroup is kRpBS * NVT_RANGE_U = 2048 vectors = 8192 rows,
256 workgroups: 2 097 152 rows are one full round each; 2 * 2 097 152 + 5003 three rounds with a
ragged end.  Sort path: tiles of kS32Tile = 8192 words (radix passes) and kScTile = 4096 (run
lengths).

Weights: 1 .. 999 and, on a few keys, single weights up to 2^40, so that per-key sums pass 2^32 on
every weighted instantiation.  Weight 0 and negative weights are left out: include/nvt_hip.h does
not define them (the merge step only ever adds counts >= 1).

Left out, by name: the vocabulary ordering kernels (cls_scatter, range_patch, flat_build, the radix
and small sorts) beyond the order of the one table the piecewise case builds; the multi-GPU exchange (dist._hip_merge_counts) and string
keys; the cold-start prefix sketch (nvt_prefix_distinct: columns of >= 2 M rows with hint 0).
"""
import zlib

import numpy as np
import pytest
import torch

import count_reference as R
import encode_reference as ER

pytestmark = pytest.mark.gpu

NP = {"int32": np.int32, "int64": np.int64}
LO = {"int32": np.iinfo(np.int32).min, "int64": np.iinfo(np.int64).min}
HI = {"int32": np.iinfo(np.int32).max, "int64": np.iinfo(np.int64).max}
VEC = {"int32": 4, "int64": 2}
TINY = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 65, 255, 256, 257, 1023, 1025]
ROUND = 256 * 8192          # range path: one full round of every partition workgroup


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


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------
def keyset(dist, m, dtype):
    """m distinct keys (never the smallest integer of the type)."""
    j = np.arange(m, dtype=np.int64)
    if dist == "scrambled":      # x -> a x + b mod 2^31 is a bijection (a odd): spread over [0, 2^31)
        k = ((j + 1) * 2654435761 + 12345) % (2**31)
    elif dist == "dense":
        k = j
    elif dist == "stride16":     # low 16 bits zero, both signs
        k = (j - m // 2) << 16
    elif dist == "stride20":
        k = (j - m // 2) << 20
    elif dist == "collide":      # int64: five low words, the rest of the key above bit 32, both signs
        k = (j % 5) + ((j // 5 - m // 10) << 32)
    else:
        raise AssertionError(dist)
    i = np.iinfo(NP[dtype])
    assert np.unique(k).size == m and k.min() > i.min and k.max() <= i.max, (dist, m, dtype)
    return k.astype(NP[dtype])


def column(dist, n, m, dtype, rng, shape="zipf", extremes=True):
    """n rows over (at most) m distinct keys of `dist`; shape: zipf / uniform / single / distinct."""
    if n == 0:
        return np.empty(0, NP[dtype])
    if shape == "distinct":
        keys = rng.permutation(keyset(dist, n, dtype))
    elif shape == "single":
        keys = np.full(n, keyset(dist, 3, dtype)[2])
    else:
        pool = rng.permutation(keyset(dist, max(1, min(m, n)), dtype))
        pos = (np.minimum(rng.zipf(1.2, n) - 1, pool.size - 1) if shape == "zipf"
               else rng.integers(0, pool.size, n))
        keys = pool[pos]
    if extremes and n >= 8 and shape != "single":   # the smallest and the largest value, valid rows or not
        keys[rng.integers(0, n, 2)] = LO[dtype]
        if dist != "dense":    # (dense ids beside one far outlier are the range path's fallback case)
            keys[rng.integers(0, n, 2)] = HI[dtype]
    return keys


def patterns(n, rng):
    """(name, validity as bool or None): no bitmap at all (None) + seven bitmaps."""
    first = np.zeros(n, bool)
    first[:1] = True
    last = np.zeros(n, bool)
    last[n - 1:] = True
    return [("no-bitmap", None), ("all-set", np.ones(n, bool)), ("all-clear", np.zeros(n, bool)),
            ("alternating", np.arange(n) % 2 == 0), ("first-bit-only", first), ("last-bit-only", last),
            ("byte-runs", (np.arange(n) // 8) % 3 != 1), ("random10", rng.random(n) >= 0.1)]


def poison(keys, valid, dtype, rng):
    """Bytes under the null rows: keys that occur in the column, the smallest key, random keys."""
    if valid is None or valid.all():
        return keys
    keys = keys.copy()
    idx = np.flatnonzero(~valid)
    keys[idx[0::3]] = keys[rng.integers(0, keys.size, idx[0::3].size)]
    keys[idx[1::3]] = LO[dtype]
    i = np.iinfo(NP[dtype])
    keys[idx[2::3]] = rng.integers(i.min, i.max, idx[2::3].size).astype(NP[dtype])
    return keys


def weights_for(keys, rng):
    """1 .. 999; the rows of a few keys (the smallest key of the type among them, when it is there)
    carry 2^33 .. 2^40, so their sums pass 2^32 from a single row on."""
    n = keys.size
    w = rng.integers(1, 1000, n).astype(np.int64)
    if n:
        heavy = np.unique(keys[rng.integers(0, n, 3)])
        heavy = np.append(heavy, np.array([np.iinfo(keys.dtype).min], keys.dtype))
        rows = np.flatnonzero(np.isin(keys, heavy))
        rows = rows[:: max(1, rows.size // 2000)]              # (keeps every total far below 2^63)
        w[rows] = np.int64(1) << rng.integers(33, 41, rows.size)
        w[rng.integers(0, n, 1)] = np.int64(1) << 40           # null row or not
    return w


# ---------------------------------------------------------------------------------------------
# one launch, one check
# ---------------------------------------------------------------------------------------------
def launch(K, keys, valid=None, weights=None, path=None, hint=0, hot=None, bits=8, pieces=None,
           allow_range=True, cap=None):
    """-> (result, relaunches, job).  path None: the driver picks it from the hint."""
    job = K.DenseCountJob(dev(keys), None if valid is None else dev(R.pack_bits(valid)), dev(weights),
                          hint=hint, allow_range=allow_range, pieces=pieces, min_range_bits=bits)
    if path is not None:
        job.path = path
    job.hot = hot
    if cap is not None:
        job.cap_guess = cap
    before = K.STATS["count_relaunches"]
    res = K.dense_count_many([job])[0]
    return res, K.STATS["count_relaunches"] - before, job


def check(K, res, keys, valid, weights, path, what):
    """Everything a count result promises, against count_ref."""
    k, c, nulls, info = res
    n = keys.size
    ek, ec, en = R.count_ref(keys, valid, weights)
    what = f"{what} rows={n} [path {info['path']}]"
    if n == 0:   # the driver answers an empty column itself: nothing is launched
        assert info == dict(path=0, distinct=0, max_count=0, rows=0) and nulls == 0 and k.numel() == 0, what
        return ek, ec
    assert info["path"] == path, f"{what}: expected path {path}: {info}"
    hk, hc = host(k), host(c)
    assert hc.dtype == np.int64 and hk.dtype == keys.dtype, what
    ordered = path in (K.PATH_RANGE, K.PATH_SORT)
    if not ordered:   # hash paths and the fallback: any order, every key once
        o = np.argsort(hk, kind="stable")
        hk, hc = hk[o], hc[o]
        assert np.unique(hk).size == hk.size, f"{what}: a key occurs twice in the list"
    R.list_mismatch(hk, hc, ek, ec, what)
    assert nulls == en, f"{what}: nulls {nulls}, expected {en}"
    assert info["rows"] == n, f"{what}: rows {info['rows']}"
    assert info["distinct"] == ek.size, f"{what}: distinct {info['distinct']}, expected {ek.size}"
    # include/nvt_hip.h: state[NVT_ST_MAXCOUNT] is the largest count of the list on EVERY path
    exp_max = int(ec.max()) if ec.size else 0
    assert info["max_count"] == exp_max, f"{what}: max_count {info['max_count']}, expected {exp_max}"
    if ordered:
        assert info["sorted_by_key"], what
        hist = host(info["cls_hist"]).astype(np.int64) & 0xFFFFFFFF
        ER.first_mismatch(hist, R.class_hist_ref(ec), what + ": cls_hist")
        assert info["n_big"] == R.n_big_ref(ec), f"{what}: n_big {info['n_big']}, expected {R.n_big_ref(ec)}"
    return ek, ec


def fits(K, keys, valid, weights, path, what, **kw):
    """A case designed to fit its path: ends there, nothing relaunched."""
    res, relaunched, _ = launch(K, keys, valid, weights, path=path, **kw)
    if keys.size:
        assert res[3]["path"] == path and relaunched == 0, \
            f"{what} rows={keys.size}: forced path {path}, ended on {res[3]['path']} after {relaunched} relaunches"
    return check(K, res, keys, valid, weights, path, what)


# distinct keys that ALWAYS fit: 300 keys cannot fill a 384-entry merge table (max_fill(512)) of
# range_merge_kernel even if every key had the same home range, nor the 512-step probe limit
LDS_KEYS = {6: 40, 0: 3000, 7: 3000}


def lds(K, path, keys, valid, weights, what):
    return fits(K, keys, valid, weights, path, f"lds {what}", hint=LDS_KEYS[path])


def part(K, path, hot, keys, valid, weights, what, hint=60_000):
    eligible = keys.dtype == np.int32 and weights is None
    assert not hot or eligible
    return fits(K, keys, valid, weights, path, f"part{'+hot' if hot else ''} {what}", hint=hint, hot=bool(hot))


def rng_path(K, bits, keys, valid, what, hint=20_000, pieces=None):
    res, relaunched, job = launch(K, keys, valid, None, path=K.PATH_RANGE, hint=hint, bits=bits, pieces=pieces)
    what = f"range {1 << bits} buckets {what}"
    if keys.size:
        assert relaunched == 0 and res[3]["path"] == K.PATH_RANGE, f"{what} rows={keys.size}: {res[3]}"
        assert job.range_bits() == bits and res[3]["range_bits"] == bits and not job.range_failed, what
        assert res[3]["range_table"] is not None and res[3]["range_bits_floor"] == bits, what
    check(K, res, keys, valid, None, K.PATH_RANGE, what)
    return res


def sort_path(K, keys, valid, what):
    return fits(K, keys, valid, None, K.PATH_SORT, f"sort {what}", hint=max(keys.size, 1))


def fallback(K, keys, valid, weights, what):
    return fits(K, keys, valid, weights, -1, f"fallback {what}", hint=1000)


# family -> (dtype, weighted, runner(K, keys, valid, weights, what))
FAMILIES = {
    "lds6-i32": ("int32", False, lambda K, k, v, w, s: lds(K, 6, k, v, w, s)),
    "lds0-i32": ("int32", False, lambda K, k, v, w, s: lds(K, 0, k, v, w, s)),
    "lds7-i64": ("int64", False, lambda K, k, v, w, s: lds(K, 7, k, v, w, s)),
    "lds0-i64-weighted": ("int64", True, lambda K, k, v, w, s: lds(K, 0, k, v, w, s)),
    "lds7-i32-weighted": ("int32", True, lambda K, k, v, w, s: lds(K, 7, k, v, w, s)),
    "part1-i32": ("int32", False, lambda K, k, v, w, s: part(K, 1, False, k, v, w, s)),
    "part1-hot": ("int32", False, lambda K, k, v, w, s: part(K, 1, True, k, v, w, s)),
    "part2-hot": ("int32", False, lambda K, k, v, w, s: part(K, 2, True, k, v, w, s)),
    "part2-i64": ("int64", False, lambda K, k, v, w, s: part(K, 2, False, k, v, w, s)),
    "part3-i32-weighted": ("int32", True, lambda K, k, v, w, s: part(K, 3, False, k, v, w, s)),
    "part1-i64-weighted": ("int64", True, lambda K, k, v, w, s: part(K, 1, False, k, v, w, s)),
    "range256": ("int32", False, lambda K, k, v, w, s: rng_path(K, 8, k, v, s)),
    "range1024": ("int32", False, lambda K, k, v, w, s: rng_path(K, 10, k, v, s)),
    "sort": ("int32", False, lambda K, k, v, w, s: sort_path(K, k, v, s)),
    "fallback-i32": ("int32", False, lambda K, k, v, w, s: fallback(K, k, v, w, s)),
    "fallback-i32-weighted": ("int32", True, lambda K, k, v, w, s: fallback(K, k, v, w, s)),
    "fallback-i64-weighted": ("int64", True, lambda K, k, v, w, s: fallback(K, k, v, w, s)),
}


def family_keys(fam):
    """Distinct keys a family's cases use (the LDS paths must fit their tables)."""
    return 40 if fam.startswith("lds6") else 3000 if fam.startswith("lds") else 20_000


# ---------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("path", [6, 0, 7])
def test_lds_paths_at_every_slab_batch_and_vector_edge(K, path, dtype):
    B = 256 * 128 * VEC[dtype]
    rng = np.random.default_rng(seed_of("lds", path, dtype))
    for i, n in enumerate(TINY + [B - 1, B, B + 1, B + VEC[dtype] + 1, 16 * B + 3]):
        keys = column("scrambled" if dtype == "int32" else "collide", n, LDS_KEYS[path], dtype, rng)
        valid = [None, rng.random(n) >= 0.1, np.arange(n) % 3 != 1][i % 3]
        lds(K, path, poison(keys, valid, dtype, rng), valid, None, f"{dtype} sizes")


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("path", [6, 0, 7])
def test_lds_paths_weighted_sums_beyond_32_bits(K, path, dtype):
    rng = np.random.default_rng(seed_of("ldsw", path, dtype))
    for i, n in enumerate([1, 5, 262_143, 262_145, 1_048_576 + 5]):
        keys = column("scrambled", n, LDS_KEYS[path], dtype, rng)
        valid = [None, rng.random(n) >= 0.1][i % 2]
        keys = poison(keys, valid, dtype, rng)
        w = weights_for(keys, rng)
        ek, ec = lds(K, path, keys, valid, w, f"{dtype} weighted")
        assert n < 1000 or (ec >= 2**32).any(), "the case must carry a sum beyond 32 bits"


PART_VARIANTS = [("int32", False, False), ("int32", False, True), ("int32", True, False),
                 ("int64", False, False), ("int64", True, False)]


@pytest.mark.parametrize("dtype,weighted,hot", PART_VARIANTS,
                         ids=["i32", "i32-hot", "i32-weighted", "i64", "i64-weighted"])
@pytest.mark.parametrize("path", [1, 2, 3])
def test_partitioned_paths_at_tile_and_chunk_edges(K, path, dtype, weighted, hot):
    rng = np.random.default_rng(seed_of("part", path, dtype, weighted, hot))
    sizes = [1, 8191, 8192, 8193, 65_535, 65_537, 3 * 65_536 + 8192 + 5]
    if hot:   # 257 tiles: all kHotBlocks = 256 histogram workgroups hold hot counters, one has two tiles
        sizes.append(257 * 8192 + 5)
    for i, n in enumerate(sizes):
        keys = column("scrambled" if dtype == "int32" else "collide", n, 20_000, dtype, rng)
        valid = [rng.random(n) >= 0.1, None][i % 2]
        keys = poison(keys, valid, dtype, rng)
        w = weights_for(keys, rng) if weighted else None
        ek, ec = part(K, path, hot, keys, valid, w, f"{path} {dtype} sizes")
        assert not weighted or n < 1000 or (ec >= 2**32).any()


def chunk_rows(path, n):
    """path_cfg(): rows of a bucket's primary chunk."""
    return min(max(n // 256 + n // 256 // 7 + 1, 65_536), 1 << 20) if path == 1 else 65_536


@pytest.mark.parametrize("dtype,weighted,hot", PART_VARIANTS,
                         ids=["i32", "i32-hot", "i32-weighted", "i64", "i64-weighted"])
@pytest.mark.parametrize("path", [1, 2, 3])
def test_partitioned_paths_split_a_bucket_inflated_by_one_key(K, path, dtype, weighted, hot):
    """One key holds 90 % of 600 k rows beside 50 k other keys: its bucket is a primary chunk plus
    excess chunks whose partial lists part_merge_kernel adds up (with the filter in front the hot
    key is absorbed by the image instead, when the sample shows it twice: it does, 9 rows in 10)."""
    n = 600_000
    rng = np.random.default_rng(seed_of("skew", path, dtype, weighted, hot))
    pool = keyset("scrambled" if dtype == "int32" else "collide", 60_001, dtype)
    big = pool[0]
    keys = np.full(n, big)
    keys[rng.permutation(n)[:60_000]] = pool[1:]          # every other key once
    keys[rng.integers(0, n, 3)] = LO[dtype]
    valid = rng.random(n) >= 0.05
    keys = poison(keys, valid, dtype, rng)
    rows_of_big = int(((keys == big) & valid).sum())
    if hot:   # the sample shows the key far more than twice: it is in the image, its rows are
        #       counted by part_hist_hot_kernel's LDS counters and leave the partition
        seen = np.ones(n, bool)
        seen[unsampled_rows(n)] = False
        assert int(((keys == big) & valid & seen).sum()) > 1000, "the sample must show the frequent key"
    else:
        assert rows_of_big > 4 * chunk_rows(path, n), "the bucket of the frequent key must split"
    assert np.unique(keys[valid]).size >= 50_000
    w = weights_for(keys, rng) if weighted else None
    part(K, path, hot, keys, valid, w, f"{path} {dtype} skewed bucket", hint=70_000)


def test_partitioned_path_scans_a_tile_histogram_of_more_than_one_block(K):
    """Path 1 keeps 256 counters per scatter tile.  Beyond kScanSmallMax = 131 072 counters (512
    tiles) their exclusive scan is scan_chunk_kernel + scan_totals_kernel with the last step left to
    the level-1 scatter, below it one scan_small_kernel launch: 514 tiles, the last one of 3 rows."""
    n = 513 * 8192 + 3
    rng = np.random.default_rng(seed_of("scan", n))
    keys = column("scrambled", n, 20_000, "int32", rng)
    valid = rng.random(n) >= 0.1
    part(K, 1, False, poison(keys, valid, "int32", rng), valid, None, "1 int32 chunked scan")


@pytest.mark.parametrize("bits", [8, 9, 10])
def test_range_path_rounds_and_bucket_counts(K, bits):
    rng = np.random.default_rng(seed_of("range", bits))
    sizes = [1, 255, 257, 8191, 8193, ROUND - 1, ROUND, ROUND + 1] + ([2 * ROUND + 5003] if bits == 10 else [])
    for i, n in enumerate(sizes):
        keys = column(["scrambled", "dense"][i % 2], n, 30_000, "int32", rng)
        valid = [None, rng.random(n) >= 0.1][(i // 2) % 2]
        rng_path(K, bits, poison(keys, valid, "int32", rng), valid, "sizes")


def test_sort_path_tiles(K):
    rng = np.random.default_rng(seed_of("sort"))
    for i, n in enumerate([1, 4095, 4097, 8191, 8192, 8193, 2 * 8192 + 3, 100_003]):
        keys = column("scrambled", n, 5000, "int32", rng)
        if n > 1000:
            keys[100:400] = 77                # a run that crosses nothing, count >= 255
            keys[rng.integers(0, n, 9000 if n > 50_000 else 300)] = -123456   # a run across tile borders
        valid = [None, rng.random(n) >= 0.2][i % 2]
        sort_path(K, poison(keys, valid, "int32", rng), valid, "sizes")


# ---------------------------------------------------------------------------------------------
# validity and key distributions, every family
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_validity_patterns_over_poisoned_rows(K, fam):
    dtype, weighted, run = FAMILIES[fam]
    rng = np.random.default_rng(seed_of("valid", fam))
    for n in (1003, 8197, 70_001):          # (none of them a multiple of 8)
        base = column("scrambled", n, family_keys(fam), dtype, rng)
        for name, valid in patterns(n, rng):
            keys = poison(base, valid, dtype, rng)
            if name in ("no-bitmap", "all-set", "random10"):
                keys[n // 2] = LO[dtype]     # the smallest key under a VALID bit as well
                if valid is not None:
                    valid = valid.copy()
                    valid[n // 2] = True
            run(K, keys, valid, weights_for(keys, rng) if weighted else None, f"{fam} {name}")


DISTS = [("scrambled", "single"), ("scrambled", "distinct"), ("scrambled", "zipf"), ("dense", "uniform"),
         ("stride16", "zipf"), ("stride20", "zipf"), ("collide", "zipf")]


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_key_distributions(K, fam):
    dtype, weighted, run = FAMILIES[fam]
    rng = np.random.default_rng(seed_of("dist", fam))
    n = 50_021
    for dist, shape in DISTS:
        if dist == "collide" and dtype != "int64":
            continue
        m = family_keys(fam)
        if dist.startswith("stride"):
            m = min(m, 300 if fam.startswith("lds") else 2000)   # (j << 20 stays inside int32)
        if shape == "distinct":
            if fam.startswith("lds"):
                continue      # (n distinct keys do not fit an LDS path: the driver tests escalate)
            m = n
        keys = column(dist, n, m, dtype, rng, shape=shape)
        valid = rng.random(n) >= 0.1
        keys = poison(keys, valid, dtype, rng)
        run(K, keys, valid, weights_for(keys, rng) if weighted else None, f"{fam} {dist}/{shape}")


# ---------------------------------------------------------------------------------------------
# range path: the edges of the sampled map
# ---------------------------------------------------------------------------------------------
def unsampled_rows(n):
    """Rows hot_sample_kernel does not read: it takes S = min(nblk, 64) blocks of 1024 rows that
    start (nblk // S) * 1024 rows apart (nblk = ceil(n / 1024))."""
    nblk = (n + 1023) // 1024
    S = min(nblk, 64)
    step = (nblk // S) * 1024
    seen = np.zeros(n, bool)
    for it in range(S):
        seen[it * step: it * step + 1024] = True
    return np.flatnonzero(~seen)


def test_range_path_clamps_keys_outside_the_sampled_range(K):
    n = 200_003
    rng = np.random.default_rng(seed_of("clamp"))
    free = unsampled_rows(n)
    assert free.size > n // 2
    base = (2**24 + rng.integers(0, 2**28, n)).astype(np.int32)     # the sample sees [2^24, 2^24 + 2^28)
    # a handful of keys beyond each end, only in rows the sample does not read
    keys = base.copy()
    rows = rng.permutation(free)[:24]
    outside = np.array([5, 6, 7, -9, -2**31 + 1, 2**24 - 1, 2**31 - 1, 2**31 - 2, 2**30, 2**29, 2**24 + 2**28,
                        2**30 + 3], np.int32)
    keys[rows] = np.tile(outside, 2)
    nblk = (n + 1023) // 1024
    step = (nblk // 64) * 1024
    assert nblk >= 64 and ((rows % step >= 1024) | (rows >= 64 * step)).all(), \
        "the chosen rows must lie outside the sampled blocks"
    for bits in (8, 10):
        res = rng_path(K, bits, keys, None, "a handful of keys beyond both ends", hint=n)
        assert host(res[0])[0] == -2**31 + 1 and host(res[0])[-1] == 2**31 - 1
    # ~5000 distinct keys below the sampled range: more than the 128-slot tail of a bucket or a
    # 512-step probe chain holds -> the range path gives up, the sort path delivers
    keys = base.copy()
    rows = rng.permutation(free)[:15_000]
    keys[rows] = rng.integers(1000, 6000, rows.size).astype(np.int32)
    res, relaunched, job = launch(K, keys, None, None, path=K.PATH_RANGE, hint=n, bits=10)
    assert res[3]["path"] == K.PATH_SORT and res[3]["range_failed"] and relaunched >= 1, res[3]
    assert res[3]["range_fail_bits"] & 1
    check(K, res, keys, None, None, K.PATH_SORT, "5000 keys below the sampled range")


def test_range_path_degenerate_spans(K):
    rng = np.random.default_rng(seed_of("span"))
    n = 70_001
    # the whole int32 range, both ends in sampled row 0 / 1
    keys = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    keys[0], keys[1], keys[2] = LO["int32"], HI["int32"], LO["int32"] + 1
    rng_path(K, 8, keys, None, "full int32 span", hint=n)
    # a span of zero: one key; the same under a bitmap; only the smallest key; only nulls
    one = np.full(n, 123_456, np.int32)
    rng_path(K, 8, one, None, "span 0")
    valid = rng.random(n) >= 0.3
    rng_path(K, 9, poison(one, valid, "int32", rng), valid, "span 0 with nulls")
    rng_path(K, 8, np.full(n, LO["int32"], np.int32), None, "only the smallest key")
    rng_path(K, 8, poison(one, np.zeros(n, bool), "int32", rng), np.zeros(n, bool), "only nulls")
    rng_path(K, 10, np.array([HI["int32"], LO["int32"], 0, -1, HI["int32"]], np.int32), None, "five rows, both ends")


def _finalize(K, tab, counts, max_count, src):
    from nvtabular_amd import _lib

    descs = (_lib.VocabCol * 1)()
    tab.fill_vocab_desc(descs[0], counts, int(max_count), src=src)
    K.check(_lib.load().nvt_vocab_finalize_many(descs, 1, K.stream_ptr()), "nvt_vocab_finalize_many")


def test_range_path_piecewise_map_counts_and_encodes(K):
    """Dense power-law ids: the exact list (sort path) gives the splitters, the column is counted
    again through the piecewise map, and the dumped table encodes through it."""
    n, card, s = 300_000, 200_000, 1.1
    rng = np.random.default_rng(seed_of("pieces"))
    u = rng.random(n)
    keys = np.floor(((card ** (1.0 - s) - 1.0) * u + 1.0) ** (1.0 / (1.0 - s))).clip(1, card).astype(np.int32)
    keys[5] = LO["int32"]
    valid = rng.random(n) >= 0.05
    valid[5] = True
    keys = poison(keys, valid, "int32", rng)
    exact, relaunched, _ = launch(K, keys, valid, None, path=K.PATH_SORT, hint=n)
    assert relaunched == 0
    ek, ec = check(K, exact, keys, valid, None, K.PATH_SORT, "pieces: exact list")
    k, c = exact[0], exact[1]
    assert ek.size > 8192
    pieces = K.range_splitters(k, c, rows=n)
    assert pieces is not None and pieces.numel() == 65
    res = rng_path(K, 8, keys, valid, "piecewise map", hint=ek.size, pieces=pieces)
    dk, dc, _, info = res
    assert info["range_pieces"] is True
    # the dumped table, ordered by nvt_vocab_finalize_many, probed through the same map
    first = 3
    ok, oc = torch.empty_like(dk), torch.empty_like(dc)
    tab = K.EncodeTable(ok, first, unique=True, defer_build=True,
                        range_table=(info["range_table"], info["range_aux"], info["range_bits"]))
    _finalize(K, tab, oc, info["max_count"], (dk, dc, info["cls_hist"], info["n_big"], None))
    tab.wait_ready()
    vk, vc = R.vocab_order_ref(ek, ec)
    ER.first_mismatch(host(tab._vk), vk, "pieces: vocabulary order")
    unseen = np.array([0, -7, card + 5, 2**31 - 1, -2**31 + 1], np.int32)
    for what, rows, rv in (("own rows", keys, valid), ("vocabulary", vk, None), ("unseen", unseen, None)):
        for out in (torch.int64, torch.int32):
            got = tab.encode(dev(rows), None if rv is None else dev(R.pack_bits(rv)), 1, 2, 0, out)
            exp = ER.encode_ref(rows, rv, vk, first, 1, 2, 0, np.int64 if out == torch.int64 else np.int32)
            ER.first_mismatch(host(got), exp, f"pieces: encode {what}")


# ---------------------------------------------------------------------------------------------
# driver transitions
# ---------------------------------------------------------------------------------------------
def test_driver_escalates_from_a_hint_far_too_small(K):
    """Stage 1 of the LDS paths holds whatever a slab of n / 256 rows shows; it is stage 2 that
    gives up, at more than 384 keys per (class, range) table: 253 k keys are ~990 per table on
    paths 6 / 0 and ~495 on path 7."""
    rng = np.random.default_rng(seed_of("hint1"))
    n = 400_001
    for dtype, weighted, end in (("int32", False, K.PATH_RANGE), ("int64", False, 1), ("int32", True, 1)):
        keys = column("scrambled" if dtype == "int32" else "collide", n, 400_000, dtype, rng, shape="uniform")
        assert np.unique(keys).size > 230_000
        w = weights_for(keys, rng) if weighted else None
        res, relaunched, job = launch(K, keys, None, w, hint=1)
        # 6 -> 0 -> (int32, no weights: the range path | otherwise 7 -> 1)
        assert res[3]["path"] == end and relaunched == (2 if end == K.PATH_RANGE else 3), (dtype, weighted, res[3], relaunched)
        check(K, res, keys, None, w, end, f"hint 1, {dtype} weighted={weighted}")
    # 78 k distinct keys in 150 k rows (586 rows per slab, ~300 keys per range table) FIT path 6:
    # only the output list, sized for the hint, has to grow (observed: path 6, one relaunch)
    keys = column("scrambled", 150_001, 100_000, "int32", rng, shape="uniform")
    assert 65_536 < np.unique(keys).size < 90_000
    res, relaunched, job = launch(K, keys, None, None, hint=1)
    assert res[3]["path"] == 6 and relaunched == 1 and job.cap_guess == 1 << 20, (res[3], relaunched)
    check(K, res, keys, None, None, 6, "hint 1, 78 k keys in short slabs")


def test_driver_hints_too_large_zero_and_no_range(K):
    rng = np.random.default_rng(seed_of("hints"))
    n = 100_003
    keys = column("scrambled", n, 1000, "int32", rng)
    valid = rng.random(n) >= 0.1
    keys = poison(keys, valid, "int32", rng)
    k64 = keys.astype(np.int64)
    # far too large: int32 -> beyond the range path's limit = the sort path; int64 -> path 3
    sampled = K.STATS["presampled_columns"]
    for kk, hint, end in ((keys, 50_000_000, K.PATH_SORT), (k64, 50_000_000, 3), (keys, 3_000_000, K.PATH_RANGE),
                          (keys, 0, 0), (k64, 0, 0)):
        res, relaunched, job = launch(K, kk, valid, None, hint=hint)
        assert relaunched == 0 and res[3]["path"] == end, (hint, res[3])
        check(K, res, kk, valid, None, end, f"hint {hint}")
    assert n < K.SAMPLE_MIN_ROWS and K.STATS["presampled_columns"] == sampled   # hint 0, no prefix sketch
    # allow_range=False: a column the range path gave up on before goes to the sort path
    res, relaunched, job = launch(K, keys, valid, None, hint=100_000, allow_range=False)
    assert relaunched == 0 and res[3]["path"] == K.PATH_SORT
    check(K, res, keys, valid, None, K.PATH_SORT, "allow_range=False")
    # LDS overflow -> range path: 253 k keys on path 0 (~990 per range table of stage 2, 384 fit)
    wide = column("scrambled", 400_001, 400_000, "int32", rng, shape="uniform")
    assert np.unique(wide).size > 230_000
    res, relaunched, job = launch(K, wide, None, None, path=0, hint=5000)
    assert relaunched == 1 and res[3]["path"] == K.PATH_RANGE, res[3]
    check(K, res, wide, None, None, K.PATH_RANGE, "path 0 overflow -> range")
    # ... and with weights (no range path): 0 -> 7 -> 1
    w = weights_for(wide, rng)
    res, relaunched, job = launch(K, wide, None, w, path=0, hint=5000)
    assert relaunched == 2 and res[3]["path"] == 1, res[3]
    check(K, res, wide, None, w, 1, "weighted path 0 overflow -> 7 -> 1")


def test_driver_regrows_an_output_list_that_is_too_small(K):
    rng = np.random.default_rng(seed_of("cap"))
    n = 70_001
    keys = column("scrambled", n, 5000, "int32", rng, shape="uniform")
    distinct = np.unique(keys).size
    assert distinct > 4000
    # hash path: overflow bit 1 without a size -> 4 x / 2^20
    res, relaunched, job = launch(K, keys, None, None, path=1, hint=5000, hot=False, cap=100)
    assert relaunched == 1 and res[3]["path"] == 1 and job.cap_guess == 1 << 20
    check(K, res, keys, None, None, 1, "path 1, list of 100")
    # range and sort paths: state[NVT_ST_NEED] says how many entries the list needs
    for path in (K.PATH_RANGE, K.PATH_SORT):
        res, relaunched, job = launch(K, keys, None, None, path=path, hint=5000, cap=100)
        assert relaunched == 1 and res[3]["path"] == path, res[3]
        assert distinct <= job.cap_guess <= distinct + 64, (job.cap_guess, distinct)
        check(K, res, keys, None, None, path, f"path {path}, list of 100")


def test_range_overflow_below_1024_buckets_relaunches_at_1024(K):
    """More keys than 256 buckets hold (12288 each at most): NVT_OVF_FULL -> all 1024 buckets."""
    n = 3_600_000
    rng = np.random.default_rng(seed_of("full"))
    keys = rng.integers(0, 2**31 - 1, n).astype(np.int32)
    res, relaunched, job = launch(K, keys, None, None, path=K.PATH_RANGE, hint=20_000, bits=8)
    assert res[3]["path"] == K.PATH_RANGE and relaunched == 1, res[3]
    assert res[3]["range_bits"] == 10 and res[3]["range_bits_floor"] == 10
    check(K, res, keys, None, None, K.PATH_RANGE, "256 buckets -> 1024")


def test_global_tables_regrow_update_merge_compact(K):
    from nvtabular_amd import _lib

    rng = np.random.default_rng(seed_of("table"))
    n = 150_001
    for dtype in ("int32", "int64"):
        a = column("scrambled" if dtype == "int32" else "collide", n, 100_000, dtype, rng, shape="uniform")
        b = column("scrambled" if dtype == "int32" else "collide", n // 2, 100_000, dtype, rng, shape="uniform")
        va, vb = rng.random(a.size) >= 0.1, None
        a = poison(a, va, dtype, rng)
        a[7], b[9] = LO[dtype], LO[dtype]
        va[7] = True
        # the first table (2^16 slots for a hint of 1) overflows; the loop regrows and recounts
        tab, st = K.count_into_new_table([dev(a)], [dev(R.pack_bits(va))], hint=1)
        assert tab.capacity > K.MIN_COUNT_CAPACITY and not st[_lib.ST_OVERFLOW]
        ek, ec, en = R.count_ref(a, va)
        assert st[_lib.ST_NULLS] == en and st[_lib.ST_OCCUPIED] == ek.size - 1 and st[_lib.ST_SENTINEL] == ec[0]
        # a second partition into the same table, then a weighted list, then compact
        tab.update(dev(b), None)
        lk = column("scrambled", 5000, 5000, dtype, rng, shape="distinct", extremes=False)
        lk[0] = LO[dtype]
        # (int32 tables keep uint32 counts, include/nvt_hip.h: sums beyond 2^32 need an int64 table)
        lc = weights_for(lk, rng) if dtype == "int64" else rng.integers(1, 1000, lk.size).astype(np.int64)
        tab.merge(dev(lk), dev(lc))
        k, c = tab.compact()
        xk, xc = R.merge_ref([R.count_ref(a, va)[:2], R.count_ref(b, None)[:2], (lk, lc)])
        hk, hc = host(k), host(c)
        o = np.argsort(hk, kind="stable")
        assert np.unique(hk).size == hk.size and hk.dtype == NP[dtype]
        R.list_mismatch(hk[o], hc[o], xk.astype(NP[dtype]), xc, f"CountTable {dtype}")
        assert (dtype == "int32" or (xc >= 2**32).any()) and xk[0] == LO[dtype]
        assert not tab.read_state()[_lib.ST_OVERFLOW]


# ---------------------------------------------------------------------------------------------
# batches: streams, workspaces, the sample batch of 32
# ---------------------------------------------------------------------------------------------
def batch_columns():
    """48 columns of ~70 k rows: 37 that need a hot-key sample (range path / filtered paths: the
    sample batch of kHotBatch = 32 flushes twice), LDS-resident, int64, weighted, empty, one row."""
    rng = np.random.default_rng(seed_of("batch"))
    cols = []
    for i in range(48):
        n = 70_000 + 37 * i
        kind = (["range"] * 3 + ["hot1", "lds0", "range", "hot2", "range", "i64", "range", "weighted"])[i % 11]
        if i == 20:
            n, kind = 0, "lds0"
        if i == 21:
            n, kind = 1, "range"
        if i == 43:
            kind = "range"
        dtype = "int64" if kind == "i64" else "int32"
        m = 3000 if kind in ("lds0", "i64", "weighted") else 20_000
        keys = column("scrambled", n, m, dtype, rng)
        valid = rng.random(n) >= 0.1 if i % 3 else None
        keys = poison(keys, valid, dtype, rng)
        w = weights_for(keys, rng) if kind == "weighted" else None
        cols.append((kind, keys, valid, w))
    return cols


def batch_job(K, col):
    kind, keys, valid, w = col
    job = K.DenseCountJob(dev(keys), None if valid is None else dev(R.pack_bits(valid)), dev(w),
                          hint={"range": 20_000, "hot1": 20_000, "hot2": 20_000}.get(kind, 3000))
    job.path = {"range": K.PATH_RANGE, "hot1": 1, "hot2": 2, "lds0": 0, "i64": 0, "weighted": 7}[kind]
    job.hot = kind in ("hot1", "hot2")
    return job


def as_host(K, res):
    k, c, nulls, info = res
    hk, hc = host(k), host(c)
    if info["path"] not in (K.PATH_RANGE, K.PATH_SORT):
        o = np.argsort(hk, kind="stable")
        hk, hc = hk[o], hc[o]
    hist = host(info["cls_hist"]).astype(np.int64) & 0xFFFFFFFF if "cls_hist" in info else None
    return hk, hc, nulls, {x: info.get(x) for x in ("path", "distinct", "max_count", "rows", "n_big")}, hist


@pytest.fixture(scope="module")
def alone(K):
    """(columns, every column counted ALONE and checked against count_ref): computed once."""
    cols = batch_columns()
    want = {"range": K.PATH_RANGE, "hot1": 1, "hot2": 2, "lds0": 0, "i64": 0, "weighted": 7}
    out = []
    for i, col in enumerate(cols):
        before = K.STATS["count_relaunches"]
        res = K.dense_count_many([batch_job(K, col)])[0]
        assert K.STATS["count_relaunches"] == before
        check(K, res, col[1], col[2], col[3], want[col[0]], f"batch column {i} ({col[0]}) alone")
        out.append(as_host(K, res))
    return cols, out


@pytest.mark.parametrize("streams,head_start", [(1, True), (3, True), (3, False)])
def test_batch_of_48_columns_equals_every_column_alone(K, alone, monkeypatch, streams, head_start):
    cols, _ALONE = alone
    sampled = sum(1 for kind, keys, _, _ in cols if kind in ("range", "hot1", "hot2") and keys.size)
    assert sampled >= 34 and len(cols) >= 40
    monkeypatch.setattr(K, "COUNT_STREAMS", streams)
    monkeypatch.setattr(K, "HEAD_START", head_start)
    before = K.STATS["count_relaunches"]
    results = K.dense_count_many([batch_job(K, col) for col in cols])
    assert K.STATS["count_relaunches"] == before and len(results) == len(cols)
    for i, (col, res) in enumerate(zip(cols, results)):
        what = f"batch column {i} ({col[0]}, rows={col[1].size}) streams={streams} head_start={head_start}"
        hk, hc, nulls, info, hist = as_host(K, res)
        ak, ac, anulls, ainfo, ahist = _ALONE[i]
        R.list_mismatch(hk, hc, ak, ac, what)
        assert nulls == anulls and info == ainfo, f"{what}: {nulls} {info}, alone {anulls} {ainfo}"
        if ahist is not None:
            ER.first_mismatch(hist, ahist, what + ": cls_hist")


def test_merge_dense_and_merge_dense_many(K):
    rng = np.random.default_rng(seed_of("merge"))

    def lists_of(dtype, nlists, m, hi=1000):
        out = []
        for _ in range(nlists):
            k = rng.permutation(keyset("scrambled" if dtype == "int32" else "collide", m, dtype))[: m * 2 // 3]
            k[0] = LO[dtype]
            c = rng.integers(1, hi, k.size).astype(np.int64)
            c[:3] = [2**40, 2**33 + 1, 2**32 - 1]
            out.append((k, c))
        return out

    groups = [lists_of("int32", 3, 4000), lists_of("int64", 4, 3000), lists_of("int32", 1, 500), [],
              lists_of("int32", 5, 40_000), lists_of("int32", 2, 40)]
    dgroups = [[(dev(k), dev(c)) for k, c in g] for g in groups]
    got = K.merge_dense_many(dgroups)
    assert len(got) == len(groups) and got[3] is None
    for j, (g, r) in enumerate(zip(groups, got)):
        if not g:
            continue
        xk, xc = R.merge_ref(g)
        hk, hc = host(r[0]), host(r[1])
        o = np.argsort(hk, kind="stable")
        assert np.unique(hk).size == hk.size
        R.list_mismatch(hk[o], hc[o], xk, xc, f"merge_dense_many group {j}")
        assert len(g) == 1 or (r[2] == int(xc.max()) and r[2] >= 2**40)
    # merge_dense: one group; the int32 + int64 mix widens to int64
    mixed = [(groups[0][0][0], groups[0][0][1]), (groups[1][0][0], groups[1][0][1])]
    k, c, mx = K.merge_dense([(dev(a), dev(b)) for a, b in mixed])
    xk, xc = R.merge_ref(mixed)
    hk, hc = host(k), host(c)
    o = np.argsort(hk, kind="stable")
    assert hk.dtype == np.int64 and np.unique(hk).size == hk.size
    R.list_mismatch(hk[o], hc[o], xk, xc, "merge_dense int32 + int64")
    assert mx == int(xc.max())
    assert K.merge_dense([]) is None
