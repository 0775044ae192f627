"""Kernel-level matrix for Categorify's encode step (nvtabular_amd/csrc/nvt_encode.hip with its
kernel headers nvt_encode_head.hpp / nvt_encode_pipe.hpp, nvt_encode_build.hip, nvt_hash_bucket.hip):
``K.EncodeTable``, ``K.encode_many`` and ``K.hash_bucket`` called directly on torch tensors, every
label compared with the numpy references of encode_reference.py (which test_encode_reference.py
pins to the pandas oracle on the CPU).  Nothing is approximate here: every comparison is exact.

One helper per way of obtaining a table, so that every launch shape of ``encode_launch`` is reached
on purpose, and every helper asserts the kind of table it got -- ``tab.kind`` (kernels_encode.py:
``encode_kind``) and the attributes that kind stands for (a silent fallback would turn a test into
a second copy of the generic-kernel test).  The launch shapes are named by
``K.encode_launch_shape``:

    hashed       EncodeTable(vk, first)                       encode_kernel<K, OUT>
    resident     EncodeTable(vk, first, unique=True), small   encode_small_kernel<2048 / 4096> (int32 keys,
                                                              int64 labels, <= 1024 / <= 2048 keys), else
                                                              encode_hot_kernel<.., GLOBAL=false>
    cache_eager  the same, int32 keys > 8192                  cache mode, head built per launch
    i64_linear   the same, int64 keys > 6144                  encode_hot_kernel<int64, .., GLOBAL=true>
    cache_image  defer_build, ordered by nvt_vocab_finalize_many   cache mode, prebuilt head image
    flat         flat=True, key-sorted source                 encode_pipe_kernel<OUT, 2>
    dumped       DenseCountJob on the range path, its table   encode_pipe_kernel<OUT, 1>

Sizes.  stream_grid caps a grid at 256 CUs x blocks_per_cu.  The 1024-thread kernels (hot, cache,
pipe) run 256 workgroups whose lanes take U = 2 vectors of VEC keys a step: one workgroup step is
1024 * 2 * 4 = 8192 int32 rows, one trip of the full grid 2 097 152 int32 rows (1 048 576 int64
rows): TRIP.  encode_kernel and encode_small_kernel size their grids for TWICE the rows a block
takes per trip (stream_grid(n / VEC + 1, kBlock * 2, 8): a block of 256 lanes takes 256 vectors;
stream_grid(n / 2 + 1, kBlock * 8, 8): a block takes 4 waves * 4 runs of 128 rows = 2048 rows, not
4096), so they make a second grid-stride trip at ANY size beyond one block's step, from a few
thousand rows on; their grids reach the cap of 2048 blocks at 2 * TRIP and 2 * SMALL_TRIP rows.
For these two kernels TRIP / SMALL_TRIP are simply large sizes with several trips that end in a
partial vector block and a scalar tail, not trip boundaries.  The pipelined kernel has
three code paths -- the loop over the FULL steps of a workgroup, the vectors behind its last full
step, the rows behind the last vector: 2 097 152 rows are full steps alone, 4097 rows the other
two alone, 2 * 2 097 152 + 4 * 5 + 3 all three with a second full step.

Left out, by name: NVT_ENC_STATS counting; src_labels (multi-GPU labelled shards, test_gpu_merge_sorted.py);
the piecewise range map (test_gpu_range_path.py reaches it through the workflow).
"""
import zlib

import numpy as np
import pytest
import torch

import encode_reference as R

pytestmark = pytest.mark.gpu

NP = {"int32": np.int32, "int64": np.int64}
TT = {"int32": torch.int32, "int64": torch.int64}
LO = {"int32": np.iinfo(np.int32).min, "int64": np.iinfo(np.int64).min}
HEAD16 = 21504            # kHead16Keys: keys of the 6-byte LDS head
RES = {"int32": 8192, "int64": 6144}   # NVT_ENCODE_RESIDENT_*
TRIP = {"int32": 2_097_152, "int64": 1_048_576}
SMALL_TRIP = 4_194_304

SMALL_SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 129, 255, 257, 1023, 1025, 2047, 2049, 4095, 4097]
# under / over one workgroup step, one full step of workgroup 0 alone, that + leftover vectors + tail
MEDIUM_SIZES = [8185, 8191, 8193, 8199, 12288, 12288 + 4 * 1024 + 7, 100_003]
KINDS = ["hashed", "hashed64", "resident", "resident64", "cache_eager", "i64_linear", "cache_image", "flat",
         "dumped"]
KEY_DTYPE = {"hashed64": "int64", "resident64": "int64", "i64_linear": "int64"}
TABLE_KIND = {"hashed": "generic", "hashed64": "generic", "resident": "resident", "resident64": "resident",
              "cache_eager": "cache", "cache_image": "cache", "i64_linear": "linear64", "flat": "flat",
              "dumped": "dumped"}     # EncodeTable.kind of each of KINDS


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


_TABLES = {}   # filled through table(), emptied by the fixture below when the file is done


@pytest.fixture(scope="module", autouse=True)
def _free_tables():
    yield
    _TABLES.clear()
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# vocabularies
# ---------------------------------------------------------------------------------------------
def keyset(dist, n, dtype, rng):
    """n distinct keys, none of them the smallest integer of the type."""
    if n <= 0:
        return np.empty(0, NP[dtype])
    if dist == "scrambled":      # spread over [0, 2^31): x -> a x + b mod 2^31 is a bijection (a odd)
        k = (np.arange(1, n + 1, dtype=np.int64) * 2654435761 + 12345) % (2**31)
    elif dist == "dense":
        k = np.arange(n, dtype=np.int64)
    elif dist == "fullrange":    # the whole int32 range, its largest value, -1 and 0 among them
        k = np.unique(rng.integers(-2**31 + 1, 2**31 - 1, int(n * 1.1) + 16))
        k = np.setdiff1d(k, [2**31 - 1, -1, 0])
        k = np.concatenate([[2**31 - 1, -1, 0][:min(3, n)], rng.permutation(k)[:max(0, n - 3)]])
    elif dist == "collide":      # int64: five low words, the rest of the key above bit 32, both signs
        j = np.arange(n, dtype=np.int64)
        k = (j % 5) + ((j // 5 - n // 10) << 32)
    elif dist == "clustered":    # consecutive ids and a few far outliers: long runs in a flat table
        far = np.array([2**31 - 1, 2**31 - 77, 2**30 + 5, -2**30, -5], dtype=np.int64)[:min(5, n)]
        k = np.concatenate([1000 + np.arange(n - far.size, dtype=np.int64), far])
    else:
        raise AssertionError(dist)
    assert k.size == n and np.unique(k).size == n
    if dist != "dense" and dist != "clustered":
        k = rng.permutation(k)
    return k.astype(NP[dtype])


def place_sentinel(keys, where, lo):
    """The vocabulary order for the tables built from an explicitly ordered vocabulary."""
    n = keys.size + 1
    at = {"first": 0, "last": n - 1, "head": min(100, (n - 1) // 2),
          "beyond": n - 10 if n > HEAD16 + 100 else n - 1}[where]
    return np.insert(keys, at, lo)


def counts_for(keys, where, lo, rng):
    """Counts that put the smallest key where `where` says in the (count desc, key asc) order."""
    c = 1 + np.minimum(rng.zipf(2.0, keys.size), 400).astype(np.int64)    # 2 .. 401, many ties
    if where != "absent":
        keys = np.append(keys, np.array([lo], dtype=keys.dtype))
        c = np.append(c, {"first": 500, "last": 1, "head": 300, "beyond": 2}[where])
    return keys, c


class Tab:
    def __init__(self, kind, tab, vk, first, dtype, verify=None, info=None):
        self.kind, self.tab, self.vk, self.first, self.dtype = kind, tab, vk, int(first), dtype
        self.lo, self.info, self.verify = LO[dtype], info, verify or (lambda: None)

    def shape(self, out_dtype):
        """The launch shape encode_launch picks for this table (for messages and assertions)."""
        from nvtabular_amd import kernels as K

        t = self.tab
        return K.encode_launch_shape(t.kind, t.key_bytes, np.dtype(out_dtype).itemsize, t.n_vocab,
                                     t.head_image is not None)

    def describe(self, out_dtype):
        return f"{self.kind} [{self.shape(out_dtype)}] {self.dtype} keys n_vocab={self.vk.size} first={self.first}"


def _finalize(K, tab, counts, max_count, src=None):
    from nvtabular_amd import _lib

    descs = (_lib.VocabCol * 1)()
    tab.fill_vocab_desc(descs[0], counts, int(max_count), src=src)
    K.check(_lib.load().nvt_vocab_finalize_many(descs, 1, K.stream_ptr()), "nvt_vocab_finalize_many")


def build(K, kind, n_vocab, first=3, sentinel="head", dist=None, seed=0, verify=True):
    """One table of `kind` with exactly n_vocab keys; asserts that it IS of that kind."""
    dtype = KEY_DTYPE.get(kind, "int32")
    lo = LO[dtype]
    rng = np.random.default_rng(seed_of(kind, n_vocab, first, sentinel, dist, seed))
    dist = dist or ("collide" if dtype == "int64" else "scrambled")
    keys = keyset(dist, n_vocab - (sentinel != "absent"), dtype, rng)
    if kind in ("hashed", "hashed64", "resident", "resident64", "cache_eager", "i64_linear"):
        vk = keys if sentinel == "absent" else place_sentinel(keys, sentinel, lo)
        unique = not kind.startswith("hashed")
        tab = K.EncodeTable(dev(vk), first, unique=unique)
        assert tab.kind == TABLE_KIND[kind]
        if not unique:
            assert tab.table is not None and tab.vocab_keys is None and tab.range_aux is None
            assert tab.capacity == K.next_pow2(max(64, (4 if n_vocab <= (1 << 20) else 2) * n_vocab + 1))
        elif kind.startswith("resident"):
            assert 0 < n_vocab <= RES[dtype] and tab.table is None and tab.vocab_keys is not None
        else:
            assert n_vocab > RES[dtype] and tab.table is not None and tab.vocab_keys is not None
            assert tab.head_image is None and tab.range_aux is None and tab.flat_slots == 0
        return Tab(kind, tab, vk, first, dtype)
    assert n_vocab > RES["int32"], "the tables ordered by nvt_vocab_finalize_many are tested in cache mode"
    keys, counts = counts_for(keys, sentinel, lo, rng)
    assert keys.dtype == NP[dtype] and counts.dtype == np.int64
    order = np.lexsort((keys, -counts))            # count descending, key ascending
    vk = keys[order]
    info = None
    if kind == "cache_image":
        p = rng.permutation(keys.size)
        dk, dc = dev(keys[p]), dev(counts[p])
        tab = K.EncodeTable(dk, first, unique=True, defer_build=True)
        _finalize(K, tab, dc, counts.max())
        assert tab.head_image is not None and tab.table is not None and tab.range_aux is None
        assert tab.flat_slots == 0 and tab.capacity >= 2 * n_vocab
    elif kind == "flat":
        s = np.argsort(keys, kind="stable")
        dk, dc = dev(keys[s]), dev(counts[s])
        ok, oc = torch.empty_like(dk), torch.empty_like(dc)
        tab = K.EncodeTable(ok, first, unique=True, defer_build=True, range_table=None, flat=True)
        _finalize(K, tab, oc, counts.max(), src=(dk, dc, K.class_hist(dc), int((counts >= 255).sum()), None))
        assert tab.flat_slots > 0 and tab.range_aux is not None and tab.range_bits == 0
        assert tab.capacity == tab.flat_slots + n_vocab + 64 and tab.head_image is not None
    else:
        assert kind == "dumped"
        rows = rng.permutation(np.repeat(keys, counts))
        job = K.DenseCountJob(dev(rows), None, None, hint=n_vocab)
        job.path = K.PATH_RANGE
        dk, dc, nulls, info = K.dense_count_many([job])[0]
        assert info["path"] == K.PATH_RANGE and not info.get("range_failed"), info
        assert info["range_table"] is not None and info["range_bits"] >= 8 and nulls == 0
        assert int(dk.numel()) == n_vocab and info["max_count"] == int(counts.max())
        ok, oc = torch.empty_like(dk), torch.empty_like(dc)
        tab = K.EncodeTable(ok, first, unique=True, defer_build=True,
                            range_table=(info["range_table"], info["range_aux"], info["range_bits"]))
        _finalize(K, tab, oc, info["max_count"], src=(dk, dc, info["cls_hist"], info["n_big"], None))
        assert tab.range_bits == info["range_bits"] and tab.capacity == 0 and tab.flat_slots == 0
        assert tab.range_aux is not None and tab.table is info["range_table"] and tab.head_image is not None

    assert tab.kind == TABLE_KIND[kind]

    def check_vocab():
        tab.wait_ready()
        R.first_mismatch(host(tab._vk), vk, f"{kind} n_vocab={n_vocab}: vocabulary order")

    if verify:
        check_vocab()
    return Tab(kind, tab, vk, first, dtype, verify=check_vocab, info=info)


def table(K, kind, n_vocab, first=3, sentinel="head", dist=None):
    key = (kind, n_vocab, first, sentinel, dist)
    if key not in _TABLES:
        _TABLES[key] = build(K, kind, n_vocab, first, sentinel, dist)
    return _TABLES[key]


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
def make_rows(T, n, rng):
    """Half zipf over the vocabulary order (the head of the vocabulary), half uniform over all of
    it, ~2 % keys that are not in it, and the smallest key of the type in a few rows."""
    vk, dtype = T.vk, T.dtype
    if n == 0:
        return np.empty(0, NP[dtype])
    nv = vk.size
    pos = np.where(rng.random(n) < 0.5, np.minimum(rng.zipf(1.2, n) - 1, nv - 1), rng.integers(0, nv, n))
    keys = vk[pos].copy()
    un = np.flatnonzero(rng.random(n) < 0.02)
    if dtype == "int32":
        keys[un] = rng.integers(-2**31, 2**31 - 1, un.size).astype(np.int32)
    else:   # the low word of a vocabulary key under another high word, and anything
        keys[un] = np.where(rng.random(un.size) < 0.5, vk[rng.integers(0, nv, un.size)] + (np.int64(977) << 32),
                            rng.integers(-2**63, 2**63 - 1, un.size))
    if n >= 4:
        keys[rng.integers(0, n, max(1, n // 500))] = T.lo
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


def poison(T, keys, valid, rng):
    """Bytes under the null rows: keys that ARE in the vocabulary, the smallest key, random keys."""
    if valid is None or valid.all():
        return keys
    keys = keys.copy()
    idx = np.flatnonzero(~valid)
    keys[idx[0::3]] = T.vk[rng.integers(0, T.vk.size, idx[0::3].size)]
    keys[idx[1::3]] = T.lo
    i = np.iinfo(NP[T.dtype])
    keys[idx[2::3]] = rng.integers(i.min, i.max, idx[2::3].size).astype(NP[T.dtype])
    return keys


def labels_for(T, variant=0):
    """(null_label, oov_label): distinct from every vocabulary label."""
    if variant == 0 and T.first >= 3:
        return 1, 2
    return T.first + T.vk.size + 10, T.first + T.vk.size + 20


def check(K, T, keys, valid, out_dtype, nb=0, what="", labels=None, need_mix=False):
    null_label, oov_label = labels or labels_for(T)
    dv = None if valid is None else dev(R.pack_bits(valid))
    got = T.tab.encode(dev(keys), dv, null_label, oov_label, nb, TT[out_dtype])
    exp = R.encode_ref(keys, valid, T.vk, T.first, null_label, oov_label, nb, NP[out_dtype])
    msg = f"{T.describe(out_dtype)} -> {out_dtype} rows={keys.size} nb={nb} {what}"
    R.first_mismatch(host(got), exp, msg)
    if need_mix:   # the case really has head hits, table hits, unseen keys and the smallest key
        ok = np.ones(keys.size, bool) if valid is None else valid
        at = np.full(keys.size, -1, np.int64)
        hit = R.found_mask(keys, valid, T.vk)
        at[hit] = exp[hit].astype(np.int64) - T.first
        head = HEAD16 if (T.dtype == "int32" and T.vk.size > RES["int32"]) else 2048
        assert (hit & (at < min(head, T.vk.size))).any(), msg + ": no head hit"
        assert T.vk.size <= head or (at >= head).any(), msg + ": no hit beyond the head"
        assert (ok & ~hit).any(), msg + ": no unseen key"
        assert (ok & (keys == T.lo)).any(), msg + ": smallest key not among the valid rows"


def sweep(K, T, sizes, out_dtype, seed, pats=None, nb=0, need_mix=False):
    rng = np.random.default_rng(seed)
    for n in sizes:
        base = make_rows(T, n, rng)
        for name, valid in patterns(n, rng):
            if pats is not None and name not in pats:
                continue
            check(K, T, poison(T, base, valid, rng), valid, out_dtype, nb, name,
                  need_mix=need_mix and name in ("no-bitmap", "random10") and n >= 100_000)


MID_VOCAB = {"hashed": 30_011, "hashed64": 9_001, "resident": 5_000, "resident64": 3_001, "cache_eager": 65_537,
             "i64_linear": 40_003, "cache_image": 65_537, "flat": 65_537, "dumped": 65_537}


# ---------------------------------------------------------------------------------------------
# every table kind x row counts x validity patterns x label width
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", ["int64", "int32"])
@pytest.mark.parametrize("kind", KINDS + ["small2048", "small4096"])
def test_row_counts_and_validity(K, kind, out_dtype):
    small = {"small2048": 1000, "small4096": 2000}.get(kind)
    T = table(K, "resident", small) if small else table(K, kind, MID_VOCAB[kind])
    if small:
        assert (T.shape(out_dtype) == f"encode_{kind[:5]}_kernel<{kind[5:]}>") == (out_dtype == "int64")
    s = seed_of(kind, out_dtype)
    sweep(K, T, SMALL_SIZES, out_dtype, s, nb=7)
    sweep(K, T, MEDIUM_SIZES, out_dtype, s + 1, pats=("no-bitmap", "alternating", "random10"), nb=0, need_mix=True)


BIG = {   # under / over one full grid of steps, and a second trip that ends in leftover vectors and a tail
    "hashed": [TRIP["int32"] - 3, TRIP["int32"] + 4 * 5 + 3],
    "hashed64": [TRIP["int64"] - 3, TRIP["int64"] + 2 * 5 + 1],
    "small2048": [SMALL_TRIP - 3, SMALL_TRIP + 128 + 3],
    "small4096": [SMALL_TRIP + 128 * 5 + 77],
    "resident": [TRIP["int32"] - 3, TRIP["int32"] + 4 * 5 + 3],
    "resident64": [TRIP["int64"] + 2 * 5 + 1],
    "cache_eager": [TRIP["int32"] - 3, TRIP["int32"] + 4 * 5 + 3],
    "i64_linear": [TRIP["int64"] - 3, TRIP["int64"] + 2 * 5 + 1],
    "cache_image": [TRIP["int32"] + 4 * 5 + 3],
    # the pipelined kernel: full steps alone; + tail; + leftover vectors, no tail; all three in a second trip
    # 5 999 999 rows: 184 of the 256 workgroups have THREE full steps (48 batches for 16 waves), so their
    # waves reach the steady state of the pipeline (the ping-pong loop behind its two-batch prologue)
    "flat": [TRIP["int32"], TRIP["int32"] + 3, TRIP["int32"] + 4 * 1029, 2 * TRIP["int32"] + 4 * 5 + 3, 5_999_999],
    "dumped": [TRIP["int32"], TRIP["int32"] - 3, TRIP["int32"] + 4 * 1029 + 1, 2 * TRIP["int32"] + 4 * 5 + 3,
               5_999_999],
}


@pytest.mark.parametrize("out_dtype", ["int64", "int32"])
@pytest.mark.parametrize("kind", list(BIG))
def test_full_grid_and_second_trip(K, kind, out_dtype):
    small = {"small2048": 1000, "small4096": 2000}.get(kind)
    T = table(K, "resident", small) if small else table(K, kind, MID_VOCAB[kind])
    if small and out_dtype == "int64":
        assert T.shape(out_dtype).startswith("encode_small_kernel")
    assert max(BIG[kind]) <= 6_000_000
    sweep(K, T, BIG[kind], out_dtype, seed_of(kind, out_dtype, "big"), pats=("no-bitmap", "random10"), need_mix=True)


# ---------------------------------------------------------------------------------------------
# vocabulary sizes on both sides of every constant of encode_launch
# ---------------------------------------------------------------------------------------------
VOCAB_CASES = (
    [("resident", n) for n in (1, 2, 3, 1024, 1025, 2048, 2049, 8192)]
    + [("cache_eager", n) for n in (8193, HEAD16, HEAD16 + 1, 65_535, 65_537, (1 << 20) + 4097)]
    + [("resident64", n) for n in (1, 2, 3, 2049, 6144)] + [("i64_linear", n) for n in (6145, 65_537)]
    + [("hashed", n) for n in (1, 2, 3, 1025, 8193, 65_537, 1 << 20, (1 << 20) + 1)]
    + [("hashed64", n) for n in (1, 3, 6145, (1 << 20) + 1)]
    + [(k, n) for k in ("cache_image", "flat", "dumped") for n in (8193, HEAD16, HEAD16 + 1, 65_535, 65_537)]
)


@pytest.mark.parametrize("kind,n_vocab", VOCAB_CASES, ids=lambda v: str(v))
def test_vocabulary_sizes(K, kind, n_vocab):
    where = ["first", "last", "absent"][seed_of(kind, n_vocab) % 3] if n_vocab > 1 else "absent"
    T = build(K, kind, n_vocab, sentinel=where)
    expect = {1024: "encode_small_kernel<2048>", 1025: "encode_small_kernel<4096>", 2048: "encode_small_kernel<4096>",
              2049: "encode_hot_kernel<GLOBAL=false>", 8192: "encode_hot_kernel<GLOBAL=false>"}
    if kind == "resident" and n_vocab in expect:
        assert T.shape("int64") == expect[n_vocab] and T.shape("int32") == "encode_hot_kernel<GLOBAL=false>"
    for out_dtype in ("int64", "int32"):
        sweep(K, T, [20_011], out_dtype, seed_of(kind, n_vocab, out_dtype), pats=("no-bitmap", "random10"), nb=7)
        sweep(K, T, [4097, 9], out_dtype, seed_of(kind, n_vocab, out_dtype, 1), pats=("byte-runs",), nb=0)


@pytest.mark.parametrize("kind", ["flat", "dumped", "labels"])
def test_ordering_workspace_at_two_tiles(K, kind, monkeypatch):
    """The ordering workspace (order_ws, csrc/nvt_vocab_order.hip) at its smallest shape with every block
    in use: 4097 key-sorted entries = two tiles, a class-255 tail of several entries, and a table built
    from label_of[] -- flat and dumped through vocab_order_sorted_batch, flat through vocab_from_labels
    ("labels").  EncodeTable keeps a vocabulary this small in LDS, so its gate is lifted while the table
    object is made; the ordered arrays, every slot of the table and the sentinel label are then read
    back and compared with the numpy order (count descending, key ascending)."""
    n, first, lo = 4097, 3, LO["int32"]
    rng = np.random.default_rng(seed_of("two tiles", kind))
    keys = np.sort(np.append(keyset("scrambled", n - 1, "int32", rng), np.int32(lo)))
    counts = 1 + np.minimum(rng.zipf(2.0, n), 200).astype(np.int64)
    counts[1 + rng.permutation(n - 1)[:4]] = (255, 400, 255, 1000)    # the tail, with a tie
    counts[0] = 2                                                     # the smallest key: below the tail
    n_big = int((counts >= 255).sum())
    assert 4 <= n_big < 64
    order = np.lexsort((keys, -counts))
    pos = np.empty(n, np.int32)
    pos[order] = np.arange(n, dtype=np.int32)
    monkeypatch.setattr(K, "ENCODE_RESIDENT_I32", 0)
    if kind == "dumped":
        job = K.DenseCountJob(dev(rng.permutation(np.repeat(keys, counts))), None, None, hint=n)
        job.path = K.PATH_RANGE
        dk, dc, _, info = K.dense_count_many([job])[0]
        assert info["path"] == K.PATH_RANGE and not info.get("range_failed") and info["n_big"] == n_big, info
        R.first_mismatch(host(dk), keys, "two tiles: counted keys")
        ok, oc = torch.empty_like(dk), torch.empty_like(dc)
        tab = K.EncodeTable(ok, first, unique=True, defer_build=True,
                            range_table=(info["range_table"], info["range_aux"], info["range_bits"]))
        src = (dk, dc, info["cls_hist"], n_big, None)
        slots = (1 << info["range_bits"]) * (16384 + 128) + 64         # kRpRegion, kRpGuard
    else:
        dk, dc = dev(keys), dev(counts)
        ok, oc = torch.empty_like(dk), torch.empty_like(dc)
        tab = K.EncodeTable(ok, first, unique=True, defer_build=True, range_table=None, flat=True)
        src = (dk, dc, K.class_hist(dc), n_big, dev(pos) if kind == "labels" else None)
        assert tab.flat_slots > 0 and tab.capacity == tab.flat_slots + n + 64
        slots = tab.capacity
    monkeypatch.undo()
    assert tab.table is not None and tab.range_aux is not None
    tab.head_image = None                                             # (the LDS head is not what is tested)
    _finalize(K, tab, oc, counts.max(), src=src)
    tab.wait_ready()
    R.first_mismatch(host(ok), keys[order], f"two tiles, {kind}: vocabulary order")
    R.first_mismatch(host(oc), counts[order], f"two tiles, {kind}: ordered counts")
    words = host(tab.table.view(torch.uint8)).view(np.uint64)[:slots]
    words = words[(words & 0xFFFFFFFF) != 0x80000000]                 # slots that hold a key
    got_keys = (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    got_labels = (words >> 32).astype(np.int64)
    by_key = np.argsort(got_keys, kind="stable")
    R.first_mismatch(got_keys[by_key], keys[1:], f"two tiles, {kind}: keys in the table")
    R.first_mismatch(got_labels[by_key], first + pos[1:].astype(np.int64), f"two tiles, {kind}: labels in the table")
    assert int(tab.sentinel_label.item()) == first + int(pos[0])


# ---------------------------------------------------------------------------------------------
# the smallest key of the type: the tables' empty marker, and an ordinary key
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["absent", "first", "last", "head", "beyond"])
@pytest.mark.parametrize("kind", KINDS)
def test_smallest_key_everywhere(K, kind, where):
    T = table(K, kind, MID_VOCAB[kind], sentinel=where)
    at = np.flatnonzero(T.vk == T.lo)
    assert at.size == (where != "absent")
    if where in ("head", "beyond") and T.vk.size > HEAD16 + 100:
        assert (at[0] < HEAD16) == (where == "head"), (where, at)
    if where in ("first", "last"):
        assert at[0] == (0 if where == "first" else T.vk.size - 1)
    for out_dtype in ("int64", "int32"):
        rng = np.random.default_rng(seed_of(kind, where, out_dtype))
        for n in (5, 4097, 30_007):
            base = make_rows(T, n, rng)
            base[::97] = T.lo                       # valid rows AND (through poison) under nulls
            for name, valid in patterns(n, rng):
                if name in ("no-bitmap", "random10", "alternating"):
                    check(K, T, poison(T, base, valid, rng), valid, out_dtype, 7, f"smallest key {where}, {name}")


# ---------------------------------------------------------------------------------------------
# label arguments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ["small2048"])
def test_label_arguments(K, kind):
    nv = 1000 if kind == "small2048" else MID_VOCAB[kind]
    real = "resident" if kind == "small2048" else kind
    for first in (0, 3, 2_000_000_000):
        T = table(K, real, nv, first=first)
        rng = np.random.default_rng(seed_of(kind, first))
        n = 10_007
        base = make_rows(T, n, rng)
        valid = rng.random(n) >= 0.1
        keys = poison(T, base, valid, rng)
        # nb = 2^31 - 1 with int32 labels: oov_label + bucket can pass INT32_MAX by one or two; the
        # kernel's cast and the reference's astype both keep the low 32 bits.  That equality of two
        # wraps is what the code does today, not a documented behaviour; the int64 labels are.
        for nb in (0, 1, 2, 7, 2**31 - 1):
            if first > 3 and nb > 7:
                continue    # (every int32 label would wrap there: nothing but the wrap would be compared)
            for out_dtype in ("int64", "int32"):
                for variant in (0, 1):
                    if first == 2_000_000_000 and variant == 1 and out_dtype == "int32":
                        continue   # null / oov labels above the vocabulary's do not fit int32 there
                    check(K, T, keys, valid, out_dtype, nb, f"first={first} variant={variant}",
                          labels=labels_for(T, variant))


# ---------------------------------------------------------------------------------------------
# key distributions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dist,n_vocab", [
    ("hashed", "dense", 50_000), ("hashed", "fullrange", 50_000), ("resident", "dense", 8192),
    ("resident", "fullrange", 2048), ("resident", "fullrange", 8000), ("cache_eager", "dense", 100_000),
    ("cache_eager", "fullrange", 100_000), ("cache_image", "dense", 30_000), ("cache_image", "fullrange", 70_000),
    ("flat", "dense", 30_000), ("flat", "fullrange", 70_000), ("dumped", "dense", 100_000),
], ids=lambda v: str(v))
def test_key_distributions(K, kind, dist, n_vocab):
    # (dense ids and one key at the far end of the range are not spread over their range: the
    # counting pass would leave the range path, test_gpu_range_path.py)
    T = build(K, kind, n_vocab, dist=dist, sentinel="absent" if kind == "dumped" else "last")
    if dist == "fullrange":
        assert np.isin([2**31 - 1, -1, 0], T.vk).all()
    for out_dtype in ("int64", "int32"):
        sweep(K, T, [4099, 150_001], out_dtype, seed_of(kind, dist, out_dtype), pats=("no-bitmap", "random10"), nb=7,
              need_mix=True)


def test_flat_table_with_clustered_vocabulary_uses_the_gallop_search(K):
    """50 000 consecutive ids and five far outliers: the monotone map sends the ids to a handful of
    home slots, entries sit tens of thousands of slots from home (>> kFlatLinear = 8, and beyond
    what Categorify keeps a flat table for).  Encoded on the flat table as it is, still exact."""
    T = build(K, "flat", 50_006, dist="clustered", sentinel="first")
    maxdisp = int(T.tab.range_aux[T.tab.FLAT_AUX_MAXDISP].item()) & 0xFFFFFFFF
    assert maxdisp > 8 and not T.tab.flat_ok(), maxdisp
    assert T.tab.flat_slots > 0 and T.shape("int64") == "encode_pipe_kernel<2>"
    for out_dtype in ("int64", "int32"):
        rng = np.random.default_rng(seed_of("clustered", out_dtype))
        for n in (4097, TRIP["int32"] + 4 * 1029 + 3):      # per-key path; pipeline + leftovers + tail
            base = make_rows(T, n, rng)
            # unseen keys INSIDE the runs' key range, below and above it
            un = rng.random(n) < 0.02
            base[un] = rng.integers(-2**31, 2**31 - 1, int(un.sum())).astype(np.int32)
            base[::501] = 999
            base[1::501] = 1000 + 50_001
            base[2::501] = 2**31 - 2
            for name, valid in patterns(n, rng):
                if name in ("no-bitmap", "random10"):
                    check(K, T, poison(T, base, valid, rng), valid, out_dtype, 7, f"clustered maxdisp={maxdisp} {name}")


# ---------------------------------------------------------------------------------------------
# unique=False: user-supplied vocabularies (Categorify(vocabs=...) with a repeated key)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_duplicate_vocabulary_keys_first_label_wins(K, dtype):
    """enc_build_kernel: "first (lowest) label wins", for the smallest key of the type as well (it
    lives in a word of its own beside the table; every thread that sees it used to store there)."""
    rng = np.random.default_rng(seed_of("dups", dtype))
    lo = LO[dtype]
    base = keyset("collide" if dtype == "int64" else "fullrange", 6000, dtype, rng)
    vk = np.concatenate([base, base[rng.integers(0, base.size, 20_000)]])
    vk = rng.permutation(vk)
    # the smallest key 4000 times, spread over every workgroup of the build launch
    vk[1 + rng.choice(vk.size - 1, 4000, replace=False)] = lo
    first_at = int(np.flatnonzero(vk == lo)[0])
    assert first_at > 0 and np.unique(vk).size < vk.size - 4000
    kind = "hashed64" if dtype == "int64" else "hashed"
    for rep in range(3):
        tab = K.EncodeTable(dev(vk), 3, unique=False)
        assert tab.table is not None and tab.vocab_keys is None
        T = Tab(kind, tab, vk, 3, dtype)
        assert int(tab.sentinel_label.item()) == 3 + first_at, \
            f"{dtype}: label of the repeated smallest key {int(tab.sentinel_label.item())}, expected {3 + first_at}"
        for out_dtype in ("int64", "int32"):
            sweep(K, T, [9, 20_011], out_dtype, seed_of("dups", dtype, out_dtype, rep), pats=("no-bitmap", "random10"),
                  nb=7)


def test_categorify_with_a_repeated_vocabulary_key(K, tmp_path):
    """The way Categorify reaches unique=False: a vocabulary file that holds a key twice."""
    import pandas as pd

    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    lo = LO["int32"]
    vocab = np.array([7, lo, 9, 7, lo, 11, lo, 9], dtype=np.int32)
    path = str(tmp_path / "unique.c.parquet")
    pd.DataFrame({"c": vocab}, index=pd.RangeIndex(3, 3 + vocab.size)).to_parquet(path)
    op = ops.Categorify(vocabs={"c": path})
    keys = np.array([lo, 7, 9, 11, 5, lo, 9], dtype=np.int32)
    wf = nvt.Workflow(["c"] >> op)
    got = wf.fit_transform(nvt.Dataset(pd.DataFrame({"c": keys}))).to_ddf().compute()["c"].to_numpy()
    exp = R.encode_ref(keys, None, vocab, 3, 1, 2, 0, got.dtype)
    R.first_mismatch(got, exp, "Categorify(vocabs=file with repeated keys)")


# ---------------------------------------------------------------------------------------------
# encode_many
# ---------------------------------------------------------------------------------------------
def _many_items(K, tabs, lengths, seed, nb=7):
    items, refs = [], []
    for i, (T, n) in enumerate(zip(tabs, lengths)):
        rng = np.random.default_rng(seed + i)
        base = make_rows(T, n, rng)
        valid = None if i % 3 == 0 else rng.random(n) >= 0.1
        keys = poison(T, base, valid, rng)
        null_label, oov_label = labels_for(T)
        items.append((T.tab, dev(keys), None if valid is None else dev(R.pack_bits(valid)), null_label, oov_label, nb))
        refs.append((T, keys, valid, null_label, oov_label, nb))
    return items, refs


def _check_many(outs, refs, out_dtype, what):
    for i, (out, (T, keys, valid, null_label, oov_label, nb)) in enumerate(zip(outs, refs)):
        exp = R.encode_ref(keys, valid, T.vk, T.first, null_label, oov_label, nb, NP[out_dtype])
        R.first_mismatch(host(out), exp, f"{what} column {i}: {T.describe(out_dtype)} rows={keys.size}")


@pytest.mark.parametrize("out_dtype", ["int64", "int32"])
def test_encode_many_mixes_every_table_kind(K, out_dtype):
    """Eleven columns on three internal streams: every table kind, both key widths, different
    lengths (one column without rows); twice on the same tables with identical results."""
    tabs = [table(K, k, MID_VOCAB[k]) for k in KINDS] + [table(K, "resident", 1000), table(K, "resident", 2000)]
    lengths = [100_003, 50_001, 0, 70_007, 300_001, 8193, 2_097_152 + 4 * 1029 + 3, 12_288, 500_009, 4097, 1]
    items, refs = _many_items(K, tabs, lengths, seed_of("many", out_dtype))
    outs = K.encode_many(items, TT[out_dtype])
    _check_many(outs, refs, out_dtype, "encode_many")
    again = K.encode_many(items, TT[out_dtype])
    for i, (a, b) in enumerate(zip(outs, again)):
        R.first_mismatch(host(b), host(a), f"encode_many, second call, column {i}")


def test_encode_many_takes_pending_tables_by_event(K):
    """Tables whose vocabulary nvt_vocab_finalize_many is still ordering on an internal stream are
    handed to encode_many as they are (no wait_ready), as Categorify.transform does."""
    tabs = [build(K, k, nv, sentinel=s, seed=1, verify=False)
            for k, nv, s in (("cache_image", 300_001, "head"), ("flat", 400_003, "first"), ("dumped", 200_003, "beyond"),
                             ("cache_image", 65_537, "last"))]
    assert any(T.tab.pending for T in tabs), "no table was left pending: the hand-off is not exercised"
    pending = [T.tab.pending for T in tabs]
    tabs.append(table(K, "resident", 1000))
    items, refs = _many_items(K, tabs, [500_009, 300_007, 400_001, 100_003, 20_011], seed_of("pending"))
    outs = K.encode_many(items, torch.int64)
    assert not any(T.tab.pending for T in tabs)
    _check_many(outs, refs, "int64", f"encode_many(pending={pending})")
    for T in tabs:
        T.verify()


def test_encode_many_converts_key_dtypes_and_refuses_label_dtypes(K):
    T32, T64 = table(K, "cache_eager", MID_VOCAB["cache_eager"]), table(K, "resident64", MID_VOCAB["resident64"])
    rng = np.random.default_rng(seed_of("convert"))
    k32 = make_rows(T32, 10_007, rng)
    inr = T64.vk[(T64.vk >= -2**31) & (T64.vk < 2**31)]  # what an int32 column can carry
    assert inr.size >= 3
    k64 = rng.permutation(np.concatenate([np.tile(inr, 50), rng.integers(-2**31, 2**31 - 1, 1000)])).astype(np.int64)
    outs = K.encode_many([(T32.tab, dev(k32.astype(np.int64)), None, 1, 2, 7),
                          (T64.tab, dev(k64.astype(np.int32)), None, 1, 2, 7)], torch.int32)
    R.first_mismatch(host(outs[0]), R.encode_ref(k32, None, T32.vk, 3, 1, 2, 7, np.int32), "int64 keys, int32 table")
    R.first_mismatch(host(outs[1]), R.encode_ref(k64, None, T64.vk, 3, 1, 2, 7, np.int32), "int32 keys, int64 table")
    got = T32.tab.encode(dev(k32.astype(np.int64)), None, 1, 2, 7, torch.int64)
    R.first_mismatch(host(got), R.encode_ref(k32, None, T32.vk, 3, 1, 2, 7, np.int64), "EncodeTable.encode, int64 keys")
    for bad in (torch.int16, torch.float32, torch.uint8):
        with pytest.raises(TypeError, match="int32 or int64"):
            K.encode_many([(T32.tab, dev(k32), None, 1, 2, 0)], bad)
        with pytest.raises(TypeError, match="int32 or int64"):
            T32.tab.encode(dev(k32), None, 1, 2, 0, bad)
    assert K.encode_many([], torch.int64) == []


# ---------------------------------------------------------------------------------------------
# hash_bucket
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_hash_bucket_both_launch_shapes(K, dtype):
    """The vector kernel (aligned, no hash chain) and the scalar kernel (want_hash / xor_in: the
    only way to it through K.hash_bucket).  A view that is not 16-byte aligned is copied by the
    wrapper (kernels.aligned) and takes the vector kernel again: that case pins the copy."""
    i = np.iinfo(NP[dtype])
    rng = np.random.default_rng(seed_of("hash", dtype))
    sizes = SMALL_SIZES + [100_003, TRIP[dtype] + (4 if dtype == "int32" else 2) * 5 + 1]
    for n in sizes:
        keys = rng.integers(i.min, i.max, n).astype(NP[dtype])
        keys[:5] = np.array([0, -1, i.min, i.max, 1], dtype=NP[dtype])[:n]
        carry = rng.integers(-2**63, 2**63 - 1, n)
        for name, valid in patterns(n, rng):
            if n > 5000 and name not in ("no-bitmap", "random10"):
                continue
            x = keys.copy()
            if valid is not None:
                x[~valid] = np.where(np.arange(int((~valid).sum())) % 2 == 0, i.min, 12345).astype(NP[dtype])
            dk, dv = dev(x), None if valid is None else dev(R.pack_bits(valid))
            for nb in (1, 2, 2**31 - 1):
                what = f"hash_bucket {dtype} rows={n} {name} nb={nb}"
                out, none = K.hash_bucket(dk, nb, valid=dv)
                assert none is None and out.dtype == torch.int32
                R.first_mismatch(host(out), R.hash_bucket_ref(x, valid, nb), what + " [vector kernel]")
                out, h = K.hash_bucket(dk, nb, want_hash=True, valid=dv)
                R.first_mismatch(host(out), R.hash_bucket_ref(x, valid, nb), what + " [scalar kernel]")
                R.first_mismatch(host(h).view(np.uint64), R.hash64_ref(x, valid), what + " [hash]")
                out, h = K.hash_bucket(dk, nb, xor_in=dev(carry), want_hash=True, valid=dv)
                R.first_mismatch(host(out), R.hash_bucket_ref(x, valid, nb, xor_in=carry), what + " [xor chain]")
                R.first_mismatch(host(h).view(np.uint64), R.hash64_ref(x, valid, xor_in=carry), what + " [xor hash]")
                none, h = K.hash_bucket(dk, nb, want_hash=True, want_bucket=False, valid=dv)
                assert none is None
                R.first_mismatch(host(h).view(np.uint64), R.hash64_ref(x, valid), what + " [hash only]")
            if n >= 9 and valid is None:   # a view one element into the buffer: the wrapper copies it
                out, _ = K.hash_bucket(dev(x)[1:], 7)
                R.first_mismatch(host(out), R.hash_bucket_ref(x[1:], None, 7), f"hash_bucket {dtype} rows={n - 1} view+1")
