"""Kernel-level matrix for Categorify's ordering step, the stage between counting and encoding
(nvtabular_amd/csrc/nvt_sort.hip, nvt_vocab_order.hip and the nvt_vocab_finalize_many driver of
nvt_finalize.hip): ``K.vocab_sort``, ``K.class_hist`` and ``nvt_vocab_finalize_many`` called directly
on torch tensors, every ordered list, every slot of every table and every label compared with the
numpy references of order_reference.py (which test_order_reference.py pins to pandas on the CPU).
Nothing is approximate here: every comparison is exact.

Route -> entry point -> kernels, and the test that reaches it on purpose.

  vocab_sort_any (nvt_vocab_sort_i32 / _i64 = K.vocab_sort; the unsorted big vocabularies of finalize_impl)
    n <= 8192                              sort_small_kernel<K>                       test_sort_one_workgroup, test_sort_int64
    int32, 0 < max_count < 2^32            vocab_sort_onesweep: os_hist_kernel, os_base_kernel, os_scatter_kernel
                                           <FIRST / middle / LAST>, 4 + count_bytes(max_count) = 5 .. 8 passes
                                                                                      test_sort_onesweep*, test_finalize_unsorted[16385]
    int32 max_count 0 or >= 2^32, int64    generic LSD: sort_pass_hist_kernel (read-back, max_count 0 only),
                                           sort_tile_hist_kernel, sort_scatter_kernel test_sort_generic_lsd, test_sort_int64,
                                                                                      test_finalize_unsorted[9000-int64 / 9000-mc0]
  finalize_impl (nvt_vocab_finalize_many)
    unsorted int32, 2 .. 16384 entries,    vocab_sort_small_batch: sort_small_packed_many_kernel, 64 vocabularies a launch;
    0 < max_count < 2^32                   then encode_build_any + the head image     test_finalize_unsorted[2 .. 16384],
                                                                                      test_seventy_small_vocabularies
    any other unsorted vocabulary          vocab_sort_any (above) + encode_build_any  test_finalize_unsorted[16385, 9000-*]
    key-sorted, flat or dumped table       vocab_order_sorted_batch (every size up to 2^23 entries, one vocabulary too)
    key-sorted, hashed table or no table   vocab_order_from_sorted (+ vocab_order_tail_batch for a small tail)
    key-sorted with src_labels             vocab_from_labels: label_scatter_kernel, then
                                             flat table: flat_params_kernel + flat_build_kernel
                                                                                      test_eighteen_key_sorted_vocabularies
                                             hashed table: encode_insert_any; no table: the scatter alone
                                                                                      test_mixed_call
    small / big split, fork onto the three internal streams, ready events or the stream join
                                                                                      test_mixed_call
  vocab_order_sorted_batch
    every stage one launch per OrdBatch    ord_prep_kernel, cls_scatter_many_kernel, flat_params_many_kernel +
    of 16 jobs                             flat_build_many_kernel (flat), range_patch_many_kernel (dumped)
                                                                                      test_key_sorted_tile_sizes[flat / dumped],
                                                                                      test_eighteen_key_sorted_vocabularies (two batches)
    tail of 2 .. 16384, max_count < 2^32   vocab_order_tail_batch                     test_tail_shapes[flat / dumped - nbig2, edges, all,
                                                                                      nbig16384, lo_*]
    tail of 1, of > 16384, or a count      vocab_sort_any (not for 1) + range_fix_prefix_kernel
    >= 2^32                                                                           test_tail_shapes[flat / dumped - nbig1, nbig16385, huge]
  vocab_order_from_sorted
    hashed table (table && !range_aux)     encode_clear_any, cls_scatter_kernel inserting into the table itself
                                                                                      test_key_sorted_tile_sizes[hashed], test_tail_shapes[hashed-*]
    no table (n <= 8192, kind resident)    cls_scatter_kernel, ordering only          test_key_sorted_tile_sizes[notable]
    tail of 2 .. 16384, max_count < 2^32   deferred: vocab_order_tail_batch           [hashed-nbig2 .. nbig16384], test_mixed_call
    any other tail                         vocab_sort_any + encode_insert_any         [hashed-nbig1, nbig16385, huge]
    flat / dumped table                    only beyond 2^23 entries: left out (below)
  vocab_order_tail_batch                   sort_small_packed_many_kernel, then range_fix_prefix_many_kernel (flat, dumped)
                                           or encode_insert_any (hashed); nothing more without a table
  nvt_class_hist (K.class_hist)            class_hist_kernel                          test_class_hist

Where the profile families (``K.profile_begin`` / ``K.profile_end``: vocab_sort_small, vocab_sort,
vocab_order, encode_build) tell routes apart, the tests assert the number of scopes that the chunking
implies: one ``vocab_sort_small`` per launch of the batched sort, one ``vocab_sort`` per vocab_sort_any.
They do not tell vocab_order_sorted_batch from vocab_order_from_sorted (both open ``vocab_order``, and
so does every launch that builds head images), nor range_fix_prefix_kernel from its batched twin or
from encode_insert_any (all ``encode_build``): there the route follows from the descriptor alone -- a
table with range_aux is batched, a table without it or no table is not; the tail is batched when
2 <= n_big <= 16384 and 0 < max_count < 2^32 -- and each helper asserts the descriptor (``tab.kind``,
n_big, max_count) it hands over.

A table is checked twice: through ``tab.encode`` (vocabulary keys and keys that are not in it), and
slot by slot from a copy of the table itself -- a vocabulary of at most 8192 keys is encoded from
LDS whatever table it owns, so only the copy shows what the ordering wrote there.

Sizes.  The look-back kernels work on tiles of kS2Tile = 4096 entries: TILES are one tile less one,
one, one and one entry, three tiles, three and five entries, 18 tiles.  os_hist_kernel makes a
second grid-stride trip beyond 1024 * 256 entries: 266 241.

Left out, by name: the value of NVT_FLAT_AUX_MAXDISP (its fallback:
test_clustered_keys_fall_back_to_a_hashed_index); vocabularies above 2^23 entries, which take a
stream of their own and vocab_order_from_sorted with a range table; the n >= 2^30 packed-sort
fallback (vocab_sort_packed); the contents of the head image (test_gpu_encode_kernels.py).
"""
import contextlib
import zlib

import numpy as np
import pytest
import torch

import order_reference as R

pytestmark = pytest.mark.gpu

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
LO, HI = I32.min, I32.max
NULL, OOV, FIRST = 1, 2, 3
TILES = [4095, 4096, 4097, 3 * 4096, 3 * 4096 + 5, 70_001]
SMALL_MAX = 16384          # kSmallPackedMax: entries of the batched one-workgroup sort
RESIDENT = 8192            # NVT_ENCODE_RESIDENT_I32


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


_COUNTED = {}   # name -> (keys, counts, info) of a column counted on the range path, shared by the tests


@pytest.fixture(scope="module", autouse=True)
def _free_shared():
    yield
    _COUNTED.clear()
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# keys and counts
# ---------------------------------------------------------------------------------------------
def keys_i32(n, rng, lo=True):
    """n distinct int32 keys in random order over the whole range: the largest value, -1 and 0, many
    negative keys, and (lo) the smallest value of the type."""
    want = ([LO] if lo else []) + [HI, -1, 0]
    k = np.unique(rng.integers(LO + 1, HI, int(n * 1.1) + 16))
    k = np.setdiff1d(k, want)
    k = np.concatenate([want[:n], rng.permutation(k)[:max(0, n - len(want))]]).astype(np.int64)
    assert k.size == n and np.unique(k).size == n
    return rng.permutation(k).astype(np.int32)


def keys_i64(n, rng):
    """Five low words under many high words of both signs, and both ends of the type."""
    j = np.arange(n, dtype=np.int64)
    k = (j % 5) + ((j // 5 - n // 10) << 32)
    k[0], k[-1] = I64.min, I64.max
    assert np.unique(k).size == n and (k < 0).any() and (k > 0).any()
    return rng.permutation(k)


def keys_scrambled(n, rng, lo):
    """Sorted: n distinct keys spread over [0, 2^31) (x -> a x + b mod 2^31 with a odd), which the
    range path of the counting stage takes; (lo) the smallest int32 in front."""
    m = n - bool(lo)
    k = (np.arange(1, m + 1, dtype=np.int64) * 2654435761 + 12345 + int(rng.integers(0, 1000))) % (2**31)
    assert np.unique(k).size == m
    return np.sort(np.append(k, LO) if lo else k).astype(np.int32)


def plant(c, values, rng):
    at = rng.permutation(c.size)[:len(values)]
    c[at] = np.asarray(values, np.int64)[:at.size]
    return c


def counts_loguniform(n, max_count, rng):
    """Log-uniform over [1, max_count] (every live byte of the count varies), half of the entries tied
    on sixteen values, both ends planted."""
    c = np.floor(np.exp(rng.random(n) * np.log(float(max_count) + 1.0))).astype(np.int64)
    c = np.clip(c, 1, max_count)
    tied = rng.random(n) < 0.5
    c[tied] = c[rng.integers(0, n, 16)][rng.integers(0, 16, int(tied.sum()))]
    return plant(c, [max_count, 1], rng)


def counts_powerlaw(n, max_count, rng):
    """Almost all counts 1; a few entries log-uniform up to max_count, which is among them."""
    c = np.ones(n, np.int64)
    few = rng.permutation(n)[:n // 1000 + 2]
    c[few] = counts_loguniform(few.size, max_count, rng)
    return c


def counts_below_tail(n, rng):
    """1 .. 250 with many ties: nothing in class 255."""
    return np.minimum(rng.zipf(1.6, n), 250).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# A. K.vocab_sort
# ---------------------------------------------------------------------------------------------
def check_sort(K, keys, counts, max_count, what):
    assert counts.dtype == np.int64 and np.unique(keys).size == keys.size
    assert max_count == 0 or int(counts.max()) <= max_count
    order = np.lexsort((keys, -counts))
    dk, dc = dev(keys), dev(counts)
    K.vocab_sort(dk, dc, int(max_count))
    what = f"vocab_sort {keys.dtype} n={keys.size} max_count={max_count} {what}"
    R.first_mismatch(host(dk), keys[order], what + ": keys")
    R.first_mismatch(host(dc), counts[order], what + ": counts")


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 4097, 8191, 8192])
def test_sort_one_workgroup(K, n):
    rng = np.random.default_rng(seed_of("bitonic", n))
    keys = keys_i32(n, rng)
    assert LO in keys and HI in keys and (n < 3 or (keys < 0).sum() >= 2)
    for what, counts in (("ties", rng.integers(1, 6, n).astype(np.int64)),
                         ("log-uniform", counts_loguniform(n, 2**32 - 1, rng)),
                         ("beyond 32 bits", plant(rng.integers(1, 4, n).astype(np.int64), [2**40, 2**32], rng))):
        for max_count in (0, int(counts.max())):
            check_sort(K, keys, counts, max_count, f"one workgroup, {what}")


ONESWEEP_N = [8193, 12_288, 12_293, 70_001, 266_241]
ONESWEEP_MAX = [1, 255, 256, 65_535, 65_536, 2**24, 2**32 - 1]      # 5, 5, 6, 6, 7, 8, 8 passes


@pytest.mark.parametrize("max_count", ONESWEEP_MAX)
@pytest.mark.parametrize("n", ONESWEEP_N)
def test_sort_onesweep(K, n, max_count):
    rng = np.random.default_rng(seed_of("onesweep", n, max_count))
    keys = keys_i32(n, rng)
    assert LO in keys and HI in keys and (keys < 0).sum() > n // 3
    counts = counts_loguniform(n, max_count, rng)
    assert counts.max() == max_count and counts.min() == 1 and np.unique(counts).size < 0.6 * n     # heavy ties
    for b in range(4):      # every live byte of the count really varies
        if max_count >> (8 * b):
            assert np.unique((counts >> (8 * b)) & 0xFF).size > 1 or max_count == 1 << (8 * b)
    check_sort(K, keys, counts, max_count, f"onesweep, {4 + (int(max_count).bit_length() + 7) // 8} passes")


@pytest.mark.parametrize("max_count", [200, 60_000, 2**23, 2**31 + 5], ids=["5-passes", "6-passes", "7-passes", "8-passes"])
def test_sort_onesweep_power_law(K, max_count):
    """Almost every count is 1: in every pass above the lowest count byte nearly all entries fall into
    digit 0xFF (counted in registers), in pass 4 into one digit (the wave-aggregated histogram)."""
    for n in (12_293, 266_241):
        rng = np.random.default_rng(seed_of("power law", n, max_count))
        counts = counts_powerlaw(n, max_count, rng)
        assert (counts == 1).mean() > 0.99 and counts.max() == max_count
        check_sort(K, keys_i32(n, rng), counts, max_count, "onesweep, power law")


def test_sort_onesweep_loose_bound(K):
    """Counts <= 5 under the bound 2^31: eight passes, three of which see EVERY entry in digit 0xFF."""
    for n in (8193, 70_001, 266_241):
        rng = np.random.default_rng(seed_of("loose", n))
        check_sort(K, keys_i32(n, rng), rng.integers(1, 6, n).astype(np.int64), 2**31, "onesweep, loose bound")


@pytest.mark.parametrize("n", [8193, 70_001])
def test_sort_generic_lsd(K, n):
    rng = np.random.default_rng(seed_of("lsd", n))
    keys = keys_i32(n, rng)
    ties = rng.integers(1, 6, n).astype(np.int64)
    # max_count 0: the per-pass histograms are read back and the constant passes skipped
    check_sort(K, keys, ties, 0, "generic LSD, read-back, six count passes skipped")
    check_sort(K, keys, counts_loguniform(n, 2**32 - 1, rng), 0, "generic LSD, read-back, four count bytes live")
    c32 = plant(counts_loguniform(n, 2**32 - 1, rng), [2**32, 2**32, 2**32 - 1], rng)
    check_sort(K, keys, c32, 2**32, "generic LSD, max_count 2^32: five count passes")
    c40 = plant(counts_loguniform(n, 2**40, rng), [2**40, 2**33, 2**33], rng)
    check_sort(K, keys, c40, 2**40, "generic LSD, counts up to 2^40, exact bound")
    check_sort(K, keys, c40, 0, "generic LSD, counts up to 2^40, read-back")
    check_sort(K, np.sort(keys), np.ones(n, np.int64), 0, "generic LSD, read-back, sorted already")


@pytest.mark.parametrize("n", [2, 8192, 8193, 70_001])
def test_sort_int64(K, n):
    rng = np.random.default_rng(seed_of("int64", n))
    keys = keys_i64(n, rng)
    assert I64.min in keys and I64.max in keys
    assert n < 10 or np.unique(keys & 0xFFFFFFFF).size <= 7        # the keys differ above bit 32 only
    for what, counts in (("ties", rng.integers(1, 6, n).astype(np.int64)),
                         ("log-uniform", counts_loguniform(n, 2**32 - 1, rng)),
                         ("beyond 32 bits", plant(rng.integers(1, 4, n).astype(np.int64), [2**40, 2**32], rng))):
        for max_count in (0, int(counts.max())):
            check_sort(K, keys, counts, max_count, f"int64, {what}")


# ---------------------------------------------------------------------------------------------
# B / C. nvt_vocab_finalize_many
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def resident_gate_lifted(K, lifted):
    """EncodeTable keeps an int32 vocabulary of at most 8192 keys in LDS and gives it no table; while
    a table object is made for such a vocabulary on purpose, the gate is lifted."""
    old = K.ENCODE_RESIDENT_I32
    if lifted:
        K.ENCODE_RESIDENT_I32 = 0
    try:
        yield
    finally:
        K.ENCODE_RESIDENT_I32 = old


def count_on_range_path(K, name, keys, counts, rng, share=False):
    """(keys, counts, info) of a column that holds keys[i] counts[i] times, counted on the range
    path: the key-sorted list and the table it dumped.  share: counted once per module."""
    if name in _COUNTED:
        return _COUNTED[name]
    rows = rng.permutation(np.repeat(keys, counts))
    job = K.DenseCountJob(dev(rows), None, None, hint=keys.size)
    job.path = K.PATH_RANGE
    dk, dc, nulls, info = K.dense_count_many([job])[0]
    assert info["path"] == K.PATH_RANGE and not info.get("range_failed"), (name, info)
    assert info["range_table"] is not None and info["range_bits"] >= 8 and nulls == 0, (name, info)
    R.first_mismatch(host(dk), keys, f"{name}: counted keys")
    R.first_mismatch(host(dc), counts, f"{name}: counted counts")
    assert info["n_big"] == R.n_big_ref(counts) and info["max_count"] == int(counts.max()), (name, info)
    if share:
        _COUNTED[name] = (dk, dc, info)
    return dk, dc, info


class Vocab:
    """One vocabulary of a nvt_vocab_finalize_many call and everything its result is compared with.

    route: unsorted | flat | dumped | hashed | notable (the last four: a key-sorted source).
    labelled: the source carries the positions of its entries in the order (src_labels).
    override: (dumped) counts that replace the counted ones in the source list -- the table the counting
    pass dumped holds positions, not counts."""

    KIND = {"flat": "flat", "dumped": "dumped", "hashed": "cache", "notable": "resident"}

    def __init__(self, name, route, keys, counts, first=FIRST, max_count=None, labelled=False, override=None,
                 share=False):
        self.name, self.route, self.keys, self.first = name, route, keys, int(first)
        self.counted, self.counts = counts, counts if override is None else override
        self.max_count = int(self.counts.max()) if max_count is None else int(max_count)
        self.labelled, self.share = labelled, share
        self.n, self.n_big = keys.size, R.n_big_ref(self.counts)
        self.dtype = keys.dtype
        assert self.counts.dtype == np.int64 and np.unique(keys).size == keys.size
        if route != "unsorted":
            assert keys.dtype == np.int32 and (np.diff(keys.astype(np.int64)) > 0).all(), name

    def item(self, K, rng):
        """(table, counts, max_count, src) for fill_vocab_desc; asserts the kind of table."""
        n, route = self.n, self.route
        if route == "unsorted":
            dk, self.oc = dev(self.keys), dev(self.counts)
            self.tab = tab = K.EncodeTable(dk, self.first, unique=True, defer_build=True)
            res = RESIDENT if self.dtype == np.int32 else 6144
            assert tab.kind == ("resident" if n <= res else "cache" if self.dtype == np.int32 else "linear64"), self.name
            return tab, self.oc, self.max_count, None
        assert route != "notable" or n <= RESIDENT, self.name
        lifted = route != "notable" and n <= RESIDENT
        if route == "dumped":
            dk, dc, info = count_on_range_path(K, self.name, self.keys, self.counted, rng, self.share)
            hist, rtab = info["cls_hist"], (info["range_table"].clone(), info["range_aux"], info["range_bits"])
            if self.counts is not self.counted:
                dc = dev(self.counts)
                hist = K.class_hist(dc)
        else:
            dk, dc = dev(self.keys), dev(self.counts)
            hist, rtab = K.class_hist(dc), None
        ok, self.oc = torch.empty_like(dk), torch.empty_like(dc)
        with resident_gate_lifted(K, lifted):
            self.tab = tab = K.EncodeTable(ok, self.first, unique=True, defer_build=True, range_table=rtab,
                                           flat=route == "flat")
        assert tab.kind == self.KIND[route], (self.name, tab.kind)
        if route == "flat":
            assert tab.flat_slots > 0 and tab.range_aux is not None and tab.capacity == tab.flat_slots + n + 64
            self.slots = tab.capacity
        elif route == "dumped":
            assert tab.capacity == 0 and tab.flat_slots == 0 and tab.range_aux is not None and tab.table is rtab[0]
            self.slots = (1 << info["range_bits"]) * (16384 + 128) + 64      # kRpRegion, kRpGuard
        elif route == "hashed":
            assert tab.table is not None and tab.range_aux is None and tab.flat_slots == 0
            assert tab.capacity == K.next_pow2(4 * n + 1)
            self.slots = tab.capacity
        else:
            assert tab.table is None and tab.sentinel_label is None and tab.head_image is None
        if lifted:
            tab.head_image = None      # (an LDS head is built for vocabularies beyond the gate only)
        labels = dev(R.positions_ref(self.keys, self.counts)) if self.labelled else None
        return tab, self.oc, self.max_count, (dk, dc, hist, self.n_big, labels)

    def sorts(self):
        """(vocab_sort_small scopes, vocab_sort scopes) this vocabulary opens when it is finalized alone."""
        if self.route == "unsorted":
            m = self.n
        elif self.labelled:
            return 0, 0
        else:
            m = self.n_big
        small = self.dtype == np.int32 and 2 <= m <= SMALL_MAX and 0 < self.max_count < 2**32
        return (1, 0) if small else (0, 1 if m > 1 else 0)

    def check(self, K):
        tab, what = self.tab, f"{self.name} [{self.route}, n={self.n}, n_big={self.n_big}, max_count={self.max_count}]"
        tab.wait_ready()
        vk, vc = R.vocab_order_ref(self.keys, self.counts)
        R.first_mismatch(host(tab._vk), vk, what + ": vocabulary order")
        R.first_mismatch(host(self.oc), vc, what + ": ordered counts")
        i = np.iinfo(self.dtype)
        lo = i.min
        # every slot of the table itself
        if tab.table is not None and self.dtype == np.int32:
            slots = self.slots if self.route != "unsorted" else tab.capacity
            words = host(tab.table.view(torch.uint8)).view(np.uint64)[:slots]
            words = words[(words & 0xFFFFFFFF) != 0x80000000]                 # slots that hold a key
            got_keys = (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            by_key = np.argsort(got_keys, kind="stable")
            in_table = np.sort(self.keys[self.keys != lo])
            R.first_mismatch(got_keys[by_key], in_table, what + ": keys in the table")
            R.first_mismatch((words >> 32).astype(np.int64)[by_key], R.labels_ref(in_table, vk, self.first),
                             what + ": labels in the table")
        if tab.sentinel_label is not None:
            got = int(tab.sentinel_label.item())
            assert got == int(R.labels_ref(np.array([lo], self.dtype), vk, self.first)[0]), \
                f"{what}: label of the smallest key {got}"
        # through encode: every vocabulary key, then keys that are not in the vocabulary
        wide = self.keys.astype(np.int64)
        near = np.concatenate([np.minimum(wide, i.max - 1) + 1, np.maximum(wide, i.min + 1) - 1,
                               [i.min, i.max, i.min + 1, i.max - 1, 0, 5, -7]])
        if self.dtype == np.int64:     # the same low word under another high word
            near = np.concatenate([near, np.minimum(wide, i.max - 2**32) + 2**32])
        near = near.astype(self.dtype)
        assert (lo in self.keys) or (lo in near)
        assert not np.isin(near, self.keys).all()
        for part, probe in (("vocabulary keys", self.keys), ("keys around the vocabulary", near)):
            exp = R.labels_ref(probe, vk, self.first)
            exp[exp < 0] = OOV
            got = tab.encode(dev(probe), None, NULL, OOV, 0, torch.int64)
            R.first_mismatch(host(got), exp, f"{what}: encode, {part}")


def finalize(K, vocabs, seed, profile=True):
    """One nvt_vocab_finalize_many call for all of `vocabs` -> the profile scopes it opened."""
    from nvtabular_amd import _lib

    rng = np.random.default_rng(seed)
    items = [v.item(K, rng) for v in vocabs]
    descs = (_lib.VocabCol * len(items))()
    for d, (tab, counts, max_count, src) in zip(descs, items):
        tab.fill_vocab_desc(d, counts, max_count, src=src)
    torch.cuda.synchronize()
    if profile:
        K.profile_begin()
    K.check(_lib.load().nvt_vocab_finalize_many(descs, len(items), K.stream_ptr()), "nvt_vocab_finalize_many")
    return {k: v[1] for k, v in K.profile_end().items()} if profile else {}


def finalize_alone(K, v):
    scopes = finalize(K, [v], seed_of(v.name, v.route))
    small, sort = v.sorts()
    got = (scopes.get("vocab_sort_small", 0), scopes.get("vocab_sort", 0))
    assert got == (small, sort), f"{v.name} [{v.route}]: (vocab_sort_small, vocab_sort) scopes {got}, expected {(small, sort)}: {scopes}"
    if v.route != "unsorted" and not v.labelled:
        assert scopes.get("vocab_order", 0) >= 1, scopes
    v.check(K)
    return scopes


UNSORTED = [("2", "int32", 2, None), ("3", "int32", 3, None), ("8192", "int32", 8192, None),
            ("8193", "int32", 8193, None), ("16384", "int32", 16384, None), ("16385", "int32", 16385, None),
            ("9000-int64", "int64", 9000, None), ("9000-mc0", "int32", 9000, 0), ("9000-mc2^32", "int32", 9000, 2**32)]


@pytest.mark.parametrize("name,dtype,n,max_count", UNSORTED, ids=[u[0] for u in UNSORTED])
def test_finalize_unsorted(K, name, dtype, n, max_count):
    """2 .. 16384 int32 entries with a count bound below 2^32: the batched one-workgroup sort (8193 is
    padded to 16384 words of LDS); 16385: onesweep; int64, no bound, a bound of 2^32: the generic LSD."""
    rng = np.random.default_rng(seed_of("unsorted", name))
    keys = keys_i32(n, rng, lo=n % 2 == 0) if dtype == "int32" else keys_i64(n, rng)
    counts = counts_loguniform(n, 2**32 if max_count == 2**32 else 100_000, rng)
    v = Vocab("unsorted " + name, "unsorted", keys, counts, max_count=max_count)
    small, sort = v.sorts()
    assert (small == 1) == (dtype == "int32" and n <= SMALL_MAX and max_count is None), (small, sort)
    finalize_alone(K, v)


def sorted_keys(route, n, rng, lo):
    return keys_scrambled(n, rng, lo) if route == "dumped" else np.sort(keys_i32(n, rng, lo=lo))


# (a vocabulary without a table has at most 8192 entries: the tile sizes below that, and 8192 itself)
SIZES = {"flat": TILES, "dumped": TILES, "hashed": TILES, "notable": [4095, 4096, 4097, 8192]}


@pytest.mark.parametrize("route,n", [(r, n) for r in SIZES for n in SIZES[r]], ids=lambda v: str(v))
def test_key_sorted_tile_sizes(K, route, n):
    """A key-sorted source at the tile sizes of the class scatter; a tail of six entries with a tie,
    and the smallest int32 below the tail in every other case."""
    rng = np.random.default_rng(seed_of("tiles", route, n))
    lo = n % 2 == 1
    keys = sorted_keys(route, n, rng, lo)
    counts = plant(counts_below_tail(n, rng), [255, 400, 255, 1000, 256, 400], rng)
    if lo:
        counts[0] = 2
    assert R.n_big_ref(counts) in (5, 6)
    finalize_alone(K, Vocab("tile sizes", route, keys, counts, first=FIRST if n % 3 else 1000))


def tail_case(shape, route, rng):
    """(keys, counted counts, counts that replace them in the source list or None)."""
    if shape == "all":                       # n_big = n: every count in class 255, ties
        keys = sorted_keys(route, 8200, rng, False)
        return keys, 255 + np.minimum(rng.zipf(2.0, keys.size) - 1, 40).astype(np.int64), None
    if shape in ("nbig16384", "nbig16385"):  # the largest tail of the batched sort; the smallest beyond it
        keys = sorted_keys(route, 20_011, rng, False)
        c = rng.integers(1, 6, keys.size).astype(np.int64)
        big = rng.permutation(keys.size)[:int(shape[4:])]
        c[big] = 255 + rng.integers(0, 4, big.size)
        return keys, c, None
    n = 12_293
    lo = shape in ("lo_tail", "lo_below", "huge")
    keys = sorted_keys(route, n, rng, lo)
    c = counts_below_tail(n, rng)
    at = 1 + rng.permutation(n - 1)          # (entry 0 is the smallest int32 where it is a key)
    if shape == "nbig1":
        c[at[0]] = 1000
    elif shape == "nbig2":
        c[at[:2]] = 300                      # a tie: the key order decides
    elif shape == "edges":                   # 254 | 255 | 256, each several times
        c[at[:5]], c[at[5:10]], c[at[10:15]] = 254, 255, 256
    elif shape == "huge":                    # one count beyond 32 bits whose low word says "class 7"
        c[at[:300]] = 255 + rng.integers(0, 1000, 300)
        c[0] = 1
        over = c.copy()
        over[at[0]] = 2**32 + 7
        return keys, c, over
    elif shape in ("lo_tail", "lo_below", "lo_absent"):
        c[at[:9]] = [255, 255, 400, 400, 400, 9000, 256, 70_000, 255]
        if lo:
            c[0] = 400 if shape == "lo_tail" else 2
    else:
        assert shape == "nbig0", shape
    return keys, c, None


TAIL_SHAPES = ["nbig0", "nbig1", "nbig2", "all", "nbig16384", "nbig16385", "edges", "huge", "lo_tail", "lo_below",
               "lo_absent"]
N_BIG = {"nbig0": 0, "nbig1": 1, "nbig2": 2, "all": 8200, "nbig16384": 16384, "nbig16385": 16385, "edges": 10,
         "huge": 300, "lo_tail": 10, "lo_below": 9, "lo_absent": 9}


def tail_vocab(K, shape, route):
    rng = np.random.default_rng(seed_of("tail", shape, route))
    keys, counts, over = tail_case(shape, route, rng)
    if route != "dumped" and over is not None:
        counts, over = over, None
    # the dumped table with the 16385-entry tail (4.2 M counted rows) is counted once and shared
    v = Vocab(f"tail {shape}", route, keys, counts, override=over, share=shape == "nbig16385")
    assert v.n_big == N_BIG[shape] and (shape != "huge" or v.max_count >= 2**32), (shape, v.n_big, v.max_count)
    at = np.flatnonzero(keys == LO)
    assert at.size == (shape in ("lo_tail", "lo_below", "huge"))
    if at.size:
        assert (v.counts[at[0]] >= 255) == (shape == "lo_tail")
    return v


@pytest.mark.parametrize("shape", TAIL_SHAPES)
@pytest.mark.parametrize("route", ["flat", "dumped", "hashed"])
def test_tail_shapes(K, route, shape):
    """The class-255 tail at its thresholds, and the three ways its labels reach the table:
    range_fix_prefix_many_kernel (flat, dumped: 2 .. 16384 entries), range_fix_prefix_kernel (flat,
    dumped: one entry, 16385, a count beyond 32 bits), encode_insert_any (hashed).

    huge: a count of 2^32 + 7.  The class scatter packs a count into 32 bits; it used to take the
    class (7) and the count it wrote out (7) from the packed word, so the entry landed among the
    count-7 entries of the vocabulary."""
    v = tail_vocab(K, shape, route)
    small, sort = v.sorts()
    assert (small, sort) == {"nbig0": (0, 0), "nbig1": (0, 0), "nbig16385": (0, 1), "huge": (0, 1)}.get(shape, (1, 0))
    finalize_alone(K, v)


def test_seventy_small_vocabularies(K):
    """70 unsorted int32 vocabularies of 2 .. 16384 entries: two launches of the batched sort (64 + 6)
    and no other sort; each vocabulary as the reference orders it alone."""
    rng = np.random.default_rng(seed_of("seventy"))
    sizes = [2, SMALL_MAX, 3, 8192, 8193, SMALL_MAX - 1, 4097, 64, 65] + rng.integers(2, SMALL_MAX + 1, 61).tolist()
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    assert len(sizes) == 70 and min(sizes) == 2 and max(sizes) == SMALL_MAX
    vocabs = []
    for j, n in enumerate(sizes):
        keys = keys_i32(n, rng, lo=j % 3 == 0)
        bound = [5, 255, 70_000, 2**32 - 1][j % 4]
        vocabs.append(Vocab(f"vocabulary {j} of 70", "unsorted", keys, counts_loguniform(n, bound, rng), first=FIRST + j))
    scopes = finalize(K, vocabs, 0)
    assert scopes.get("vocab_sort_small") == 2 and "vocab_sort" not in scopes, scopes
    for v in vocabs:
        v.check(K)


def test_eighteen_key_sorted_vocabularies(K):
    """18 key-sorted vocabularies in one call: 17 with a flat or a dumped table go through
    vocab_order_sorted_batch in two OrdBatches (16 + 1, largest first, the kinds mixed), the one with
    a labelled source is left to vocab_from_labels.  Tails of 0, 1, a few hundred and 16385 entries."""
    rng = np.random.default_rng(seed_of("eighteen"))
    vocabs = [tail_vocab(K, "nbig16385", "dumped"), tail_vocab(K, "nbig16385", "flat")]     # 20 011 entries each
    sizes = [70_001, 30_011, 12_293, 12_288, 4097, 9001, 15_000, 8193, 25_000, 10_007, 11_003, 13_001, 14_009, 9500,
             4095]
    for j, n in enumerate(sizes):
        route = "dumped" if j % 2 else "flat"
        keys = sorted_keys(route, n, rng, lo=j % 3 == 0)
        counts = counts_below_tail(n, rng)
        at = 1 + rng.permutation(n - 1)
        tail = [0, 1, 300, 2, 150][j % 5]
        counts[at[:tail]] = 255 + rng.integers(0, 50, tail)
        if j % 3 == 0:
            counts[0] = [2, 300][j % 2]      # the smallest int32: below the tail, in the tail
        vocabs.append(Vocab(f"vocabulary {j + 2} of 18", route, keys, counts, first=FIRST + j))
    keys = sorted_keys("flat", 40_009, rng, lo=True)
    vocabs.append(Vocab("labelled vocabulary", "flat", keys, counts_loguniform(keys.size, 5000, rng), labelled=True))
    assert len(vocabs) == 18
    batched = sorted((v for v in vocabs if not v.labelled), key=lambda v: -v.n)
    assert len(batched) == 17 and {v.route for v in batched[:16]} == {"flat", "dumped"}
    last = batched[16]
    assert last.n == 4095 and last.sorts() == (1, 0) and {v.n_big for v in batched} >= {0, 1, 16385}
    assert any(100 <= v.n_big <= 1000 for v in batched) and any(v.sorts() == (1, 0) for v in batched[:16])
    vocabs = [vocabs[i] for i in rng.permutation(18)]
    scopes = finalize(K, vocabs, 1)
    # one batched tail sort per OrdBatch; the two tails of 16385 entries are sorted on their own
    assert scopes.get("vocab_sort_small") == 2 and scopes.get("vocab_sort") == 2, scopes
    for v in vocabs:
        v.check(K)


def mixed_vocabularies(rng):
    def key_sorted(name, route, n, tail, lo, labelled=False):
        keys = sorted_keys(route, n, rng, lo)
        counts = counts_below_tail(n, rng)
        counts[1 + rng.permutation(n - 1)[:tail]] = 255 + rng.integers(0, 9, tail)
        return Vocab(name, route, keys, counts, labelled=labelled)

    return [
        Vocab("small unsorted", "unsorted", keys_i32(3001, rng), counts_loguniform(3001, 70_000, rng)),
        Vocab("small unsorted with a table", "unsorted", keys_i32(12_000, rng, lo=False), counts_loguniform(12_000, 255, rng)),
        Vocab("large unsorted int32", "unsorted", keys_i32(20_011, rng), counts_loguniform(20_011, 2**24, rng)),
        Vocab("unsorted int64", "unsorted", keys_i64(9000, rng), counts_loguniform(9000, 2**40, rng)),
        key_sorted("key-sorted flat", "flat", 12_293, 200, True),
        key_sorted("key-sorted hashed", "hashed", 9001, 40, True),
        key_sorted("key-sorted hashed, no tail", "hashed", 30_011, 0, False),
        key_sorted("key-sorted without a table", "notable", 4097, 7, False),
        key_sorted("labelled, hashed table", "hashed", 9001, 30, True, labelled=True),
        key_sorted("labelled, no table", "notable", 4097, 30, True, labelled=True),
    ]


@pytest.mark.parametrize("events", [True, False], ids=["ready-events", "stream-join"])
def test_mixed_call(K, monkeypatch, events):
    """Every kind of vocabulary in one call: the small ones on the caller's stream, the others forked
    onto the internal streams, two deferred tails (a hashed table, no table) sorted by one batched
    launch behind all scatters, two labelled sources (a hashed table, no table) that are only
    scattered.  With K.ASYNC_FINALIZE every forked vocabulary hands over by its
    ready event; without it the driver joins its streams into the caller's."""
    monkeypatch.setattr(K, "ASYNC_FINALIZE", events)
    vocabs = mixed_vocabularies(np.random.default_rng(seed_of("mixed")))
    scopes = finalize(K, vocabs, 2)
    for v in vocabs:     # forked = everything but the two vocabularies of the small batch
        assert v.tab.pending == (events and not (v.route == "unsorted" and v.sorts() == (1, 0))), v.name
    # vocab_sort_small: the small batch, the flat table's tail, the two deferred tails; vocab_sort: two
    assert scopes.get("vocab_sort_small") == 3 and scopes.get("vocab_sort") == 2, scopes
    for v in vocabs:
        v.check(K)


# ---------------------------------------------------------------------------------------------
# D. K.class_hist
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 2048, 2049, 70_001])
def test_class_hist(K, n):
    rng = np.random.default_rng(seed_of("class hist", n))
    counts = np.ones(n, np.int64)                                    # the bulk: the register path
    some = rng.random(n) < 0.2
    counts[some] = rng.integers(2, 300, int(some.sum()))
    counts = plant(counts, [0, -3, 254, 255, 256, 2**40, 254, 255, 256, 0, -2**40, 2**32, 2**63 - 1, 253], rng)
    if n == 1:
        counts[0] = 1
    out = torch.full((256,), 77, dtype=torch.int32, device="cuda")
    got = K.class_hist(dev(counts), out=out)
    assert got is out
    R.first_mismatch(host(out), R.class_hist_ref(counts), f"class_hist n={n}")
    # a second list into the same buffer: the buffer is cleared, not added to
    other = rng.permutation(counts)[:n // 2]
    K.class_hist(dev(other), out=out)
    R.first_mismatch(host(out), R.class_hist_ref(other), f"class_hist n={other.size}, second call into the same buffer")
    fresh = K.class_hist(dev(counts))
    assert fresh.dtype == torch.int32 and fresh.shape == (256,)
    R.first_mismatch(host(fresh), R.class_hist_ref(counts), f"class_hist n={n}, buffer of its own")
    if n >= 255:
        h = R.class_hist_ref(counts)
        assert h[0] >= 2 and h[254] >= 2 and h[255] >= 4 and h[1] > n // 2
