"""The batched small sort of nvt_vocab_finalize_many (csrc/nvt_sort.hip: vocab_sort_small_batch) against
``numpy.lexsort``: unsorted int32 vocabularies of 2 .. 16384 entries with counts below 2^32.

  launch A   sort_small_chunk_kernel: one workgroup per chunk of at most 2048 packed words; a list of one
             chunk is finished by it
  launch B   sort_small_rank_kernel: one thread per element of a longer list, whose rank is its index in
             its own sorted chunk + a binary search in every other chunk; equal words are ordered by chunk
  no scratch sort_small_packed_many_kernel: a list above 2048 entries whose descriptor has no sort_tmp

Lengths: 2 and 3 (a chunk padded to two and four words), 2047 / 2048 / 2049 (one chunk, one full chunk,
a second chunk of ONE entry), 4097 (three chunks), 16383 / 16384 (eight chunks, the last one short or
full).  The order asked for is "count descending, key ascending", i.e. the packed word ascending.
Everything is exact."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LO, HI = np.iinfo(np.int32).min, np.iinfo(np.int32).max
CHUNK, SMALL_MAX, SMALL_BATCH = 2048, 16384, 64      # kSmallChunk, kSmallPackedMax, kSmallBatch
LENGTHS = [2, 3, 2047, 2048, 2049, 4097, 16383, 16384]


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def distinct_keys(n, rng):
    """n distinct int32 keys in random order, both ends of the type among them."""
    k = np.unique(rng.integers(LO + 1, HI, int(n * 1.1) + 16))
    k = np.concatenate([[LO, HI][:n], rng.permutation(k)[:max(0, n - 2)]])
    assert np.unique(k).size == n
    return rng.permutation(k).astype(np.int32)


def sort_lists(K, lists, scratch=True, unique=True):
    """One nvt_vocab_finalize_many call over (keys, counts) lists -> [(keys, counts)] as it left them,
    and the vocab_sort_small scopes it opened."""
    from nvtabular_amd import _lib

    descs = (_lib.VocabCol * len(lists))()
    held = []
    for d, (keys, counts) in zip(descs, lists):
        dk, dc = dev(keys), dev(counts)
        tab = K.EncodeTable(dk, 3, unique=unique, defer_build=True)
        tab.fill_vocab_desc(d, dc, int(counts.max()))
        # the descriptor is the small sort's: no event, scratch only for a list of several chunks
        assert not tab.pending and (d.sort_tmp is not None) == (keys.size > CHUNK), keys.size
        if not scratch:
            d.sort_tmp = None
        held.append((tab, dk, dc))
    torch.cuda.synchronize()
    K.profile_begin()
    K.check(_lib.load().nvt_vocab_finalize_many(descs, len(lists), K.stream_ptr()), "nvt_vocab_finalize_many")
    scopes = {k: v[1] for k, v in K.profile_end().items()}
    torch.cuda.synchronize()
    assert "vocab_sort" not in scopes, scopes
    return [(dk.cpu().numpy(), dc.cpu().numpy()) for _, dk, dc in held], scopes.get("vocab_sort_small", 0)


def check_sorted(got, lists, what):
    for j, ((gk, gc), (keys, counts)) in enumerate(zip(got, lists)):
        order = np.lexsort((keys, -counts))
        np.testing.assert_array_equal(gk, keys[order], err_msg=f"{what}: keys of list {j}, n={keys.size}")
        np.testing.assert_array_equal(gc, counts[order], err_msg=f"{what}: counts of list {j}, n={keys.size}")


def count_kinds(n, rng):
    top = 2**32 - 1
    near = top - rng.integers(0, 3, n).astype(np.int64)          # ties right under the largest 32-bit count
    near[rng.integers(0, n)] = top
    mixed = np.floor(np.exp(rng.random(n) * np.log(float(top)))).astype(np.int64).clip(1, top)
    mixed[rng.random(n) < 0.5] = mixed[rng.integers(0, n)]        # half of the list tied on one count
    return [("all counts equal", np.full(n, 7, np.int64)), ("counts near 2^32 - 1", near),
            ("log-uniform with ties", mixed)]


@pytest.mark.parametrize("n", LENGTHS)
def test_chunk_edges(K, n):
    rng = np.random.default_rng(seed_of("small sort", n))
    lists = [(distinct_keys(n, rng), c) for _, c in count_kinds(n, rng)]
    got, scopes = sort_lists(K, lists)
    assert scopes == 1
    check_sorted(got, lists, f"n={n}: " + " | ".join(w for w, _ in count_kinds(2, rng)))


@pytest.mark.parametrize("n", [3, 2049, 4097, 16384])
def test_repeated_pairs(K, n):
    """Equal (key, count) pairs, more of them than a chunk holds: the ranks stay a permutation (equal
    words are ordered by chunk, then by their index in the chunk), so every pair comes out as often
    as it went in."""
    rng = np.random.default_rng(seed_of("repeated", n))
    keys = rng.integers(-3, 3, n).astype(np.int32)
    counts = rng.integers(1, 3, n).astype(np.int64)
    keys[:2], counts[:2] = [LO, LO], [2, 2]
    lists = [(keys, counts), (np.full(n, 5, np.int32), np.full(n, 9, np.int64))]
    got, _ = sort_lists(K, lists, unique=False)
    check_sorted(got, lists, f"repeated pairs n={n}")


def test_more_lists_than_one_launch_takes(K):
    """kSmallBatch + 1 lists of mixed lengths: two batches, every list as numpy orders it alone."""
    rng = np.random.default_rng(seed_of("sixty-five"))
    sizes = LENGTHS + rng.integers(2, 6000, SMALL_BATCH + 1 - len(LENGTHS)).tolist()
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    assert len(sizes) == SMALL_BATCH + 1
    lists = [(distinct_keys(n, rng), rng.integers(1, 50, n).astype(np.int64)) for n in sizes]
    got, scopes = sort_lists(K, lists)
    assert scopes == 2
    check_sorted(got, lists, "65 lists")


def test_a_call_without_scratch(K):
    """No sort_tmp in the descriptors: lists of several chunks are sorted by one workgroup each, lists
    of one chunk as ever; the result is the same."""
    rng = np.random.default_rng(seed_of("no scratch"))
    lists = [(distinct_keys(n, rng), rng.integers(1, 300, n).astype(np.int64)) for n in (2049, 7, 16384, 2048, 9000)]
    got, scopes = sort_lists(K, lists, scratch=False)
    assert scopes == 1
    check_sorted(got, lists, "without scratch")
