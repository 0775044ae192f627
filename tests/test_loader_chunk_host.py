"""The host bookkeeping of the chunk-wide shuffle, without a GPU: ``src_begin`` from the partition
lengths, and the documented order model -- partition order from the host generator, ONE draw per
chunk -- run on the CPU generator (the device's draws differ, the structure does not)."""
import numpy as np
import pytest
import torch

from nvtabular_amd import _lib
from nvtabular_amd import kernels_loader as KD
from nvtabular_amd.loader.torch import epoch_row_order, partition_order


def test_src_begin():
    assert KD.src_begin([3]) == [0, 3]
    assert KD.src_begin([1, 255, 256, 257, 0, 1000]) == [0, 1, 256, 512, 769, 769, 1769]
    assert KD.src_begin([0, 5, 0, 0, 2, 0]) == [0, 0, 5, 5, 5, 7, 7]        # empty first, inside, last
    assert KD.src_begin([0, 0]) == [0, 0, 0]
    assert KD.src_begin([]) == [0]
    big = KD.src_begin([1 << 31, 1 << 31, 5])
    assert big == [0, 1 << 31, 1 << 32, (1 << 32) + 5]
    with pytest.raises(ValueError):
        KD.src_begin([4, -1])


def test_src_begin_finds_the_source_of_every_row():
    """The search the kernel makes -- the last s with src_begin[s] <= i -- steps over empty sources."""
    lengths = [0, 3, 0, 0, 2, 1, 0]
    begin = np.array(KD.src_begin(lengths))
    want = np.repeat(np.arange(len(lengths)), lengths)
    for i in range(begin[-1]):
        s = np.searchsorted(begin[:-1], i, side="right") - 1
        assert s == want[i] and 0 <= i - begin[s] < lengths[s]


def test_too_many_sources_are_refused_by_name():
    frames = [None] * (_lib.TAKE_MAX_SOURCES + 1)
    for call in (lambda: KD.take_frames(frames, None, []), lambda: KD.take_lists_multi(frames, [], None)):
        with pytest.raises(ValueError, match=str(_lib.TAKE_MAX_SOURCES)):
            call()
    with pytest.raises(ValueError, match="at least one"):
        KD.take_frames([], None, [])


def test_partition_order_is_the_host_generator():
    parts = [0, 2, 4, 6, 8]
    g = torch.Generator()
    g.manual_seed(99)
    want = [parts[i] for i in torch.randperm(5, generator=g).tolist()]
    assert partition_order(parts, 99) == want
    assert partition_order(parts, 99) == want
    assert sorted(partition_order(parts, 100)) == parts
    assert partition_order([], 1) == []


@pytest.mark.parametrize("ppc", [1, 2, 3, 5])
def test_order_model_draws_once_per_chunk(monkeypatch, ppc):
    lengths = [40, 0, 25, 31, 0, 17, 8]           # partitions 1 and 4 are empty
    parts = list(range(len(lengths)))
    draws = []
    real = torch.randperm

    def counted(n, *a, **kw):
        draws.append((int(n), "device" in kw))
        return real(n, *a, **kw)

    monkeypatch.setattr(torch, "randperm", counted)
    rows = epoch_row_order(lengths, parts, 7, ppc, "cpu").numpy()
    monkeypatch.undo()
    live = [p for p in partition_order(parts, 7) if lengths[p]]
    chunks = [live[k:k + ppc] for k in range(0, len(live), ppc)]
    # the first draw is the partition order (host generator), then ONE per chunk, sized to the chunk
    assert draws[0] == (len(parts), False)
    assert draws[1:] == [(sum(lengths[p] for p in c), True) for c in chunks]
    # every chunk's stretch of the epoch is a permutation of exactly that chunk's rows
    at = 0
    for c in chunks:
        n = sum(lengths[p] for p in c)
        got = sorted(map(tuple, rows[at:at + n]))
        assert got == sorted((p, r) for p in c for r in range(lengths[p]))
        at += n
    assert at == len(rows) == sum(lengths)
    # the draws are the generator's: the same seed repeats, the chunk draw numbers the rows in chunk order
    g = torch.Generator()
    g.manual_seed(7)
    first = chunks[0]
    base = np.array([(p, r) for p in first for r in range(lengths[p])])
    np.testing.assert_array_equal(rows[:len(base)], base[torch.randperm(len(base), generator=g).numpy()])
    np.testing.assert_array_equal(epoch_row_order(lengths, parts, 7, ppc, "cpu").numpy(), rows)
    assert (epoch_row_order(lengths, parts, 8, ppc, "cpu").numpy() != rows).any()
