"""Plain numpy references of Categorify's ordering step -- the (count descending, key ascending)
order of a (key, count) list, the class histogram the one-pass ordering reads, and the labels the
ordered vocabulary gives its keys -- for the kernel-level tests of csrc/nvt_sort.hip,
nvt_vocab_order.hip and the nvt_vocab_finalize_many driver of nvt_finalize.hip
(test_gpu_order_kernels.py).  test_order_reference.py pins them to pandas on the CPU.  Nothing here
shares code with the device side: the order is ``np.lexsort``, the labels ``np.unique`` +
``searchsorted``.
"""
import numpy as np

from count_reference import n_big_ref, vocab_order_ref  # noqa: F401  (re-exported for the tests)
from encode_reference import first_mismatch  # noqa: F401


def class_hist_ref(counts) -> np.ndarray:
    """int32[256] histogram of min(max(count, 0), 255): what nvt_class_hist writes (a negative count,
    which no counting pass produces, lands in class 0; 255 holds every count at or above it)."""
    c = np.asarray(counts).astype(np.int64)
    return np.bincount(np.clip(c, 0, 255), minlength=256).astype(np.int32)


def positions_ref(keys, counts) -> np.ndarray:
    """int32[n]: the position of every entry of the list in its (count descending, key ascending)
    order -- what a multi-GPU fit hands over as ``src_labels``."""
    keys, counts = np.asarray(keys), np.asarray(counts)
    order = np.lexsort((keys, -counts.astype(np.int64)))
    pos = np.empty(keys.size, np.int32)
    pos[order] = np.arange(keys.size, dtype=np.int32)
    return pos


def labels_ref(keys, vk, first_label) -> np.ndarray:
    """int64 label of every key of ``keys``: ``first_label`` + its position in the ordered,
    duplicate-free vocabulary ``vk``; -1 for a key that is not in it.  The smallest integer of the
    key type is a key like any other: -1 when the vocabulary does not hold it."""
    keys = np.asarray(keys).astype(np.int64)
    vk = np.asarray(vk).astype(np.int64)
    out = np.full(keys.size, -1, np.int64)
    if vk.size == 0 or keys.size == 0:
        return out
    uniq, pos = np.unique(vk, return_index=True)
    assert uniq.size == vk.size, "labels_ref: the vocabulary holds a key twice"
    at = np.minimum(np.searchsorted(uniq, keys), uniq.size - 1)
    found = uniq[at] == keys
    out[found] = int(first_label) + pos[at[found]].astype(np.int64)
    return out
