"""numpy restatement of the contract of nvt_key_labels (include/nvt_hip.h), pinned against
``pandas.factorize`` by test_hive_reference.py and compared bit for bit with the kernel by
test_gpu_key_labels_kernels.py.

Two rows have the same key when their tags are equal; with one key component a row with a null bit
belongs to the null key whatever its tag.  Labels are ranks of the keys in first-appearance order."""
import numpy as np

LABEL_MAX = 4096


def key_labels(tags, nulls, words=None, nkeys=1):
    """-> (label uint32[n], first_row uint32[D], D, status).  status 1: more than LABEL_MAX keys
    (labels and first rows are then not defined: None); status 2: nkeys >= 2 and two rows with equal
    tags whose words or null bits differ."""
    tags = np.asarray(tags).astype(np.uint64, copy=False)
    nulls = np.asarray(nulls, dtype=np.uint8)
    n = len(tags)
    seen, first, label = {}, [], np.zeros(n, dtype=np.uint32)
    for i in range(n):
        key = "null" if (nkeys == 1 and nulls[i]) else int(tags[i])
        l = seen.get(key)
        if l is None:
            l = seen[key] = len(first)
            first.append(i)
        label[i] = l
    D = len(first)
    if D > LABEL_MAX:
        return None, None, D, 1
    first = np.asarray(first, dtype=np.uint32)
    status = 0
    if nkeys >= 2 and n:
        words = np.asarray(words).reshape(nkeys, n)
        fr = first[label]
        if (nulls != nulls[fr]).any() or (words != words[:, fr]).any():
            status = 2
    return label, first, D, status


def key_labels_fast(tags, nulls, nkeys=1):
    """The same labels for large inputs (np.unique instead of a Python loop); no collision check."""
    tags = np.asarray(tags).astype(np.uint64, copy=False)
    nulls = np.asarray(nulls, dtype=np.uint8)
    is_null = (nulls != 0) if nkeys == 1 else np.zeros(len(tags), dtype=bool)
    _, first_of, inv = np.unique(np.stack([np.where(is_null, 0, tags), is_null.astype(np.uint64)]), axis=1,
                                 return_index=True, return_inverse=True)
    order = np.argsort(first_of, kind="stable")
    rank = np.empty(len(order), dtype=np.uint32)
    rank[order] = np.arange(len(order), dtype=np.uint32)
    D = len(order)
    if D > LABEL_MAX:
        return None, None, D, 1
    return rank[np.ravel(inv)], first_of[order].astype(np.uint32), D, 0
