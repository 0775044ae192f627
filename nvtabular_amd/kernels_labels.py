"""Dense labels of a low-cardinality key on the device: the host driver of ``nvt_key_labels``
(include/nvt_hip.h), behind ``Dataset.to_parquet(partition_on=...)``.

``key_labels`` hashes the key columns of one frame with ``nvt_join_hash`` (through
``kernels_join.key_descs``, the way ``kernels_partition.partition_ids`` does) and labels every row with
the rank of its key tuple in first-appearance order.  ``split_plan`` adds the stable counting sort of
``kernels_partition.plan_from_ids``: rows of label 0 in row order, then those of label 1, ...

Read-backs: ``key_labels`` makes ONE (the two state words and ``first_row`` in one block);
``split_plan`` makes no further one -- ``counts`` stays on the device for the caller to bring over
together with whatever else it needs (hive.HiveSplitter: the key values at the first rows).  A split
of one input partition is two read-backs.

Same conventions as kernels_partition: launches under ``kernels.LAUNCH_LOCK`` on torch's current
stream, errors through ``_lib.check``, workspace from torch's allocator, one ``K.stat_add`` per
launch."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_join import key_descs
from .kernels_partition import _device_of, key_modes, plan_from_ids

_NARROW = (torch.int8, torch.int16)


def _key_column(col):
    """int8 / int16 keys are widened: nvt_join_hash reads int32, int64 and uint8."""
    col = col.materialize()
    return col.like(col.data.to(torch.int64), col.valid) if col.data.dtype in _NARROW else col


def labels_from_tags(tag, nulls, words, nkeys: int, keys=()):
    """``nvt_key_labels`` on the outputs of ``nvt_join_hash`` -> (label int32[n] on the device, D,
    first rows as a host array).  One read-back."""
    lib = _lib.load()
    n = int(tag.numel())
    dev = tag.device
    label = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return label, 0, np.zeros(0, dtype=np.int64)
    need = C.c_uint64()
    check(lib.nvt_key_labels_ws_bytes(n, C.byref(need)), "nvt_key_labels_ws_bytes")
    with K.LAUNCH_LOCK:
        # one block for the read-back: state[0 .. 2) as uint64, then first_row as uint32[LABEL_MAX]
        out = torch.zeros(2 + _lib.LABEL_MAX // 2, dtype=torch.int64, device=dev)
        ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 16
        K.stat_add("key_labels")
        check(lib.nvt_key_labels(tag.data_ptr(), nulls.data_ptr(), K.ptr(words), nkeys, n, label.data_ptr(),
                                 out.data_ptr() + 16, out.data_ptr(), ws.data_ptr() + off, need.value,
                                 K.stream_ptr()), "nvt_key_labels")
        K.stat_add("key_labels_readback")
        host = K.read_back(out)
    D, status = int(host[0]), int(host[1])
    if status == 1:
        raise ValueError(f"more than {_lib.LABEL_MAX} distinct values of the key columns {list(keys)} in one "
                         f"partition of {n} rows (the limit of nvt_key_labels)")
    if status == 2:
        raise ValueError(f"key columns {list(keys)}: two different key tuples share a 64-bit fingerprint")
    first = host[2:].view(np.uint32)[:D].astype(np.int64)
    return label, D, first


def key_labels(frame, keys: Sequence[str], modes: Optional[tuple] = None):
    """(label int32[n] on the device, D, first_rows as a host array): ``label[i]`` is the rank of row
    i's key tuple among the D distinct tuples of ``frame`` in first-appearance order, ``first_rows[l]``
    the first row of tuple l.  Nulls equal nulls.  More than 4096 distinct tuples: ValueError."""
    _lib.require_gpu()
    lib = _lib.load()
    keys = list(keys)
    if not 1 <= len(keys) <= _lib.JOIN_MAX_KEYS:
        raise NotImplementedError(f"1 to {_lib.JOIN_MAX_KEYS} key columns, got {len(keys)}")
    n = len(frame)
    dev = _device_of([frame])
    nk = len(keys)
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), 0, np.zeros(0, dtype=np.int64)
    cols = [_key_column(frame[k]) for k in keys]
    modes = modes or key_modes([frame], keys)
    with K.LAUNCH_LOCK:
        descs, alive = key_descs(cols, modes)
        tag = torch.empty(n, dtype=torch.int64, device=dev)
        nulls = torch.empty(n, dtype=torch.uint8, device=dev)
        words = torch.empty((nk, n), dtype=torch.int64, device=dev) if nk > 1 else None
        K.stat_add("join_hash")
        check(lib.nvt_join_hash(descs, nk, n, tag.data_ptr(), K.ptr(words), nulls.data_ptr(), K.stream_ptr()),
              "nvt_join_hash")
        out = labels_from_tags(tag, nulls, words, nk, keys)
        del alive
    return out


def split_plan(frame, keys: Sequence[str]):
    """(perm int64[n], counts int64[D] on the device, first_rows on the host): ``perm`` lists the rows
    of key tuple 0 in row order, then those of tuple 1, ... (tuples in first-appearance order)."""
    label, D, first = key_labels(frame, keys)
    if D == 0:
        return torch.empty(0, dtype=torch.int64, device=label.device), torch.zeros(0, dtype=torch.int64,
                                                                                     device=label.device), first
    perm, counts = plan_from_ids(label, D)
    return perm, counts, first
