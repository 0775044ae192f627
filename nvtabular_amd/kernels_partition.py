"""Hash partitioning of rows by key on the device: the host driver of ``nvt_partition_*``
(include/nvt_hip.h), behind ``Dataset.shuffle_by_keys``.

``partition_plan`` hashes the key columns of one frame with ``nvt_join_hash`` (the join's key
canonicalisation: several columns, -0.0 == 0.0, nulls equal nulls), turns the tags into partition
ids (``nvt_partition_ids``) and sorts the row indices by id with a stable counting sort
(``nvt_partition_plan``).  ``shuffle_frames`` plans every input partition, reads the whole
[inputs, P] count matrix back ONCE, allocates the outputs and launches one segmented gather
(``nvt_partition_gather_many``) per output partition and batch of 16 columns: output partition p
holds the rows of input 0 with id p in their original order, then those of input 1, ... -- the
shuffle is stable.

Key columns go through the descriptors of ``kernels_join`` (not ``device.key_view``, which truncates
float keys to integers); a pending fill is materialised first.  A key that is a float column in any
input partition is hashed as a double in all of them, so an integer partition and a float partition
(pandas' int-with-null artefact) agree on the id of equal values.

List columns do not take the kernel path: the input partitions' list columns are concatenated
(offsets rebased) and each output partition is one ``DeviceFrame.take_rows`` over the planned row
order -- torch plumbing with two small reads per input partition and one host synchronisation per
output partition and list column.  The concatenation is a THIRD copy of the list columns (leaves,
offsets, bitmaps) next to the inputs and the outputs; it is dropped when the call returns.

Same conventions as kernels_join: launches under ``kernels.LAUNCH_LOCK`` on torch's current stream,
errors through ``_lib.check``, workspace from torch's allocator, one ``K.stat_add`` per launch."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check
from .kernels_join import key_descs, key_class

_WIDTHS = {torch.bool: 1, torch.uint8: 1, torch.int8: 1, torch.int16: 2, torch.float16: 2, torch.int32: 4, torch.float32: 4, torch.int64: 8,
           torch.float64: 8}


def _bitmap_bytes(m: int) -> int:
    return (m + 63) // 64 * 8


def _device_of(frames):
    for f in frames:
        for _, col in f.items():
            return col.data.device
    from .device import default_device

    return default_device()


def key_modes(frames, keys: Sequence[str]) -> tuple:
    """NVT_JOIN_INT / NVT_JOIN_FLOAT per key column, the same for every input partition."""
    modes = []
    for k in keys:
        classes = {key_class(f[k]) for f in frames}   # TypeError for a list column
        if "s" in classes and len(classes) > 1:
            raise TypeError(f"key column {k!r} holds strings in some partitions and numbers in others")
        modes.append(_lib.JOIN_FLOAT if "f" in classes else _lib.JOIN_INT)
    return tuple(modes)


def partition_ids(frame, keys: Sequence[str], P: int, modes: Optional[tuple] = None) -> torch.Tensor:
    """int32 tensor (uint32 values below P) with the partition of every row of ``frame``."""
    lib = _lib.load()
    n = len(frame)
    dev = _device_of([frame])
    nk = len(keys)
    modes = modes or key_modes([frame], keys)
    pid = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return pid
    with K.LAUNCH_LOCK:
        stream = K.stream_ptr()
        descs, alive = key_descs([frame[k] for k in keys], modes)
        tag = torch.empty(n, dtype=torch.int64, device=dev)
        nulls = torch.empty(n, dtype=torch.uint8, device=dev)
        words = torch.empty((nk, n), dtype=torch.int64, device=dev) if nk > 1 else None
        K.stat_add("join_hash")
        check(lib.nvt_join_hash(descs, nk, n, tag.data_ptr(), K.ptr(words), nulls.data_ptr(), stream),
              "nvt_join_hash")
        K.stat_add("partition_ids")
        check(lib.nvt_partition_ids(tag.data_ptr(), n, P, pid.data_ptr(), stream), "nvt_partition_ids")
        del alive
    return pid


def plan_from_ids(pid: torch.Tensor, P: int):
    """(perm int64[n], counts int64[P]) of ``nvt_partition_plan`` for the ids ``pid``."""
    lib = _lib.load()
    n = int(pid.numel())
    dev = pid.device
    perm = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return perm, torch.zeros(P, dtype=torch.int64, device=dev)
    counts = torch.empty(P, dtype=torch.int64, device=dev)
    need = C.c_uint64()
    check(lib.nvt_partition_plan_ws_bytes(n, P, C.byref(need)), "nvt_partition_plan_ws_bytes")
    with K.LAUNCH_LOCK:
        ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 16
        K.stat_add("partition_plan")
        check(lib.nvt_partition_plan(pid.data_ptr(), n, P, perm.data_ptr(), counts.data_ptr(),
                                     ws.data_ptr() + off, need.value, K.stream_ptr()), "nvt_partition_plan")
    return perm, counts


def partition_plan(frame, keys: Sequence[str], P: int, modes: Optional[tuple] = None):
    """(perm, counts) of one frame: ``perm`` lists the rows of partition 0 in row order, then those
    of partition 1, ...; ``counts`` (int64[P], on the device) the rows per partition."""
    _lib.require_gpu()
    keys = list(keys)
    if not 1 <= len(keys) <= _lib.JOIN_MAX_KEYS:
        raise NotImplementedError(f"1 to {_lib.JOIN_MAX_KEYS} key columns, got {len(keys)}")
    if not 1 <= P <= _lib.PARTITION_MAX:
        raise ValueError(f"P must be 1 to {_lib.PARTITION_MAX}, got {P}")
    return plan_from_ids(partition_ids(frame, keys, P, modes), P)


def _scalar_columns(frames, name):
    """The column in every input partition (fills applied, contiguous), its dtype and merged
    {surrogate -> str} dictionary."""
    cols = [f[name].materialize() for f in frames]
    dtypes = {c.dtype for c in cols}
    if len(dtypes) != 1:
        raise TypeError(f"column {name!r} has different dtypes across partitions: {sorted(map(str, dtypes))}")
    dtype = dtypes.pop()
    if dtype not in _WIDTHS:
        raise TypeError(f"unsupported column dtype {dtype} ({name!r})")
    return cols, dtype, _merge_strings(cols)


def _merge_strings(cols):
    luts = [c.strings for c in cols if c.strings is not None]
    if not luts:
        return None
    merged = luts[0]
    for lut in luts[1:]:
        if lut is not merged:
            merged = {**merged, **lut}
    return merged


def _shuffle_list_column(name, frames, perms, cnt, off, P):
    """A list column of every output partition: concatenate the inputs (offsets rebased), then one
    ``take_rows`` per output partition in the planned row order.  A null list row is what the ingest
    makes of it: a row of length 0.  Holds one extra copy of the column while it runs."""
    from .device import DeviceColumn, DeviceFrame

    cols = [f[name].materialize() for f in frames]
    dev = cols[0].data.device
    strings = _merge_strings(cols)
    with_valid = any(c.valid is not None for c in cols)
    leaves, bits, offs, row_base = [], [], [torch.zeros(1, dtype=torch.int64, device=dev)], []
    leaf_base = rows = 0
    for c in cols:
        o = c.offsets
        lo, hi = (int(o[0]), int(o[-1])) if len(c) else (0, 0)   # the leaves the rows name
        leaves.append(c.data[lo:hi])
        if with_valid:
            bits.append(K.unpack_bitmap(c.valid, int(c.data.numel()))[lo:hi] if c.valid is not None
                        else torch.ones(hi - lo, dtype=torch.bool, device=dev))
        offs.append(o[1:] - lo + leaf_base)
        leaf_base += hi - lo
        row_base.append(rows)
        rows += len(c)
    valid = None
    if with_valid:
        from .device import pack_bitmap_device

        valid = pack_bitmap_device(torch.cat(bits))
    leaves = torch.cat(leaves)
    big = DeviceFrame({name: DeviceColumn(leaves, valid, torch.cat(offs), None, strings,
                                            logical=cols[0].logical)})
    out = []
    for p in range(P):
        index = torch.cat([perms[i][int(off[i, p]): int(off[i, p] + cnt[i, p])] + row_base[i]
                           for i in range(len(frames))])
        out.append(big.take_rows(index)[name])
    return out


def shuffle_frames(frames, keys: Sequence[str], P: int) -> List:
    """``frames`` (DeviceFrames with the same columns) -> P DeviceFrames: every row goes to the
    partition its key hashes to, in input order.  All inputs and all outputs are resident at once."""
    from .device import DeviceColumn, DeviceFrame

    _lib.require_gpu()
    frames = list(frames)
    keys = list(keys)
    if not frames:
        raise ValueError("shuffle_frames needs at least one input partition")
    if not 1 <= len(keys) <= _lib.JOIN_MAX_KEYS:
        raise NotImplementedError(f"1 to {_lib.JOIN_MAX_KEYS} key columns, got {len(keys)}")
    if not 1 <= P <= _lib.PARTITION_MAX:
        raise ValueError(f"P must be 1 to {_lib.PARTITION_MAX}, got {P}")
    names = frames[0].columns
    for f in frames:
        if f.columns != names:
            raise ValueError("the input partitions have different columns")
    modes = key_modes(frames, keys)
    lib = _lib.load()
    dev = _device_of(frames)
    I = len(frames)
    with K.annotate("shuffle_by_keys"), K.LAUNCH_LOCK:
        plans = [partition_plan(f, keys, P, modes) for f in frames]
        perms = [p for p, _ in plans]
        cnt = K.read_back(torch.stack([c for _, c in plans])).astype(np.int64)   # [I, P]: the one read-back
        off = np.zeros((I, P), dtype=np.int64)
        np.cumsum(cnt[:, :-1], axis=1, out=off[:, 1:])
        m = cnt.sum(axis=0)

        scalar = [n for n in names if not frames[0][n].is_list]
        lists = [n for n in names if frames[0][n].is_list]
        src = {n: _scalar_columns(frames, n) for n in scalar}
        data = {n: [c.data.contiguous() for c in src[n][0]] for n in scalar}   # (kept alive to the end)
        for n in scalar:
            for c in src[n][0]:
                if c.is_list:
                    raise TypeError(f"column {n!r} is a list column in some partitions only")

        # the device tables of every launch in one upload: per output partition its segments
        # {idx, start}, then per column the source pointers and (where any segment has one) bitmaps
        segs_of = [[i for i in range(I) if cnt[i, p] > 0] for p in range(P)]
        if max((len(s) for s in segs_of), default=0) > _lib.PARTITION_MAX_SEGS:
            raise NotImplementedError(f"more than {_lib.PARTITION_MAX_SEGS} input partitions feed one output")
        words: List[int] = []
        seg_at, src_at, valid_at = {}, {}, {}
        for p in range(P):
            ins = segs_of[p]
            if not ins:
                continue
            seg_at[p] = len(words)
            start = 0
            for i in ins:
                words += [perms[i].data_ptr() + 8 * int(off[i, p]), start]
                start += int(cnt[i, p])
            for n in scalar:
                src_at[p, n] = len(words)
                words += [data[n][i].data_ptr() for i in ins]
                if any(src[n][0][i].valid is not None for i in ins):
                    valid_at[p, n] = len(words)
                    words += [K.ptr(src[n][0][i].valid) or 0 for i in ins]
        table = torch.from_numpy(np.array(words or [0], dtype=np.uint64).view(np.int64)).to(dev)
        base = table.data_ptr()
        stream = K.stream_ptr()

        out = [dict() for _ in range(P)]
        for p in range(P):
            mp = int(m[p])
            jobs = []
            for n in scalar:
                cols, dtype, strings = src[n]
                dst = torch.empty(mp, dtype=dtype, device=dev)
                dst_valid = None
                if (p, n) in valid_at:
                    dst_valid = torch.empty(_bitmap_bytes(mp), dtype=torch.uint8, device=dev)
                out[p][n] = DeviceColumn(dst, dst_valid, None, None, strings, logical=cols[0].logical)
                if mp:
                    jobs.append((n, dst, dst_valid))
            for j0 in range(0, len(jobs), _lib.PARTITION_MAX_COLS):
                batch = jobs[j0: j0 + _lib.PARTITION_MAX_COLS]
                descs = (_lib.PartitionCol * len(batch))()
                for d, (n, dst, dst_valid) in zip(descs, batch):
                    d.src = base + 8 * src_at[p, n]
                    d.src_valid = base + 8 * valid_at[p, n] if (p, n) in valid_at else None
                    d.dst = dst.data_ptr()
                    d.dst_valid = K.ptr(dst_valid)
                    d.width = _WIDTHS[dst.dtype]
                K.stat_add("partition_gather")
                check(lib.nvt_partition_gather_many(descs, len(batch), base + 8 * seg_at[p], len(segs_of[p]), mp,
                                                    stream), "nvt_partition_gather_many")
        for n in lists:
            for p, col in enumerate(_shuffle_list_column(n, frames, perms, cnt, off, P)):
                out[p][n] = col
        del data, table
    return [DeviceFrame({n: out[p][n] for n in names}) for p in range(P)]
