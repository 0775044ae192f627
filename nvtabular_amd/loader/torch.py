"""``TorchAsyncItr``: the batches of a Dataset as device tensors, on the batch-gather kernels.

One chunk (``parts_per_chunk`` partitions) at a time is gathered -- shuffled, cast and laid out -- by
``kernels_loader.take_frames`` into buffers allocated for that chunk, and the batches handed out are
views of those buffers.  Nothing is copied per batch."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional

import torch
import torch.utils.data

from .. import kernels_list as KL
from .. import kernels_loader as KD
from ..device import DeviceColumn, DeviceFrame, as_device_frame
from ..schema import Tags
from .backend import _augment_schema


def partition_order(parts: List[int], seed: int) -> List[int]:
    """The epoch's order of the partitions ``parts``: ``torch.randperm`` of a host generator."""
    host_gen = torch.Generator()
    host_gen.manual_seed(int(seed))
    return [parts[i] for i in torch.randperm(len(parts), generator=host_gen).tolist()]


def epoch_row_order(lengths: List[int], parts: List[int], seed: int, parts_per_chunk: int, device) -> torch.Tensor:
    """The order contract of ``shuffle=True`` as code: the rows of an epoch over an in-memory dataset,
    as ``(partition, row in partition)`` pairs, int64 ``[rows, 2]`` on ``device``.  ``lengths[p]``:
    rows of partition p; ``parts``: this rank's partitions.  The loader does not run this -- it
    gathers with the same draws -- the tests hold the two against each other."""
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    live = [p for p in partition_order(list(parts), seed) if lengths[p] > 0]
    out = [torch.empty((0, 2), dtype=torch.int64, device=device)]
    for k in range(0, len(live), parts_per_chunk):
        chunk = live[k:k + parts_per_chunk]
        rows = torch.cat([torch.stack([torch.full((lengths[p],), p, dtype=torch.int64, device=device),
                                       torch.arange(lengths[p], device=device)], dim=1) for p in chunk])
        out.append(rows[torch.randperm(len(rows), device=device, generator=gen)])     # the chunk's one draw
    return torch.cat(out)


class TorchAsyncItr(torch.utils.data.IterableDataset):
    """Batches of ``dataset`` as torch tensors on the device, every batch exactly ``batch_size`` rows
    except possibly the last: the tail of a chunk that is shorter than a batch spills over into the
    next chunk, where it comes first and is not shuffled again.

    Parameters follow the reference (``cats`` / ``conts`` / ``labels``: column names, taken from the
    schema's CATEGORICAL / CONTINUOUS / TARGET tags when None; ``shuffle``; ``seed_fn``;
    ``parts_per_chunk``; ``global_size`` / ``global_rank``; ``drop_last``; ``sparse_names``,
    ``sparse_max``, ``sparse_as_dense``), plus ``stacked``:

    * ``stacked=False``: ``x[name]`` is a contiguous 1-D tensor in the column's own dtype; a list
      column gives ``x[name + "__values"]`` and ``x[name + "__offsets"]`` (int64, B + 1 entries from
      0), or with ``sparse_as_dense`` a ``[B, sparse_max[name]]`` matrix, truncated and padded with 0.
    * ``stacked=True``: ``x["cats"]`` is int64 ``[B, ncat]`` and ``x["conts"]`` float32
      ``[B, ncont]``, columns in the order given; lists as above.
    * ``y``: None without labels, float32 ``[B]`` for one label, ``[B, nlab]`` for several.

    A null row gives 0 in an integer tensor and NaN in a float tensor.  String columns raise
    ``TypeError``: Categorify them first.

    ``shuffle=True`` permutes the order of the partitions and then the rows of every CHUNK as a
    whole: the ``parts_per_chunk`` partitions of a chunk are shuffled together, so more partitions
    per chunk give better mixed batches.  The order is a contract (``epoch_row_order`` states it as
    code): the partition order is ``torch.randperm`` of a host generator seeded with ``seed_fn()``
    (a random seed when None); a device generator gets the same seed and every chunk, in chunk
    order, makes ONE draw ``torch.randperm(rows of the chunk's partitions)`` that numbers those rows
    in the order the chunk holds its partitions (empty partitions are skipped before chunks are
    formed).  The spill rows of the previous chunk stay in front as they are.  A streamed source
    (parquet files, a transformed dataset) keeps its partition order: ``Dataset.to_iter`` is a
    forward iterator.

    Despite the name nothing here is asynchronous to the caller: every launch goes on the current
    stream, the loader starts no thread and no second stream, and the only overlap is the prefetch of
    ``Dataset.to_iter``.  A buffer is allocated per chunk and never written again, so a batch the
    caller keeps stays valid.  There is no CPU path: ``device="cpu"`` raises ``ValueError``."""

    def __init__(self, dataset, cats=None, conts=None, labels=None, batch_size=1, shuffle=False, seed_fn=None,
                 parts_per_chunk=1, device=None, global_size=None, global_rank=None, drop_last=False,
                 sparse_names=None, sparse_max=None, sparse_as_dense=False, stacked=False):
        if device is not None and torch.device(device if not isinstance(device, int) else f"cuda:{device}").type != "cuda":
            raise ValueError("TorchAsyncItr runs on the GPU only: there is no CPU path in this package")
        labels = [labels] if isinstance(labels, str) else labels
        seen: Dict[str, str] = {}
        for role, names in (("cats", cats), ("conts", conts), ("labels", labels)):
            for name in names or []:
                if name in seen:
                    raise ValueError(f"column '{name}' is given as {seen[name]} and as {role}")
                seen[name] = role
        schema = _augment_schema(dataset.schema, cats, conts, labels, sparse_names, sparse_max, sparse_as_dense)
        dataset._schema = schema
        self.dataset = dataset
        self.schema = schema

        def role(names, tag):
            return list(names) if names is not None else schema.select_by_tag(tag).column_names

        if cats is None and conts is None and labels is None:
            self.cat_names, self.cont_names, self.label_names = (
                role(None, Tags.CATEGORICAL), role(None, Tags.CONTINUOUS), role(None, Tags.TARGET))
            dup = [n for n in self.cat_names + self.cont_names
                   if (n in self.cat_names) + (n in self.cont_names) + (n in self.label_names) > 1]
            if dup:
                raise ValueError(f"columns tagged with two roles: {sorted(set(dup))}")
        else:
            self.cat_names, self.cont_names, self.label_names = list(cats or []), list(conts or []), list(labels or [])
        if not (self.cat_names or self.cont_names or self.label_names):
            raise ValueError("no columns: name cats / conts / labels or tag the dataset's schema")
        if int(batch_size) < 1 or int(parts_per_chunk) < 1:
            raise ValueError("batch_size and parts_per_chunk must be positive")
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.seed_fn = seed_fn
        self.parts_per_chunk = int(parts_per_chunk)
        self.device = device
        self.global_size = int(global_size or 1)
        self.global_rank = int(global_rank or 0)
        if not 0 <= self.global_rank < self.global_size:
            raise ValueError("global_rank must be in [0, global_size)")
        self.drop_last = bool(drop_last)
        self.sparse_names = list(sparse_names or [])
        self.sparse_max = dict(sparse_max or {})
        self.sparse_as_dense = bool(sparse_as_dense)
        if self.sparse_as_dense:
            for name in self.sparse_names:
                if name not in self.sparse_max:
                    raise ValueError(f"sparse_as_dense needs sparse_max['{name}']")
        self.stacked = bool(stacked)
        self._rows = None
        self._stop = False

    # ---- rows of this rank -------------------------------------------------------------------------
    @property
    def _columns(self) -> List[str]:
        return self.cat_names + self.cont_names + self.label_names

    def _my_parts(self) -> List[int]:
        return [i for i in range(self.dataset.npartitions) if i % self.global_size == self.global_rank]

    def _num_rows(self) -> int:
        if self._rows is None:
            ds = self.dataset
            if getattr(ds, "_filter", None) is not None:
                # Dataset(filters=...): neither the frames' lengths nor the footers know the rows that pass
                rows = sum(len(p) for p in self._partitions(None))
            elif getattr(ds, "_frames", None) is not None:
                rows = 0
                for i in self._my_parts():
                    f = ds._frames[i]
                    rows += f.num_rows if hasattr(f, "num_rows") else len(f)
            elif getattr(ds, "_pieces", None) is not None:
                import pyarrow.parquet as pq

                rows = 0
                for i in self._my_parts():
                    path, groups = ds._pieces[i]
                    md = pq.ParquetFile(path).metadata
                    rows += sum(md.row_group(g).num_rows for g in groups)
            else:
                rows = sum(len(p) for p in self._partitions(None))
            self._rows = rows
        return self._rows

    def __len__(self):
        n = self._num_rows() / self.batch_size
        return int(math.floor(n) if self.drop_last else math.ceil(n))

    def stop(self):
        """End the running epoch after the current batch."""
        self._stop = True

    def _partitions(self, order):
        ds = self.dataset
        cols = self._columns
        if getattr(ds, "_frames", None) is not None:
            for i in (order if order is not None else self._my_parts()):
                frame, _ = as_device_frame(ds._frames[i])
                if getattr(ds, "_filter", None) is not None:
                    frame = ds._filter_frame(frame)
                yield frame[[c for c in cols if c in frame]]
            return
        shard = (self.global_rank, self.global_size) if self.global_size > 1 else None
        yield from ds.to_iter(columns=cols, shard=shard)

    # ---- one chunk -----------------------------------------------------------------------------------
    def _layout(self, frame):
        """Which tensor every column goes to: decided on the first partition."""
        for name in self._columns:
            if name not in frame:
                raise ValueError(f"column '{name}' is not in the dataset")
            if frame[name].strings is not None:
                raise TypeError(f"column '{name}' holds strings: Categorify it before it reaches the dataloader")
        self._lists = [n for n in self.cat_names + self.cont_names if frame[n].is_list]
        self._scalar_cats = [n for n in self.cat_names if n not in self._lists]
        self._scalar_conts = [n for n in self.cont_names if n not in self._lists]
        for n in self.label_names:
            if frame[n].is_list:
                raise TypeError(f"label column '{n}' is a list column")

    def _gather(self, frames, spill, gen):
        """The chunk's buffers: the spill rows as they are, then the rows of all partitions of the
        chunk under ONE permutation."""
        dev = frames[0][self._columns[0]].data.device
        srows = spill["rows"] if spill else 0
        m = sum(len(f) for f in frames)
        M = srows + m
        bufs: Dict[str, torch.Tensor] = {}
        mats = []
        if self.stacked:
            if self._scalar_cats:
                mats.append(("cats", self._scalar_cats, torch.int64))
            if self._scalar_conts:
                mats.append(("conts", self._scalar_conts, torch.float32))
        else:
            for n in self._scalar_cats + self._scalar_conts:
                bufs[n] = torch.empty(M, dtype=frames[0][n].materialize().data.dtype if frames[0][n].fill is not None
                                      else frames[0][n].data.dtype, device=dev)
        for key, names, dt in mats:
            bufs[key] = torch.empty((M, len(names)), dtype=dt, device=dev)
        if self.label_names:
            shape = (M,) if len(self.label_names) == 1 else (M, len(self.label_names))
            bufs["__y__"] = torch.empty(shape, dtype=torch.float32, device=dev)
        if spill:
            for k, t in spill["bufs"].items():
                bufs[k][:srows].copy_(t)
        # the chunk's one draw: a row number in the partitions laid one behind the other
        index = torch.randperm(m, device=dev, generator=gen) if self.shuffle else None
        plan = []
        if self.stacked:
            for key, names, _ in mats:
                plan += [KD.Take(n, bufs[key], column=c, row=srows) for c, n in enumerate(names)]
        else:
            for n in self._scalar_cats + self._scalar_conts:
                plain = all(f[n].valid is None and f[n].fill is None and f[n].data.dtype == bufs[n].dtype
                            for f in frames)
                if plain and (index is None or len(frames) == 1):
                    self._plain(n, frames, index, bufs[n][srows:])
                else:
                    plan.append(KD.Take(n, bufs[n], row=srows))
        if self.label_names:
            y = bufs["__y__"]
            plan += [KD.Take(n, y, column=None if y.dim() == 1 else c, row=srows)
                     for c, n in enumerate(self.label_names)]
        KD.take_frames(frames, index, plan, m)
        lists = {}
        if self._lists:
            # the spill's lists are one more source in front, taken in order: the chunk's lists come
            # out whole, with ONE read-back (the leaf total and the offsets at the batch boundaries)
            sources, lindex = frames, index
            if srows:
                sources = [DeviceFrame({n: DeviceColumn(v, None, o) for n, (v, o) in spill["lists"].items()})] + frames
                if index is not None:
                    lindex = torch.cat([torch.arange(srows, device=dev), index + srows])
            cuts = list(range(0, M, self.batch_size)) + [M]
            want = torch.tensor(cuts, dtype=torch.int64, device=dev)
            got, bounds = KD.take_lists_multi(sources, self._lists, lindex, M, want_offsets=want)
            for n in self._lists:
                values, offsets, _ = got[n]
                lists[n] = (values, offsets, {c: int(b) for c, b in zip(cuts, bounds[n])})
        return M, bufs, lists

    @staticmethod
    def _plain(name, frames, index, out):
        """Dict mode, a column without bitmap, fill or cast, in order or from ONE partition: a plain
        copy in the column's own dtype.  Shuffled across several partitions it goes with the other
        columns through the multi-source kernel (profiles/loader_notes.md has both measurements)."""
        if index is None:
            row = 0
            for f in frames:
                out[row:row + len(f)].copy_(f[name].data)
                row += len(f)
        else:
            # torch's gather, which measured faster than the batched kernel for this layout
            torch.index_select(frames[0][name].data, 0, index, out=out)

    def _list_batch(self, name, values, offsets, leafpos, a, b, out):
        lo, hi = leafpos[a], leafpos[b]
        v, o = values[lo:hi], offsets[a:b + 1] - lo
        width = self.sparse_max.get(name)
        if width is not None:
            col = DeviceFrame({name: DeviceColumn(v, None, o)})
            dense = self.sparse_as_dense
            cut = KL.slice_lists(col, [name], 0, int(width), pad_width=int(width) if dense else None, pad_value=0)[name]
            if dense:
                out[name] = cut.data.view(b - a, int(width))
                return
            v, o = cut.data, cut.offsets
        elif self.sparse_as_dense and name in self.sparse_names:
            raise ValueError(f"sparse_as_dense needs sparse_max['{name}']")
        out[name + "__values"] = v
        out[name + "__offsets"] = o

    def _emit(self, M, bufs, lists, upto):
        B = self.batch_size
        for a in range(0, upto, B):
            b = min(a + B, M)
            x = {}
            for k, t in bufs.items():
                if k != "__y__":
                    x[k] = t[a:b]
            for n, (values, offsets, leafpos) in lists.items():
                self._list_batch(n, values, offsets, leafpos, a, b, x)
            y = bufs["__y__"][a:b] if "__y__" in bufs else None
            yield x, y

    def __iter__(self):
        self._stop = False
        order = self._my_parts()
        gen = None
        if self.shuffle:
            seed = int(self.seed_fn()) if self.seed_fn is not None else int.from_bytes(os.urandom(7), "little")
            order = partition_order(order, seed)
        parts = self._partitions(order)
        B = self.batch_size
        spill = None
        pending: List = []
        nxt = next(parts, None)
        first = True
        while nxt is not None or spill is not None:
            frames = []
            while nxt is not None and len(frames) < self.parts_per_chunk:
                if first:
                    self._layout(nxt)
                    if self.shuffle:
                        gen = torch.Generator(device=nxt[self._columns[0]].data.device)
                        gen.manual_seed(seed)
                    first = False
                if len(nxt):
                    frames.append(nxt)
                nxt = next(parts, None)
            last = nxt is None
            if not frames:
                if spill is None or self.drop_last:
                    return
                M, bufs, lists = spill["rows"], spill["bufs"], {
                    n: (v, o, {0: 0, spill["rows"]: int(v.numel())}) for n, (v, o) in spill["lists"].items()}
                yield from self._emit(M, bufs, lists, M)
                return
            M, bufs, lists = self._gather(frames, spill, gen)
            full = M - M % B
            upto = M if (last and not self.drop_last) else full
            for batch in self._emit(M, bufs, lists, upto):
                yield batch
                if self._stop:
                    return
            spill = None
            if not last and full < M:
                spill = {"rows": M - full, "bufs": {k: t[full:] for k, t in bufs.items()}, "lists": {}}
                shared = {}     # columns that share their offsets keep sharing them in the spill
                for n, (values, offsets, leafpos) in lists.items():
                    lo = leafpos[full]
                    if offsets.data_ptr() not in shared:
                        shared[offsets.data_ptr()] = offsets[full:] - lo
                    spill["lists"][n] = (values[lo:], shared[offsets.data_ptr()])
            if last:
                return


class DLDataLoader(torch.utils.data.DataLoader):
    """``torch.utils.data.DataLoader`` over a ``TorchAsyncItr`` (pass ``batch_size=None`` and an
    identity ``collate_fn``), with the two attributes fastai reads: ``device`` and the length of
    the wrapped loader."""

    @property
    def device(self):
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def __len__(self):
        return len(self.dataset)
