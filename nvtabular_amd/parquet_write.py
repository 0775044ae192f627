"""The PLAIN write driver behind ``Dataset.to_parquet``: partitions on the device -> row groups
staged in pinned host memory -> ``parquet_plain.PlainParquetWriter``.

Every partition is cut into row groups; a row group's columns are copied into pinned host buffers
on a side stream (nulls: values compacted and the validity bitmap re-packed on the device first)
while the previous row group is written -- all its column chunks at once, by a pool of threads
calling pwrite at offsets laid out beforehand.
List columns: the repetition / definition levels of a row group are packed on the device
(kernels_parquet_list: the columns that share an offsets tensor share one plan and one repetition
stream); ONE read-back per row group and offsets tensor brings the page table, the stream sizes and
the non-null counts, then the level bytes and the non-null leaves are copied out like the values of
a flat column ("List columns in the PLAIN parquet writer").
Dictionary pages (``use_dictionary``): the non-null values of every OFFERED column of a row group
go through kernels_parquet_dict (dictionary build + index pack, enqueued for all of them first);
ONE read-back per row group brings their state records {d, overflow} and page starts, the chunk
rule (``parquet_plain.dict_pays``) is applied on the host, and each chunk then copies out what it
really needs: dictionary + packed indices, or the plain values ("Dictionary pages in
the PLAIN parquet writer").
String columns: the column's {surrogate -> str} dict goes to the device once per to_parquet call as an
entry table (kernels_parquet_str_out.StringTables); per row group the non-null surrogates become entry
ids and a byte plan, the page table and the count of unknown surrogates ride in the read-back of the
dictionary states, then the BYTE_ARRAY body is filled on the device and copied out like the values of
a number column.  An offered string column costs one more read-back per row group (shared by all of
them): the size of its dictionary page ("String columns in the PLAIN parquet writer").
Snappy pages (``device_compression="snappy"``): behind the dictionary decision and the string fills the
values regions of ALL chunks of the row group -- the non-null values, a string chunk's BYTE_ARRAY body,
a dictionary chunk's dictionary page -- go through kernels_snappy (plan, compress, gather: three
batched calls), ONE read-back brings the compressed bytes of every page, ``parquet_plain.snappy_pays``
decides per chunk, and a chunk copies out its dense compressed bytes or, where snappy does not make
it smaller, what it copies out today ("Snappy pages in the PLAIN parquet writer")."""
from __future__ import annotations

import os
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from contextlib import nullcontext
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from . import kernels as K
from . import kernels_parquet_dict as KPD
from . import kernels_parquet_list as KPL
from . import kernels_parquet_narrow as KPN
from . import kernels_parquet_str_out as KSO
from . import kernels_snappy as KS
from . import parquet_plain as PP
from .device import pack_bitmap_device
from .parquet_plain import BoolPages, ByteArrayPages, DictPages, ListLevels, PlainParquetWriter, SnappyPages

# seconds of the last plain write: staging (enqueue + pinned allocation), waiting for copies, writing;
# snappy_s (a part of stage_s): plan, compress and gather of a row group's chunks, the read-back of
# their page sizes and the enqueueing of the copies behind it;
# levels_s (a part of stage_s): packing the levels of list columns and waiting for their page tables;
# dict_s (a part of stage_s): enqueueing dictionary build + pack and waiting for the state records;
# strings_s (a part of stage_s): entry ids, byte plans and fills of string columns, and the read-back
# of their dictionary page sizes
LAST_TIMING = {}
_TORCH_OF = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}
# flat device columns of these dtypes go out as INT32 annotated INTEGER{8 | 16} / as BOOLEAN
_NARROW_OF = {torch.int8: np.dtype("int8"), torch.int16: np.dtype("int16"), torch.bool: np.dtype(bool)}


class _Column(NamedTuple):
    """One column of a partition as it goes out (after the requested cast)."""
    name: str
    data: torch.Tensor                       # the rows' values; a list column: its leaves
    mask: Optional[torch.Tensor]             # bool per row (list column: per leaf), None: no nulls
    logical: Any                             # datetime64 dtype of a flat column, or None
    offsets: Optional[torch.Tensor] = None   # of a list column
    bitmap: Optional[torch.Tensor] = None    # leaf bitmap of a list column (what `mask` unpacks)
    offered: bool = False                    # its chunks are dictionary-encoded where that pays
    table: Any = None                        # EntryTable of a string column (``data``: its surrogates)


class _HostColumn(NamedTuple):
    """One column of a staged row group, as PlainParquetWriter.write_row_group takes it."""
    name: str
    values: Any          # the non-null values / leaves (pinned; may still be in flight), or a DictPages
    valid: Any           # None, the rows' validity bitmap (uint8 array) or a list column's ListLevels
    logical: Any
    dtype: Any = None    # the file's dtype where the values' is not it (int8 / int16: the values are int32)


class _RowGroup(NamedTuple):
    file: int        # index of the part file
    columns: list    # of _HostColumn
    rows: int
    event: Any       # recorded behind the copies on the side stream (None: host frames)
    keep: list       # device tensors and pinned buffers the copies and the writes still use
    stats: Optional[list]   # per column: {min, max} as a 2-element array (in flight) or None


def _string_table(name, col, dtypes, tables):
    """The EntryTable of a flat string column the PLAIN writer takes, else None: surrogates on the
    device, no ``dtypes`` entry, every value of the dict a ``str`` of at most 2^30 - 4 bytes."""
    if col.offsets is not None or not col.data.is_cuda or col.data.dtype != torch.int64 or \
            col.logical is not None or (dtypes and name in dtypes):
        return None
    return tables.get(col.strings)


def plain_eligible(frame, dtypes, tables=None) -> bool:
    """Every column a flat int32 / int64 / float32 / float64 column (after the requested
    casts), a flat int8 / int16 / bool column on the device without a ``dtypes`` entry, a datetime column in ms / us / ns, a flat string column on the device whose dict holds
    only ``str`` values, or a list column on the device whose leaves are
    int32 / int64 / float32 / float64 numbers: the hand-written PLAIN writer takes the partition;
    anything else (datetime64[s] too: parquet has no seconds unit; lists of strings, string columns
    on the host, with a ``dtypes`` entry or with bytes / mixed objects in their dict, lists of bool and
    8 / 16-bit leaves, uint8, narrow columns on the host; a cast of a list column or to a narrow type)
    goes to pyarrow.  ``tables``: the StringTables of the
    to_parquet call (the entry table built for this verdict is the one the write uses)."""
    if len(frame.columns) == 0:
        return False
    tables = tables if tables is not None else KSO.StringTables()
    for name, col in frame.items():
        if col.strings is not None:
            if _string_table(name, col, dtypes, tables) is None:
                return False
            continue
        if col.data.dtype in _NARROW_OF:
            # int8 / int16 / bool: flat, on the device, as they are (a dtypes= cast stays with pyarrow,
            # whose safe cast raises on overflow)
            if col.offsets is not None or not col.data.is_cuda or col.logical is not None or \
                    (dtypes and name in dtypes):
                return False
            continue
        if col.data.dtype not in _TORCH_OF.values():
            return False
        if col.offsets is not None and (not col.data.is_cuda or col.logical is not None or
                                        (dtypes and name in dtypes)):
            return False
        if col.logical is not None and (PP.timestamp_unit(col.logical) is None or (dtypes and name in dtypes)):
            return False
        if dtypes and name in dtypes and not PP.supported_dtype(np.dtype(dtypes[name])):
            return False
    return True


def _dict_eligible(col, dtypes, name) -> bool:
    """A column of a plain-eligible frame whose chunks can be dictionary-encoded: int32 / int64 (after
    the requested cast; datetime counts are int64), flat or as list leaves, or a string column, on
    the device."""
    if col.strings is not None:
        return bool(col.data.is_cuda)
    dt = np.dtype(dtypes[name]) if (dtypes and name in dtypes) else None
    is_int = (dt in (np.dtype("int32"), np.dtype("int64"))) if dt is not None else \
        col.data.dtype in (torch.int32, torch.int64, torch.int8, torch.int16)
    return bool(is_int and col.strings is None and col.data.is_cuda)


def dictionary_columns(frame, dtypes, use_dictionary):
    """``to_parquet(use_dictionary=...)`` for a frame ``plain_eligible`` takes -> the names of the
    columns offered for dictionary encoding.  None / False: none; True: every eligible column (float
    columns stay PLAIN silently); a list of names: those -- a name that is no column or no eligible
    column raises ValueError."""
    if use_dictionary is None or use_dictionary is False:
        return frozenset()
    eligible = [name for name, col in frame.items() if _dict_eligible(col, dtypes, name)]
    if use_dictionary is True:
        return frozenset(eligible)
    if isinstance(use_dictionary, (str, bytes)):
        raise ValueError(f"to_parquet: use_dictionary takes None, a bool or a list of column names, not {use_dictionary!r}")
    names = list(use_dictionary)
    cols = [name for name, _ in frame.items()]
    for name in names:
        if name not in cols:
            raise ValueError(f"to_parquet: use_dictionary names '{name}', which is no column of {cols}")
        if name not in eligible:
            raise ValueError(f"to_parquet: use_dictionary names '{name}': only int32 / int64, datetime and string "
                             f"columns and lists of int32 / int64 on the device are dictionary-encoded (these: {eligible})")
    return frozenset(names)


def device_permutation(n: int, frame):
    return torch.randperm(n, device=next((col.data.device for _, col in frame.items()), None))


def _to_host(t):
    if not t.is_cuda:
        return t.contiguous()
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


def _prepare(part, n, dtypes, offered=frozenset(), tables=None):
    """-> ([_Column] of a partition of n rows, [[list columns that share one offsets tensor]]: they share
    plan, page table and repetition stream).  ``offered``: names of the columns whose chunks may be
    dictionary-encoded.  ``tables``: the StringTables of the call."""
    cols, groups = [], {}
    tables = tables if tables is not None else KSO.StringTables()
    for name, col in part.items():
        col = col.materialize()
        if col.strings is not None:
            table = _string_table(name, col, dtypes, tables)
            if table is None:   # (the first partition decided for the PLAIN writer; never cast silently)
                raise ValueError(f"to_parquet: partition schema differs: string column '{name}' of this partition "
                                 "is not one the PLAIN writer takes (host data, a list, or a dict value that is "
                                 "no str)")
            mask = K.unpack_bitmap(col.valid, n) if col.valid is not None else None
            cols.append(_Column(name, col.data, mask, None, offered=name in offered, table=table))
            continue
        if col.offsets is not None:
            leaves = col.data.contiguous()
            mask = K.unpack_bitmap(col.valid, leaves.numel()) if col.valid is not None else None
            cols.append(_Column(name, leaves, mask, None, col.offsets.contiguous(), col.valid,
                                name in offered and leaves.is_cuda and leaves.dtype in (torch.int32, torch.int64)))
            groups.setdefault((cols[-1].offsets.data_ptr(), cols[-1].offsets.numel()), []).append(cols[-1])
            continue
        data = col.data
        if dtypes and name in dtypes:
            data = data.to(_TORCH_OF[str(np.dtype(dtypes[name]))])
        mask = K.unpack_bitmap(col.valid, n) if col.valid is not None else None
        cols.append(_Column(name, data, mask, col.logical, offered=name in offered and data.is_cuda and
                            data.dtype in (torch.int32, torch.int64, torch.int8, torch.int16)))
    return cols, list(groups.values())


def _pack_levels(groups, s0, s1, keep):
    """Rows [s0, s1) of the list columns: {name: (their ListLevels, the slice of their leaves)}.
    All groups are enqueued first; each read-back is the one host synchronisation of its offsets
    tensor.  The level bytes are in flight when this returns (``keep`` holds their buffers)."""
    levels = {}
    t_lv = time.perf_counter()
    packed = [KPL.pack_levels(members[0].offsets, s0, s1, [c.bitmap for c in members],
                              min(int(c.data.numel()) for c in members), PP.PAGE_VALUES) for members in groups]
    for members, dl in zip(groups, packed):
        lt = dl.read_back()
        LAST_TIMING["levels_s"] += time.perf_counter() - t_lv
        hrep = _to_host(dl.rep[:lt.rep_bytes])
        hdefs = [_to_host(d[:lt.def_bytes]) for d in dl.defs]
        keep.append((dl, hrep, hdefs))
        for c, st in zip(members, dl.stream_of):
            levels[c.name] = (ListLevels(lt.slots, lt.nonnull[st], hrep.numpy(), lt.rep_at, hdefs[st].numpy(),
                                         lt.def_at), slice(lt.leaf_lo, lt.leaf_hi))
        t_lv = time.perf_counter()
    return levels


def _min_max(vals):
    """{min, max} of the values on their way to a pinned 2-element tensor; no values: None."""
    if not vals.numel():
        return None
    if vals.dtype.is_floating_point:   # (NaN is no minimum / maximum)
        nan = torch.isnan(vals)
        lo = torch.where(nan, torch.full_like(vals, float("inf")), vals).amin()
        hi = torch.where(nan, torch.full_like(vals, float("-inf")), vals).amax()
    else:
        lo, hi = torch.aminmax(vals)
    return _to_host(torch.stack([lo, hi]))


def _column_values(c: _Column, s0, s1, levels):
    """Rows [s0, s1) of one column, still where the column is -> (the non-null values / leaves, None or the
    rows' validity bitmap or the list column's ListLevels, the rows' bool mask of a flat column or None)."""
    vals, valid, m = c.data[s0:s1], None, None
    if c.offsets is not None and s1 > s0:
        valid, leaves = levels[c.name]
        vals = c.data[leaves] if c.mask is None else c.data[leaves][c.mask[leaves]]
    elif c.offsets is not None:
        vals, valid = c.data[:0], ListLevels([], [], b"", [], b"", [])
    elif c.mask is not None:
        m = c.mask[s0:s1]
        vals = vals[m]
        valid = pack_bitmap_device(m) if m.is_cuda else torch.from_numpy(np.packbits(m.numpy(), bitorder="little"))
    return vals, valid, m


def _page_start(vals, valid, m, rows, page_rows=None):
    """int64[pages + 1] on the device: the positions in ``vals`` (the non-null values) at which the data
    pages of the chunk start -- a list column: from the non-null counts of its page table; a flat column:
    from the per-page popcounts of the row mask, or by arithmetic when there is no mask.  ``page_rows``:
    the rows per page of a flat column (None: PAGE_VALUES; a string column's follow its longest entry)."""
    dev = vals.device
    if isinstance(valid, ListLevels):
        ps = np.concatenate([[0], np.cumsum(valid.nonnull)]).astype(np.int64)
        return torch.from_numpy(ps).to(dev)
    page_rows = PP.PAGE_VALUES if page_rows is None else page_rows
    npages = max(1, -(-rows // page_rows))
    if m is None:
        return torch.clamp(torch.arange(npages + 1, device=dev, dtype=torch.int64) * page_rows, max=rows)
    padded = torch.zeros(npages * page_rows, dtype=torch.bool, device=dev)
    padded[:rows] = m
    counts = padded.view(npages, page_rows).sum(dim=1, dtype=torch.int64)
    return torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])


def _file_dtype(c: _Column):
    """int8 / int16 of a narrow column (its values travel as int32), else None."""
    return _NARROW_OF.get(c.data.dtype) if c.data.dtype in (torch.int8, torch.int16) else None


def _widen_narrow(cols, staged, rows, keep):
    """The narrow columns of a row group behind the compaction: the non-null values of ALL int8 / int16
    columns become int32 in one launch (from here on their chunks are int32 chunks: dictionary, snappy
    and statistics see nothing else), the non-null values of every bool column the bytes of its BOOLEAN
    pages.  -> (staged with the widened values, {column index: packed bytes on the device})."""
    narrow = [ci for ci, c in enumerate(cols) if _file_dtype(c) is not None and staged[ci][0].is_cuda]
    wide = KPN.widen_many([staged[ci][0].contiguous() for ci in narrow])
    staged = list(staged)
    for ci, w in zip(narrow, wide):
        keep.append(staged[ci][0])
        staged[ci] = (w,) + tuple(staged[ci][1:])
    bools = {}
    for ci, (c, (vals, valid, m)) in enumerate(zip(cols, staged)):
        if c.data.dtype == torch.bool and c.offsets is None and vals.is_cuda:
            vals = vals.contiguous()
            bools[ci] = KPN.bool_pack(vals, _page_start(vals, valid, m, rows))
    return staged, bools


def _stage_column(c: _Column, vals, valid, encoded, statistics, keep, packed=None):
    """One column of a row group on its way to the host -> (_HostColumn, min / max or None).
    ``encoded``: None, or (DeviceDict, d, overflow, page starts) of an offered column after the read-back.
    ``packed``: the bytes of a bool chunk's pages on the device (``_widen_narrow``)."""
    hv = None
    if packed is not None:   # (a bool chunk: a null count, no min / max)
        hp = _to_host(packed)   # (ceil(nv / 8) + pages bytes: the bound; the host lays the pages out from the bitmap)
        hb = _to_host(valid).numpy() if valid is not None else None
        keep.append((vals, valid, packed, hp))
        return _HostColumn(c.name, BoolPages(hp.numpy(), int(vals.numel())), hb, None), None
    if encoded is not None:
        dd, d, overflow, ps = encoded
        nv = np.diff(ps)
        if not overflow and PP.dict_pays(d, nv, vals.element_size()):
            W = PP.dict_index_width(d)
            hd, hp = _to_host(dd.dictionary[:d]), _to_host(dd.packed[:PP.dict_page_offsets(nv, W)[1]])
            hv = DictPages(hd.numpy(), hp.numpy(), W, nv)
            keep.append((dd, hd, hp))
    if hv is None:
        hv = _to_host(vals).numpy()
    hb = valid if isinstance(valid, ListLevels) or valid is None else _to_host(valid).numpy()
    mm = _min_max(vals) if statistics else None
    keep.append((vals, valid, mm, hv))
    return _HostColumn(c.name, hv, hb, c.logical, _file_dtype(c)), (mm.numpy() if mm is not None else None)


class _StrChunk:
    """One string column's chunk of a row group between its plan and its fill."""

    def __init__(self, col, surrogates, valid, ids, page_start, pos, page_at, bad):
        self.col, self.surrogates, self.valid, self.ids = col, surrogates, valid, ids
        self.page_start, self.pos, self.page_at, self.bad = page_start, pos, page_at, bad

    def device_words(self):
        return [self.page_at, self.page_start, self.bad]

    def take_words(self, arrays):
        """The front of ``arrays`` (what the read-back made of ``device_words``) becomes the host's
        page table; an unknown surrogate raises."""
        page_at, page_start, bad = arrays[:3]
        del arrays[:3]
        if int(bad[0]):
            raise ValueError(f"to_parquet: column '{self.col.name}': {int(bad[0])} values whose surrogate is no key "
                             "of the column's dictionary of strings")
        self.page_at_host, self.nv = page_at, np.diff(page_start)


def _plan_strings(cols, staged, rows):
    """{column index: _StrChunk} of the string columns of a row group of ``rows`` rows: entry ids and
    byte plan enqueued, nothing read back."""
    strs = {}
    for ci, (c, (vals, valid, m)) in enumerate(zip(cols, staged)):
        if c.table is None:
            continue
        keys, offsets, _ = c.table.on(vals.device)
        vals = vals.contiguous()
        bad = torch.zeros(1, dtype=torch.int64, device=vals.device)
        page_start = _page_start(vals, valid, m, rows, c.table.page_rows)
        ids = KSO.entry_ids(keys, vals, bad)
        pos, page_at = KSO.plan(ids, offsets, page_start)
        strs[ci] = _StrChunk(c, vals, valid, ids, page_start, pos, page_at, bad)
    return strs


def _fill_strings(strs, dicts, states, keep):
    """{column index: form} of the string chunks after the read-back, their bodies filled on the
    device: ("dict", dictionary page body, d, W, the DeviceDict) or ("plain", body or None, bytes).
    The chunk rule in bytes: an offered chunk takes the dictionary iff it has at most 2^20 distinct
    entries and dictionary page + indices are SMALLER than its PLAIN body; the dictionary pages'
    sizes are ONE more read-back for all of them."""
    cand = {}
    for ci, sc in strs.items():
        d, overflow = states[ci][:2] if ci in dicts else (0, 1)
        if not overflow and 1 <= d <= PP.DICT_MAX_ENTRIES:
            cand[ci] = KSO.plan(dicts[ci].dictionary[:d], sc.col.table.on(sc.ids.device)[1])[0]
    sizes = {}
    if cand:
        K.stat_add("pq_str_dict_readback")
        sizes = dict(zip(cand, K.read_back(torch.cat([p[-1:] for p in cand.values()])).tolist()))
    forms = {}
    for ci, sc in strs.items():
        _, offsets, chars = sc.col.table.on(sc.ids.device)
        total = int(sc.page_at_host[-1])
        if ci in cand:
            d, W = states[ci][0], PP.dict_index_width(states[ci][0])
            if sizes[ci] <= PP.MAX_PAGE_BYTES and sizes[ci] + PP.dict_index_bytes(sc.nv, W) < total:
                body = KSO.fill(dicts[ci].dictionary[:d], offsets, chars, cand[ci], sizes[ci])
                keep.append((dicts[ci], cand[ci], body))
                forms[ci] = ("dict", body, d, W, dicts[ci])
                continue
        body = KSO.fill(sc.ids, offsets, chars, sc.pos, total) if total else None
        keep.append(body)
        forms[ci] = ("plain", body, total)
    return forms


def _snappy_geometry(rows, page_rows, nulls, levels):
    """[(num_values, level bytes)] of the data pages of a chunk: a list chunk's from its ListLevels,
    a flat chunk's ``rows`` rows cut every ``page_rows``."""
    if levels is not None:
        return [(s, PP.list_level_bytes(s)) for s in levels.slots]
    cuts = list(range(0, rows, page_rows)) + [rows] if rows else [0, 0]
    return [(b - a, PP.flat_level_bytes(b - a, nulls)) for a, b in zip(cuts[:-1], cuts[1:])]


def _stage_snappy(cols, staged, strs, dicts, states, rows, statistics, keep, bools):
    """``device_compression="snappy"``: every chunk of the row group in the form it takes (after
    ``dict_pays``) -> ([_HostColumn], [min / max or None]).  Plan, compress and gather are enqueued for
    the values regions of ALL chunks at once (a dictionary chunk: its dictionary page), ONE read-back
    brings their per-page compressed sizes (and the page starts only the device has),
    ``parquet_plain.snappy_pays`` decides per chunk on the host, and every chunk then copies out
    only what it needs: the dense compressed bytes, or the raw values as today."""
    forms = _fill_strings(strs, dicts, states, keep)
    dev = next((v.device for v, _, _ in staged if v.is_cuda), None)
    whole = torch.arange(2, dtype=torch.int64, device=dev) if dev is not None else None   # one page: [0, 1] units
    regions, plans, extra = [], {}, []
    for ci, (c, (vals, valid, m)) in enumerate(zip(cols, staged)):
        nulls = (strs[ci].valid if ci in strs else valid) is not None
        levels = valid if isinstance(valid, ListLevels) else None
        if ci in strs:
            sc, form = strs[ci], forms[ci]
            geo = _snappy_geometry(rows, sc.col.table.page_rows, nulls, None)
            if form[0] == "dict":
                plan = dict(kind="dict", geo=geo, nv=sc.nv, d=form[2], W=form[3], dd=form[4], raw=int(form[1].numel()),
                            region=KS.Region(form[1], whole, int(form[1].numel()), 4))
            elif form[2]:
                plan = dict(kind="plain", geo=geo, raw=np.diff(sc.page_at_host), region=KS.Region(form[1], sc.page_at, 1, 4))
            else:
                continue
        elif not vals.numel() or not vals.is_cuda or ci in bools:   # (bool chunks are written uncompressed)
            continue
        else:
            size = vals.element_size()
            geo = _snappy_geometry(rows, PP.PAGE_VALUES, nulls, levels)
            d, overflow, ps = states[ci] if ci in dicts else (0, 1, None)
            if ci in dicts and not overflow and PP.dict_pays(d, np.diff(ps), size):
                plan = dict(kind="dict", geo=geo, nv=np.diff(ps), d=d, W=PP.dict_index_width(d), dd=dicts[ci], raw=d * size,
                            region=KS.Region(dicts[ci].dictionary[:d], whole, d * size, size))
            else:
                src = vals.contiguous()
                dps = dicts[ci].page_start if ci in dicts else _page_start(src, valid, m, rows)
                plan = dict(kind="plain", geo=geo, raw=None if ps is None else np.diff(ps) * size,
                            region=KS.Region(src, dps, size, size))
                if ps is None:
                    plan["extra"] = len(extra)
                    extra.append(dps)
        plan["at"] = len(regions)
        regions.append(plan["region"])
        plans[ci] = plan
    got, more = [], []
    if regions:
        ds = KS.compress(regions)
        got, more = KS.read_back(ds, extra=extra)
        keep.append(ds.dense)
    host, stats = [], []
    for ci, (c, (vals, valid, m)) in enumerate(zip(cols, staged)):
        plan = plans.get(ci)
        hv = None
        if plan is not None:
            ps, geo = got[plan["at"]], plan["geo"]
            if ps.error:
                raise RuntimeError(f"to_parquet: column '{c.name}': the snappy kernels report error {ps.error} "
                                   "(a fragment outgrew its slot, or the page table its fragment records)")
            if plan["kind"] == "dict":
                idx = [PP.dict_index_bytes([k], plan["W"]) for k in plan["nv"]]
                sizes = PP.snappy_chunk_bytes([(nvl, lv + i, 0, 0, 8) for (nvl, lv), i in zip(geo, idx)],
                                              (plan["d"], plan["raw"], ps.total))
            else:
                raw = plan["raw"] if plan["raw"] is not None else np.diff(more[plan["extra"]]) * vals.element_size()
                if len(raw) != len(geo) or len(ps.sizes) != len(geo):
                    raise RuntimeError(f"to_parquet: column '{c.name}': {len(geo)} data pages, {len(raw)} regions")
                sizes = PP.snappy_chunk_bytes([(nvl, lv, int(u), int(s), 0)
                                               for (nvl, lv), u, s in zip(geo, raw, ps.sizes)])
            if PP.snappy_pays(*sizes):
                hd = _to_host(ds.dense[plan["at"]][:ps.total])
                dt = PP.STRING_DTYPE if ci in strs else np.dtype(str(vals.dtype).replace("torch.", ""))
                page_rows = strs[ci].col.table.page_rows if ci in strs else None
                if plan["kind"] == "dict":
                    dd = plan["dd"]
                    hp = _to_host(dd.packed[:PP.dict_page_offsets(plan["nv"], plan["W"])[1]])
                    hv = SnappyPages(dt, hd.numpy(), [ps.total], [plan["raw"]], page_rows,
                                     (plan["W"], hp.numpy(), plan["nv"], plan["d"]))
                    keep.append((dd, hp))
                else:
                    hv = SnappyPages(dt, hd.numpy(), ps.sizes, raw, page_rows)
                keep.append(hd)
        if ci in strs:
            sc = strs[ci]
            if hv is None:
                hc = _host_string(sc, forms[ci], keep)
            else:
                hb = _to_host(sc.valid).numpy() if sc.valid is not None else None
                keep.append((sc, hv, hb))
                hc = _HostColumn(sc.col.name, hv, hb, None)
            mm = None   # (no min / max for string chunks)
        elif hv is None:
            hc, mm = _stage_column(c, vals, valid, (dicts[ci],) + states[ci] if ci in dicts else None, statistics, keep,
                                   bools.get(ci))
        else:
            hb = valid if isinstance(valid, ListLevels) or valid is None else _to_host(valid).numpy()
            mm = _min_max(vals) if statistics else None
            keep.append((vals, valid, mm, hv))
            hc, mm = _HostColumn(c.name, hv, hb, c.logical, _file_dtype(c)), (mm.numpy() if mm is not None else None)
        host.append(hc)
        stats.append(mm)
    return host, stats


def _host_string(sc, form, keep):
    """One string chunk on its way to pinned memory, as it is written without a codec -> _HostColumn."""
    if form[0] == "dict":
        _, body, d, W, dd = form
        hd, hp = _to_host(body), _to_host(dd.packed[:PP.dict_page_offsets(sc.nv, W)[1]])
        hv = DictPages(hd.numpy(), hp.numpy(), W, sc.nv, entries=d, page_rows=sc.col.table.page_rows)
        keep.append((hd, hp))
    else:
        _, body, total = form
        hbody = _to_host(body) if total else None
        hv = ByteArrayPages(hbody.numpy() if total else np.zeros(0, dtype=np.uint8), sc.page_at_host, sc.nv,
                            sc.col.table.page_rows)
        keep.append(hbody)
    hb = _to_host(sc.valid).numpy() if sc.valid is not None else None
    keep.append((sc, hv, hb))
    return _HostColumn(sc.col.name, hv, hb, None)


def _stage_strings(strs, dicts, states, keep):
    """{column index: _HostColumn} of the string chunks after the read-back: the bodies are filled on
    the device (``_fill_strings``) and are on their way to pinned memory."""
    forms = _fill_strings(strs, dicts, states, keep)
    return {ci: _host_string(sc, forms[ci], keep) for ci, sc in strs.items()}


def _stage_row_group(j, cols, groups, s0, s1, copy_s, statistics, snappy=False) -> _RowGroup:
    """Enqueue everything that brings rows [s0, s1) to the host, on ``copy_s`` (None: the frame is
    on the host already), and record one event behind it.  ``snappy``: the chunks' pages are
    compressed on the device where that makes them smaller (``_stage_snappy``)."""
    host, keep, stats = [], [], ([] if statistics else None)
    t_st = time.perf_counter()
    with torch.cuda.stream(copy_s) if copy_s is not None else nullcontext():
        levels = _pack_levels(groups, s0, s1, keep) if (s1 > s0 and groups) else {}
        staged = [_column_values(c, s0, s1, levels) for c in cols]
        staged, bools = _widen_narrow(cols, staged, s1 - s0, keep)
        # string columns: entry ids and the byte plan of every one of them (no read-back of their own)
        t_ss = time.perf_counter()
        strs = _plan_strings(cols, staged, s1 - s0)
        LAST_TIMING["strings_s"] += time.perf_counter() - t_ss
        # dictionary pages: build + pack of every offered column that has values, then ONE read-back
        # (the page tables of the string columns and their unknown surrogates ride along)
        t_dc = time.perf_counter()
        dicts = {ci: KPD.encode(strs[ci].ids, strs[ci].page_start) if ci in strs else
                 KPD.encode(vals.contiguous(), _page_start(vals, valid, m, s1 - s0))
                 for ci, (c, (vals, valid, m)) in enumerate(zip(cols, staged)) if c.offered and vals.numel()}
        if strs:
            got, more = KPD.read_back_states(list(dicts.values()), [t for sc in strs.values() for t in sc.device_words()])
            for sc in strs.values():
                sc.take_words(more)
        else:
            got = KPD.read_back_states(list(dicts.values()))
        states = dict(zip(dicts, got))
        if dicts:
            LAST_TIMING["dict_s"] += time.perf_counter() - t_dc
        elif strs:   # (the read-back waited for entry ids and plans alone)
            LAST_TIMING["strings_s"] += time.perf_counter() - t_dc
        t_ss = time.perf_counter()
        if snappy:
            # snappy pages: plan + compress + gather of every chunk in the form it takes, ONE read-back
            host, mms = _stage_snappy(cols, staged, strs, dicts, states, s1 - s0, statistics, keep, bools)
            stats = mms if statistics else None
            LAST_TIMING["snappy_s"] += time.perf_counter() - t_ss
            staged = []   # (every column is staged)
        hosts = _stage_strings(strs, dicts, states, keep) if not snappy else {}
        if strs and not snappy:
            LAST_TIMING["strings_s"] += time.perf_counter() - t_ss
        for ci, (c, (vals, valid, m)) in enumerate(zip(cols, staged)):
            if ci in hosts:
                hc, mm = hosts[ci], None   # (no min / max for string chunks)
            else:
                hc, mm = _stage_column(c, vals, valid, (dicts[ci],) + states[ci] if ci in dicts else None, statistics,
                                       keep, bools.get(ci))
            host.append(hc)
            if statistics:
                stats.append(mm)
        event = None
        if copy_s is not None:
            event = torch.cuda.Event()
            event.record(copy_s)
    LAST_TIMING["stage_s"] += time.perf_counter() - t_st
    return _RowGroup(j, host, s1 - s0, event, keep, stats)


class _PartFiles:
    """The part files of one to_parquet call: file j is opened by its first row group, which sets
    its schema.  ``pool`` runs the column writes, at most ``max_inflight`` row groups at a time."""

    def __init__(self, output_path, fname, pool, max_inflight):
        self.output_path, self.fname, self.pool, self.max_inflight = output_path, fname, pool, max_inflight
        self.writers, self.names, self.rows = {}, {}, {}
        self.inflight = deque()   # (futures, row group) of row groups whose column writes are still running

    def flush(self, rg: _RowGroup):
        t0 = time.perf_counter()
        # the host does not wait for the copies: every column task synchronises with the event
        # itself before it writes.  Only validity bitmaps must be here already (the pages are
        # laid out from their popcounts).
        if rg.event is not None and any(isinstance(c.valid, np.ndarray) for c in rg.columns):
            rg.event.synchronize()
        ready = rg.event.synchronize if rg.event is not None else None
        t1 = time.perf_counter()
        LAST_TIMING["wait_copy_s"] += t1 - t0
        schema = ([c.name for c in rg.columns], [c.dtype if c.dtype is not None else c.values.dtype for c in rg.columns],
                  [c.logical for c in rg.columns], [isinstance(c.valid, ListLevels) for c in rg.columns])
        w = self.writers.get(rg.file)
        if w is None:
            self.names[rg.file] = self.fname(rg.file)
            w = self.writers[rg.file] = PlainParquetWriter(
                os.path.join(self.output_path, self.names[rg.file]), schema[0], schema[1], pool=self.pool,
                logical=schema[2], lists=schema[3])
        elif (w.names, w.dtypes, w.logical, w.lists) != schema:
            # (pyarrow's ParquetWriter raises on a schema change too; never cast silently)
            raise ValueError(
                f"to_parquet: partition schema {[(c.name, str(c.values.dtype)) for c in rg.columns]} differs from "
                f"the schema {list(zip(w.names, map(str, w.dtypes)))} of {self.names[rg.file]}")
        # the column writes of this row group go to the pool and are NOT waited for: row groups
        # of other files (other inodes: buffered writes to ONE file serialise on its inode lock,
        # ~10 GB/s) and the next copies proceed meanwhile
        futs = w.write_row_group([(c.values, c.valid) for c in rg.columns], rg.rows, wait=False, ready=ready,
                                 stats=rg.stats)
        self.inflight.append((futs, rg))
        while len(self.inflight) > self.max_inflight:
            for f in self.inflight.popleft()[0]:
                f.result()
        LAST_TIMING["write_s"] += time.perf_counter() - t1
        self.rows[rg.file] = self.rows.get(rg.file, 0) + rg.rows

    def close(self):
        t_cl = time.perf_counter()
        for w in self.writers.values():
            w.close()
        LAST_TIMING["close_s"] = time.perf_counter() - t_cl

    def abort(self):
        """No fds leaked, no truncated footer-less part files left behind."""
        for futs, _ in self.inflight:
            for f in futs:
                try:
                    f.result()
                except Exception:
                    pass
        for w in self.writers.values():
            w.abort()


def _timed_input(parts):
    """The partitions; the time spent waiting for each (the upstream transform) goes to input_s."""
    parts = iter(parts)
    while True:
        t_in = time.perf_counter()
        part = next(parts, None)
        LAST_TIMING["input_s"] += time.perf_counter() - t_in
        if part is None:
            return
        yield part


def _row_ranges(i, n, k, row_group, touched):
    """(file index, first row, row behind the last) of the row groups that partition i of n rows is
    cut into.  A piece without rows is still a row group if its file has none yet (``touched``)."""
    pieces = [(i, 0, n)] if k is None else [(j, (n * j) // k, (n * (j + 1)) // k) for j in range(k)]
    for j, a, b in pieces:
        if b <= a and j in touched:
            continue
        touched.add(j)
        for s0 in (range(a, b, row_group) if b > a else [a]):
            yield j, s0, min(b, s0 + row_group)


def _piece_ranges(pieces, row_group):
    """The row groups of the pieces [(file index, first row, row behind the last)] of a split partition
    (``hive.HiveSplitter.split``): every piece has rows and is cut every ``row_group`` rows."""
    for j, a, b in pieces:
        for s0 in range(a, b, row_group):
            yield j, s0, min(b, s0 + row_group)


def write_plain(parts, output_path, fname, k, shuffle, dtypes, statistics, row_group, max_inflight, threads,
                offered=frozenset(), tables=None, snappy=False, splitter=None):
    """Dataset.to_parquet for the frames ``plain_eligible`` takes: partition i goes to file i, or
    with ``k`` is cut into k pieces for files 0 .. k-1; every piece is cut into row groups of
    ``row_group`` rows, each staged and handed to its file's writer while the next is staged.
    ``offered``: the columns whose chunks are dictionary-encoded where that makes them smaller.
    ``tables``: the StringTables ``plain_eligible`` judged the first partition with (None: a fresh one).
    ``snappy``: ``device_compression="snappy"`` -- chunks on the device are written SNAPPY where that
    makes them smaller.
    ``splitter`` (``partition_on``; then ``k`` is None and ``fname`` the splitter's): every partition is
    permuted once so that the rows of a key tuple are contiguous, its key columns are dropped, and
    the tuple's row range goes to the file of its directory.
    -> (names {file index: name}, rows {file index: rows}, file indices in order)."""
    LAST_TIMING.update(wait_copy_s=0.0, write_s=0.0, stage_s=0.0, total_s=0.0, input_s=0.0, close_s=0.0,
                       levels_s=0.0, dict_s=0.0, strings_s=0.0, snappy_s=0.0)
    t_all = time.perf_counter()
    tables = tables if tables is not None else KSO.StringTables()
    copy_s = None
    touched = set()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        files = _PartFiles(output_path, fname, pool, max_inflight)
        try:
            for i, part in enumerate(_timed_input(parts)):
                n = len(part)
                if shuffle is not None and n > 1:
                    part = part.take_rows(device_permutation(n, part))
                pieces = None
                if splitter is not None:
                    part, pieces = splitter.split(part)
                    if not pieces:
                        continue
                cols, groups = _prepare(part, n, dtypes, offered, tables)
                on_gpu = any(c.data.is_cuda for c in cols)
                if on_gpu and copy_s is None:
                    copy_s = torch.cuda.Stream()
                if on_gpu:
                    copy_s.wait_stream(torch.cuda.current_stream())
                for j, s0, s1 in (_row_ranges(i, n, k, row_group, touched) if pieces is None else
                                  _piece_ranges(pieces, row_group)):
                    files.flush(_stage_row_group(j, cols, groups, s0, s1, copy_s if on_gpu else None, statistics,
                                                 snappy and on_gpu))
            files.close()
        except BaseException:
            files.abort()
            raise
    LAST_TIMING["total_s"] = time.perf_counter() - t_all
    return files.names, files.rows, sorted(files.writers)
