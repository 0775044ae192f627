"""Hive-partitioned parquet: ``key=value`` directories on the way out and on the way in.

Host code: how a key value becomes a path segment and back, how a directory tree is discovered, how
the dtypes of the key columns are decided, and the two small objects that carry the key columns
through ``Dataset``: ``HivePart`` (a partition read from a leaf directory plus the constants its path
spells) and ``HiveSplitter`` (the per-partition split of ``Dataset.to_parquet(partition_on=...)``,
which is the only part that needs the device; its imports are local).

Layout, as ``pyarrow.parquet.write_to_dataset`` writes and ``pyarrow.dataset`` reads it:
``root/<k1>=<v1>/<k2>=<v2>/<file>``; a segment value is ``urllib.parse.quote(str(value), safe="")``,
the empty string gives ``k=``, a null gives ``__HIVE_DEFAULT_PARTITION__``; the key columns are not
in the files and are appended behind the files' columns in path order when the dataset is read."""
from __future__ import annotations

import json
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple
from urllib.parse import quote, unquote

import numpy as np

NULL_SEGMENT = "__HIVE_DEFAULT_PARTITION__"
FD_HEADROOM = 64          # descriptors left to the rest of the process next to the open part files
_INT = re.compile(r"-?[0-9]+\Z")


# ---- segments -----------------------------------------------------------------------------------
def encode_segment(value) -> str:
    """The value part of a ``key=value`` directory name; ``None`` is the null marker."""
    return NULL_SEGMENT if value is None else quote(str(value), safe="")


def decode_segment(segment: str) -> Optional[str]:
    """The text a segment spells, ``None`` for the null marker."""
    return None if segment == NULL_SEGMENT else unquote(segment)


def dir_name(keys: Sequence[str], values: Sequence) -> str:
    """``k1=v1/k2=v2`` for one key tuple."""
    return "/".join(f"{k}={encode_segment(v)}" for k, v in zip(keys, values))


def parse_dir(name: str) -> Optional[Tuple[str, str]]:
    """(key, raw segment) of a directory named ``key=segment``, else None."""
    key, eq, seg = name.partition("=")
    return (key, seg) if eq and key else None


# ---- discovery ----------------------------------------------------------------------------------
class HiveLayout:
    """A discovered tree: ``keys`` in path order, ``files`` in sorted walk order, ``values[file]`` the
    decoded segment texts (None: null) and ``dtypes`` one numpy dtype name or "string" per key."""

    def __init__(self, root, keys, files, values, dtypes=None):
        self.root, self.keys, self.files, self.values = root, list(keys), list(files), dict(values)
        self.dtypes = list(dtypes) if dtypes is not None else None
        self._dicts: Dict[tuple, dict] = {}

    def string_dict(self, key: str, text: Optional[str], surrogate=None) -> dict:
        """The one-entry {surrogate -> str} dict of a string key value -- the same object every time,
        so the partitions of a directory share it."""
        d = self._dicts.get((key, text))
        if d is None:
            d = self._dicts[key, text] = {} if text is None else {int(surrogate): text}
        return d


def _parquet_files(path: str) -> List[str]:
    return sorted(os.path.join(path, f) for f in os.listdir(path)
                  if f.endswith(".parquet") and os.path.isfile(os.path.join(path, f)))


def discover(root: str) -> Optional[HiveLayout]:
    """The hive layout under ``root``, or None when ``root`` holds parquet files at its top level or
    no ``name=value`` directory.  Files whose paths disagree on the key names or their order raise
    ValueError."""
    root = str(root)
    if not os.path.isdir(root) or _parquet_files(root):
        return None
    files, values = [], {}
    keys: Optional[List[str]] = None

    def walk(path, names, texts):
        nonlocal keys
        subs = sorted(d for d in os.listdir(path) if os.path.isdir(os.path.join(path, d)) and parse_dir(d))
        here = _parquet_files(path) if names else []
        if here:
            if keys is None:
                keys = list(names)
            elif keys != list(names):
                raise ValueError(f"hive dataset {root}: {here[0]} is partitioned on {list(names)}, other files on "
                                 f"{keys}")
            for f in here:
                files.append(f)
                values[f] = tuple(texts)
        for d in subs:
            k, seg = parse_dir(d)
            walk(os.path.join(path, d), names + [k], texts + [decode_segment(seg)])

    walk(root, [], [])
    if not files:
        return None
    return HiveLayout(root, keys, files, values)


def read_partition_on(root: str) -> Optional[List[dict]]:
    """``partition_on`` of the ``_metadata.json`` that ``Dataset.to_parquet`` wrote, else None."""
    try:
        with open(os.path.join(str(root), "_metadata.json")) as f:
            got = json.load(f).get("partition_on")
    except (OSError, ValueError):
        return None
    return got if isinstance(got, list) else None


def infer_dtypes(keys: Sequence[str], values, recorded: Optional[List[dict]] = None) -> List[str]:
    """One dtype per key: what ``_metadata.json`` recorded for that name, else ``int64`` when every
    non-null segment of the key, over all files, matches ``-?[0-9]+``, else ``string``."""
    known = {e.get("col_name"): e.get("dtype") for e in (recorded or []) if isinstance(e, dict)}
    out = []
    for i, k in enumerate(keys):
        if known.get(k):
            out.append(str(known[k]))
            continue
        texts = [v[i] for v in values if v[i] is not None]
        out.append("int64" if all(_INT.match(t) for t in texts) else "string")
    return out


def check_clash(keys: Sequence[str], file_columns: Sequence[str], where: str = ""):
    clash = [k for k in keys if k in set(file_columns)]
    if clash:
        raise ValueError(f"hive dataset {where}: the key columns {clash} are also columns inside the files")


def layout_of(root: str) -> Optional[HiveLayout]:
    """``discover`` plus the key dtypes."""
    lay = discover(root)
    if lay is not None:
        lay.dtypes = infer_dtypes(lay.keys, lay.values.values(), read_partition_on(root))
    return lay


# ---- reading: the key columns of a partition ------------------------------------------------------
def key_column(layout: HiveLayout, key: str, dtype: str, text: Optional[str], n: int, device):
    """The constant column a path spells: n times the value, or n nulls for the null marker.  A string
    value is a constant surrogate (the bits every other string path computes) with a one-entry dict."""
    import torch

    from .device import DeviceColumn, torch_dtype

    valid = torch.zeros((n + 63) // 64 * 8, dtype=torch.uint8, device=device) if text is None else None
    if dtype == "string":
        from .strings import string_key64

        surrogate = 0 if text is None else int(string_key64([text])[0])
        return DeviceColumn(torch.full((n,), surrogate, dtype=torch.int64, device=device), valid, None, None,
                            layout.string_dict(key, text, surrogate))
    value = 0 if text is None else int(text)
    return DeviceColumn(torch.full((n,), value, dtype=torch_dtype(np.dtype(dtype)), device=device), valid)


class HivePart:
    """One partition of a hive dataset on the host: what the file reader returned for the file's
    columns (a StagedPartition, an Arrow table, or None when only key columns were asked for) and the
    key columns to attach when it becomes a DeviceFrame."""

    def __init__(self, inner, rows: int, layout: HiveLayout, texts, want: Sequence[str]):
        self.inner, self.rows, self.layout, self.texts, self.want = inner, int(rows), layout, tuple(texts), list(want)

    @property
    def num_rows(self):
        return self.rows

    def __len__(self):
        return self.rows

    def to_device(self, device=None):
        from .device import DeviceFrame, as_device_frame, default_device

        device = device or default_device()
        frame = as_device_frame(self.inner, device)[0] if self.inner is not None else DeviceFrame()
        lay = self.layout
        for k, dt, text in zip(lay.keys, lay.dtypes, self.texts):
            if k in self.want:
                frame[k] = key_column(lay, k, dt, text, self.rows, device)
        return frame


# ---- writing: the split of one to_parquet call -----------------------------------------------------
def check_descriptors(max_partitions: int):
    """The writers hold one descriptor per open part file: refuse a ``max_partitions`` that does not
    fit under the soft RLIMIT_NOFILE (raised to the hard limit first where that is allowed)."""
    import resource

    need = int(max_partitions) + FD_HEADROOM
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    if soft != resource.RLIM_INFINITY and soft < need:
        want = need if hard == resource.RLIM_INFINITY else min(need, hard)
        if want > soft:
            try:
                resource.setrlimit(resource.RLIMIT_NOFILE, (want, hard))
                soft = want
            except (ValueError, OSError):
                pass
        if soft < need:
            raise ValueError(f"to_parquet: max_partitions={max_partitions} open part files do not fit under this "
                             f"process's limit of {soft} open files (RLIMIT_NOFILE; {FD_HEADROOM} are left to the "
                             "rest of the process): lower max_partitions or raise the limit")


def key_dtype_name(col) -> str:
    """What ``_metadata.json`` records for a key column."""
    from .device import numpy_dtype

    return "string" if col.strings is not None else str(numpy_dtype(col.data.dtype))


def check_key_columns(frame, keys: Sequence[str]):
    """A key is a flat integer or flat string column: anything else raises TypeError."""
    import torch

    ints = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
    for k in keys:
        col = frame[k]
        if col.is_list or col.logical is not None or (col.strings is None and col.data.dtype not in ints):
            kind = "a list" if col.is_list else (str(col.logical) if col.logical is not None else str(col.data.dtype))
            raise TypeError(f"to_parquet: partition_on column {k!r} is {kind}; keys are flat integer or string "
                            "columns: cast it first")


class HiveSplitter:
    """Splits every input partition of one to_parquet call by its key tuple.  ``split`` permutes the
    partition once so that the rows of a tuple are contiguous (in input order), drops the key columns
    and names the row range of every tuple with the call-wide index of its directory, in first-seen
    order; ``fname`` is that directory's part file, relative to the output path.

    Two read-backs per input partition: the labels' state and first rows (kernels_labels), then the
    counts together with the key values at the first rows."""

    def __init__(self, output_path: str, keys: Sequence[str], rank: int, suffix: str, max_partitions: int):
        self.output_path, self.keys, self.rank, self.suffix = output_path, list(keys), rank, suffix
        self.max_partitions = int(max_partitions)
        self.index: Dict[str, int] = {}      # directory -> file index
        self.dirs: List[str] = []
        self.dtypes: Optional[List[str]] = None

    def fname(self, j: int) -> str:
        os.makedirs(os.path.join(self.output_path, self.dirs[j]), exist_ok=True)
        return f"{self.dirs[j]}/part_{self.rank}{self.suffix}"

    def split(self, part):
        """-> (the permuted partition without its key columns, [(file index, first row, row behind the
        last)])."""
        import torch

        from . import kernels as K
        from .kernels_labels import split_plan

        check_key_columns(part, self.keys)
        if self.dtypes is None:
            self.dtypes = [key_dtype_name(part[k]) for k in self.keys]
        n = len(part)
        if n == 0:
            return part.drop(self.keys), []
        perm, counts, first = split_plan(part, self.keys)
        D = len(first)
        idx = torch.from_numpy(first).to(perm.device)
        words = [counts]
        cols = [part[k].materialize() for k in self.keys]
        for col in cols:
            words.append(col.data[idx].to(torch.int64))
            words.append(((col.valid[idx >> 3] >> (idx & 7).to(torch.uint8)) & 1).to(torch.int64)
                         if col.valid is not None else torch.ones(D, dtype=torch.int64, device=perm.device))
        K.stat_add("hive_split_readback")
        host = K.read_back(torch.cat(words)).reshape(1 + 2 * len(cols), D)
        values = []
        for c, col in enumerate(cols):
            v, ok = host[1 + 2 * c], host[2 + 2 * c]
            if col.strings is not None:
                values.append([col.strings[int(s)] if o else None for s, o in zip(v, ok)])
            else:
                values.append([int(s) if o else None for s, o in zip(v, ok)])
        ranges, s0 = [], 0
        for g in range(D):
            d = dir_name(self.keys, [vals[g] for vals in values])
            j = self.index.get(d)
            if j is None:
                if len(self.dirs) >= self.max_partitions:
                    raise ValueError(f"to_parquet: partition_on={self.keys} gives more than max_partitions="
                                     f"{self.max_partitions} directories")
                j = self.index[d] = len(self.dirs)
                self.dirs.append(d)
            c = int(host[0][g])
            ranges.append((j, s0, s0 + c))
            s0 += c
        return part.drop(self.keys).take_rows(perm), ranges
