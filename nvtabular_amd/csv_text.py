"""The host half of ``Dataset(engine="csv")``: which files, which names and dtypes, and where the
partitions are cut.  The bytes of a partition are parsed on the device (kernels_csv.py).

A partition is a byte range of one file of about ``part_size`` bytes, extended forward to the
next newline.  The cut points are found when the Dataset is built, by reading a small window at
every nominal boundary, so ``npartitions`` is known up front and no partition depends on another.

Deviations from ``pandas.read_csv`` ("CSV in"): only the empty field is null (``NA``,
``null`` ... are strings), short rows are an error, blank lines are rows, whitespace is kept, a
quoted field cannot hold a newline; ``parse_dates`` takes column names only and one fixed ISO-8601
grammar ("Datetime columns")."""
from __future__ import annotations

import csv
import glob
import io
import os
import re
from typing import Dict, List, Optional, Tuple

import numpy as np

TEXT_SUFFIXES = (".csv", ".tsv", ".txt")
COMPRESSED_SUFFIXES = (".gz", ".bz2", ".zip", ".xz", ".zst", ".lz4", ".z")
DEFAULT_PART_SIZE = 128 << 20
MAX_PART_SIZE = 1 << 30          # field offsets are 32-bit and a range grows by one line at most
SAMPLE_BYTES = 64 << 10          # dtype inference reads this much of the first file
_WINDOW = 64 << 10               # bytes read per step when looking for the newline after a cut
DTYPES = ("int32", "int64", "float32", "float64", "string")
DATETIME = "datetime64[ns]"      # the dtype of a column named in parse_dates (never inferred)
_UNITS = {"": 1, "b": 1, "k": 10 ** 3, "kb": 10 ** 3, "m": 10 ** 6, "mb": 10 ** 6, "g": 10 ** 9, "gb": 10 ** 9,
          "kib": 1 << 10, "mib": 1 << 20, "gib": 1 << 30}


def parse_size(part_size) -> int:
    """``part_size`` (None, an int or a string such as "128MB" / "1 GiB") -> bytes, 1 to 1 GiB."""
    if part_size is None:
        return DEFAULT_PART_SIZE
    if isinstance(part_size, str):
        m = re.fullmatch(r"\s*(\d+(?:\.\d+)?)\s*([A-Za-z]*)\s*", part_size)
        if m is None or m.group(2).lower() not in _UNITS:
            raise ValueError(f"part_size: cannot read {part_size!r} (an int or e.g. '128MB', '1GiB')")
        size = int(float(m.group(1)) * _UNITS[m.group(2).lower()])
    elif isinstance(part_size, (int, np.integer)) and not isinstance(part_size, bool):
        size = int(part_size)
    else:
        raise ValueError(f"part_size: cannot read {part_size!r} (an int or e.g. '128MB', '1GiB')")
    if not 1 <= size <= MAX_PART_SIZE:
        raise ValueError(f"part_size must be 1 byte to 1 GiB, got {part_size!r}")
    return size


def _is_path(x) -> bool:
    return isinstance(x, (str, os.PathLike))


def _listing(d: str) -> List[str]:
    """The regular files of a directory, sorted, without hidden and ``_``-prefixed ones."""
    names = sorted(n for n in os.listdir(d) if not n.startswith((".", "_")))
    return [os.path.join(d, n) for n in names if os.path.isfile(os.path.join(d, n))]


def expand_files(paths) -> List[str]:
    """Paths, directories and globs -> files, sorted within a directory or glob.  A directory
    contributes its .csv / .tsv / .txt files, or every regular file when it has none of those."""
    if _is_path(paths):
        paths = [paths]
    files: List[str] = []
    for p in paths:
        p = str(p)
        if os.path.isdir(p):
            found = _listing(p)
            files += [f for f in found if f.lower().endswith(TEXT_SUFFIXES)] or found
        elif any(ch in p for ch in "*?["):
            files += sorted(glob.glob(p))
        else:
            files.append(p)
    return files


def _compressed(path: str) -> bool:
    return path.lower().endswith(COMPRESSED_SUFFIXES)


def _first_file(src) -> Optional[str]:
    """The file that decides the engine when none is named: the first of the sorted listing of a
    directory or glob.  A directory that holds any .parquet file is a parquet directory, as it
    always was (the parquet reader takes its ``*.parquet`` and ignores what lies beside them)."""
    p = str(src if _is_path(src) else src[0])
    if os.path.isdir(p):
        found = _listing(p)
        parquet = [f for f in found if f.lower().endswith(".parquet")]
        return (parquet or found or [None])[0]
    if any(ch in p for ch in "*?["):
        return (sorted(glob.glob(p)) or [None])[0]
    return p


def select_engine(src, engine) -> Optional[str]:
    """"csv" when ``src`` (a path or a list of paths) is read as delimited text, None when it goes
    where it always went.  With ``engine=None`` the first file's suffix decides."""
    if not (_is_path(src) or (isinstance(src, (list, tuple)) and src and _is_path(src[0]))):
        return None
    if engine == "csv":
        bad = [f for f in expand_files(src) if _compressed(f)]
        if bad:
            raise NotImplementedError(f"compressed text is not supported: {bad[0]}")
        return "csv"
    first = _first_file(src) if engine is None else None
    if first is None:
        return None
    low = first.lower()
    if _compressed(low) and os.path.splitext(low)[0].endswith(TEXT_SUFFIXES):
        raise NotImplementedError(f"compressed text is not supported: {first}")
    return "csv" if low.endswith(TEXT_SUFFIXES) else None


def _dtype_name(name: str, dt) -> str:
    if dt is str or dt is object or (isinstance(dt, str) and dt in ("string", "str", "object")):
        return "string"
    try:
        s = str(np.dtype(dt))
    except TypeError:
        s = str(dt)
    if s == "object":
        return "string"
    if s not in DTYPES:
        hint = f"; name the column in parse_dates=['{name}'] to read ISO-8601 text" if s.startswith("datetime64") else ""
        raise TypeError(f"column '{name}': dtype {dt!r} is not supported by the csv engine "
                        f"(int32, int64, float32, float64 or string){hint}")
    return s


class CsvSource:
    """Files, names, dtypes and byte ranges of a delimited-text dataset."""

    def __init__(self, paths, sep=",", names=None, header="infer", dtypes=None, part_size=None, quotechar='"',
                 parse_dates=None):
        """``parse_dates``: names of the columns that hold ISO-8601 text
        (``YYYY-MM-DD[(T| )HH:MM[:SS[.fffffffff]]]``, no zone); they become datetime64[ns]."""
        if not isinstance(sep, str) or len(sep.encode()) != 1 or sep in "\r\n":
            raise ValueError(f"sep must be one single-byte character other than a line end, got {sep!r}")
        if quotechar is not None and (not isinstance(quotechar, str) or len(quotechar.encode()) != 1
                                      or quotechar in "\r\n" or quotechar == sep):
            raise ValueError(f"quotechar must be one single-byte character other than sep, got {quotechar!r}")
        if header not in ("infer", None, 0) or header is False:
            raise ValueError(f"header must be 'infer', 0 or None, got {header!r}")
        if header is None and names is None:
            raise ValueError("header=None needs names=[...]")
        self.sep, self.quotechar = sep, quotechar
        self.part_size = parse_size(part_size)
        self.files = expand_files(paths)
        if not self.files:
            raise FileNotFoundError(f"no text files under {paths}")
        for f in self.files:
            if _compressed(f):
                raise NotImplementedError(f"compressed text is not supported: {f}")
        self.has_header = header == 0 or (header == "infer" and names is None)
        if names is not None:
            self.names = [str(n) for n in names]
        else:
            self.names = self._header_fields(self.files[0])[0]
        if not self.names or len(set(self.names)) != len(self.names):
            raise ValueError(f"column names must be unique and not empty: {self.names}")
        given = dict(dtypes or {})
        unknown = [c for c in given if c not in self.names]
        if unknown:
            raise ValueError(f"dtypes: unknown column(s) {unknown}")
        self.dtypes: Dict[str, str] = {c: _dtype_name(c, dt) for c, dt in given.items()}
        if parse_dates is None or parse_dates is False:
            parse_dates = []
        if isinstance(parse_dates, str) or not isinstance(parse_dates, (list, tuple)) or \
                not all(isinstance(c, str) for c in parse_dates):
            raise ValueError(f"parse_dates must be a list of column names, got {parse_dates!r}")
        unknown = [c for c in parse_dates if c not in self.names]
        if unknown:
            raise ValueError(f"parse_dates: unknown column(s) {unknown}")
        both = [c for c in parse_dates if c in given]
        if both:
            raise ValueError(f"column(s) {both} are named in both dtypes and parse_dates")
        self.dtypes.update({c: DATETIME for c in parse_dates})
        if len(self.dtypes) < len(self.names):
            self._infer_dtypes()
        self.dtypes = {c: self.dtypes[c] for c in self.names}
        self.ranges: List[Tuple[str, int, int]] = []
        for f in self.files:
            self.ranges += self._cut(f)

    # ---- header / inference ---------------------------------------------------------------------
    def _header_fields(self, path):
        """(names on the first line, its length in bytes with the line end)."""
        with open(path, "rb") as f:
            line = f.readline()
        text = line.decode("utf-8").rstrip("\r\n")
        kw = dict(quoting=csv.QUOTE_NONE) if self.quotechar is None else dict(quotechar=self.quotechar)
        rows = list(csv.reader([text], delimiter=self.sep, **kw))
        return (rows[0] if rows else []), len(line)

    def _infer_dtypes(self):
        import pandas as pd

        with open(self.files[0], "rb") as f:
            sample = f.read(SAMPLE_BYTES + 1)
        if len(sample) > SAMPLE_BYTES:     # more file behind the sample: cut it at a line end
            cut = sample.rfind(b"\n", 0, SAMPLE_BYTES)
            sample = sample[:cut + 1] if cut >= 0 else sample[:SAMPLE_BYTES]
        # the columns whose dtype was given are read as text: the sample may hold an empty field in
        # an integer column, which pandas refuses and this engine reads as a null
        explicit = {c: str for c in self.dtypes}
        kw = dict(quoting=csv.QUOTE_NONE) if self.quotechar is None else dict(quotechar=self.quotechar)
        df = pd.read_csv(io.BytesIO(sample), sep=self.sep, names=self.names, header=0 if self.has_header else None,
                         keep_default_na=False, na_values=[""], dtype=explicit, index_col=False, **kw)
        for c in self.names:
            if c in self.dtypes:
                continue
            kind = df[c].dtype.kind
            if kind == "i":
                self.dtypes[c] = "int64"
            elif kind == "f":
                self.dtypes[c] = "float64"
            elif kind == "O":
                self.dtypes[c] = "string"
            else:
                raise TypeError(f"column '{c}' looks like {df[c].dtype}, which the csv engine does not read: "
                                f"pass dtypes={{'{c}': ...}} (int32, int64, float32, float64 or string)")

    # ---- partitions -------------------------------------------------------------------------------
    def _cut(self, path):
        size = os.path.getsize(path)
        start = self._header_fields(path)[1] if self.has_header else 0
        start = min(start, size)
        cuts = [start]
        with open(path, "rb") as f:
            nominal = start + self.part_size
            while nominal < size:
                # the first newline at or after byte nominal - 1 ends the range
                pos, cut = nominal - 1, None
                while pos < size and cut is None:
                    f.seek(pos)
                    window = f.read(_WINDOW)
                    at = window.find(b"\n")
                    if at >= 0:
                        cut = pos + at + 1
                    pos += len(window)
                if cut is None or cut >= size:
                    break
                if cut > cuts[-1]:
                    cuts.append(cut)
                nominal += self.part_size
        cuts.append(size)   # (every cut before it is below size; an empty file body is one empty range)
        return [(path, a, b) for a, b in zip(cuts, cuts[1:])]

    def read_range(self, i: int, pinned: bool = True):
        """(buffer, n): the bytes of partition i in a host buffer whose size is a multiple of 16,
        n of them text.  The text always ends in a newline (one is added to a file's last range
        when the file lacks it)."""
        path, a, b = self.ranges[i]
        n = b - a
        if n + 1 >= (1 << 31):
            raise ValueError(f"{path}: a partition of {n} bytes (one line?) exceeds the 2 GiB the index addresses")
        size = max(16, (n + 1 + 15) & ~15)
        if pinned:
            import torch

            buf = torch.empty(size, dtype=torch.uint8, pin_memory=True)
            arr = buf.numpy()
        else:
            buf = arr = np.empty(size, dtype=np.uint8)
        if n:
            with open(path, "rb") as f:
                f.seek(a)
                got = f.readinto(memoryview(arr)[:n])
            if got != n:
                raise IOError(f"{path}: read {got} of {n} bytes (the file changed?)")
            if arr[n - 1] != 0x0A:
                arr[n] = 0x0A
                n += 1
        return buf, n

    def where(self, i: int) -> str:
        path, a, b = self.ranges[i]
        return f"{path} (bytes {a}-{b})" if len(self.ranges) > len(self.files) else path

    def schema(self):
        from .schema import ColumnSchema, Schema

        return Schema([ColumnSchema(c, object if d == "string" else np.dtype(d)) for c, d in self.dtypes.items()])

    def read_partition(self, i: int, columns=None, device=None):
        """Partition i as a DeviceFrame (the columns named, in file order; all with None)."""
        from . import kernels_csv as KC
        from .device import default_device

        device = device or default_device()
        want = [c for c in self.names if columns is None or c in columns]
        buf, n = self.read_range(i)
        if n == 0:
            return KC.empty_frame(want, self.dtypes, device)
        text = buf.to(device, non_blocking=True)
        quote = -1 if self.quotechar is None else self.quotechar.encode()[0]
        return KC.parse_text(text, n, buf.numpy(), self.sep.encode()[0], quote, self.names, self.dtypes, want,
                             self.where(i))
