"""Dataset: a partitioned table source (re-creation of the slice of
merlin.io.Dataset the hot path touches: SURVEY section 8(b) "Dataset").

Sources: pandas DataFrame, DeviceFrame, pyarrow Table, parquet path(s) or a list
of already-partitioned frames.  ``to_iter()`` yields HBM-resident DeviceFrames;
parquet row groups are decoded by the hand-written reader where it takes the file
(parquet_plain.py: ``PlainParquetFile.decodable``, ``StagedPartition``), else by pyarrow
straight into Arrow buffers, and copied to the device without going through pandas.
``to_parquet`` hands frames to the PLAIN write driver (parquet_write.py) or to pyarrow.
"""
from __future__ import annotations

import glob
import os
import threading
from typing import Iterable, List, Optional

import pandas as pd

from .device import DeviceFrame, as_device_frame
from .parquet_plain import READER_CHUNKS, PlainParquetFile, StagedPartition, read_row_groups_staged
from .kernels_parquet_str_out import StringTables
from .parquet_write import LAST_TIMING, device_permutation, dictionary_columns, plain_eligible, write_plain  # noqa: F401
from .schema import ColumnSchema, Schema


_STATS_LOCK = threading.Lock()   # Dataset.filter_stats is updated from the prefetch thread
DECODE_AHEAD = int(os.environ.get("NVT_DECODE_AHEAD", "3"))  # parquet partitions decoded concurrently ahead of the consumer


class _Collection:
    """What ``Dataset.to_ddf()`` returns: ``.compute()`` gives one pandas frame."""

    def __init__(self, ds: "Dataset"):
        self._ds = ds

    def compute(self, **_):
        return self._ds.compute()

    def head(self, n=5):
        return self.compute().head(n)

    @property
    def columns(self):
        return self._ds.schema.column_names

    @property
    def npartitions(self):
        return self._ds.npartitions


class Dataset:
    def __init__(self, path_or_source, engine=None, cpu=None, part_size=None,
                 part_mem_fraction=None, npartitions=None, names=None, schema=None,
                 row_groups_per_part=1, sep=",", header="infer", dtypes=None, quotechar='"', parse_dates=None,
                 filters=None, **kwargs):
        """``engine``: "parquet", "csv" or None (a first file ending in .csv / .tsv / .txt selects
        csv; anything else is read as parquet).  ``sep``, ``names``, ``header``, ``dtypes``,
        ``part_size``, ``quotechar`` and ``parse_dates`` belong to the csv engine (csv_text.py):
        delimited text is cut into byte ranges of about ``part_size`` and parsed on the device; the
        columns named in ``parse_dates`` (ISO-8601 text) become datetime64[ns].

        A parquet directory without ``*.parquet`` files at its top level but with ``name=value``
        subdirectories is read as a hive-partitioned dataset (hive.py): the leaf directories' files
        are the pieces, in sorted walk order, and the key columns follow the files' columns in path
        order.  Their values come from the paths (``__HIVE_DEFAULT_PARTITION__`` is a null); their
        dtypes from ``_metadata.json`` (``partition_on``, as ``to_parquet`` records it), else int64
        when every non-null segment of a key is ``-?[0-9]+`` and string otherwise.

        ``filters``: ``None`` (default) reads every row.  A list of ``(column, op, value)`` tuples (one
        conjunction) or a list of such lists (an OR of conjunctions) reads the rows that pass, with the
        semantics of ``pyarrow.parquet.read_table(filters=...)`` (filters.py): ``op`` is ``==``, ``=``,
        ``!=``, ``<``, ``<=``, ``>``, ``>=``, ``in`` or ``not in``; a null fails every comparison and
        ``in`` and passes ``not in``; NaN fails every comparison but ``!=``; ``-0.0 == 0.0``; ``in []``
        keeps nothing.  Integers, bools and datetimes compare exactly in int64, floats in float64: a
        float32 column is widened, the constant is not narrowed.  ``in`` on a float column compares
        every member as ``==`` in float64; pyarrow narrows the members to the column's type instead, so
        the two agree for members that type represents exactly.  Integer columns take integers (and
        floats of integral value), float columns ints and floats, bool columns ``True`` / ``False``,
        string columns ``str`` with ``==``, ``!=``, ``in``, ``not in`` only, datetime columns
        ``pandas.Timestamp`` / ``datetime.datetime`` / ``numpy.datetime64`` that are a whole count of the
        column's unit; hive key columns are ordinary columns.  Everything is checked here, before a
        file is read: a malformed filter, an unknown operator or column, more than 16 distinct columns
        or 64 terms raise ``ValueError``, a list column or a constant of another kind ``TypeError``; a
        callable source takes no filter.  Hive files whose path fails every conjunction are dropped
        before their footer is opened, row groups whose min / max / null-count statistics prove that no
        row passes are dropped from ``_pieces`` (``filter_stats`` counts both), and every partition
        that is read is filtered on the device by one ``nvt_compact_keep_terms`` launch plus the
        compaction (kernels_compact.filter_frame).  A partition that loses every row stays, with 0
        rows.  The schema does not change."""
        self.cpu = bool(cpu)  # accepted for API compatibility; compute always runs on the GPU
        self.engine = engine
        self._schema = schema
        self._parts_fn = None
        self._filter = None   # filters.Filter: applied to every partition where it becomes a DeviceFrame
        self.filter_stats = None
        dnf = None
        if filters is not None:
            from .filters import normalize

            dnf = normalize(filters)
            self.filter_stats = {"files_pruned": 0, "row_groups_pruned": 0, "row_groups_kept": 0,
                                 "rows_in": 0, "rows_out": 0}
        src = path_or_source
        if callable(src):  # lazy partition generator (transformed datasets)
            if dnf is not None:
                raise ValueError("filters= needs a source with a schema up front; a callable source has none")
            self._parts_fn = src
            self._n = npartitions
        elif isinstance(src, (pd.DataFrame, DeviceFrame)) or _is_arrow_table(src):
            self._init_frames(_split(src, npartitions or 1))
        elif isinstance(src, (list, tuple)) and src and not isinstance(src[0], (str, os.PathLike)):
            self._init_frames(list(src))
        elif _csv_engine(src, engine):
            self._init_csv(src, sep, names, header, dtypes, part_size, quotechar, parse_dates)
        else:
            self._init_parquet(src, row_groups_per_part, names, dnf)
        if dnf is not None and self._filter is None:
            from .filters import validate

            self._filter = validate(dnf, self.schema)

    # ---- sources ---------------------------------------------------------------
    def _init_frames(self, frames):
        self._frames = frames
        self._n = len(frames)
        if self._schema is None:
            f0 = frames[0]
            self._schema = Schema.from_frame(f0.schema if _is_arrow_table(f0) else f0)
        self._parts_fn = lambda columns=None: iter(self._frames)

    def _init_csv(self, paths, sep, names, header, dtypes, part_size, quotechar, parse_dates=None):
        """Delimited text: one partition per byte range (csv_text.CsvSource), parsed on the device
        when it is read.  There is no ``_pieces``: row counts come from reading the partitions."""
        from .csv_text import CsvSource

        self.engine = "csv"
        src = self._csv = CsvSource(paths, sep=sep, names=names, header=header, dtypes=dtypes,
                                    part_size=part_size, quotechar=quotechar, parse_dates=parse_dates)
        self._n = len(src.ranges)
        if self._schema is None:
            self._schema = src.schema()
        self._forwards_shard = True   # a global list of byte ranges: rank r reads every world-th one

        def gen(columns=None, shard=None):
            for i in range(len(src.ranges)):
                if shard is None or i % shard[1] == shard[0]:
                    yield src.read_partition(i, columns)

        self._parts_fn = gen

    def _init_parquet(self, paths, row_groups_per_part, names, dnf=None):
        import pyarrow.parquet as pq

        from . import filters as F

        if isinstance(paths, (str, os.PathLike)):
            paths = [str(paths)]
        files: List[str] = []
        hive = None   # the layout of a hive-partitioned directory (hive.HiveLayout)
        for p in paths:
            p = str(p)
            if os.path.isdir(p):
                found = sorted(glob.glob(os.path.join(p, "*.parquet")))
                if not found and len(paths) == 1:
                    # no parquet file at the top level: key=value directories are walked
                    from .hive import layout_of

                    hive = layout_of(p)
                    found = hive.files if hive is not None else []
                files += found
            elif any(ch in p for ch in "*?["):
                files += sorted(glob.glob(p))
            else:
                files.append(p)
        if not files:
            raise FileNotFoundError(f"no parquet files under {paths}")
        self._hive = hive
        alive = {}    # file -> the conjunctions its hive path leaves standing (filters only)
        if dnf is not None and hive is not None:
            # the key terms decide on the path alone: a file no conjunction survives is dropped
            # before its footer is opened (the key columns' dtypes come from the layout)
            import numpy as np

            key_schema = Schema([ColumnSchema(k, object if dt == "string" else np.dtype(dt))
                                 for k, dt in zip(hive.keys, hive.dtypes)])
            on_keys = F.validate(dnf, key_schema, partial=True)
            kept = []
            for f in files:
                typed = {k: F.segment_value(t, dt) for k, dt, t in zip(hive.keys, hive.dtypes, hive.values[f])}
                alive[f] = on_keys.alive_on_keys(typed)
                if alive[f]:
                    kept.append(f)
                else:
                    self.filter_stats["files_pruned"] += 1
            first_file = kept[0] if kept else files[0]
            files = kept
        else:
            first_file = files[0]
        self._files = files
        if self._schema is None:
            import numpy as np
            import pyarrow as pa

            file_schema = pq.ParquetFile(first_file).schema_arrow
            if hive is not None:   # the key columns behind the files' columns, in path order
                for name, dt in zip(hive.keys, hive.dtypes):
                    file_schema = file_schema.append(pa.field(name, pa.string() if dt == "string" else
                                                              pa.from_numpy_dtype(np.dtype(dt))))
            self._schema = Schema.from_frame(file_schema)
        flt = self._filter = F.validate(dnf, self.schema) if dnf is not None else None
        pieces = []
        for f in files:
            md = pq.ParquetFile(f)
            if hive is not None:
                from .hive import check_clash

                check_clash(hive.keys, md.schema_arrow.names, f)
            groups = list(range(md.num_row_groups))
            if flt is not None:
                # row groups whose statistics prove that no row passes are never read
                meta, fields = md.metadata, md.schema_arrow
                columns = F.flat_columns(meta)
                pruned = {g for g in groups if flt.prunes_row_group(meta.row_group(g), columns, fields, alive.get(f))}
                self.filter_stats["row_groups_pruned"] += len(pruned)
                self.filter_stats["row_groups_kept"] += len(groups) - len(pruned)
            else:
                pruned = ()
            for g0 in range(0, len(groups), row_groups_per_part):
                part = [g for g in groups[g0: g0 + row_groups_per_part] if g not in pruned]
                if part:   # (a piece that loses all of its row groups disappears)
                    pieces.append((f, part))
        self._pieces = pieces
        self._n = len(pieces)

        # files the hand-written reader takes (flat numeric columns, three-level lists of such
        # leaves and flat string columns; PLAIN or dictionary-encoded values, uncompressed or snappy:
        # parquet_plain.PlainParquetFile.decodable); everything else is
        # decoded by pyarrow and counted in parquet_plain.READER_CHUNKS
        plain_files = {}

        def plain_file(f):
            if f not in plain_files:
                pf = None
                if PLAIN_PARQUET_READ:
                    try:
                        pf = PlainParquetFile(f)
                        if not pf.decodable:
                            pf = None
                    except Exception:
                        pf = None
                plain_files[f] = pf
            return plain_files[f]

        def read(piece, columns):
            if hive is None:
                return read_file(piece, columns)
            # the key columns are not passed to the file readers: the path spells them, and they are
            # attached where the partition becomes a DeviceFrame (hive.HivePart.to_device)
            from .hive import HivePart

            f, groups = piece
            want = hive.keys if columns is None else [c for c in columns if c in hive.keys]
            file_cols = None if columns is None else [c for c in columns if c not in hive.keys]
            if file_cols is not None and not file_cols:   # only key columns: the footer has the row count
                md = pq.ParquetFile(f).metadata
                return HivePart(None, sum(md.row_group(g).num_rows for g in groups), hive, hive.values[f], want)
            inner = read_file(piece, file_cols)
            return HivePart(inner, inner.num_rows, hive, hive.values[f], want)

        def read_file(piece, columns):
            f, groups = piece
            pf = plain_file(f)
            if pf is not None:
                try:
                    return StagedPartition(read_row_groups_staged(pf, groups, columns, pool=_plain_read_pool()))
                except Exception as e:  # (a page kind the footer did not announce: pyarrow reads it)
                    from . import _lib

                    if not isinstance(e, _lib.NvtHipError):
                        raise
                    plain_files[f] = None
            table = pq.ParquetFile(f).read_row_groups(groups, columns=columns)
            READER_CHUNKS["pyarrow"] += table.num_columns * len(groups)   # (counted: never silent)
            return table

        def gen(columns=None, only=None):
            # decode a few partitions ahead on host threads (one read spreads over the columns of
            # its row groups; several reads in flight keep more of the host cores busy)
            from collections import deque
            from concurrent.futures import ThreadPoolExecutor

            todo = [p for i, p in enumerate(pieces) if only is None or only(i)]
            if len(todo) <= 1:
                for piece in todo:
                    yield read(piece, columns)
                return

            with ThreadPoolExecutor(max_workers=DECODE_AHEAD) as pool:
                window = deque()
                it = iter(todo)
                for piece in it:
                    window.append(pool.submit(read, piece, columns))
                    if len(window) >= DECODE_AHEAD:
                        break
                while window:
                    table = window.popleft().result()
                    nxt = next(it, None)
                    if nxt is not None:
                        window.append(pool.submit(read, nxt, columns))
                    yield table

        self._parts_fn = gen

    # ---- public surface -----------------------------------------------------------
    @property
    def schema(self) -> Schema:
        if callable(self._schema):
            # a transformed dataset: the fitted output schema (embedding sizes ...) is folded
            # together on first use, not before the first partition's kernels are enqueued
            self._schema = self._schema()
        if self._schema is None:
            first = next(iter(self._parts_fn()))
            self._schema = Schema.from_frame(first)
        return self._schema

    @property
    def npartitions(self):
        if self._n is None:
            self._n = sum(1 for _ in self._parts_fn())
        return self._n

    def _host_parts(self, cols, shard):
        """Partitions of this rank.  Under torch.distributed (shard = (rank, world)):

        * a parquet dataset is a GLOBAL list of files / row groups that every rank opens the
          same way: rank r takes every world-th partition and decodes only those;
        * frames handed over in memory (DataFrame, DeviceFrame, Arrow table, list of them) were
          built by THIS process: they are the rank's own shard already and are all kept;
        * a derived dataset (Workflow.transform) defers to its source."""
        if getattr(self, "_pieces", None) is not None:
            if shard is not None:
                yield from self._parts_fn(cols, only=lambda i: i % shard[1] == shard[0])
            else:
                yield from self._parts_fn(cols)
            return
        if getattr(self, "_forwards_shard", False):
            yield from self._parts_fn(cols, shard=shard)
            return
        it = self._parts_fn(cols) if _accepts_columns(self._parts_fn) else self._parts_fn()
        yield from it

    def to_iter(self, columns: Optional[Iterable[str]] = None, shard=None, prefetch=None):
        """Yield DeviceFrame partitions.  shard=(rank, world) keeps every world-th one.

        Parquet sources are double-buffered: a background thread decodes the NEXT row-group
        range with pyarrow (GIL released), stages it in pinned memory and issues the
        host-to-device copies on a side stream while the consumer's kernels run on the
        current stream; the hand-over is a stream event, not a device synchronise."""
        cols = list(columns) if columns is not None else None
        if prefetch is None:
            prefetch = hasattr(self, "_pieces")
        read, post = cols, None
        if self._filter is not None:
            # a filter column the caller leaves out is read, and dropped after the filter
            if cols is not None:
                read = cols + [c for c in self._filter.columns if c not in cols]
            post = self._filter_frame
        if not prefetch:
            for part in self._host_parts(read, shard):
                frame, _ = as_device_frame(part)
                if post is not None:
                    frame = post(frame)
                if cols is not None:
                    frame = frame[[c for c in cols if c in frame]]
                yield frame
            return
        yield from _prefetch_frames(self._host_parts(read, shard), cols, post=post)

    def _filter_frame(self, frame):
        """The rows of one partition that pass ``filters=`` (every consumer gets its partitions through
        here); ``filter_stats`` counts the rows in and out."""
        from .kernels_compact import filter_frame

        out = filter_frame(frame, self._filter)
        with _STATS_LOCK:
            self.filter_stats["rows_in"] += len(frame)
            self.filter_stats["rows_out"] += len(out)
        return out

    def to_ddf(self, columns=None, **_):
        return _Collection(self if columns is None else self._select(columns))

    def _select(self, columns):
        cols = list(columns)
        return Dataset(lambda columns=None: (p[cols] for p in self.to_iter(cols)),
                       schema=self.schema.select_by_name(cols), npartitions=self._n)

    def compute(self) -> pd.DataFrame:
        parts = [p.to_pandas() for p in self.to_iter()]
        if not parts:
            return pd.DataFrame(columns=self.schema.column_names)
        return pd.concat(parts, ignore_index=True)

    def head(self, n=5):
        for p in self.to_iter():
            return p.to_pandas().head(n)
        return pd.DataFrame()

    def to_cpu(self):
        self.cpu = True
        return self

    def to_gpu(self):
        self.cpu = False
        return self

    def shuffle_by_keys(self, keys, hive_data=None, npartitions=None) -> "Dataset":
        """Move every row to the partition its key hashes to (merlin.io.Dataset.shuffle_by_keys): all
        rows with the same values in ``keys`` end up in one partition, which is what per-partition
        operators such as ``ops.Groupby`` and ``ops.DifferenceLag(partition_cols=...)`` assume.

        * ``keys``: a column name or a list of 1 to 4 names; string, integer, bool and float columns
          (a null is a key value of its own, -0.0 equals 0.0); list columns cannot be keys.
        * ``npartitions``: output partitions, 1 to 4096; default ``self.npartitions``.  A partition
          that receives no rows is still there, empty and with the right dtypes.
        * ``hive_data``: ``None`` / ``False`` shuffle on the device.  ``True`` (the reference's
          short cut for hive-partitioned directories) is not supported.

        The shuffle runs eagerly on the device (kernels_partition.shuffle_frames) and is stable: an
        output partition holds its rows of input partition 0 in their original order, then those
        of input partition 1, and so on.  All input partitions and all output partitions are
        resident at once -- about twice the dataset in HBM (list columns: a third copy of them while
        the call runs); nothing is spilled to the host.
        Returns a new in-memory Dataset with the same schema and column order."""
        from . import _lib, dist

        keys = [keys] if isinstance(keys, str) else list(keys)
        if not keys:
            raise ValueError("shuffle_by_keys needs at least one key column")
        if len(keys) > _lib.JOIN_MAX_KEYS:
            raise NotImplementedError(f"shuffle_by_keys takes at most {_lib.JOIN_MAX_KEYS} key columns, "
                                      f"got {len(keys)}")
        if hive_data:
            raise NotImplementedError("hive-partitioned directories are not tracked by this Dataset")
        P = self.npartitions if npartitions is None else int(npartitions)
        if not 1 <= P <= _lib.PARTITION_MAX:
            raise ValueError(f"npartitions must be 1 to {_lib.PARTITION_MAX}, got {P}")
        schema = self.schema
        missing = [k for k in keys if k not in schema]
        if missing:
            raise ValueError(f"shuffle_by_keys: unknown key columns {missing}")
        lists = [k for k in keys if schema[k].is_list]
        if lists:
            raise TypeError(f"shuffle_by_keys: list columns cannot be keys: {lists}")
        if dist.world_size() > 1:
            raise NotImplementedError("shuffle_by_keys across ranks is not supported")
        from .kernels_partition import shuffle_frames

        return Dataset(shuffle_frames(list(self.to_iter()), keys, P), schema=schema)

    def to_parquet(self, output_path, shuffle=None, out_files_per_proc=None, dtypes=None,
                   cats=None, conts=None, labels=None, preserve_files=False, suffix=".parquet",
                   num_threads=0, compression=None, statistics=False, use_dictionary=None,
                   device_compression=None, partition_on=None, max_partitions=1024, **_):
        """Write the (transformed) dataset as parquet (merlin.io.Dataset.to_parquet; contract in
        tests/unit/workflow/test_workflow.py:171-187,363-396,444-500 and
        bench/datasets/tools/nvt_etl.py:154-171 of the reference).

        * ``out_files_per_proc=k``: every partition is cut into k pieces, piece j appended to
          ``part_j.parquet`` -- k files per process (``part_{rank*k + j}`` under torchrun).
          ``None``: one file per input partition.
        * ``shuffle``: ``Shuffle.PER_PARTITION`` permutes the rows of each partition (on the
          device, before the copy out); ``Shuffle.PER_WORKER`` additionally permutes each
          output file as a whole (its pieces are held on the host until the end); ``None`` /
          ``False`` keeps the row order.
        * ``dtypes``: {column: dtype} casts applied on the way out (an entry that names a list
          column sends the frame to pyarrow, whose cast does not convert lists).
        * ``compression``: ``None`` (default) lets frames of flat int32 / int64 / float32 / float64 and
          datetime columns, list columns with such number leaves (written as the standard
          three-level list, levels packed on the device) and flat string columns on the device
          (BYTE_ARRAY / UTF8 pages filled on the device from the surrogates and the column's dict;
          lists of strings, string columns on the host, with a ``dtypes`` entry, with a dict value
          that is not a ``str`` or with an entry longer than 2^30 - 4 bytes send the frame to
          pyarrow) take the hand-written PLAIN writer (uncompressed pages, no dictionary, no column statistics: files are larger
          than pyarrow's snappy + dictionary output and carry no min / max for predicate
          pushdown -- the price of writing at tens of GB/s); any codec name (``"snappy"``,
          ``"zstd"``, ``"none"`` ...) selects pyarrow's writer with that codec, statistics and
          dictionary pages, as the reference's writer produces.  ``NVT_PLAIN_PARQUET=0`` makes
          pyarrow the default.
        * ``statistics=True``: the PLAIN writer also records min / max of every column chunk
          (computed on the device next to the copy out); the null count of every chunk is always
          written.  String columns get no min / max.  pyarrow's writer always writes statistics.
        * ``use_dictionary`` (pyarrow's name and value shapes): ``None`` / ``False`` (default) write
          exactly the PLAIN pages described above.  ``True`` offers every flat int32 / int64 column
          (after a ``dtypes`` cast), every datetime column, every flat string column (its
          dictionary page holds the chunk's distinct strings; the rule below is then in bytes) and
          every list column of int32 / int64
          leaves to the PLAIN writer's dictionary encoding, which runs on the device (columns of a
          frame on the host are not offered); float columns stay PLAIN silently (repeated floats
          are not dictionary-encoded).  A list of column names offers only those; a
          name that is no column, or no such column, raises ``ValueError`` before any file is
          created.  An offered column chunk gets a dictionary page (its distinct values, ascending)
          and ``RLE_DICTIONARY`` data pages whose indices are bit-packed on the device, but only when
          that makes the chunk smaller and it has at most 2^20 distinct values -- otherwise that
          chunk stays PLAIN, so the option never makes a file larger ("Dictionary pages
          in the PLAIN parquet writer").  When the frame goes to pyarrow's writer anyway (lists of
          strings, a codec, ``Shuffle.PER_WORKER`` with ``out_files_per_proc``, ``NVT_PLAIN_PARQUET=0``), a
          value other than ``None`` is handed to pyarrow as its own ``use_dictionary``.
        * ``device_compression``: ``None`` (default) writes exactly the files described above.
          ``"snappy"`` (case-insensitive) keeps the frame with the PLAIN writer and compresses its
          pages on the device: the pages are cut where they are cut today, a page body becomes a
          snappy raw stream (the level bytes inside one literal, the values region parsed on the
          device, one wave per 32 KiB fragment), and a column chunk is written SNAPPY only when that
          makes it smaller, page headers included -- otherwise it is written as today, so the option
          never makes a file larger (an incompressible float column costs one pass and nothing on
          disk).  The rule is applied after ``use_dictionary``'s, to the form the chunk takes: a
          dictionary chunk compresses its dictionary page.  Any other value, or a ``compression``
          next to it, raises ``ValueError`` before any file exists; ``compression="snappy"`` alone
          still selects pyarrow's writer.  When the frame goes to pyarrow's writer anyway, the value
          is handed to pyarrow as its ``compression`` ("Snappy pages in the PLAIN parquet
          writer").
        * ``partition_on``: ``None`` (default) writes exactly the files described above.  A column name
          or a list of 1 to 4 names writes a hive-partitioned dataset, laid out as
          ``pyarrow.parquet.write_to_dataset`` does: every input partition is split by the key tuple
          on the device (kernels_labels: a dense label per row, then one stable permutation), and the
          rows of a tuple are appended, in input order, as row groups of
          ``<k1>=<v1>/<k2>=<v2>/part_<rank><suffix>``; the key columns are not in the files.  A
          segment value is ``urllib.parse.quote(str(value), safe="")``, the empty string gives
          ``k=``, a null ``__HIVE_DEFAULT_PARTITION__``.  Keys are flat integer or flat string columns
          (nullable or not); a float, bool, datetime or list key raises ``TypeError`` (cast first); a
          name that is no column, a repeated name, keys that leave no data column,
          ``out_files_per_proc`` or ``Shuffle.PER_WORKER`` next to it raise ``ValueError`` -- all
          before anything is created.  ``Shuffle.PER_PARTITION`` shuffles first, then splits.  Every
          other option keeps its meaning, applied to the frame without its key columns.  At most
          4096 distinct tuples per input partition.  ``_metadata.json`` records the keys and their
          dtypes (``"partition_on"``), which ``Dataset(path)`` restores.
        * ``max_partitions`` (pyarrow's keyword and default): more directories than this over the
          whole call raise ``ValueError`` (the part files written so far are removed); one
          descriptor is held per directory, so a value that does not fit under the process's limit
          of open files is refused before anything is written.
        * writes ``_metadata`` (parquet summary of all row groups), ``_file_list.txt`` and
          ``_metadata.json`` (file stats + cats / conts / labels) next to the data files.
        """
        import itertools

        import pyarrow.parquet as pq

        from . import dist

        shuffle = Shuffle.coerce(shuffle)
        if device_compression is not None:   # (argument errors come before anything is created)
            if not isinstance(device_compression, str) or device_compression.lower() != "snappy":
                raise ValueError(f"to_parquet: device_compression takes None or 'snappy', not {device_compression!r}")
            if compression is not None:
                raise ValueError("to_parquet: compression= selects pyarrow's writer and device_compression= the PLAIN "
                                 f"writer's codec: pass one of them, not both ({compression!r}, {device_compression!r})")
            device_compression = "snappy"
        keys = self._partition_keys(partition_on, out_files_per_proc, shuffle, max_partitions)
        os.makedirs(str(output_path), exist_ok=True)
        output_path = str(output_path)
        rank, world = dist.rank(), dist.world_size()
        k = int(out_files_per_proc) if out_files_per_proc else None

        def fname(j):
            return f"part_{(rank * k + j) if k else (j * world + rank)}{suffix}"

        parts = iter(self.to_iter(shard=(rank, world) if world > 1 else None))
        first = next(parts, None)
        parts = itertools.chain([first], parts) if first is not None else iter(())
        splitter = None
        if keys:
            from . import _lib
            from .hive import HiveSplitter, check_key_columns

            _lib.require_gpu()
            splitter = HiveSplitter(output_path, keys, rank, suffix, max_partitions)
            fname = splitter.fname
            if first is not None:
                check_key_columns(first, keys)   # (TypeError before any file or directory is created)
                first = first.drop(keys)         # the writers' eligibility rules see the data columns
        tables = StringTables()   # the entry tables of string columns, for this call
        # (a frame on the host has nothing to compress its pages with: pyarrow gets the codec)
        on_host = device_compression is not None and first is not None and \
            not all(col.data.is_cuda for _, col in first.items())
        if first is not None and PLAIN_PARQUET and compression is None and not on_host and \
                not (shuffle == Shuffle.PER_WORKER and k) and plain_eligible(first, dtypes, tables):
            # fixed-width numeric columns, lists of them and flat string columns on the device: PLAIN
            # pages written straight from pinned column buffers (parquet_write.py; a string column's
            # BYTE_ARRAY pages are filled on the device from its surrogates and its dict's entries) --
            # no compression, no statistics, dictionary pages only on request.  Lists of strings,
            # string columns on the host, with a dtypes= entry or with a dict value that is no str,
            # bools and narrow leaves go to pyarrow below
            offered = dictionary_columns(first, dtypes, use_dictionary)   # (raises before any file exists)
            names, rows, order = write_plain(parts, output_path, fname, k, shuffle, dtypes, bool(statistics),
                                             PLAIN_ROW_GROUP, PLAIN_INFLIGHT, PLAIN_WRITE_THREADS, offered, tables,
                                             snappy=device_compression is not None, splitter=splitter)
            collector = [pq.read_metadata(os.path.join(output_path, names[j])) for j in order]
            schema = pq.read_schema(os.path.join(output_path, names[order[0]])) if order else None
        else:
            codec = compression if compression is not None else device_compression
            pq_kw = {} if codec is None else {"compression": codec}
            if use_dictionary is not None:
                pq_kw["use_dictionary"] = use_dictionary
            names, rows, order, schema, collector = _write_pyarrow(parts, output_path, fname, k, shuffle, dtypes, pq_kw,
                                                                   splitter)
        for md, j in zip(collector, order):
            md.set_file_path(names[j])
        recorded = None
        if splitter is not None:
            recorded = [{"col_name": c, "dtype": dt} for c, dt in zip(keys, splitter.dtypes or [])]
        _write_summary(output_path, [(names[j], rows.get(j, 0)) for j in order], schema, collector,
                       cats, conts, labels, recorded)
        return None

    def _partition_keys(self, partition_on, out_files_per_proc, shuffle, max_partitions):
        """``to_parquet(partition_on=...)`` -> the key names ([]: not partitioned).  Everything that
        can be refused from the arguments and the schema is refused here, before anything exists."""
        if partition_on is None:
            return []
        keys = [partition_on] if isinstance(partition_on, str) else list(partition_on)
        from . import _lib
        from .hive import check_descriptors

        if not 1 <= len(keys) <= _lib.JOIN_MAX_KEYS:
            raise ValueError(f"to_parquet: partition_on takes 1 to {_lib.JOIN_MAX_KEYS} column names, got {len(keys)}")
        if len(set(keys)) != len(keys):
            raise ValueError(f"to_parquet: partition_on repeats a column: {keys}")
        if out_files_per_proc:
            raise ValueError("to_parquet: partition_on writes one part file per directory and process; "
                             "out_files_per_proc cannot be combined with it")
        if shuffle == Shuffle.PER_WORKER:
            raise ValueError("to_parquet: Shuffle.PER_WORKER cannot be combined with partition_on "
                             "(Shuffle.PER_PARTITION can: it shuffles, then splits)")
        if int(max_partitions) < 1:
            raise ValueError(f"to_parquet: max_partitions must be at least 1, got {max_partitions}")
        schema = self.schema
        missing = [c for c in keys if c not in schema]
        if missing:
            raise ValueError(f"to_parquet: partition_on names {missing}, which are no columns of {schema.column_names}")
        if len(schema) <= len(keys):
            raise ValueError(f"to_parquet: partition_on={keys} leaves no data column to write")
        for c in keys:
            cs = schema[c]
            kind = getattr(cs.dtype, "kind", "O")
            if cs.is_list or kind in "fbMm":
                raise TypeError(f"to_parquet: partition_on column {c!r} is {'a list of ' if cs.is_list else ''}"
                                f"{cs.dtype}; keys are flat integer or string columns: cast it first")
        check_descriptors(int(max_partitions))
        return keys


def _write_pyarrow(parts, output_path, fname, k, shuffle, dtypes, pq_kw, splitter=None):
    """Dataset.to_parquet with pyarrow's writer (strings, bools, a codec, Shuffle.PER_WORKER with
    ``k`` files ...): partition i goes to file i, or with ``k`` is cut into k pieces for files
    0 .. k-1; with ``splitter`` (``partition_on``) the partition is split by key tuple on the device
    and every tuple's rows go to the file of its directory.
    -> (names {file index: name}, rows {file index: rows}, file indices in order, the
    files' Arrow schema, their FileMetaData in that order)."""
    import threading
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    import pyarrow as pa
    import pyarrow.parquet as pq

    rng = np.random.default_rng()
    writers, held, names, rows_in = {}, {}, {}, {}
    touched = set()
    collector = []
    # Parquet encoding (dictionary + compression) is host work that pyarrow does with the
    # GIL released: file j is always written by lane j % NLANES, in order, so up to NLANES
    # files are encoded at once while the next partition is transformed and copied out.
    NLANES = 4
    lanes = [ThreadPoolExecutor(max_workers=1) for _ in range(NLANES)]
    inflight = threading.BoundedSemaphore(2 * NLANES)  # bounds the host memory queued up
    pending = []

    def write(j, table):
        try:
            w = writers.get(j)
            if w is None:
                names[j] = fname(j)
                w = writers[j] = pq.ParquetWriter(os.path.join(output_path, names[j]), table.schema,
                                                  metadata_collector=collector, **pq_kw)
            w.write_table(table)
            rows_in[j] = rows_in.get(j, 0) + table.num_rows
        finally:
            inflight.release()

    def emit(j, table):
        if shuffle == Shuffle.PER_WORKER and k:
            held.setdefault(j, []).append(table)
            return
        inflight.acquire()
        pending.append(lanes[j % NLANES].submit(write, j, table))

    def abort():
        """A failed partitioned write: no footer-less part files are left behind."""
        for f in pending:
            try:
                f.result()
            except Exception:
                pass
        for j, w in writers.items():
            try:
                w.close()
                os.remove(os.path.join(output_path, names[j]))
            except Exception:
                pass

    try:
        for i, part in enumerate(parts):
            n = len(part)
            if shuffle is not None and n > 1:
                part = part.take_rows(device_permutation(n, part))
            pieces = None
            if splitter is not None:
                part, pieces = splitter.split(part)
                if not pieces:
                    continue
            table = part.to_arrow()  # pinned async copies, no pandas round trip
            for c, t in (dtypes or {}).items():
                if c in table.column_names:
                    ci = table.column_names.index(c)  # NOT `i`: that is the partition index
                    table = table.set_column(ci, c, table.column(c).cast(pa.from_numpy_dtype(np.dtype(t))))
            if pieces is not None:
                for j, s0, s1 in pieces:
                    emit(j, table.slice(s0, s1 - s0))
                continue
            if k is None:
                emit(i, table)
                continue
            bounds = [(n * j) // k for j in range(k + 1)]
            for j in range(k):
                if bounds[j + 1] > bounds[j] or j not in touched:
                    touched.add(j)
                    emit(j, table.slice(bounds[j], bounds[j + 1] - bounds[j]))
    except BaseException:
        if splitter is not None:
            abort()
        raise
    for f in pending:
        f.result()  # re-raises a writer's exception here
    for ex in lanes:
        ex.shutdown(wait=True)
    for j, pieces in sorted(held.items()):
        table = pa.concat_tables(pieces)
        if table.num_rows > 1:
            table = table.take(pa.array(rng.permutation(table.num_rows)))
        inflight.acquire()
        write(j, table)
    schema = None
    order = sorted(writers)
    for j in order:   # (every ParquetWriter appends its FileMetaData to the collector on close)
        schema = schema or writers[j].schema
        writers[j].close()
    return names, rows_in, order, schema, collector


def _write_summary(output_path, files, schema, collector, cats, conts, labels, partition_on=None):
    """``_metadata`` (parquet summary of all row groups), ``_file_list.txt`` and ``_metadata.json``
    next to the data files.  ``files``: this rank's [(name, rows)]; ``collector``: their
    FileMetaData with the file paths set.  Under torch.distributed rank 0 writes for every rank.
    ``partition_on``: the [{col_name, dtype}] of a hive-partitioned write (file names are then paths
    relative to ``output_path``; the keys are no columns of ``schema``, so ``pick`` drops them)."""
    import json

    import pyarrow.parquet as pq

    from . import dist

    if dist.world_size() > 1:
        import torch.distributed as td

        gathered = [None] * dist.world_size()
        td.all_gather_object(gathered, files)
        td.barrier()
        files = [x for g in gathered for x in g]
    if dist.rank() != 0 or schema is None:
        return
    if dist.world_size() > 1:  # summary over every rank's files
        collector = []
        for name, _ in files:
            md = pq.read_metadata(os.path.join(output_path, name))
            md.set_file_path(name)
            collector.append(md)
    pq.write_metadata(schema, os.path.join(output_path, "_metadata"), metadata_collector=collector)
    with open(os.path.join(output_path, "_file_list.txt"), "w") as f:
        f.write(str(len(files)) + "\n")
        for name, _ in files:
            f.write(name + "\n")
    cols = schema.names
    pick = lambda lst: [{"col_name": c, "index": cols.index(c)} for c in (lst or []) if c in cols]
    meta = {"file_stats": [{"file_name": name, "num_rows": int(nr)} for name, nr in files],
            "cats": pick(cats), "conts": pick(conts), "labels": pick(labels)}
    if partition_on is not None:
        meta["partition_on"] = partition_on
    with open(os.path.join(output_path, "_metadata.json"), "w") as f:
        json.dump(meta, f)


PLAIN_PARQUET = os.environ.get("NVT_PLAIN_PARQUET", "1") != "0"
PLAIN_PARQUET_READ = os.environ.get("NVT_PLAIN_PARQUET_READ", "1") != "0"
PLAIN_READ_THREADS = int(os.environ.get("NVT_PARQUET_READ_THREADS", "32"))
_PLAIN_READ_POOL = None


def _plain_read_pool():
    global _PLAIN_READ_POOL
    if _PLAIN_READ_POOL is None:
        from concurrent.futures import ThreadPoolExecutor

        _PLAIN_READ_POOL = ThreadPoolExecutor(max_workers=PLAIN_READ_THREADS, thread_name_prefix="nvt-pqread")
    return _PLAIN_READ_POOL


# the PLAIN writer (parquet_write.write_plain): pwrite threads, rows per row group, row groups being written at once
PLAIN_WRITE_THREADS = int(os.environ.get("NVT_PARQUET_THREADS", "16"))
PLAIN_ROW_GROUP = int(os.environ.get("NVT_PARQUET_ROW_GROUP", str(1 << 22)))
PLAIN_INFLIGHT = int(os.environ.get("NVT_PARQUET_INFLIGHT", "8"))


class Shuffle:
    """merlin.io.Shuffle: how ``Dataset.to_parquet`` randomises rows."""

    PER_PARTITION = "per-partition"
    PER_WORKER = "per-worker"
    FULL = "full"  # treated as PER_WORKER: there is one writer process per GPU

    @staticmethod
    def coerce(value):
        if value is None or value is False:
            return None
        if value is True:
            return Shuffle.PER_WORKER
        if value in (Shuffle.PER_PARTITION, Shuffle.PER_WORKER):
            return value
        if value == Shuffle.FULL:
            return Shuffle.PER_WORKER
        raise ValueError(f"unknown shuffle option {value!r}")


def _prefetch_frames(host_parts, cols, depth: int = 2, post=None):
    """``post`` (the dataset's filter) runs on the producer thread, on the side stream and in front of
    the event: its read-back of the kept row count stalls the prefetch, not the consumer."""
    import queue
    import threading

    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(device=dev)
    q: "queue.Queue" = queue.Queue(maxsize=depth)
    _END = object()
    stop = threading.Event()  # set when the consumer abandons the generator early

    def put(item) -> bool:
        while not stop.is_set():
            try:
                q.put(item, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def producer():
        try:
            torch.cuda.set_device(dev)
            for part in host_parts:
                if stop.is_set():
                    return
                with torch.cuda.stream(side):
                    frame, _ = as_device_frame(part, dev)
                    if post is not None:
                        frame = post(frame)
                    if cols is not None:
                        frame = frame[[c for c in cols if c in frame]]
                    ev = torch.cuda.Event()
                    ev.record(side)
                if not put((frame, ev)):
                    return
            put(_END)
        except BaseException as e:  # surface decode / copy errors in the consumer
            put(e)

    t = threading.Thread(target=producer, daemon=True)
    t.start()
    try:
        while True:
            item = q.get()
            if item is _END:
                break
            if isinstance(item, BaseException):
                raise item
            frame, ev = item
            torch.cuda.current_stream().wait_event(ev)
            for _, col in frame.items():  # the buffers were allocated on the side stream
                for tns in (col.data, col.valid, col.offsets):
                    if tns is not None:
                        tns.record_stream(torch.cuda.current_stream())
            yield frame
    finally:
        # early exit (Dataset.head(), Workflow._capture_dtypes break after one partition, an
        # exception in the consumer): release the producer, drop the device-resident
        # partitions it still holds and join it -- it used to stay blocked in q.put forever
        stop.set()
        try:
            while True:
                q.get_nowait()
        except queue.Empty:
            pass
        t.join(timeout=30)


def _csv_engine(src, engine) -> bool:
    from .csv_text import select_engine

    return select_engine(src, engine) == "csv"


def _is_arrow_table(x) -> bool:
    try:
        import pyarrow as pa

        return isinstance(x, pa.Table)
    except ImportError:  # pragma: no cover
        return False


def _accepts_columns(fn) -> bool:
    try:
        from inspect import signature

        return "columns" in signature(fn).parameters
    except (TypeError, ValueError):
        return False


def _split(frame, n):
    if n <= 1:
        return [frame]
    total = len(frame)
    step = -(-total // n)
    step = -(-step // 8) * 8  # bitmap-friendly boundaries
    out = []
    for s in range(0, total, step):
        e = min(total, s + step)
        if isinstance(frame, pd.DataFrame):
            out.append(frame.iloc[s:e].reset_index(drop=True))
        elif isinstance(frame, DeviceFrame):
            out.append(frame.slice_rows(s, e))
        else:
            out.append(frame.slice(s, e - s))
    return out
