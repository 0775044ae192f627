"""JoinExternal (reference: nvtabular/ops/join_external.py): joins every partition to an external
table, ``df.merge(ext, left_on=on, right_on=on_ext, how=how)`` with the result in left-row order and
the index renumbered from 0.

Row semantics:

* output rows follow the left rows in order;
* a left row with k matching external rows yields k rows, in external-table order (pandas' own merge
  order, and what a stable sort on the reference's ``__tmp__`` column keeps);
* a left row with no match yields one row whose external columns are null (``how="left"``) or no
  row (``how="inner"``).

Keys match when pandas' merge would match them: integers of any width by value; floats by value
(-0.0 equals 0.0, and a float key matches an integer key of the same value, which covers pandas'
int-with-null artefact); strings by their 64-bit surrogate (a collision inside one column already
raises, a collision between a left and an external string is accepted as vanishingly rare); a null
component (validity bit 0, NaN, None) matches a null component, as in pandas, unlike SQL.  A string
key against a numeric key raises ``ValueError``.  1 to 4 key columns.

Columns: the left frame's columns, then the external columns (``columns_ext``, default all of them)
in the reference's ``dict.fromkeys`` order.  An external key column named like its left key is not
repeated (the left column is kept unchanged); any other name on both sides raises ``ValueError``.
External columns keep their dtype and carry nulls in a validity bitmap (an int column stays int;
``to_pandas()`` then gives float64 with NaN, as ``merge`` does); string columns keep the external
table's dictionary.  External list columns raise ``TypeError``.  Every kind of left column is carried
through (validity, strings, list columns, pending FillMissing constants).

The external table (``pandas.DataFrame``, ``pyarrow.Table``, ``DeviceFrame``, ``Dataset`` or parquet
path(s); several partitions are concatenated) and its hash index are built on the device on the first
``transform``, under ``kernels.LAUNCH_LOCK``, and stay resident.  The per-partition path follows from
``how`` and from whether the external keys are unique (kernels_join.py): a left join on unique keys is
one probe-gather launch per 16 external columns that shares the left columns' tensors; an inner join
on unique keys is a row compaction; duplicate keys expand one lane per output row, and left list
columns then go through ``DeviceFrame.take_rows``.  ``cache`` and ``kind_ext`` are accepted for API
compatibility.
"""
from __future__ import annotations

import pandas as pd

from ..device import DeviceFrame, as_device_frame
from ..schema import ColumnSchema, Schema
from ..selector import ColumnSelector
from .base import Operator


def _names(x):
    if x is None:
        return None
    return [x] if isinstance(x, str) else list(x)


def _to_device(part, cols) -> DeviceFrame:
    """One partition of the external table on the device, converted in THIS thread: the build runs
    under LAUNCH_LOCK, which the staging threads of DeviceFrame.from_arrow would wait for."""
    import pyarrow as pa

    from ..device import DeviceColumn

    if isinstance(part, pa.Table):
        return DeviceFrame({c: DeviceColumn.from_arrow(part.column(c)) for c in cols})
    frame, _ = as_device_frame(part)
    return frame[cols]


class JoinExternal(Operator):
    def __init__(self, df_ext, on, how="left", on_ext=None, columns_ext=None, drop_duplicates_ext=None,
                 kind_ext=None, cache="host", **kwargs):
        super().__init__()
        from ..io import Dataset

        if how not in ("left", "inner"):
            raise ValueError("Only left join is currently supported.")
        self.on = _names(on)
        self.on_ext = _names(on_ext) or list(self.on)
        if not 1 <= len(self.on) <= 4 or len(self.on) != len(self.on_ext):
            raise ValueError("on and on_ext must name the same number of key columns (1 to 4)")
        self.how = how
        self.df_ext = df_ext if isinstance(df_ext, Dataset) else Dataset(df_ext)
        self.columns_ext = _names(columns_ext)
        self.drop_duplicates_ext = drop_duplicates_ext
        self.kind_ext = kind_ext
        self.cache = cache
        self.kwargs = kwargs
        schema = self.df_ext.schema
        ext_cols = self.columns_ext or schema.column_names
        missing = [c for c in list(ext_cols) + self.on_ext if c not in schema]
        if missing:
            raise ValueError(f"JoinExternal: columns {missing} are not in the external table")
        absent_keys = [c for c in self.on_ext if c not in ext_cols]
        if absent_keys:
            raise ValueError(f"JoinExternal: columns_ext must include the external keys {absent_keys}")
        lists = [c for c in ext_cols if schema[c].is_list]
        if lists:
            raise TypeError(f"JoinExternal: list columns in the external table are not supported: {lists}")
        self._ext_schema = schema.select_by_name(list(ext_cols))
        self._ext_cols = list(ext_cols)
        self._ext_frame = None
        self._indexes = {}
        self.builds = 0

    # ---- columns ---------------------------------------------------------------------------
    def _shared_keys(self):
        return {a for a, b in zip(self.on, self.on_ext) if a == b}

    def _check_names(self, left_names):
        clash = (set(left_names) & set(self._ext_cols)) - self._shared_keys()
        if clash:
            raise ValueError(f"JoinExternal: columns {sorted(clash)} are on both sides of the join; "
                             f"rename them (pandas would add _x / _y suffixes)")
        missing = [c for c in self.on if c not in left_names]
        if missing:
            raise ValueError(f"JoinExternal: join keys {missing} are not among the input columns")

    def _payload(self, left_names):
        left = set(left_names)
        return [c for c in self._ext_cols if c not in left]

    def compute_selector(self, input_schema, selector, parents_selector=None, dependencies_selector=None):
        sel = parents_selector or ColumnSelector()
        self._validate_matching_cols(input_schema, sel, "computing input selector")
        return sel

    def column_mapping(self, col_selector):
        combined = dict.fromkeys(list(col_selector.names) + self._ext_cols).keys()
        return {name: [name] for name in combined}

    def compute_output_schema(self, input_schema, col_selector, prev_output_schema=None):
        self._check_names(col_selector.names)
        out = []
        for name in self.column_mapping(col_selector):
            if name in col_selector.names and name in input_schema:
                out.append(input_schema[name])
            elif name in col_selector.names:
                out.append(ColumnSchema(name))
            else:
                out.append(ColumnSchema(name, self._ext_schema[name].dtype))
        return Schema(out)

    # ---- the external table, built once -------------------------------------------------------
    def _external_frame(self) -> DeviceFrame:
        if self._ext_frame is not None:
            return self._ext_frame
        import pyarrow as pa

        flt = getattr(self.df_ext, "_filter", None)
        if flt is None:
            parts = [_to_device(p, self._ext_cols) for p in self.df_ext._host_parts(self._ext_cols, None)]
        else:
            # Dataset(filters=...): the filter's columns are read too, and the rows that pass are taken
            # in THIS thread (to_iter's prefetch thread would wait for LAUNCH_LOCK, which is held here)
            read = self._ext_cols + [c for c in flt.columns if c not in self._ext_cols]
            parts = [self.df_ext._filter_frame(_to_device(p, read))[self._ext_cols]
                     for p in self.df_ext._host_parts(read, None)]
        if len(parts) == 1 and not self.drop_duplicates_ext:
            frame = parts[0][self._ext_cols]
        elif not parts:
            frame = DeviceFrame.from_pandas(pd.DataFrame(
                {c: pd.Series([], dtype=self._ext_schema[c].dtype or "float64") for c in self._ext_cols}))
        else:
            table = pa.concat_tables([p[self._ext_cols].to_arrow() for p in parts], promote_options="default")
            if self.drop_duplicates_ext:
                df = table.to_pandas(types_mapper=pd.ArrowDtype).drop_duplicates(ignore_index=True)
                table = pa.Table.from_pandas(df, preserve_index=False)
            frame = _to_device(table, self._ext_cols)
        self._ext_frame = frame
        return frame

    def _index(self, left: DeviceFrame):
        from .. import kernels_join as KJ

        ext = self._external_frame()
        for c in self.on_ext:
            if ext[c].logical is not None:
                raise TypeError(f"JoinExternal: key column '{c}' of the external table is {ext[c].logical}; "
                                f"a datetime column cannot be a join key, convert it first")
        modes = KJ.key_modes([KJ.key_class(left[c]) for c in self.on],
                             [KJ.key_class(ext[c]) for c in self.on_ext], self.on, self.on_ext)
        payload = tuple(self._payload(left.columns))
        key = (modes, payload)
        ix = self._indexes.get(key)
        if ix is None:
            ix = self._indexes[key] = KJ.ExternalIndex(ext, self.on_ext, list(payload), modes)
            self.builds += 1
        return ix

    def datetime_rejects(self, col_selector, frame):
        # carried columns of both sides keep their type; a key is hashed and compared by class
        # (integer / float / string), which a datetime is none of
        return [c for c in self.on if c in frame and frame[c].logical is not None]

    def transform(self, col_selector: ColumnSelector, df):
        from .. import kernels_join as KJ

        frame, was_pandas = as_device_frame(df)
        self._check_names(frame.columns)
        ix = self._index(frame)   # (transform runs under LAUNCH_LOCK: two threads build once)
        out = KJ.join_frame(frame, self.on, ix, self.how, self._payload(frame.columns))
        return out.to_pandas() if was_pandas else out
