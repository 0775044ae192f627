"""``Dataset(filters=...)``: the host half of a declarative row predicate.

A filter is pyarrow's / dask's DNF: a list of ``(column, op, value)`` tuples (one conjunction) or a
list of such lists (an OR of conjunctions); ``op`` is one of ``==  =  !=  <  <=  >  >=  in  not in``.
This module parses and normalises it, types every constant against a ``Schema``, tests a conjunction
on the key values a hive path spells and on the min / max / null-count statistics of a row group
(so that files and row groups no row of which can pass are never read), and lowers the DNF to the
descriptors of ``nvt_compact_keep_terms`` (include/nvt_hip.h), which evaluates it per row on the
device.  Pure Python: nothing here needs a GPU.

Semantics (those of ``pyarrow.parquet.read_table(filters=...)``): a null fails every comparison
and ``in`` and passes ``not in``; NaN fails every comparison but ``!=``; ``-0.0 == 0.0``; ``in []``
keeps nothing.  Integers, bools (0 / 1), datetime counts and string surrogates compare in int64,
floats in float64 (a float32 column is widened, the constant is not narrowed).  ``in`` on a float
column compares every member as ``==`` in float64, where pyarrow narrows the members to the column's
type: the two agree for members the column's type represents exactly."""
from __future__ import annotations

import datetime as _dt
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

OPS = ("==", "!=", "<", "<=", ">", ">=", "in", "not in")
ORDERED = ("<", "<=", ">", ">=")
SET_OPS = ("in", "not in")
MAX_COLS, MAX_TERMS = 16, 64          # include/nvt_hip.h NVT_FILTER_MAX_COLS / NVT_FILTER_MAX_TERMS
OP_CODE = {op: i for i, op in enumerate(OPS)}   # NVT_FILTER_EQ .. NVT_FILTER_NOT_IN
_UNIT_NS = {"s": 10**9, "ms": 10**6, "us": 10**3, "ns": 1}
_I64 = (-(1 << 63), (1 << 63) - 1)


# ---- parsing ---------------------------------------------------------------------------------------
def _is_term(t) -> bool:
    return isinstance(t, tuple) and len(t) == 3 and isinstance(t[0], str)


def normalize(filters) -> List[List[Tuple[str, str, object]]]:
    """The DNF as a list of conjunctions, each a list of ``(column, op, value)`` with ``=`` spelled
    ``==``.  ``[]``, an empty conjunction, a malformed term and an unknown operator raise ValueError."""
    if not isinstance(filters, (list, tuple)) or len(filters) == 0:
        raise ValueError(f"filters must be a non-empty list of (column, op, value) tuples or of lists of them, "
                         f"got {filters!r}")
    conjs = [list(filters)] if all(_is_term(t) for t in filters) else [c for c in filters]
    out = []
    for conj in conjs:
        if not isinstance(conj, (list, tuple)) or len(conj) == 0 or not all(_is_term(t) for t in conj):
            raise ValueError(f"filters: a conjunction is a non-empty list of (column, op, value) tuples, got {conj!r}")
        terms = []
        for col, op, value in conj:
            op = "==" if op == "=" else op
            if not isinstance(op, str) or op not in OPS:
                raise ValueError(f"filters: unknown operator {op!r} on column {col!r}; operators are {', '.join(OPS)}")
            terms.append((col, op, value))
        out.append(terms)
    return out


# ---- typing ----------------------------------------------------------------------------------------
class Term:
    """One typed comparison.  ``kind``: "int", "float", "bool", "string", "datetime", or None for a
    column the schema at hand does not hold (``validate(partial=True)``: such a term is never
    decided on the host).  ``value``: what the host compares with -- an int (ints, bools as 0 / 1,
    datetime counts in the column's ``unit``), a float or a str; for ``in`` / ``not in`` the sorted
    tuple of the distinct members."""

    __slots__ = ("column", "op", "kind", "value", "unit")

    def __init__(self, column, op, kind, value, unit=None):
        self.column, self.op, self.kind, self.value, self.unit = column, op, kind, value, unit

    def __repr__(self):
        return f"Term({self.column!r}, {self.op!r}, {self.value!r})"


def kind_of(cs) -> Tuple[str, Optional[str]]:
    """(kind, datetime unit) of a ColumnSchema; a list column or an unknown dtype raises TypeError."""
    if cs.is_list:
        raise TypeError(f"filters: column {cs.name!r} is a list column; list columns cannot be filtered")
    dt = cs.dtype
    if dt is object or dt is str:
        return "string", None
    try:
        dt = np.dtype(dt)
    except TypeError:
        raise TypeError(f"filters: column {cs.name!r} has the dtype {cs.dtype!r}, which cannot be filtered") from None
    if dt.kind in "iu":
        return "int", None
    if dt.kind == "f":
        return "float", None
    if dt.kind == "b":
        return "bool", None
    if dt.kind in "OUS":
        return "string", None
    if dt.kind == "M":
        unit = np.datetime_data(dt)[0]
        if unit not in _UNIT_NS:
            raise TypeError(f"filters: column {cs.name!r} is {dt}; datetime columns are datetime64[s|ms|us|ns]")
        return "datetime", unit
    raise TypeError(f"filters: column {cs.name!r} has the dtype {dt}, which cannot be filtered")


def _constant(column, kind, unit, v):
    """The constant ``v`` in the host domain of a column of ``kind``."""
    what = f"filters: column {column!r} is {'a ' if kind != 'int' else 'an '}{kind} column"
    is_bool = isinstance(v, (bool, np.bool_))
    is_int = isinstance(v, (int, np.integer)) and not is_bool
    is_float = isinstance(v, (float, np.floating))
    if kind == "int":
        if is_float and math.isfinite(v) and float(v) == math.floor(v):
            v, is_int = int(v), True
        if not is_int:
            raise TypeError(f"{what}: it is compared with integers (or floats of integral value), not {v!r}")
        v = int(v)
        if not _I64[0] <= v <= _I64[1]:
            raise ValueError(f"{what}: {v} does not fit int64")
        return v
    if kind == "float":
        if not (is_int or is_float):
            raise TypeError(f"{what}: it is compared with ints and floats, not {v!r}")
        return float(v)
    if kind == "bool":
        if not is_bool:
            raise TypeError(f"{what}: it is compared with True / False, not {v!r}")
        return int(bool(v))
    if kind == "string":
        if not isinstance(v, str):
            raise TypeError(f"{what}: it is compared with str, not {v!r}")
        return str(v)
    # datetime
    import pandas as pd

    if not isinstance(v, (pd.Timestamp, _dt.datetime, np.datetime64)):
        raise TypeError(f"{what}: it is compared with pandas.Timestamp, datetime.datetime or numpy.datetime64, "
                        f"not {v!r}")
    ts = pd.Timestamp(v)
    if ts is pd.NaT:
        raise ValueError(f"{what}: NaT is no constant (a null fails every comparison)")
    if ts.tzinfo is not None:
        ts = ts.tz_convert("UTC").tz_localize(None)   # the UTC instant, as the columns hold them
    ns = int(ts.as_unit("ns").value)
    count, rest = divmod(ns, _UNIT_NS[unit])
    if rest:
        raise ValueError(f"{what} in [{unit}]: {v!r} is not a whole number of {unit}")
    return count


class Filter:
    """A validated DNF: ``dnf`` is a list of conjunctions of ``Term``; inside a conjunction the terms
    on one column are adjacent (the kernel then loads that column once).  ``columns``: the distinct
    columns in order of first use."""

    def __init__(self, dnf: List[List[Term]]):
        self.columns: List[str] = list(dict.fromkeys(t.column for conj in dnf for t in conj))
        order = {c: i for i, c in enumerate(self.columns)}
        self.dnf = [sorted(conj, key=lambda t: order[t.column]) for conj in dnf]   # (stable)
        self._lowered: Dict[tuple, "Lowered"] = {}

    @property
    def nterms(self) -> int:
        return sum(len(c) for c in self.dnf)

    def as_tuples(self):
        return [[(t.column, t.op, t.value) for t in conj] for conj in self.dnf]

    # -- hive: a conjunction on the key values of a file --------------------------------------------
    def alive_on_keys(self, keys: Dict[str, object]) -> List[int]:
        """The conjunctions that can still hold in a file whose path spells ``keys`` ({key column:
        typed value, None for the null directory}): those none of whose key terms is false."""
        return [i for i, conj in enumerate(self.dnf)
                if all(term_holds(t, keys[t.column]) for t in conj if t.column in keys and t.kind is not None)]

    # -- row groups ---------------------------------------------------------------------------------
    def prunes_row_group(self, rg, columns: Dict[str, int], fields, alive: Optional[Sequence[int]] = None) -> bool:
        """True when the statistics of row group ``rg`` (pyarrow RowGroupMetaData) prove that none of
        its rows passes: every conjunction of ``alive`` (default: all) has a term that prunes.
        ``columns``: {flat column name: its index in the row group}; ``fields``: the file's Arrow
        schema."""
        for i in (range(len(self.dnf)) if alive is None else alive):
            if not any(term_prunes(t, column_stats(t, rg, columns, fields)) for t in self.dnf[i]):
                return False
        return True

    # -- the kernel's descriptors --------------------------------------------------------------------
    def lower(self, floats: Dict[str, bool]) -> "Lowered":
        """The descriptors of nvt_compact_keep_terms for frames whose filter columns are float
        (``floats[name]`` true: the terms compare in float64) or integer (int64) on the device."""
        key = tuple(bool(floats[c]) for c in self.columns)
        low = self._lowered.get(key)
        if low is None:
            low = self._lowered[key] = Lowered(self, key)
        return low


def validate(dnf, schema, partial: bool = False) -> Filter:
    """Type the normalised ``dnf`` against ``schema``.  Raises ValueError for a column that is not in
    the schema (``partial``: such a term is kept untyped instead), more than MAX_COLS distinct
    columns or MAX_TERMS terms and a datetime constant that is no whole count of the column's unit;
    TypeError for a list column, an ordered comparison on a string column and a constant of
    another kind than the column's."""
    names = list(dict.fromkeys(col for conj in dnf for col, _, _ in conj))
    nterms = sum(len(conj) for conj in dnf)
    if len(names) > MAX_COLS:
        raise ValueError(f"filters: {len(names)} distinct columns; at most {MAX_COLS} are taken")
    if nterms > MAX_TERMS:
        raise ValueError(f"filters: {nterms} terms; at most {MAX_TERMS} are taken")
    out = []
    for conj in dnf:
        terms = []
        for col, op, value in conj:
            if col not in schema:
                if partial:
                    terms.append(Term(col, op, None, value))
                    continue
                raise ValueError(f"filters: {col!r} is no column of {schema.column_names}")
            kind, unit = kind_of(schema[col])
            if kind == "string" and op in ORDERED:
                raise TypeError(f"filters: column {col!r} holds strings, which are compared with ==, !=, in and "
                                f"not in only, not {op!r}")
            if op in SET_OPS:
                if isinstance(value, (str, bytes)) or not isinstance(value, (list, tuple, set, frozenset, np.ndarray)):
                    raise TypeError(f"filters: {op!r} on column {col!r} takes a list of values, not {value!r}")
                members = {_constant(col, kind, unit, v) for v in value}
                if kind == "float":   # a NaN equals nothing; -0.0 and 0.0 are one member
                    members = {0.0 if m == 0.0 else m for m in members if not math.isnan(m)}
                value = tuple(sorted(members))
            else:
                value = _constant(col, kind, unit, value)
            terms.append(Term(col, op, kind, value, unit))
        out.append(terms)
    return Filter(out)


# ---- the host's verdicts ---------------------------------------------------------------------------
def term_holds(term: Term, v) -> bool:
    """The term on one host value of its column's domain (None: a null)."""
    if v is None:
        return term.op == "not in"
    c, op = term.value, term.op
    if op == "==":
        return v == c
    if op == "!=":
        return v != c
    if op == "<":
        return v < c
    if op == "<=":
        return v <= c
    if op == ">":
        return v > c
    if op == ">=":
        return v >= c
    return (v in c) == (op == "in")


def segment_value(text: Optional[str], dtype: str):
    """The typed value of a hive path segment (hive.decode_segment's text; None: the null
    directory): the text of a string key, else the integer it spells (as hive.key_column reads it)."""
    if text is None:
        return None
    return text if dtype == "string" else int(text)


class ColumnStats:
    """min / max of a column chunk in the term's host domain (None: not known) and whether every
    value is null."""

    __slots__ = ("min", "max", "all_null")

    def __init__(self, mn, mx, all_null):
        self.min, self.max, self.all_null = mn, mx, all_null


_PHYSICAL = {"int": ("INT32", "INT64"), "float": ("FLOAT", "DOUBLE"), "bool": ("BOOLEAN",),
             "string": ("BYTE_ARRAY",), "datetime": ("INT64",)}


def column_stats(term: Term, rg, columns: Dict[str, int], fields) -> Optional[ColumnStats]:
    """What the footer says about the term's column in row group ``rg``, or None when it says nothing
    usable: the column is not in the file (a hive key), statistics are missing, or their type does
    not fit the term's kind."""
    j = columns.get(term.column)
    if j is None or term.kind is None:
        return None
    chunk = rg.column(j)
    st = chunk.statistics
    if st is None or chunk.physical_type not in _PHYSICAL[term.kind]:
        return None
    all_null = bool(st.has_null_count and st.null_count == chunk.num_values and chunk.num_values > 0)
    if not st.has_min_max:
        return ColumnStats(None, None, all_null)
    import pyarrow as pa

    typ = fields.field(term.column).type
    mn, mx = st.min, st.max
    kind = term.kind
    if kind == "int":
        fits = pa.types.is_integer(typ) and type(mn) is int and type(mx) is int
    elif kind == "float":
        fits = pa.types.is_floating(typ) and type(mn) is float and type(mx) is float and \
            not (math.isnan(mn) or math.isnan(mx))
    elif kind == "bool":
        fits = pa.types.is_boolean(typ) and type(mn) is bool and type(mx) is bool
        mn, mx = int(mn), int(mx)
    elif kind == "string":
        fits = (pa.types.is_string(typ) or pa.types.is_large_string(typ)) and \
            isinstance(mn, (str, bytes)) and isinstance(mx, (str, bytes))
        if fits:   # parquet orders BYTE_ARRAY by unsigned bytes: compare the UTF-8 encodings
            mn = mn.encode() if isinstance(mn, str) else mn
            mx = mx.encode() if isinstance(mx, str) else mx
    else:
        fits = pa.types.is_timestamp(typ) and typ.unit == term.unit
        if fits:
            try:
                mn = _constant(term.column, "datetime", term.unit, mn)
                mx = _constant(term.column, "datetime", term.unit, mx)
            except (TypeError, ValueError):
                fits = False
    if not fits:
        return ColumnStats(None, None, all_null)
    return ColumnStats(mn, mx, all_null)


def term_prunes(term: Term, st: Optional[ColumnStats]) -> bool:
    """True when the statistics prove that the term holds for no row of the chunk.  ``!=`` and ``not in``
    never prune; a chunk of nulls only fails the other operators; ``==`` and ``in`` prune by range, the
    ordered operators by the bound they look at."""
    if st is None or term.op in ("!=", "not in"):
        return False
    if st.all_null:
        return True
    if st.min is None:
        return False
    c, op = term.value, term.op
    if term.kind == "string":
        c = tuple(m.encode() for m in c) if op == "in" else c.encode()
    if op == "==":
        return c < st.min or c > st.max
    if op == "in":
        return all(m < st.min or m > st.max for m in c)
    if op == "<":
        return st.min >= c
    if op == "<=":
        return st.min > c
    if op == ">":
        return st.max <= c
    return st.max < c      # ">="


def flat_columns(md) -> Dict[str, int]:
    """{name: column index} of the flat (not nested) columns of a parquet file's metadata."""
    out = {}
    schema = md.schema
    for j in range(md.num_columns):
        col = schema.column(j)
        if "." not in col.path and col.max_repetition_level == 0:
            out[col.path] = j
    return out


# ---- lowering ----------------------------------------------------------------------------------------
class Lowered:
    """The DNF as nvt_compact_keep_terms takes it: ``columns`` (names, the descriptor order),
    ``floats`` (per column: compared in float64), ``terms`` [(col, op code, conj, set_len, set_off,
    value)] sorted by conj with ``value`` an int (int64) or a float, and ``sets`` -- uint64 words,
    every ``in`` / ``not in`` run sorted and distinct, doubles as their bit patterns with -0.0 stored as
    0.0.  String constants are keyed with strings.string_key64, as every string column is."""

    def __init__(self, flt: Filter, floats: Sequence[bool]):
        self.filter = flt
        self.columns = list(flt.columns)
        self.floats = tuple(floats)
        index = {c: i for i, c in enumerate(self.columns)}
        self.terms: List[tuple] = []
        runs: List[np.ndarray] = []
        off = 0
        for conj_id, conj in enumerate(flt.dnf):
            for t in conj:
                j = index[t.column]
                as_float = self.floats[j]
                if t.op in SET_OPS:
                    run = self._words(t, t.value, as_float)
                    self.terms.append((j, OP_CODE[t.op], conj_id, int(run.size), off, 0))
                    runs.append(run)
                    off += int(run.size)
                else:
                    word = self._words(t, (t.value,), as_float, scalar=True)
                    self.terms.append((j, OP_CODE[t.op], conj_id, 0, 0, word))
        self.sets = np.concatenate(runs) if runs else np.zeros(0, dtype=np.uint64)
        self._device_sets: Dict[object, object] = {}

    @staticmethod
    def _words(t: Term, members, as_float: bool, scalar: bool = False):
        if t.kind is None:
            raise ValueError(f"filters: column {t.column!r} was never typed")
        if t.kind == "string":
            from .strings import string_key64

            vals = string_key64(list(members)) if len(members) else np.zeros(0, dtype=np.int64)
            if as_float:
                raise TypeError(f"filters: column {t.column!r} holds floats on the device, not strings")
        elif as_float:
            vals = np.asarray([float(m) for m in members], dtype=np.float64)
            vals = vals + 0.0                      # -0.0 -> 0.0
        else:
            if any(isinstance(m, float) and m != math.floor(m) for m in members):
                raise TypeError(f"filters: column {t.column!r} holds integers on the device; {members!r} "
                                "is not integral")
            vals = np.asarray([int(m) for m in members], dtype=np.int64)
        if scalar:
            return float(vals[0]) if as_float else int(vals[0])
        vals = np.unique(vals)                     # sorted and distinct (surrogates have their own order)
        return vals.view(np.uint64)
