"""DataStats (reference: nvtabular/ops/data_stats.py): per-column dtype, min, max, mean, std,
percentage of missing rows and, for every column that is not floating point, the cardinality.

fit  = per partition ONE ``nvt_col_profile_many`` launch for the numeric columns and ONE
       ``nvt_dense_count_many`` call (the counting drivers of Categorify.fit) for the columns that
       get a cardinality; the per-partition (key, count) lists are merged eight at a time and once
       over the ranks.  Nothing is written to disk.
String columns are int64 surrogate keys plus a host dictionary: their statistics are those of the
string LENGTHS (the reference replaces the column by ``str.len()``), derived from the length of
every distinct string weighted by its count -- O(distinct) host work, no per-row string pass.
transform = identity.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K
from ..device import as_device_frame, key_view, numpy_dtype
from ..selector import ColumnSelector
from ._profile import _PROFILED, ProfileFit, length_stats, per_nan
from .base import StatOperator
from .normalize import finalize_moments

MERGE_FAN_IN = 8   # per-partition lists merged at a time (_mid_level_groupby's split_every)


class _CountFit:
    """The (key, count) list of one column, folded over the partitions."""

    def __init__(self):
        self.parts, self.nulls, self.rows, self.hint = [], 0, 0, 0
        self.strings = None   # {surrogate key: str} of a string column


class DataStats(StatOperator):
    def __init__(self):
        super().__init__()
        self.col_names = []
        self.col_types = []
        self.col_dtypes = []
        self.output = {}

    def fit_begin(self, col_selector: ColumnSelector):
        names = list(col_selector.names)
        return {"names": names, "profile": ProfileFit(names), "counts": {}, "pending": None, "dtypes": {},
                "device": None}

    def fit_partition(self, state, col_selector, df):
        frame, _ = as_device_frame(df)
        jobs, owners = [], []
        for name in state["names"]:
            col = frame[name]
            state["device"] = col.data.device
            if col.is_list:
                raise NotImplementedError(f"DataStats: list column {name!r} is not supported")
            if col.fill is not None:
                col = col.materialize()
            is_str = col.strings is not None
            if not is_str and col.data.dtype not in _PROFILED:
                raise TypeError(f"DataStats: column {name!r} has unsupported dtype {col.data.dtype}")
            state["dtypes"].setdefault(name, "object" if is_str else str(numpy_dtype(col.data.dtype)))
            if not is_str and col.data.dtype.is_floating_point:
                continue
            fit = state["counts"].setdefault(name, _CountFit())
            if is_str:
                fit.strings = fit.strings if fit.strings is not None else {}
                fit.strings.update(col.strings)
            keys, valid = key_view(col)
            jobs.append(K.DenseCountJob(keys, valid, None, hint=fit.hint))
            owners.append(fit)
        state["profile"].partition(frame)
        # this partition's counting is enqueued before the previous partition's lists are read back
        batch = K.CountBatch(jobs) if jobs else None
        self._absorb(state)
        state["pending"] = (batch, owners) if batch is not None else None

    @staticmethod
    def _absorb(state):
        item, state["pending"] = state["pending"], None
        if item is None:
            return
        batch, owners = item
        due = []
        for fit, (dk, dc, nulls, info) in zip(owners, batch.results()):
            fit.hint = max(64, info["distinct"], fit.hint)
            fit.nulls += nulls
            fit.rows += info["rows"]
            fit.parts.append((dk, dc, info["max_count"]))
            if len(fit.parts) >= MERGE_FAN_IN:
                due.append(fit)
        DataStats._merge(due)

    @staticmethod
    def _merge(fits):
        fits = [f for f in fits if len(f.parts) > 1]
        if not fits:
            return
        outs = K.merge_dense_many([f.parts for f in fits], hints=[f.hint for f in fits])
        for f, tab in zip(fits, outs):
            f.parts = [tab] if tab is not None else []
            if tab is not None:
                f.hint = max(f.hint, int(tab[0].numel()))

    def fit_end(self, state, col_selector):
        from .. import dist

        self._absorb(state)
        names, dtypes, counts = state["names"], state["dtypes"], state["counts"]
        if dist.world_size() > 1:
            # a rank whose shard was empty has seen no column: the column kinds are agreed first
            # (host objects; every rank takes the same branches below)
            dtypes = dist.merge_host_dicts(dtypes) or {}
        self._merge(list(counts.values()))
        counted = [n for n in names if n in dtypes and (dtypes[n] == "object" or np.dtype(dtypes[n]).kind != "f")]
        lists = {}
        if counted:
            dev = state["device"] or torch.device("cuda", torch.cuda.current_device())
            tabs = []
            for n in counted:
                fit = counts.get(n) or _CountFit()
                if fit.parts:
                    k, c, _ = fit.parts[0]
                else:
                    k = torch.empty(0, dtype=torch.int64, device=dev)
                    c = torch.empty(0, dtype=torch.int64, device=dev)
                tabs.append((k, c, [int(fit.nulls), int(fit.rows)]))
            for n, (k, c, sc, _) in zip(counted, dist.merge_counts_many(tabs)):
                lists[n] = (k, c, int(sc[0]), int(sc[1]))
        profile = state["profile"].end()
        # string columns: ONE read-back of all their (key, count) lists, ONE union of their
        # dictionaries over the ranks (keyed by column and surrogate key)
        str_cols = [n for n in names if dtypes.get(n) == "object"]
        pairs_of = {n: [] for n in str_cols}
        if str_cols:
            mine = {(n, key): s for n in str_cols for key, s in ((counts.get(n) or _CountFit()).strings or {}).items()}
            lut = dist.merge_host_dicts(mine) or {}
            full = [n for n in str_cols if int(lists[n][0].numel())]
            if full:
                kc = K.read_back(torch.stack([torch.cat([lists[n][0].to(torch.int64) for n in full]),
                                              torch.cat([lists[n][1].to(torch.int64) for n in full])]))
                at = 0
                for n in full:
                    m = int(lists[n][0].numel())
                    pairs_of[n] = [(len(lut[(n, int(key))]), int(cnt))
                                   for key, cnt in zip(kc[0, at:at + m].tolist(), kc[1, at:at + m].tolist())]
                    at += m
        out = {}
        for n in names:
            if n not in dtypes:
                continue
            st = {"dtype": dtypes[n]}
            if dtypes[n] == "object":
                k, c, nulls, rows = lists[n]
                st["min"], st["max"], st["mean"], st["std"] = length_stats(pairs_of[n])
                st["per_nan"] = per_nan(rows - nulls, rows)
                st["cardinality"] = int(k.numel())
            else:
                p = profile[n]
                nan = float("nan")
                st["min"] = nan if p["min"] is None else p["min"]
                st["max"] = nan if p["max"] is None else p["max"]
                st["mean"], _, st["std"] = finalize_moments(p["valid"], p["sum"], p["sumsq"])
                st["per_nan"] = per_nan(p["valid"], p["rows"])
                if n in lists:
                    st["cardinality"] = int(lists[n][0].numel())
            out[n] = st
        return out

    def fit_finalize(self, stats):
        self.col_names = list(stats)
        self.col_dtypes = [s["dtype"] for s in stats.values()]
        self.col_types = ["cats" if "cardinality" in s else "conts" for s in stats.values()]
        self.output = stats

    def transform(self, col_selector: ColumnSelector, df):
        return df

    def clear(self):
        self.col_names, self.col_types, self.col_dtypes = [], [], []
        self.output = {}
