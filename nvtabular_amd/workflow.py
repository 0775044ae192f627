"""Workflow: fit / transform orchestration (reference:
nvtabular/workflow/workflow.py:45-358; executor semantics from merlin-core's
DaskExecutor / LocalExecutor).

fit runs the StatOperators in *phases* (a StatOperator is ready once every
StatOperator upstream of it has been fitted); all operators of a phase consume
each partition once, so e.g. Categorify and FillMissing>>Normalize of the Criteo
workflow are fitted in a single pass over the data.  With torch.distributed
initialised, each rank fits its shard of the partitions and the per-op
``fit_end`` merges over RCCL (dist.py).
"""
from __future__ import annotations

import json
import logging
import os
import time
from typing import Dict, List, Optional

import pandas as pd

from . import dist
from .device import DeviceFrame, as_device_frame
from .kernels import annotate, pass_memo
from .io import Dataset
from .node import Node, iter_nodes
from .ops.base import StatOperator
from .schema import Schema

LOG = logging.getLogger("nvtabular_amd")
BRANCH_STREAMS = os.environ.get("NVT_BRANCH_STREAMS", "0") == "1"   # (read once, at import)


class _FittedSchema:
    """Lazy output schema of a transformed Dataset: resolved on first use, picklable (resolves
    before pickling), and pinned to the fit that was current when transform() was called."""

    def __init__(self, wf):
        self._wf = wf
        self._gen = getattr(wf, "_fit_generation", 0)
        self._value = None

    def __call__(self):
        if self._value is None:
            if getattr(self._wf, "_fit_generation", 0) != self._gen:
                import warnings

                # (the partitions of a transformed Dataset are produced lazily from the Workflow
                # too, like the reference's dask graph: rows AND schema follow the latest fit)
                warnings.warn("the Workflow was re-fit after transform(): this Dataset's rows and "
                              "schema now follow the later fit", RuntimeWarning, stacklevel=3)
            self._value = self._wf.output_schema
            self._wf = None
        return self._value

    def __getstate__(self):
        return {"_value": self(), "_wf": None, "_gen": self._gen}


class Workflow:
    def __init__(self, output_node, client=None):
        self.output_node = Node.construct_from(output_node)
        self.client = client  # accepted for API compatibility (no dask here)
        self.input_schema: Optional[Schema] = None
        self._output_schema: Optional[Schema] = None
        self._stale_schema_root: Optional[Schema] = None  # set by fit(): properties need a refresh
        self._fit_root_schema: Optional[Schema] = None  # input schema the node schemas were built for
        self.output_dtypes = None

    @property
    def output_schema(self) -> Optional[Schema]:
        """Output schema; after fit() the fitted properties (embedding sizes, domains) are
        folded in lazily on first access so that transform can start right away."""
        if self._stale_schema_root is not None:
            root, self._stale_schema_root = self._stale_schema_root, None
            self.fit_schema(root)
        return self._output_schema

    @output_schema.setter
    def output_schema(self, value):
        self._output_schema = value

    # ---- schema ----------------------------------------------------------------
    def fit_schema(self, input_schema: Schema) -> "Workflow":
        for node in iter_nodes(self.output_node):
            node.compute_schemas(input_schema)
        roots = self._root_columns()
        self.input_schema = input_schema.select_by_name(roots)
        self.output_schema = self.output_node.output_schema
        self.output_dtypes = {c.name: c.dtype for c in self.output_schema}
        return self

    def _root_columns(self) -> List[str]:
        cols = []
        for node in iter_nodes(self.output_node):
            if node.op is None and node.input_schema is not None:
                for n in node.input_schema.column_names:
                    if n not in cols:
                        cols.append(n)
        return cols

    def _input_columns(self):
        return self._root_columns()

    # ---- execution of the graph on one partition ----------------------------------
    def _run(self, node: Node, root: DeviceFrame, cache: Dict[int, DeviceFrame]) -> DeviceFrame:
        key = id(node)
        if key in cache:
            return cache[key]
        if node.op is None:
            out = root[node.output_schema.column_names]
        else:
            inp = self._node_input(node, root, cache)
            _guard_datetime(node, inp)
            with annotate(node.op.range_name("transform")):
                out = node.op.transform(node.input_columns, inp)
            out, _ = as_device_frame(out)
            names = node.output_schema.column_names
            if all(n in out for n in names):
                out = out[names]
        cache[key] = out
        return out

    def _node_input(self, node: Node, root: DeviceFrame, cache) -> DeviceFrame:
        upstream = node.parents_with_dependencies
        lanes = self._branch_streams(upstream, cache)
        if lanes is None:
            # branches whose operators still have fit results in flight on internal streams
            # (Categorify's large vocabularies) are evaluated last: the kernels of the other
            # branches run underneath that work.  The column order of the result is unchanged.
            order = sorted(range(len(upstream)), key=lambda i: _async_pending(upstream[i]))
            done = {i: self._run(upstream[i], root, cache) for i in order}
            ups = [done[i] for i in range(len(upstream))]
        else:
            # Independent branches (e.g. the Categorify and the FillMissing >> Normalize halves
            # of the Criteo workflow) run on different HIP streams: an encode workgroup holds
            # 128 KiB of LDS and 16 waves, a fill+normalize workgroup needs no LDS, so both
            # kinds are resident on a CU together and the streaming kernels fill the bandwidth
            # the table-bound ones leave idle.
            import torch

            main = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(main)
            ups = []
            for u, st in zip(upstream, lanes):
                st.wait_event(ready)
                with torch.cuda.stream(st):
                    ups.append(self._run(u, root, cache))
            for st in set(lanes):
                main.wait_stream(st)
            for f in ups:  # created on a side stream, consumed (and freed) on the main one
                for _, col in f.items():
                    for t in (col.data, col.valid, col.offsets):
                        if t is not None and t.is_cuda:
                            t.record_stream(main)
        # shallow copies: ops such as FillMissing mutate the frame they are given
        return DeviceFrame.concat_columns(ups).copy()

    def _branch_streams(self, upstream, cache):
        """One stream per upstream subtree when there are several, none of them is cached yet
        and they share no operator node (a shared node would be computed on one stream and
        read on another without ordering); None = run sequentially on the current stream."""
        if len(upstream) < 2 or not BRANCH_STREAMS:
            # opt-in: on the Criteo workflow the encode and fill+normalize kernels are both
            # HBM-bound, so running the two branches side by side only gained 1 % (19.9 ->
            # 19.7 ms) while blurring every per-kernel timing
            return None
        try:
            import torch

            if not torch.cuda.is_available():
                return None
        except Exception:
            return None
        seen: set = set()
        busy = 0
        for u in upstream:
            ids = {id(n) for n in iter_nodes(u) if n.op is not None}
            if ids & seen or any(i in cache for i in ids):
                return None
            seen |= ids
            busy += 1 if ids else 0
        if busy < 2:
            return None
        dev = torch.cuda.current_device()
        pool = getattr(self, "_streams", None)
        if pool is None or pool[0] != dev:
            pool = (dev, [torch.cuda.Stream(device=dev) for _ in range(2)])
            self._streams = pool
        out, k = [], 0
        for u in upstream:
            has_ops = any(n.op is not None for n in iter_nodes(u))
            out.append(pool[1][k % len(pool[1])] if has_ops else torch.cuda.current_stream())
            k += 1 if has_ops else 0
        return out

    # ---- fit ------------------------------------------------------------------------
    def fit(self, dataset: Dataset) -> "Workflow":
        self.clear_stats()
        self._fit_generation = getattr(self, "_fit_generation", 0) + 1
        # (re)fitting on an unchanged input schema: the graph's column schemas are already in
        # place (only fitted properties change, and those are refreshed lazily after the fit)
        if getattr(self, "_fit_root_schema", None) is None or not (dataset.schema == self._fit_root_schema):
            self.fit_schema(dataset.schema)
            self._fit_root_schema = dataset.schema
        nodes = iter_nodes(self.output_node)
        stat_nodes = [n for n in nodes if isinstance(n.op, StatOperator)]
        # an operator whose selector reads fitted properties (DropLowCardinality): the graph's schemas
        # and selectors are recomputed behind every fit phase, not lazily with the output schema
        refresh = any(getattr(n.op, "selector_from_fit", False) for n in nodes if n.op is not None)
        fitted: set = set()
        shard = (dist.rank(), dist.world_size()) if dist.world_size() > 1 else None
        roots = self._root_columns()
        while len(fitted) < len(stat_nodes):
            phase = [
                n for n in stat_nodes
                if id(n) not in fitted
                and all(id(a) in fitted for a in _stat_ancestors(n))
            ]
            if not phase:
                raise RuntimeError("failed to schedule StatOperators (dependency cycle?)")
            states = {id(n): n.op.fit_begin(n.input_columns) for n in phase}
            for part in dataset.to_iter(columns=roots, shard=shard):
                cache: Dict[int, DeviceFrame] = {}
                with pass_memo():  # one pass over this partition: shared intermediates
                    for n in phase:
                        inp = self._node_input(n, part, cache)
                        _guard_datetime(n, inp)
                        with annotate(n.op.range_name("fit")):
                            n.op.fit_partition(states[id(n)], n.input_columns, inp)
            # operators whose fit_end only reads a few scalars back (Normalize) go first: their
            # read-back is the step's one host synchronisation, and Categorify's fit_end (which
            # finds its counts already complete) then enqueues the vocabulary sorts and table
            # builds with nothing between them and the transform kernels that follow.
            # (stable sort: the order is the same on every rank, as the collectives need)
            for n in sorted(phase, key=lambda n: getattr(n.op, "fit_end_priority", 0)):
                with annotate(n.op.range_name("fit")):
                    n.op.fit_finalize(n.op.fit_end(states[id(n)], n.input_columns))
                fitted.add(id(n))
            if refresh:
                self.fit_schema(dataset.schema)
        # what the first transform would otherwise build in front of its first lookup (the lookup
        # images shared by the groupby operators of a key column) is enqueued behind the fit's last
        # kernels: it runs while the host walks into the transform
        for n in stat_nodes:
            prepare = getattr(n.op, "prepare_transform", None)
            if prepare is not None:
                prepare()
        # properties such as embedding sizes depend on the fitted state: refreshed lazily
        self._stale_schema_root = None if refresh else dataset.schema
        if any(getattr(n.op, "dynamic_dtypes", False) for n in nodes if n.op is not None):
            self._capture_dtypes(dataset)
        return self

    def _capture_dtypes(self, dataset):
        for part in dataset.to_iter(columns=self._root_columns()):
            out = self._run(self.output_node, part, {})
            sample = Schema.from_frame(out)
            cols = []
            for c in self.output_schema:
                s = sample.get(c.name)
                cols.append(c.with_dtype(s.dtype, s.is_list, s.is_ragged) if s is not None else c)
            self.output_schema = Schema(cols)
            self.output_node.output_schema = self.output_schema
            self.output_dtypes = {c.name: c.dtype for c in self.output_schema}
            break

    # ---- transform ---------------------------------------------------------------------
    def transform(self, data):
        if isinstance(data, Dataset):
            if self._output_schema is None:
                self.fit_schema(data.schema)
            roots = self._root_columns()

            def gen(columns=None, shard=None):
                for part in data.to_iter(columns=roots, shard=shard):
                    with pass_memo():  # operators on the same key column share one lookup
                        out_part = self._run(self.output_node, part, {})
                    yield out_part

            # (schema: lazily -- folding the fitted properties in is host work, and asking
            # Categorify for its embedding sizes would enqueue the vocabulary ordering ahead of
            # the kernels of the first partition that can run underneath it)
            # The fitted state the schema is folded from is captured NOW (the operators' fit
            # generation), so a re-fit between transform() and the first `.schema` access cannot
            # leak a later fit's schema into this dataset.
            out = Dataset(gen, schema=_FittedSchema(self), npartitions=data.npartitions)
            out._forwards_shard = True  # rank sharding is decided by the source dataset
            return out
        if isinstance(data, pd.DataFrame):
            if self._output_schema is None:
                self.fit_schema(Schema.from_frame(data))
            frame, _ = as_device_frame(data[self._root_columns()])
            with pass_memo():
                return self._run(self.output_node, frame, {}).to_pandas()
        if isinstance(data, DeviceFrame):
            if self._output_schema is None:
                self.fit_schema(Schema.from_frame(data))
            with pass_memo():
                return self._run(self.output_node, data, {})
        raise TypeError(f"Workflow.transform: unsupported input {type(data)}")

    def fit_transform(self, dataset: Dataset) -> Dataset:
        self.fit(dataset)
        return self.transform(dataset)

    # ---- persistence: graph.json + artifacts/ (reference workflow.py:256-297, 299-358) ------
    def save(self, path):
        """Save as ``metadata.json`` + ``graph.json`` + ``artifacts/node_<id>/`` -- the
        reference's pickle-free layout (graph_serializer.py:15-29), see graph_json.py."""
        import sys

        from . import __version__ as version
        from .graph_json import serialize_graph

        path = str(path)
        os.makedirs(path, exist_ok=True)
        _ = self.output_schema  # fold the fitted properties into the node schemas first
        meta = {
            "versions": {"nvtabular": version, pd.__name__: pd.__version__, "python": sys.version},
            "generated_timestamp": int(time.time()),
            "engine": "nvtabular_amd",
        }
        with open(os.path.join(path, "metadata.json"), "w") as f:
            json.dump(meta, f)
        serialize_graph(self, path)

    @classmethod
    def load(cls, path, client=None) -> "Workflow":
        path = str(path)
        if not os.path.exists(os.path.join(path, "graph.json")):
            # workflow.pkl files of the first revision are not read: unpickling runs arbitrary
            # code (the reference ships a restricted unpickler for the same reason)
            raise FileNotFoundError(f"{path} holds no graph.json (pickled workflows are not loaded)")
        from .graph_json import deserialize_graph

        wf = cls(deserialize_graph(path), client=client)
        wf._output_schema = wf.output_node.output_schema
        if wf._output_schema is not None:
            wf.output_dtypes = {c.name: c.dtype for c in wf._output_schema}
        roots = []
        for node in iter_nodes(wf.output_node):
            if node.op is None and node.input_schema is not None:
                roots += [c for c in node.input_schema if c.name not in {r.name for r in roots}]
        wf.input_schema = Schema(roots) if roots else None
        return wf

    def clear_stats(self):
        for node in iter_nodes(self.output_node):
            if isinstance(node.op, StatOperator):
                node.op.clear()


def _guard_datetime(node: Node, inp: DeviceFrame):
    """An operator that computes on numbers is not handed a datetime column (int64 counts under
    a logical type): it would normalise, clip or average epoch counts without a word."""
    for name in node.op.datetime_rejects(node.input_columns, inp):
        raise TypeError(f"{node.op.label}: column '{name}' is {inp[name].logical}; convert it first, "
                        f"e.g. ['{name}'] >> LambdaOp(lambda c: c.dt.hour)")


def _async_pending(node: Node) -> bool:
    return any(n.op is not None and n.op.async_pending for n in iter_nodes(node))


def _stat_ancestors(node: Node) -> List[Node]:
    out = []
    for u in node.parents_with_dependencies:
        for a in iter_nodes(u):
            if isinstance(a.op, StatOperator):
                out.append(a)
    return out


_DEVICE_ATTRS = ("_encoders", "_device_stats")


def _strip_device_state(wf):
    saved = []
    for node in iter_nodes(wf.output_node):
        for attr in _DEVICE_ATTRS:
            if node.op is not None and getattr(node.op, attr, None):
                saved.append((node.op, attr, getattr(node.op, attr)))
                setattr(node.op, attr, {})
    return saved


def _restore_device_state(saved):
    for op, attr, val in saved:
        setattr(op, attr, val)
