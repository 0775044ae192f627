"""Embedding layers on the device: the host driver of ``nvt_emb_*`` (include/nvt_hip.h) and the
autograd function behind ``framework_utils.torch.layers``.

``LayerTables`` holds what a layer's launches share: the descriptor array (rebuilt when a parameter's
``data_ptr`` changes, e.g. after ``.to()`` or ``load_state_dict``), the slice of every table in the
concatenated output and the device counter of ids outside their table.  ``embed`` runs the fused
forward -- ``nvt_emb_gather_cat`` for an id matrix, ``nvt_emb_bag`` for bags -- and, through
``_EmbedFn.backward``, plan + reduce: one gradient per table, sparse (coalesced, ascending ids) for
the tables named sparse and written row by row into a zeroed dense tensor for the others.  One
read-back per backward (the unique-row counts that size the outputs).

Same conventions as kernels_similarity: launches under ``kernels.LAUNCH_LOCK`` on torch's current
stream, errors through ``_lib.check``, workspace from torch's allocator, ``K.stat_add`` per call."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import kernels as K
from ._lib import check

MODES = {"sum": _lib.EMB_SUM, "mean": _lib.EMB_MEAN}
MAX_TOTAL_ROWS = (1 << 32) - 2   # include/nvt_hip.h: the rows of all tables of a layer together
MAX_ENTRIES = (1 << 30) - 1      # ids / bag values of one call (the device word sort)
_ID_CODE = {torch.int32: _lib.NVT_I32, torch.int64: _lib.NVT_I64}


class LayerTables:
    """The tables of one layer: shapes, output slices, cached descriptors, out-of-range counter."""

    def __init__(self, shapes, sparse=()):
        shapes = [(int(r), int(d)) for r, d in shapes]
        if not 1 <= len(shapes) <= _lib.EMB_MAX_TABLES:
            raise ValueError(f"a layer has 1 to {_lib.EMB_MAX_TABLES} embedding tables, not {len(shapes)}")
        for rows, dim in shapes:
            if rows < 1 or dim < 1:
                raise ValueError(f"embedding table shape {(rows, dim)}: at least one row and one column")
        if sum(r for r, _ in shapes) > MAX_TOTAL_ROWS:
            raise ValueError("the tables of a layer hold fewer than 2^32 - 1 rows together")
        self.shapes = shapes
        self.sparse = tuple(bool(s) for s in sparse) or (False,) * len(shapes)
        self.out_cols = sum(d for _, d in shapes)
        self._ptrs = None
        self._array = None
        self._counters = {}

    def array(self, weights):
        ptrs = tuple(w.data_ptr() for w in weights)
        if ptrs != self._ptrs:
            arr = (_lib.EmbTable * len(weights))()
            col = 0
            for i, (w, (rows, dim)) in enumerate(zip(weights, self.shapes)):
                if tuple(w.shape) != (rows, dim) or w.dtype != torch.float32 or not w.is_contiguous():
                    raise ValueError(f"embedding table {i}: contiguous float32 {(rows, dim)} expected, "
                                     f"got {w.dtype} {tuple(w.shape)}")
                arr[i].weight, arr[i].rows, arr[i].dim, arr[i].out_col = w.data_ptr(), rows, dim, col
                col += dim
            self._ptrs, self._array = ptrs, arr
        return self._array

    def counter(self, device) -> torch.Tensor:
        """int64[1] on ``device``: ids outside their table seen by the forward calls so far."""
        c = self._counters.get(device)
        if c is None:
            c = self._counters[device] = torch.zeros(1, dtype=torch.int64, device=device)
        return c


def _bag_array(bags):
    arr = (_lib.EmbBagCol * len(bags))()
    for i, (values, offsets) in enumerate(bags):
        arr[i].values, arr[i].offsets, arr[i].nvalues = K.ptr(values) if values.numel() else None, offsets.data_ptr(), \
            values.numel()
    return arr


def _forward(tables: LayerTables, ids, bags, mode, weights):
    lib = _lib.load()
    dev = weights[0].device
    batch = ids.shape[0] if ids is not None else bags[0][1].numel() - 1
    out = torch.empty((batch, tables.out_cols), dtype=torch.float32, device=dev)
    if batch == 0:
        return out
    with K.LAUNCH_LOCK:
        arr = tables.array(weights)
        oor = tables.counter(dev)
        if ids is not None:
            K.stat_add("emb_gather_cat")
            check(lib.nvt_emb_gather_cat(ids.data_ptr(), _ID_CODE[ids.dtype], batch, arr, len(weights), out.data_ptr(),
                                         tables.out_cols, oor.data_ptr(), K.stream_ptr()), "nvt_emb_gather_cat")
        else:
            K.stat_add("emb_bag")
            check(lib.nvt_emb_bag(_bag_array(bags), _ID_CODE[bags[0][0].dtype], batch, arr, len(weights), MODES[mode],
                                  out.data_ptr(), tables.out_cols, oor.data_ptr(), K.stream_ptr()), "nvt_emb_bag")
    return out


def _backward(tables: LayerTables, ids, bags, mode, weights, grad_out):
    """One gradient per table: plan, the one read-back, reduce."""
    lib = _lib.load()
    dev = grad_out.device
    nt = len(weights)
    grad_out = K.aligned(grad_out.to(torch.float32))
    batch = grad_out.shape[0]
    entries = ids.numel() if ids is not None else sum(v.numel() for v, _ in bags)
    if entries > MAX_ENTRIES:
        raise ValueError(f"{entries} ids in one batch: the device sort takes fewer than 2^30")
    need = C.c_uint64()
    check(lib.nvt_emb_grad_ws_bytes(entries, C.byref(need)), "nvt_emb_grad_ws_bytes")
    with K.LAUNCH_LOCK:
        arr = tables.array(weights)
        bag_arr = _bag_array(bags) if bags is not None else None
        dtype = _ID_CODE[ids.dtype if ids is not None else bags[0][0].dtype]
        K.stat_add("emb_grad")
        stream = K.stream_ptr()
        ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
        state = torch.empty(5 + nt, dtype=torch.int64, device=dev)
        check(lib.nvt_emb_grad_plan(ids.data_ptr() if ids is not None else None, bag_arr, dtype, batch, arr, nt,
                                    tables.out_cols, ws.data_ptr(), need.value, state.data_ptr(), stream),
              "nvt_emb_grad_plan")
        pending = K.PendingReadBack(state)
        # the dense gradients are zeroed behind the plan while the counts travel
        dense = [None if sp else torch.zeros_like(w) for sp, w in zip(tables.sparse, weights)]
        counts = [int(x) for x in pending.get()]   # the one host synchronisation
        partials = torch.empty(max(counts[4], 4), dtype=torch.float32, device=dev)
        outs = (_lib.EmbGradOut * nt)()
        keep = []
        for c, (rows, dim) in enumerate(tables.shapes):
            if tables.sparse[c]:
                uniq = torch.empty(counts[5 + c], dtype=torch.int64, device=dev)
                vals = torch.empty((counts[5 + c], dim), dtype=torch.float32, device=dev)
                outs[c].ids, outs[c].values, outs[c].count = K.ptr(uniq), K.ptr(vals), counts[5 + c]
                if counts[5 + c] == 0:
                    outs[c].ids, outs[c].values = ws.data_ptr(), None   # (an empty gradient: nothing is written)
                keep.append((uniq, vals))
            else:
                outs[c].ids, outs[c].values, outs[c].count = None, dense[c].data_ptr(), rows
                keep.append(None)
        host_counts = (C.c_int64 * len(counts))(*counts)
        check(lib.nvt_emb_grad_reduce(0 if ids is not None else 1, batch, entries, arr, nt, MODES[mode],
                                      grad_out.data_ptr(), tables.out_cols, ws.data_ptr(), need.value, host_counts,
                                      partials.data_ptr(), partials.numel(), outs, stream), "nvt_emb_grad_reduce")
    grads = []
    for c, (rows, dim) in enumerate(tables.shapes):
        if tables.sparse[c]:
            uniq, vals = keep[c]
            grads.append(torch.sparse_coo_tensor(uniq.unsqueeze(0), vals, (rows, dim), is_coalesced=True))
        else:
            grads.append(dense[c])
    return grads


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tables, ids, bags, mode, *weights):
        ctx.tables, ctx.ids, ctx.bags, ctx.mode = tables, ids, bags, mode
        ctx.save_for_backward(*weights)
        return _forward(tables, ids, bags, mode, [w.detach() for w in weights])

    @staticmethod
    def backward(ctx, grad_out):
        weights = ctx.saved_tensors
        if grad_out.shape[0] == 0:
            grads = [torch.zeros_like(w) for w in weights]
        else:
            grads = _backward(ctx.tables, ctx.ids, ctx.bags, ctx.mode, weights, grad_out)
        return (None, None, None, None, *grads)


def _check_ids(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype not in _ID_CODE:
        raise TypeError(f"{what} are int32 or int64, not {t.dtype}")
    return K.aligned(t)


def embed(tables: LayerTables, weights, ids=None, bags=None, mode: str = "sum") -> torch.Tensor:
    """float32 [B, sum of dims]: the rows ``ids[B, ntables]`` names, side by side -- or, with ``bags``
    (per table ``(values, offsets[B + 1])``), the sum / mean of every bag's rows.  Differentiable in
    ``weights``; the launches run on the current stream."""
    _lib.require_gpu()
    weights = list(weights)
    for t in ([ids] if ids is not None else [x for pair in bags for x in pair]) + weights:
        if not t.is_cuda:
            raise _lib.NvtHipError("the embedding layers run on the MI355X: tensor on the CPU (there is no CPU "
                                   "fallback in this engine)")
    if ids is not None:
        if ids.dim() != 2 or ids.shape[1] != len(weights):
            raise ValueError(f"ids of shape [B, {len(weights)}] expected, got {tuple(ids.shape)}")
        ids = _check_ids(ids, "ids")
        if ids.numel() > MAX_ENTRIES:
            raise ValueError(f"{ids.numel()} ids in one batch: a call takes fewer than 2^30")
    else:
        if len(bags) != len(weights):
            raise ValueError(f"{len(weights)} (values, offsets) pairs expected, got {len(bags)}")
        dtype = torch.int32 if all(v.dtype == torch.int32 for v, _ in bags) else torch.int64
        norm = []
        for values, offsets in bags:
            if values.dtype not in _ID_CODE:
                raise TypeError(f"bag values are int32 or int64, not {values.dtype}")
            if offsets.dim() != 1 or offsets.numel() != bags[0][1].numel() or offsets.numel() < 1:
                raise ValueError("every column of a batch has B + 1 offsets")
            norm.append((K.aligned(values.reshape(-1).to(dtype)), K.aligned(offsets.to(torch.int64))))
        bags = norm
    return _EmbedFn.apply(tables, ids, bags, mode, *weights)
