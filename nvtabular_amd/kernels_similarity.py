"""Row-wise sparse similarity on the device: the host driver of ``nvt_similarity_*`` and
``nvt_row_similarity`` (include/nvt_hip.h), behind ``ops.ColumnSimilarity``.

``check_features`` validates a feature matrix (torch sparse COO / CSR tensor, scipy.sparse matrix, or a
plain ``(row, col, data, shape)`` tuple) without converting it, ``as_coo`` reads it as shape plus
index / value arrays; ``prepare`` weights, orders and coalesces it on the device into a ``Features``
(canonical CSR, float64) with ONE read-back:
the coalesced nnz, together with the count of entries outside the shape.  ``row_similarity`` then
runs the class pass and the three dot launches per partition without any host synchronisation.

Same conventions as kernels_join: launches under ``kernels.LAUNCH_LOCK`` on torch's current stream,
errors through ``_lib.check``, workspace from torch's allocator, one ``K.stat_add`` counter per call."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

METRICS = {"inner": _lib.SIM_INNER, "cosine": _lib.SIM_COSINE, "tfidf": _lib.SIM_TFIDF}
MAX_DIM = (1 << 31) - 1       # shape[0], shape[1] (int32 column indices, nvt_row_similarity)
MAX_ENTRIES = (1 << 30) - 1   # the device word sort orders fewer than 2^30 entries


class Features(NamedTuple):
    """A prepared feature matrix: canonical CSR on the device."""
    indptr: torch.Tensor    # int64 [rows + 1]
    indices: torch.Tensor   # int32 [nnz]
    weights: torch.Tensor   # float64 [nnz]
    rows: int

    def struct(self) -> "_lib.Csr":
        s = _lib.Csr()
        s.indptr, s.indices, s.weights, s.rows = (self.indptr.data_ptr(), K.ptr(self.indices), K.ptr(self.weights),
                                                  self.rows)
        return s


def _scipy_sparse():
    try:
        import scipy.sparse as sp
    except ImportError:
        return None
    return sp


def check_features(features):
    """The cheap half of ``as_coo``: ``TypeError`` for anything that is no feature matrix and
    ``ValueError`` past the limits, from the type, the shape and the stored-entry count alone (no
    conversion, no copy).  The shape is returned."""
    sp = _scipy_sparse()
    if isinstance(features, torch.Tensor) and features.layout in (torch.sparse_coo, torch.sparse_csr) \
            and features.dim() == 2:
        shape = tuple(features.shape)
        nnz = features._values().shape[0] if features.layout == torch.sparse_coo else features.values().shape[0]
    elif sp is not None and sp.issparse(features):
        shape, nnz = tuple(features.shape), features.nnz
    elif isinstance(features, tuple) and len(features) == 4:
        shape = tuple(int(x) for x in features[3])
        row, col, data = features[:3]
        if not (len(row) == len(col) == len(data)):
            raise ValueError("a feature matrix has row, col and data of one length")
        nnz = len(data)
    else:
        raise TypeError("a feature matrix is a torch sparse COO / CSR tensor, a scipy.sparse matrix or a "
                        f"(row, col, data, shape) tuple, not {type(features).__name__}")
    if len(shape) != 2 or not (1 <= shape[0] <= MAX_DIM and 1 <= shape[1] <= MAX_DIM):
        raise ValueError(f"feature matrix shape {shape}: two sides, each 1 to 2^31 - 1")
    if nnz > MAX_ENTRIES:
        raise ValueError(f"feature matrix with {nnz} entries: the device sort takes fewer than 2^30")
    return shape


def as_coo(features):
    """(row, col, data, (n_rows, n_cols)) of a feature matrix, entries as stored (no coalescing)."""
    shape = check_features(features)
    if isinstance(features, torch.Tensor) and features.layout == torch.sparse_coo:
        idx = features._indices()
        row, col, data = idx[0], idx[1], features._values()
    elif isinstance(features, torch.Tensor):
        crow = features.crow_indices()
        row = torch.repeat_interleave(torch.arange(shape[0], device=crow.device), crow[1:] - crow[:-1])
        col, data = features.col_indices(), features.values()
    elif isinstance(features, tuple):
        row, col, data = (x if isinstance(x, torch.Tensor) else np.asarray(x) for x in features[:3])
    else:
        m = features.tocoo()
        row, col, data = m.row, m.col, m.data
    for x in (row, col):
        if x.dtype.is_floating_point if isinstance(x, torch.Tensor) else x.dtype.kind not in "iu":
            raise TypeError(f"row and col of a feature matrix are integers, not {x.dtype}")
    return row, col, data, shape


def prepare(features, metric: str, device=None) -> Features:
    """Weight (``metric``), order by (row, col) and coalesce a feature matrix on the device."""
    _lib.require_gpu()
    lib = _lib.load()
    row, col, data, (n_rows, n_cols) = as_coo(features)
    with K.LAUNCH_LOCK:
        dev = device or torch.device("cuda")
        row, col = (torch.as_tensor(x).to(dev, torch.int64).contiguous() for x in (row, col))
        data = torch.as_tensor(data).to(dev, torch.float64).contiguous()
        nnz = int(data.numel())
        K.stat_add("similarity_prepare")
        stream = K.stream_ptr()
        need = C.c_uint64()
        check(lib.nvt_similarity_prepare_ws_bytes(nnz, n_rows, n_cols, C.byref(need)), "nvt_similarity_prepare_ws_bytes")
        ws = torch.empty(need.value // 8, dtype=torch.int64, device=dev)
        state = torch.empty(2, dtype=torch.int64, device=dev)
        check(lib.nvt_similarity_prepare(K.ptr(row) if nnz else None, K.ptr(col) if nnz else None,
                                         K.ptr(data) if nnz else None, nnz, n_rows, n_cols, METRICS[metric],
                                         ws.data_ptr(), need.value, state.data_ptr(), stream), "nvt_similarity_prepare")
        nnz_out, bad = (int(x) for x in K.read_back(state))   # the one host synchronisation
        if bad:
            raise ValueError(f"feature matrix: {bad} entries lie outside its shape {(n_rows, n_cols)}")
        indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        indices = torch.empty(nnz_out, dtype=torch.int32, device=dev)
        weights = torch.empty(nnz_out, dtype=torch.float64, device=dev)
        if nnz_out:
            check(lib.nvt_similarity_coalesce(ws.data_ptr(), need.value, nnz, n_rows, n_cols, nnz_out, indptr.data_ptr(),
                                              indices.data_ptr(), weights.data_ptr(), stream), "nvt_similarity_coalesce")
        return Features(indptr, indices, weights, n_rows)


def row_similarity(left, left_valid, right, right_valid, lf: Features, rf: Features) -> torch.Tensor:
    """float64[n]: the dot product of row ``left[i]`` of ``lf`` and row ``right[i]`` of ``rf``; NaN for a
    null or out-of-range id, 0.0 where a row has no entry.  ``left`` / ``right``: int32 or int64."""
    _lib.require_gpu()
    lib = _lib.load()
    if left.dtype != right.dtype:
        left, right = left.to(torch.int64), right.to(torch.int64)
    if left.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"id columns are int32 or int64, not {left.dtype}")
    left, right = left.contiguous(), right.contiguous()
    n = int(left.numel())
    out = torch.empty(n, dtype=torch.float64, device=left.device)
    if n == 0:
        return out
    need = C.c_uint64()
    check(lib.nvt_row_similarity_ws_bytes(n, C.byref(need)), "nvt_row_similarity_ws_bytes")
    with K.LAUNCH_LOCK:
        ws = torch.empty(need.value // 8, dtype=torch.int64, device=left.device)
        K.stat_add("row_similarity")
        check(lib.nvt_row_similarity(left.data_ptr(), K.ptr(left_valid), right.data_ptr(), K.ptr(right_valid),
                                     K.dtype_code(left.dtype), n, C.byref(lf.struct()), C.byref(rf.struct()),
                                     out.data_ptr(), ws.data_ptr(), need.value, K.stream_ptr()),
              "nvt_row_similarity")
    return out
