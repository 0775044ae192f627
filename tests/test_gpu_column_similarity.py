"""ops.ColumnSimilarity on the device (csrc/nvt_similarity.hip) against similarity_reference.py.

``inner`` on small integers is exact; ``cosine`` and ``tfidf`` hold |got - ref| <= (L + 16) 2^-52 S with
L the matching columns of the row pair and S the sum of |a_k b_k| over them: the kernel adds L
products in another order than the reference, and every weight carries a handful of roundings (log,
multiply, divide, square root, coalescing sum).  The bound is derived, not measured."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import _lib, kernels as K, kernels_similarity as KS, ops
from similarity_reference import assert_within_bound, similarity, weights

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 2, 8, 9, 63, 64, 65, 5000)
NCOLS = 6000


@functools.lru_cache(maxsize=None)
def boundary_case(metric):
    """One matrix with a row of every length in LENGTHS: half of a row (rounded down) lies at the start
    of one shared permutation of the columns below 2500, the rest in a slice of its own, so two rows
    overlap in anything from no column to all of them.  Returned with the 81 ordered pairs of its rows
    and their reference (sim, L, S)."""
    rng = np.random.default_rng(7)
    shared, private, row, col = rng.permutation(2500), 2500, [], []
    for r, m in enumerate(LENGTHS):
        own = m - m // 2
        col += [shared[: m // 2], np.arange(private, private + own)]
        row += [np.full(m, r)]
        private += own
    assert private <= NCOLS
    row, col = np.concatenate(row), np.concatenate(col)
    order = rng.permutation(len(row))
    row, col = row[order], col[order]
    data = rng.integers(1, 4, len(row)).astype(np.float64) if metric == "inner" else rng.uniform(0.5, 2.0, len(row))
    pairs = np.array([(a, b) for a in range(9) for b in range(9)])
    coo = (row, col, data, (len(LENGTHS), NCOLS))
    dense = weights(*coo, metric)
    return coo, pairs, similarity(pairs[:, 0], pairs[:, 1], dense, dense)


def data_rows(metric, n):
    """The 81 pairs repeated to n data rows in shuffled order: (coo, ids [n, 2], reference of the rows)."""
    coo, pairs, table = boundary_case(metric)
    which = np.random.default_rng(n).permutation(np.resize(np.arange(81), n))
    return coo, pairs[which], tuple(t[which] for t in table)


def bitmap(valid):
    return torch.from_numpy(np.packbits(np.asarray(valid, dtype=np.uint8), bitorder="little")).cuda()


def run_rows(metric, n, dtype):
    coo, ids, ref = data_rows(metric, n)
    short = np.minimum(np.array(LENGTHS)[ids[:, 0]], np.array(LENGTHS)[ids[:, 1]])
    for lo, hi in ((0, 0), (1, 8), (9, 64), (65, 5000)):   # the empty class and the three widths
        assert ((short >= lo) & (short <= hi)).any()
    f = KS.prepare(coo, metric)
    a, b = (torch.from_numpy(ids[:, k].copy()).to("cuda", dtype) for k in (0, 1))
    got = KS.row_similarity(a, None, b, None, f, f).cpu().numpy()
    assert (got[short == 0] == 0.0).all()
    assert_within_bound(got, ref, exact=metric == "inner")


# the class pass takes 1024 rows per workgroup and round: one workgroup, and five with a ragged last one
@pytest.mark.parametrize("n", [1000, 5000])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("metric", ["inner", "cosine", "tfidf"])
def test_class_boundaries(metric, dtype, n):
    run_rows(metric, n, dtype)


def test_second_round_of_a_full_grid():
    """More rows than the capped grids cover at once (2048 workgroups of 1024 rows in the class pass, of
    64, 16 and 4 rows in the products): the second round of the class pass reserves list slots behind
    the first, and the groups of the product kernels stride over their lists.  Exact."""
    run_rows("inner", 2048 * 1024 + 1500, torch.int32)


# unsorted, (2, 3) stored twice on the left, a stored zero on both sides
LEFT = ([4, 2, 0, 2, 5, 2, 0, 3], [1, 3, 8, 0, 3, 3, 1, 3], [1.5, 2.0, 0.0, 1.0, 3.0, 0.5, 2.5, 1.0], (6, 9))
RIGHT = ([3, 0, 1, 3, 1, 0], [3, 1, 10, 0, 3, 8], [2.0, 1.0, 4.0, 0.0, 0.25, 3.0], (4, 11))
IDS = (np.array([2, 2, 0, 4, 5, 3, 1, 0, 2]), np.array([3, 1, 0, 0, 1, 3, 2, 3, 0]))


def as_form(coo, form):
    row, col, data, shape = coo
    if form == "tuple":
        return coo
    if form == "scipy":
        return pytest.importorskip("scipy.sparse").coo_matrix((data, (row, col)), shape=shape)
    return torch.sparse_coo_tensor(torch.tensor([row, col]), torch.tensor(data, dtype=torch.float32), shape)


@pytest.mark.parametrize("form", ["torch", "tuple", "scipy"])
def test_preparation_is_entry_by_entry(form):
    a, b = IDS
    ref = similarity(a, b, weights(*LEFT, "tfidf"), weights(*RIGHT, "tfidf"))
    merged = similarity(a, b, weights(*LEFT, "tfidf", merge_first=True), weights(*RIGHT, "tfidf"))
    assert np.abs(ref[0] - merged[0]).max() > 1e-3   # the inputs tell the two orders apart
    lf, rf = KS.prepare(as_form(LEFT, form), "tfidf"), KS.prepare(as_form(RIGHT, form), "tfidf")
    assert lf.weights.dtype == torch.float64 and lf.indices.dtype == torch.int32 and lf.indptr.dtype == torch.int64
    assert lf.indptr.tolist() == [0, 2, 2, 4, 5, 6, 7] and lf.indices.tolist() == [1, 8, 0, 3, 3, 1, 3]
    got = KS.row_similarity(torch.from_numpy(a).cuda(), None, torch.from_numpy(b).cuda(), None, lf, rf)
    assert_within_bound(got.cpu().numpy(), ref)


def test_nulls_range_and_empty_frame():
    a = np.array([2, 2, 6, -1, 2**40, 1, 2, 0, 5, 2, 4])       # 6 = shape[0]; row 1 of LEFT is empty
    b = np.array([3, 3, 0, 0, 0, 3, 4, 2, -1, 2, 0])           # 4 = shape[0]; row 2 of RIGHT is empty
    a_ok = np.array([1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=bool)
    b_ok = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=bool)
    ref = similarity(a, b, weights(*LEFT, "cosine"), weights(*RIGHT, "cosine"), ~a_ok, ~b_ok)
    assert np.isnan(ref[0]).sum() == 7 and (ref[0][[5, 7]] == 0.0).all()
    lf, rf = KS.prepare(LEFT, "cosine"), KS.prepare(RIGHT, "cosine")
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = KS.row_similarity(ta, bitmap(a_ok), tb, bitmap(b_ok), lf, rf).cpu().numpy()
    assert_within_bound(got, ref)
    assert (got[[5, 7]] == 0.0).all()
    assert KS.row_similarity(ta[:0], None, tb[:0], None, lf, rf).shape == (0,)
    with pytest.raises(ValueError, match="outside its shape"):
        KS.prepare(([0, 6], [0, 0], [1.0, 1.0], (6, 9)), "inner")


def test_workflow_two_partitions_and_one_preparation():
    coo, ids, _ = data_rows("cosine", 1000)
    df = pd.DataFrame({"a": ids[:, 0], "b": ids[:, 1], "c": ids[::-1, 0].astype(np.int32)})
    dense = weights(*coo, "cosine")
    wf = nvt.Workflow([["a", "b"], ["a", "c"]] >> ops.ColumnSimilarity(coo, metric="cosine"))
    out = wf.fit_transform(nvt.Dataset(df, npartitions=2)).to_ddf().compute()
    assert list(out.columns) == ["a_b_sim", "a_c_sim"] and (out.dtypes == np.float64).all()
    for name, other in (("a_b_sim", "b"), ("a_c_sim", "c")):
        assert_within_bound(out[name].to_numpy(), similarity(df["a"], df[other], dense, dense))
    before = K.STATS["similarity_prepare"]
    wf.transform(nvt.Dataset(df, npartitions=2)).to_ddf().compute()
    assert K.STATS["similarity_prepare"] == before
    with pytest.raises(TypeError, match="'x'"):
        ops.ColumnSimilarity(coo).transform(nvt.ColumnSelector([["a", "x"]]), df.assign(x=df["a"] * 0.5))


def test_c_entry_point_keeps_its_bounds_and_refuses_bad_arguments():
    lib = _lib.load()
    coo, ids, ref = data_rows("inner", 1000)
    f = KS.prepare(coo, "inner")
    n = len(ids)
    a, b = (torch.from_numpy(ids[:, k].copy()).cuda() for k in (0, 1))
    need = C.c_uint64()
    assert lib.nvt_row_similarity_ws_bytes(n, C.byref(need)) == 0
    ws = torch.empty(need.value // 8, dtype=torch.int64, device="cuda")
    out = torch.full((n + 64,), -7.25, dtype=torch.float64, device="cuda")
    csr = f.struct()
    args = [a.data_ptr(), None, b.data_ptr(), None, _lib.NVT_I64, n, C.byref(csr), C.byref(csr), out.data_ptr(),
            ws.data_ptr(), need.value, K.stream_ptr()]
    assert lib.nvt_row_similarity(*args) == 0
    host = out.cpu().numpy()
    assert (host[n:] == -7.25).all()
    assert_within_bound(host[:n], ref, exact=True)
    for at, bad in ((0, None), (2, None), (8, None), (9, None), (6, None), (4, _lib.NVT_F64), (4, _lib.NVT_U8),
                    (5, 2**31), (10, need.value - 1)):
        refused = list(args)
        refused[at] = bad
        assert lib.nvt_row_similarity(*refused) == _lib.NVT_EINVAL, (at, bad)
    assert lib.nvt_row_similarity_ws_bytes(2**31, C.byref(need)) == _lib.NVT_EINVAL
