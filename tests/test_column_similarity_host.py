"""ops.ColumnSimilarity without a GPU: construction, column names, output schema, refusals."""
import numpy as np
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import kernels_similarity as KS, ops
from nvtabular_amd.schema import ColumnSchema, Schema, Tags
from nvtabular_amd.selector import ColumnSelector

F = ([0, 1, 1], [0, 2, 2], [1.0, 2.0, 3.0], (2, 3))


def test_constructor_validation():
    for metric in ("tfidf", "cosine", "inner"):
        assert ops.ColumnSimilarity(F, metric=metric, on_device=False).metric == metric
    with pytest.raises(ValueError, match="unknown distance metric"):
        ops.ColumnSimilarity(F, metric="jaccard")
    for bad in (np.eye(3), torch.eye(3), [[1.0]], (1, 2, 3), None):
        with pytest.raises(TypeError, match="feature matrix"):
            ops.ColumnSimilarity(bad)
        with pytest.raises(TypeError, match="feature matrix"):
            ops.ColumnSimilarity(F, right_features=bad if bad is not None else "x")
    with pytest.raises(TypeError, match="integers"):   # (found when the entries are read, not at construction)
        KS.as_coo(([0.5], [0], [1.0], (2, 3)))
    for shape in ((0, 3), (2, 2**31), (2**31, 2)):
        with pytest.raises(ValueError, match="shape"):
            ops.ColumnSimilarity(([0], [0], [1.0], shape))
    with pytest.raises(ValueError, match="one length"):
        ops.ColumnSimilarity(([0, 1], [0], [1.0], (2, 3)))
    assert ops.ColumnSimilarity(torch.eye(3).to_sparse()).right_features is None
    assert ops.ColumnSimilarity(torch.eye(3).to_sparse_csr(), right_features=F).right_features is F
    import nvtabular
    from nvtabular.ops.column_similarity import ColumnSimilarity

    assert nvtabular.ops.ColumnSimilarity is ColumnSimilarity is ops.ColumnSimilarity


def test_names_and_schema():
    op = ops.ColumnSimilarity(F, metric="cosine")
    sel = ColumnSelector([["a", "b"], ["a", "c"]])
    assert op.column_mapping(sel) == {"a_b_sim": ["a", "b"], "a_c_sim": ["a", "c"]}
    wf = nvt.Workflow([["a", "b"], ["a", "c"]] >> op)
    wf.fit_schema(Schema([ColumnSchema(n, np.int64, tags=[Tags.CATEGORICAL]) for n in "abc"]))
    out = wf.output_schema
    assert out.column_names == ["a_b_sim", "a_c_sim"]
    for name in out.column_names:
        col = out[name]
        assert np.dtype(col.dtype) == np.float64 and not col.is_list and list(col.tags) == [Tags.CONTINUOUS]


@pytest.mark.parametrize("groups", [["a", "b"], [["a", "b", "c"]], [["a"]], [["a", "b"], "c"]])
def test_groups_have_exactly_two_names(groups):
    with pytest.raises(ValueError, match="exactly two"):
        ops.ColumnSimilarity(F).column_mapping(ColumnSelector(groups))


def test_save_is_deferred(tmp_path):
    wf = nvt.Workflow([["a", "b"]] >> ops.ColumnSimilarity(F))
    wf.fit_schema(Schema([ColumnSchema(n, np.int64) for n in "ab"]))
    with pytest.raises(NotImplementedError, match="ColumnSimilarity"):
        wf.save(str(tmp_path / "wf"))
