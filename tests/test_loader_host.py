"""The dataloader's host side: names, schema roles, construction errors and len().  No GPU."""
import numpy as np
import pandas as pd
import pytest

import nvtabular_amd as nvt
from nvtabular_amd.schema import ColumnSchema, Schema, Tags


def _ds(rows=100, parts=3):
    df = pd.DataFrame({"a": np.arange(rows), "b": np.arange(rows) % 7, "x": np.arange(rows) / 3.0,
                       "label": np.arange(rows) % 2})
    return nvt.Dataset(df, npartitions=parts)


def test_import_under_both_names():
    import nvtabular  # noqa: F401
    import nvtabular.loader.backend as ref_backend
    import nvtabular.loader.torch as ref_torch
    import nvtabular_amd.loader.backend as backend
    import nvtabular_amd.loader.torch as ours
    from nvtabular.loader.torch import DLDataLoader, TorchAsyncItr

    assert TorchAsyncItr is ours.TorchAsyncItr and DLDataLoader is ours.DLDataLoader
    assert ref_torch is ours and ref_backend is backend


def test_augment_schema_tags_roles():
    from nvtabular_amd.loader.backend import _augment_schema

    s = Schema([ColumnSchema("a"), ColumnSchema("x"), ColumnSchema("label"), ColumnSchema("other")])
    out = _augment_schema(s, cats=["a"], conts=["x"], labels="label")
    assert out["a"].tags == (Tags.CATEGORICAL,) and out["x"].tags == (Tags.CONTINUOUS,)
    assert out["label"].tags == (Tags.TARGET,) and out["other"].tags == ()
    assert s["a"].tags == ()            # the input schema is not changed
    with pytest.raises(ValueError, match="nope"):
        _augment_schema(s, cats=["nope"])


def test_roles_default_to_the_schema_tags():
    from nvtabular_amd.loader.torch import TorchAsyncItr

    ds = _ds()
    ds._schema = Schema([ColumnSchema("a", tags=[Tags.CATEGORICAL]), ColumnSchema("b", tags=[Tags.CATEGORICAL]),
                         ColumnSchema("x", tags=[Tags.CONTINUOUS]), ColumnSchema("label", tags=[Tags.TARGET])])
    it = TorchAsyncItr(ds, batch_size=10)
    assert (it.cat_names, it.cont_names, it.label_names) == (["a", "b"], ["x"], ["label"])
    it = TorchAsyncItr(_ds(), cats=["b"], labels="label", batch_size=10)
    assert (it.cat_names, it.cont_names, it.label_names) == (["b"], [], ["label"])
    assert Tags.TARGET in it.dataset.schema["label"].tags and Tags.CATEGORICAL in it.dataset.schema["b"].tags


def test_construction_errors():
    from nvtabular_amd.loader.torch import TorchAsyncItr

    with pytest.raises(ValueError, match="'a'"):
        TorchAsyncItr(_ds(), cats=["a"], conts=["a"])
    with pytest.raises(ValueError, match="'a'"):
        TorchAsyncItr(_ds(), cats=["a"], labels=["a"])
    with pytest.raises(ValueError, match="missing"):
        TorchAsyncItr(_ds(), cats=["missing"])
    with pytest.raises(ValueError, match="CPU"):
        TorchAsyncItr(_ds(), cats=["a"], device="cpu")
    with pytest.raises(ValueError, match="no columns"):
        TorchAsyncItr(_ds())
    with pytest.raises(ValueError, match="sparse_max"):
        TorchAsyncItr(_ds(), cats=["a"], sparse_names=["a"], sparse_as_dense=True)


@pytest.mark.parametrize("batch_size", [10, 9, 8])
@pytest.mark.parametrize("drop_last", [True, False])
def test_len(batch_size, drop_last):
    from nvtabular_amd.loader.torch import TorchAsyncItr

    it = TorchAsyncItr(_ds(100), cats=["a"], labels=["label"], batch_size=batch_size, drop_last=drop_last)
    want = 100 // batch_size if drop_last else -(-100 // batch_size)
    assert len(it) == want
    it.batch_size = 2 * batch_size       # settable between epochs
    assert len(it) == (100 // (2 * batch_size) if drop_last else -(-100 // (2 * batch_size)))
    parts = [pd.DataFrame({"a": np.arange(k)}) for k in (30, 20, 25, 25)]
    two = [TorchAsyncItr(nvt.Dataset(parts), cats=["a"], batch_size=7, global_size=2, global_rank=r) for r in (0, 1)]
    assert [len(t) for t in two] == [-(-55 // 7), -(-45 // 7)]      # partitions 0, 2 and 1, 3
