"""framework_utils.torch without a GPU: import paths, construction, parameter names, the no-GPU error
and the host-side refusals of the nvt_emb_* entry points."""
import ctypes as C

import pytest
import torch

from nvtabular_amd import _lib

SHAPES = ({"a": (10, 4), "b": (7, 3)}, {"m": (5, 8)})


def _model():
    from nvtabular.framework_utils.torch.models import Model

    return Model(SHAPES, 2, 0.0, [8, 4], [0.0, 0.0], max_output=5.0, bag_mode="mean")


def test_import_paths_resolve_to_the_new_modules():
    import nvtabular.framework_utils
    import nvtabular.framework_utils.torch
    import nvtabular.framework_utils.torch.layers as layers
    import nvtabular.framework_utils.torch.models as models
    import nvtabular_amd.framework_utils.torch.layers as amd_layers
    import nvtabular_amd.framework_utils.torch.models as amd_models

    assert layers is amd_layers and models is amd_models
    assert nvtabular.framework_utils.torch.__name__ == "nvtabular_amd.framework_utils.torch"
    assert layers.ConcatenatedEmbeddings is models.ConcatenatedEmbeddings


def test_state_dict_names_match_the_reference_and_load():
    from nvtabular.framework_utils.torch.layers import ConcatenatedEmbeddings, MultiHotEmbeddings

    model = _model()
    emb_keys = [k for k in model.state_dict() if "embedding_layers" in k]
    assert emb_keys == ["initial_cat_layer.embedding_layers.0.weight", "initial_cat_layer.embedding_layers.1.weight",
                        "mh_cat_layer.embedding_layers.0.weight"]
    # weights of torch's own modules under those names load
    src = {"embedding_layers.0.weight": torch.nn.Embedding(10, 4).weight.data,
           "embedding_layers.1.weight": torch.nn.Embedding(7, 3).weight.data}
    layer = ConcatenatedEmbeddings(SHAPES[0], sparse_columns=["b"])
    layer.load_state_dict(src)
    assert torch.equal(layer.embedding_layers[1].weight.data, src["embedding_layers.1.weight"])
    bag = torch.nn.EmbeddingBag(5, 8, mode="sum")
    MultiHotEmbeddings(SHAPES[1]).load_state_dict({"embedding_layers.0.weight": bag.weight.data})
    with pytest.raises(ValueError, match="not in embedding_table_shapes"):
        ConcatenatedEmbeddings(SHAPES[0], sparse_columns=["zz"])
    with pytest.raises(NotImplementedError):
        MultiHotEmbeddings(SHAPES[1], mode="max")


def test_forward_on_cpu_tensors_raises_the_no_gpu_error():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    model = _model()
    x_cat = (torch.zeros(3, 2, dtype=torch.int64), {"m": (torch.zeros(3, dtype=torch.int64), torch.arange(3))})
    with pytest.raises(_lib.NvtHipError, match="no CPU fallback"):
        model(x_cat, torch.zeros(3, 2))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: nothing is read through them."""
    lib = _lib.load()
    raw = (C.c_uint8 * 4096)()
    base = (C.addressof(raw) + 255) & ~255
    ids, out, oor, ws = base, base + 1024, base + 2048, base + 2304

    def tables(rows=10, dim=4, out_col=0):
        t = (_lib.EmbTable * 1)()
        t[0].weight, t[0].rows, t[0].dim, t[0].out_col = base + 3072, rows, dim, out_col
        return t

    def refused(rc, word):
        assert rc == _lib.NVT_EINVAL and word in lib.nvt_last_error(), (rc, lib.nvt_last_error())

    gather = lambda t, batch=4, n=1, cols=4: lib.nvt_emb_gather_cat(ids, _lib.NVT_I64, batch, t, n, out, cols, oor, None)
    refused(gather(None), b"null descriptors")
    refused(gather(tables(dim=0)), b"dim")
    refused(gather(tables(rows=0)), b"rows")
    refused(gather(tables(rows=2**32 - 1)), b"rows")          # the row limit
    refused(gather(tables(out_col=4)), b"behind out_cols")
    refused(gather(tables(), n=65), b"NVT_EMB_MAX_TABLES")
    refused(gather(tables(), batch=2**30), b"2^30")           # the entry limit
    refused(gather(tables(), batch=2**32), b"batch")
    refused(lib.nvt_emb_gather_cat(ids, 7, 4, tables(), 1, out, 4, oor, None), b"dtype")
    refused(lib.nvt_emb_gather_cat(None, _lib.NVT_I64, 4, tables(), 1, out, 4, oor, None), b"null ids")
    bag = (_lib.EmbBagCol * 1)()
    bag[0].values, bag[0].offsets, bag[0].nvalues = ids, ids, 2**32
    refused(lib.nvt_emb_bag(bag, _lib.NVT_I64, 4, tables(), 1, 0, out, 4, oor, None), b"2^30")
    bag[0].nvalues = 8
    refused(lib.nvt_emb_bag(bag, _lib.NVT_I64, 4, tables(), 1, 2, out, 4, oor, None), b"mode")
    refused(lib.nvt_emb_bag(None, _lib.NVT_I64, 4, tables(), 1, 0, out, 4, oor, None), b"null bag columns")
    need = C.c_uint64()
    refused(lib.nvt_emb_grad_ws_bytes(2**32, C.byref(need)), b"2^30")
    assert lib.nvt_emb_grad_ws_bytes(1000, C.byref(need)) == 0 and need.value > 0
    plan = lambda t, i=ids, b=None: lib.nvt_emb_grad_plan(i, b, _lib.NVT_I64, 4, t, 1, 4, ws, 1 << 40, oor, None)
    refused(plan(None), b"null descriptors")
    refused(plan(tables(dim=0)), b"dim")
    refused(plan(tables(), i=None), b"either ids or bag columns")
    refused(plan(tables(), b=bag), b"either ids or bag columns")
    refused(lib.nvt_emb_grad_plan(ids, None, _lib.NVT_I64, 4, tables(), 1, 4, ws, 64, oor, None), b"workspace smaller")
    counts = (C.c_int64 * 6)(1, 1, 1, 1, 0, 1)
    go = (_lib.EmbGradOut * 1)()
    reduce = lambda t, entries=4, o=go: lib.nvt_emb_grad_reduce(0, 4, entries, t, 1, 0, out, 4, ws, 1 << 40, counts,
                                                                None, 0, o, None)
    refused(reduce(None), b"null descriptors")
    refused(reduce(tables(), entries=5), b"entries = batch")
    refused(reduce(tables(), entries=2**32), b"2^30")
    refused(reduce(tables(), o=None), b"null grad_out")
    refused(reduce(tables()), b"null or unaligned gradient")
    assert gather(tables(), batch=0) == 0                      # nothing to do
