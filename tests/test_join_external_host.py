"""ops.JoinExternal without a GPU: construction errors, the output schema (the reference's
column_mapping order and the external dtypes), Workflow.save, and argument validation of the
nvt_join_* C entries (rejected on the host side with NVT_EINVAL before any launch)."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest


def _lib():
    import os

    from nvtabular_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def _ext():
    return pd.DataFrame({"item": np.arange(5, dtype=np.int64), "price": np.linspace(1, 2, 5),
                         "brand": ["a", "b", "c", "d", "e"], "stock": np.arange(5, dtype=np.int32)})


def test_exported_under_both_names():
    import nvtabular
    import nvtabular.ops.join_external as alias
    from nvtabular_amd import ops

    assert ops.JoinExternal is nvtabular.ops.JoinExternal is alias.JoinExternal


def test_how_right_raises():
    from nvtabular_amd import ops

    with pytest.raises(ValueError):
        ops.JoinExternal(_ext(), on="item", how="right")


def test_external_list_columns_raise_type_error():
    from nvtabular_amd import ops

    ext = pd.DataFrame({"item": [1, 2], "tags": [[1, 2], [3]]})
    with pytest.raises(TypeError):
        ops.JoinExternal(ext, on="item")
    ops.JoinExternal(ext, on="item", columns_ext=["item"])   # not selected: fine


def _workflow(op, cols):
    import nvtabular_amd as nvt

    wf = nvt.Workflow(cols >> op)
    return wf


def _fit_schema(wf, df):
    from nvtabular_amd.schema import Schema

    wf.fit_schema(Schema.from_frame(df))
    return wf


def test_non_key_column_on_both_sides_raises():
    from nvtabular_amd import ops

    left = pd.DataFrame({"item": np.arange(3), "price": np.ones(3)})
    wf = _workflow(ops.JoinExternal(_ext(), on="item"), ["item", "price"])
    with pytest.raises(ValueError, match="both sides"):
        _fit_schema(wf, left)


def test_string_key_against_int_key_raises():
    from nvtabular_amd import kernels_join as KJ

    with pytest.raises(ValueError, match="string"):
        KJ.key_modes(["s"], ["i"], ["k"], ["k"])
    with pytest.raises(ValueError, match="string"):
        KJ.key_modes(["i", "f"], ["i", "s"], ["a", "b"], ["a", "b"])
    assert KJ.key_modes(["i", "f", "s", "i"], ["f", "i", "s", "i"], "abcd", "abcd") == (1, 1, 0, 0)


def test_output_schema_follows_the_reference_column_mapping():
    from nvtabular_amd import ops

    left = pd.DataFrame({"user": np.arange(3, dtype=np.int32), "item": np.arange(3, dtype=np.int32),
                         "y": np.zeros(3, np.float32)})
    wf = _fit_schema(_workflow(ops.JoinExternal(_ext(), on="item"), ["user", "item", "y"]), left)
    assert list(wf.output_dtypes) == ["user", "item", "y", "price", "brand", "stock"]
    assert wf.output_dtypes["item"] == np.dtype("int32")          # the left key is kept
    assert wf.output_dtypes["price"] == np.dtype("float64")
    assert wf.output_dtypes["stock"] == np.dtype("int32")
    assert wf.output_dtypes["brand"] == np.dtype("O")

    # on != on_ext: both key columns are present; columns_ext order is kept
    ext = _ext().rename(columns={"item": "item_id"})
    op = ops.JoinExternal(ext, on="item", on_ext="item_id", columns_ext=["stock", "item_id"])
    wf = _fit_schema(_workflow(op, ["user", "item", "y"]), left)
    assert list(wf.output_dtypes) == ["user", "item", "y", "stock", "item_id"]
    assert wf.output_dtypes["item_id"] == np.dtype("int64")


def test_external_schema_from_arrow_keeps_int_dtype():
    import pyarrow as pa

    from nvtabular_amd import ops

    ext = pa.table({"k": pa.array([1, 2, 3], pa.int64()), "v": pa.array([1, None, 3], pa.int64())})
    left = pd.DataFrame({"k": np.arange(3)})
    wf = _fit_schema(_workflow(ops.JoinExternal(ext, on="k"), ["k"]), left)
    assert wf.output_dtypes["v"] == np.dtype("int64")


def test_workflow_save_raises_not_implemented(tmp_path):
    from nvtabular_amd import ops

    left = pd.DataFrame({"item": np.arange(3)})
    wf = _fit_schema(_workflow(ops.JoinExternal(_ext(), on="item"), ["item"]), left)
    with pytest.raises(NotImplementedError):
        wf.save(str(tmp_path / "wf"))


def test_join_entries_reject_bad_arguments():
    from nvtabular_amd import _lib as L

    lib = _lib()
    cap, nbytes = C.c_uint64(), C.c_uint64()
    assert lib.nvt_join_table_bytes(10, None, C.byref(nbytes)) == -1
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_join_table_bytes(0, C.byref(cap), C.byref(nbytes)) == 0 and cap.value == 64
    assert lib.nvt_join_table_bytes(1000, C.byref(cap), C.byref(nbytes)) == 0
    assert cap.value == 2048 and nbytes.value == 2048 * 16

    vals = (C.c_int64 * 4)()
    key = (L.JoinKey * 1)(L.JoinKey(C.addressof(vals), None, L.NVT_I64, L.JOIN_INT))
    out = (C.c_uint64 * 4)()
    nulls = (C.c_uint8 * 4)()
    assert lib.nvt_join_hash(None, 1, 4, out, None, nulls, None) == -1
    assert lib.nvt_join_hash(key, 0, 4, out, None, nulls, None) == -1
    assert b"nkeys" in lib.nvt_last_error()
    assert lib.nvt_join_hash(key, 5, 4, out, None, nulls, None) == -1
    assert lib.nvt_join_hash(key, 1, 4, None, None, nulls, None) == -1
    bad = (L.JoinKey * 1)(L.JoinKey(C.addressof(vals), None, L.NVT_F64, L.JOIN_INT))
    assert lib.nvt_join_hash(bad, 1, 4, out, None, nulls, None) == -1
    assert b"float" in lib.nvt_last_error()
    two = (L.JoinKey * 2)(key[0], key[0])
    assert lib.nvt_join_hash(two, 2, 4, out, None, nulls, None) == -1       # words needed
    assert lib.nvt_join_hash(key, 1, 0, None, None, None, None) == 0        # nothing to do

    slots = (C.c_uint64 * 130)()
    base = (C.addressof(slots) + 15) & ~15
    assert lib.nvt_join_insert(None, 64, 0, out, out, out, 1, None) == -1
    assert lib.nvt_join_insert(base, 48, 0, out, out, out, 1, None) == -1
    assert b"power of two" in lib.nvt_last_error()
    assert lib.nvt_join_insert(base + 8, 64, 0, out, out, out, 1, None) == -1
    assert b"aligned" in lib.nvt_last_error()
    assert lib.nvt_join_insert(base, 64, 0, out, out, out, 33, None) == -1   # load above 0.5
    assert lib.nvt_join_insert(base, 64, 0, None, None, None, 1, None) == -1
    assert lib.nvt_join_insert(base, 64, 0, None, None, None, 0, None) == 0

    ix = L.JoinIndex(slots=base, capacity=64, nkeys=1)
    first = (C.c_int64 * 4)()
    assert lib.nvt_join_probe(None, key, 1, 4, 0, first, None, None, None, None) == -1
    assert lib.nvt_join_probe(C.byref(ix), key, 1, 4, 0, None, None, None, None, None) == -1
    assert lib.nvt_join_probe(C.byref(ix), two, 2, 4, 0, first, None, None, None, None) == -1
    assert b"number of key columns" in lib.nvt_last_error()
    noslots = L.JoinIndex(slots=None, capacity=64, nkeys=1)
    assert lib.nvt_join_probe(C.byref(noslots), key, 1, 4, 0, first, None, None, None, None) == -1
    assert lib.nvt_join_probe(C.byref(ix), key, 1, 0, 0, None, None, None, None, None) == 0

    dst = (C.c_int64 * 4)()
    valid = (C.c_uint64 * 1)()
    col = L.JoinCol(C.addressof(vals), None, C.addressof(dst), C.addressof(valid), 8)
    cols = (L.JoinCol * 1)(col)
    assert lib.nvt_join_probe_gather(C.byref(ix), key, 1, 4, None, 1, None, None) == -1
    assert lib.nvt_join_probe_gather(C.byref(ix), key, 1, 4, cols, 0, None, None) == -1
    assert lib.nvt_join_probe_gather(C.byref(ix), key, 1, 4, cols, 17, None, None) == -1
    novalid = (L.JoinCol * 1)(L.JoinCol(C.addressof(vals), None, C.addressof(dst), None, 8))
    assert lib.nvt_join_probe_gather(C.byref(ix), key, 1, 4, novalid, 1, None, None) == -1
    assert b"dst_valid" in lib.nvt_last_error()
    badw = (L.JoinCol * 1)(L.JoinCol(C.addressof(vals), None, C.addressof(dst), C.addressof(valid), 2))
    assert lib.nvt_join_gather(first, 4, badw, 1, None) == -1
    assert b"width" in lib.nvt_last_error()
    assert lib.nvt_join_gather(None, 4, cols, 1, None) == -1
    assert lib.nvt_join_gather(None, 0, cols, 1, None) == 0

    need = C.c_uint64()
    assert lib.nvt_join_scan_ws_bytes(100, None) == -1
    assert lib.nvt_join_scan_ws_bytes(100, C.byref(need)) == 0 and need.value >= 8
    counts = (C.c_uint32 * 101)()
    ws = (C.c_uint64 * 4)()
    assert lib.nvt_join_offsets(None, 100, ws, need.value, None) == -1
    assert lib.nvt_join_offsets(counts, 100, None, need.value, None) == -1
    assert lib.nvt_join_offsets(counts, 100, ws, 0, None) == -1
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_join_expand(None, first, 4, 8, first, first, None) == -1
    assert lib.nvt_join_expand(counts, first, 0, 8, first, first, None) == -1
    assert lib.nvt_join_expand(counts, first, 4, 1 << 32, first, first, None) == -1
    assert lib.nvt_join_expand(None, None, 0, 0, None, None, None) == 0
