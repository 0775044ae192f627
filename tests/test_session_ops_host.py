"""Host side of the session operators (ops.ListSlice / ops.ValueCount / ops.DifferenceLag):
constructor normalisation, schemas through Workflow graph construction, the reference's module
aliases, and the argument validation of the new C entry points -- nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import nvtabular_amd as nvt
from nvtabular_amd import _lib, ops
from nvtabular_amd.schema import ColumnSchema, Schema, Tags

INT64_MAX = (1 << 63) - 1


@pytest.mark.parametrize("args, start, end, max_elements", [
    ((10,), 0, 10, 10),
    ((1, 11), 1, 11, 10),
    ((-10,), -10, INT64_MAX, 10),
    ((-10, -2), -10, -2, 8),
    ((-5, 0), -5, 0, 5),
    ((0,), 0, INT64_MAX, None),
    ((1, -1), 1, -1, None),
    ((5, 3), 5, 3, 0),       # end <= start, same sign: every row is empty
    ((-2, -4), -2, -4, 0),
])
def test_list_slice_constructor(args, start, end, max_elements):
    op = ops.ListSlice(*args)
    assert (op.start, op.end, op.max_elements) == (start, end, max_elements)
    assert op.pad is False and op.pad_value == 0.0


def test_list_slice_unbounded_pad_raises():
    with pytest.raises(ValueError, match="no length bound"):
        ops.ListSlice(0, pad=True)
    with pytest.raises(ValueError, match="no length bound"):
        ops.ListSlice(1, -1, pad=True)
    assert ops.ListSlice(-5, 0, pad=True).max_elements == 5   # bounded: fine


def _list_schema():
    return Schema([
        ColumnSchema("a", np.int64, tags=[Tags.CATEGORICAL], is_list=True, is_ragged=True),
        ColumnSchema("b", np.float32, is_list=True, is_ragged=True, properties={"keep": 1}),
        ColumnSchema("u", np.int64),
        ColumnSchema("x", np.int64),
    ])


@pytest.mark.parametrize("args, pad, vc, ragged", [
    ((-20,), False, {"min": 0, "max": 20}, True),
    ((-20,), True, {"min": 20, "max": 20}, False),
    ((1, 11), False, {"min": 0, "max": 10}, True),
    ((0,), False, {"min": 0, "max": None}, True),
    ((1, -1), False, {"min": 0, "max": None}, True),
])
def test_list_slice_schema(args, pad, vc, ragged):
    wf = nvt.Workflow(["a", "b"] >> ops.ListSlice(*args, pad=pad))
    wf.fit_schema(_list_schema())
    out = wf.output_schema
    assert out.column_names == ["a", "b"]
    for name, dt in (("a", np.int64), ("b", np.float32)):
        c = out[name]
        assert c.dtype == np.dtype(dt)
        assert c.is_list is True and c.is_ragged is ragged
        assert Tags.LIST in c.tags
        assert c.properties["value_count"] == vc
    assert Tags.CATEGORICAL in out["a"].tags and out["b"].properties["keep"] == 1


def test_value_count_schema_and_clear():
    op = ops.ValueCount()
    wf = nvt.Workflow(["a", "b"] >> op)
    wf.fit_schema(_list_schema())
    for name in ("a", "b"):   # not fitted: nothing is known
        c = wf.output_schema[name]
        assert c.properties["value_count"] == {"min": 0, "max": None}
        assert c.is_list and c.is_ragged
    op.fit_finalize({"a": {"value_count": {"min": 20, "max": 20}},
                     "b": {"value_count": {"min": 1, "max": 7}}})
    wf.fit_schema(_list_schema())
    a, b = wf.output_schema["a"], wf.output_schema["b"]
    assert a.properties["value_count"] == {"min": 20, "max": 20} and a.is_list and not a.is_ragged
    assert b.properties["value_count"] == {"min": 1, "max": 7} and b.is_list and b.is_ragged
    assert b.properties["keep"] == 1 and b.dtype == np.dtype(np.float32)
    assert isinstance(op, ops.StatOperator)
    op.clear()
    assert op.stats == {}


def test_value_count_after_list_slice_schema():
    wf = nvt.Workflow(["a"] >> ops.ListSlice(-20, pad=True) >> ops.ValueCount())
    wf.fit_schema(_list_schema())
    assert wf.output_schema["a"].is_list


def test_difference_lag_names_schema_dependencies():
    op = ops.DifferenceLag("u", shift=[1, -1])
    assert op.partition_cols == ["u"] and op.shifts == [1, -1]
    assert op.dependencies == ["u"]
    assert ops.DifferenceLag(["u", "v"]).shifts == [1]
    assert op.column_mapping(nvt.ColumnSelector(["x"])) == {
        "x_difference_lag_1": ["x"], "x_difference_lag_-1": ["x"]}
    node = ["x"] >> op
    assert [d.selector.names for d in node.dependencies] == [["u"]]
    wf = nvt.Workflow(node)
    wf.fit_schema(_list_schema())
    out = wf.output_schema
    assert out.column_names == ["x_difference_lag_1", "x_difference_lag_-1"]
    for c in out:
        assert c.dtype == np.dtype(np.float32) and not c.is_list and not c.is_ragged
        assert Tags.CONTINUOUS in c.tags


def test_reference_module_aliases():
    import nvtabular  # noqa: F401
    from nvtabular.ops.difference_lag import DifferenceLag
    from nvtabular.ops.list_slice import ListSlice
    from nvtabular.ops.value_counts import ValueCount

    assert ListSlice is ops.ListSlice and ValueCount is ops.ValueCount and DifferenceLag is ops.DifferenceLag


def test_not_in_graph_json_registry(tmp_path):
    """The three operators are not serialised: Workflow.save raises the serializer's own error."""
    from nvtabular_amd import graph_json

    wf = nvt.Workflow(["a"] >> ops.ListSlice(5))
    wf.fit_schema(_list_schema())
    with pytest.raises(Exception) as e:
        graph_json.serialize_graph(wf, str(tmp_path))
    assert "ListSlice" in str(e.value)


def test_list_entries_reject_bad_arguments():
    lib = _lib.load()
    EINVAL = _lib.NVT_EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    need = C.c_uint64()
    assert lib.nvt_list_slice_ws_bytes(5000, None) == EINVAL and b"null" in lib.nvt_last_error()
    assert lib.nvt_list_slice_ws_bytes(5000, C.byref(need)) == 0 and need.value == 4 * 8
    # offsets plan
    assert lib.nvt_list_slice_offsets(None, 4, 0, 2, p, p, 64, None) == EINVAL
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_list_slice_offsets(p, 4, 0, 2, None, p, 64, None) == EINVAL
    assert lib.nvt_list_slice_offsets(p, 4, 0, 2, p, None, 64, None) == EINVAL
    assert b"workspace" in lib.nvt_last_error()
    assert lib.nvt_list_slice_offsets(p, 4, 0, 2, p, p, 8, None) == EINVAL      # workspace too small
    assert lib.nvt_list_slice_offsets(p, 0, 0, 2, p, p, 64, None) == EINVAL      # no rows
    # leaf move
    col = _lib.ListCol(src=p, dst=p, width=8)
    arr = (_lib.ListCol * 1)(col)
    assert lib.nvt_list_slice_many(None, 1, p, 4, 0, 2, p, 8, 0, None) == EINVAL
    assert b"null" in lib.nvt_last_error()
    assert lib.nvt_list_slice_many(arr, 0, p, 4, 0, 2, p, 8, 0, None) == EINVAL
    assert b"ncols" in lib.nvt_last_error()
    bad = (_lib.ListCol * 1)(_lib.ListCol(src=p, dst=p, width=2))
    assert lib.nvt_list_slice_many(bad, 1, p, 4, 0, 2, p, 8, 0, None) == EINVAL
    assert b"width" in lib.nvt_last_error()
    assert lib.nvt_list_slice_many(arr, 1, p, 4, 0, 2, p, 8, 2, None) == EINVAL  # ragged AND padded
    assert lib.nvt_list_slice_many(arr, 1, p, 4, 0, 2, None, 8, 0, None) == EINVAL  # neither
    assert lib.nvt_list_slice_many(arr, 1, p, 4, 0, 2, None, 9, 2, None) == EINVAL  # total != n * width
    nodst = (_lib.ListCol * 1)(_lib.ListCol(src=p, dst=None, width=8))
    assert lib.nvt_list_slice_many(nodst, 1, p, 4, 0, 2, p, 8, 0, None) == EINVAL
    novalid = (_lib.ListCol * 1)(_lib.ListCol(src=p, dst=p, src_valid=p, dst_valid=None, width=8))
    assert lib.nvt_list_slice_many(novalid, 1, p, 4, 0, 2, p, 8, 0, None) == EINVAL
    assert lib.nvt_list_slice_many(arr, 1, p, 4, 0, 2, p, 0, 0, None) == 0        # nothing to move
    # ValueCount
    assert lib.nvt_list_len_minmax(None, 1, None) == EINVAL and b"null" in lib.nvt_last_error()
    lens = (_lib.ListLenCol * 1)(_lib.ListLenCol(offsets=p, n=4, acc=None))
    assert lib.nvt_list_len_minmax(lens, 0, None) == EINVAL
    assert lib.nvt_list_len_minmax(lens, 1, None) == EINVAL and b"null" in lib.nvt_last_error()
    empty = (_lib.ListLenCol * 1)(_lib.ListLenCol(offsets=p, n=0, acc=None))
    assert lib.nvt_list_len_minmax(empty, 1, None) == 0                            # zero rows: no launch


def test_difference_lag_entry_rejects_bad_arguments():
    lib = _lib.load()
    EINVAL = _lib.NVT_EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    keys = (_lib.LagKey * 5)(*[_lib.LagKey(x=p, dtype=_lib.NVT_I64) for _ in range(5)])
    cols = (_lib.LagCol * 1)(_lib.LagCol(x=p, out=p, shift=1, dtype=_lib.NVT_I64))
    assert lib.nvt_difference_lag_many(keys, 5, cols, 1, 8, None) == EINVAL
    assert b"4 partition columns" in lib.nvt_last_error()
    assert lib.nvt_difference_lag_many(None, 1, cols, 1, 8, None) == EINVAL and b"null" in lib.nvt_last_error()
    assert lib.nvt_difference_lag_many(keys, 1, None, 1, 8, None) == EINVAL and b"null" in lib.nvt_last_error()
    assert lib.nvt_difference_lag_many(keys, 1, cols, 0, 8, None) == EINVAL and b"ncols" in lib.nvt_last_error()
    bad = (_lib.LagCol * 1)(_lib.LagCol(x=p, out=p, shift=1, dtype=9))
    assert lib.nvt_difference_lag_many(keys, 1, bad, 1, 8, None) == EINVAL and b"dtype" in lib.nvt_last_error()
    badkey = (_lib.LagKey * 1)(_lib.LagKey(x=p, dtype=-1))
    assert lib.nvt_difference_lag_many(badkey, 1, cols, 1, 8, None) == EINVAL
    noout = (_lib.LagCol * 1)(_lib.LagCol(x=p, out=None, shift=1, dtype=_lib.NVT_I64))
    assert lib.nvt_difference_lag_many(keys, 1, noout, 1, 8, None) == EINVAL
    assert lib.nvt_difference_lag_many(keys, 1, cols, 1, 0, None) == 0             # zero rows: no launch


def test_operators_check_their_inputs_without_a_gpu():
    """Type checks come before any launch (the frames are built from host tensors)."""
    import torch

    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    off = torch.tensor([0, 2, 3], dtype=torch.int64)
    frame = DeviceFrame({
        "l": DeviceColumn(torch.arange(3), None, off),
        "s": DeviceColumn(torch.arange(3), None, off, None, {0: "a", 1: "b", 2: "c"}),
        "x": DeviceColumn(torch.arange(2)),
        "b": DeviceColumn(torch.tensor([True, False])),
        "t": DeviceColumn(torch.arange(2), None, None, None, {0: "a", 1: "b"}),
    })
    with pytest.raises(TypeError, match="not a list column"):
        ops.ListSlice(2).transform(nvt.ColumnSelector(["x"]), frame)
    with pytest.raises(NotImplementedError, match="string"):
        ops.ListSlice(2, pad=True).transform(nvt.ColumnSelector(["s"]), frame)
    for target in ("b", "t"):
        with pytest.raises(TypeError):
            ops.DifferenceLag("x").transform(nvt.ColumnSelector([target]), frame[["x", "b", "t"]])
    with pytest.raises(TypeError, match="list"):
        ops.DifferenceLag("x").transform(nvt.ColumnSelector(["l"]), frame[["x", "l"]])
    with pytest.raises(TypeError, match="partition"):
        ops.DifferenceLag("l").transform(nvt.ColumnSelector(["x"]), frame[["x", "l"]])
    with pytest.raises(NotImplementedError, match="partition"):
        ops.DifferenceLag(["x"] * 5).transform(nvt.ColumnSelector(["x"]), frame[["x"]])
    # an empty frame needs no launch
    empty = DeviceFrame({"l": DeviceColumn(torch.empty(0, dtype=torch.int32), None,
                                           torch.zeros(1, dtype=torch.int64))})
    out = ops.ListSlice(-3, pad=True).transform(nvt.ColumnSelector(["l"]), empty)
    assert len(out) == 0 and out["l"].data.dtype == torch.int32 and out["l"].offsets.tolist() == [0]
