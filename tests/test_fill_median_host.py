"""ops.FillMedian without a GPU: export, schema, graph-JSON serialisation and the C-ABI names."""
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_operator_is_exported():
    import nvtabular
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.ops.base import StatOperator
    from nvtabular_amd.ops.fill import FillMedian

    assert ops.FillMedian is FillMedian and issubclass(FillMedian, StatOperator)
    assert nvtabular.ops.FillMedian is FillMedian
    op = FillMedian()
    assert op.add_binary_cols is False and op.medians == {}
    assert FillMedian(add_binary_cols=True).add_binary_cols is True
    assert "memory" in FillMedian.__doc__.lower()
    assert nvt.Workflow(["a"] >> ops.FillMedian() >> ops.Normalize()) is not None


def test_column_mapping_and_schema_for_both_flags():
    import nvtabular_amd as nvt
    from nvtabular_amd import ops
    from nvtabular_amd.schema import ColumnSchema, Schema
    from nvtabular_amd.selector import ColumnSelector

    sel = ColumnSelector(["x", "y"])
    assert ops.FillMedian().column_mapping(sel) == {"x": ["x"], "y": ["y"]}
    assert ops.FillMedian(add_binary_cols=True).column_mapping(sel) == {
        "x": ["x"], "y": ["y"], "x_filled": ["x"], "y_filled": ["y"]}
    root = Schema([ColumnSchema("x", dtype=np.float32), ColumnSchema("y", dtype=np.int64)])
    plain = nvt.Workflow(["x", "y"] >> ops.FillMedian())
    plain.fit_schema(root)
    assert plain.output_schema.column_names == ["x", "y"]
    assert plain.output_schema["x"].dtype == np.float32 and plain.output_schema["y"].dtype == np.int64
    flagged = nvt.Workflow(["x", "y"] >> ops.FillMedian(add_binary_cols=True))
    flagged.fit_schema(root)
    out = flagged.output_schema
    assert out.column_names == ["x", "y", "x_filled", "y_filled"]
    assert out["x"].dtype == np.float32 and out["y"].dtype == np.int64
    assert out["x_filled"].dtype == np.dtype(bool) and out["y_filled"].dtype == np.dtype(bool)


def test_graph_json_round_trip_of_hand_set_medians(tmp_path):
    import nvtabular_amd as nvt
    from nvtabular_amd import graph_json, ops
    from nvtabular_amd.schema import ColumnSchema, Schema

    op = ops.FillMedian(add_binary_cols=True)
    op.medians = {"x": 1.5, "y": -3.0, "z": 0.1 + 0.2}
    wf = nvt.Workflow(["x", "y", "z"] >> op)
    wf.fit_schema(Schema([ColumnSchema(c, dtype=np.float64) for c in "xyz"]))
    path = str(tmp_path)
    graph_json.serialize_graph(wf, path)
    rec = [r for r in json.load(open(os.path.join(path, "graph.json")))["nodes"]
           if r["op_class"] == "nvtabular.ops.fill.FillMedian"]
    assert len(rec) == 1 and rec[0]["op_params"] == {"add_binary_cols": True}
    assert rec[0]["op_state"] == {"medians": op.medians}
    node = graph_json.deserialize_graph(path)
    back = node.op
    assert type(back) is ops.FillMedian and back.add_binary_cols is True
    assert back.medians == op.medians          # bit for bit through JSON
    assert node.output_schema.column_names == ["x", "y", "z", "x_filled", "y_filled", "z_filled"]


def test_c_abi_names_in_header_and_ctypes_table():
    from nvtabular_amd import _lib

    src = open(os.path.join(ROOT, "include", "nvt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("nvt_select_hist_many", "nvt_select_step", "nvt_select_finish"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    # the constants the driver mirrors
    defs = dict(re.findall(r"#define\s+(NVT_SELECT_\w+)\s+(\d+)\s", src))
    assert int(defs["NVT_SELECT_CAND_CAP"]) == _lib.SELECT_CAND_CAP == 65536
    assert int(defs["NVT_SELECT_BINS"]) == _lib.SELECT_BINS == 2048
    assert int(defs["NVT_SELECT_MAX_COLS"]) == _lib.SELECT_MAX_COLS
    for word in ("M", "RANK_LO", "RANK_HI", "KEY_LO", "KEY_HI", "DONE", "NCAND", "USE_CAND", "PATH", "BITS",
                 "ALLOW_CAND", "HIST"):
        assert int(defs[f"NVT_SELECT_ST_{word}"]) == getattr(_lib, f"SELECT_ST_{word}"), word
    assert _lib.SELECT_STATE_WORDS == 16 + 2 * 2048 + 65536
    assert "nvt_select.hip" in open(os.path.join(ROOT, "nvtabular_amd", "csrc", "Makefile")).read()


def test_select_entries_refuse_bad_arguments_before_any_launch():
    import ctypes as C

    from nvtabular_amd import _lib

    lib = _lib.load()
    raw = (C.c_uint8 * 256)()
    base = (C.addressof(raw) + 63) & ~63

    def refused(rc, *words):
        assert rc == _lib.NVT_EINVAL, (rc, lib.nvt_last_error())
        for w in words:
            assert w in lib.nvt_last_error(), (w, lib.nvt_last_error())

    d = (_lib.SelectCol * 1)()
    d[0].x, d[0].n, d[0].dtype = base, 4, _lib.NVT_F64
    refused(lib.nvt_select_hist_many(None, 1, 0, base, None), b"null descriptors")
    refused(lib.nvt_select_hist_many(d, 1, 6, base, None), b"pass")
    refused(lib.nvt_select_hist_many(d, 1, -1, base, None), b"pass")
    refused(lib.nvt_select_hist_many(d, 1, 0, None, None), b"state")
    refused(lib.nvt_select_hist_many(d, -1, 0, base, None), b"ncols")
    d[0].dtype = _lib.NVT_U8
    refused(lib.nvt_select_hist_many(d, 1, 0, base, None), b"dtype")
    d[0].dtype = 17
    refused(lib.nvt_select_hist_many(d, 1, 0, base, None), b"dtype")
    d[0].dtype, d[0].x = _lib.NVT_I32, base + 4
    refused(lib.nvt_select_hist_many(d, 1, 0, base, None), b"aligned")
    d[0].x = None
    refused(lib.nvt_select_hist_many(d, 1, 0, base, None), b"x must be non-null")
    assert lib.nvt_select_hist_many(None, 0, 0, None, None) == 0
    refused(lib.nvt_select_step(None, 1, 0, None), b"state")
    refused(lib.nvt_select_step(base, 1, 6, None), b"pass")
    assert lib.nvt_select_step(None, 0, 0, None) == 0
    refused(lib.nvt_select_finish(None, 1, None), b"state")
    refused(lib.nvt_select_finish(base, -1, None), b"ncols")
    assert lib.nvt_select_finish(None, 0, None) == 0


def test_keys_are_order_preserving_on_the_host():
    from nvtabular_amd import kernels_select as KS

    for dt, vals in ((np.float64, [-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf]),
                     (np.float32, [-np.inf, -3.0, -0.0, 0.0, 1e-45, 2.5, np.inf]),
                     (np.int32, [-2**31, -1, 0, 1, 2**31 - 1]), (np.int64, [-2**63, -1, 0, 1, 2**63 - 1])):
        keys = [KS.key_of(v, dt) for v in vals]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), dt
        for v, k in zip(vals, keys):
            assert KS.value_of(k, dt).tobytes() == np.array([v], dtype=dt).tobytes()
    # numpy's linear interpolation at t = 0.5, in the column's own difference type
    assert KS.median_of(np.float64(1.0), np.float64(2.0)) == 1.5
    assert KS.median_of(np.int64(3), np.int64(3)) == 3.0
    assert KS.median_of(np.int32(-1), np.int32(2)) == 0.5
